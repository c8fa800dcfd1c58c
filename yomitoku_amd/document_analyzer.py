"""Page orchestrators: OCR, LayoutAnalyzer, DocumentAnalyzer (reference ocr.py:6-63,
layout_analyzer.py:7-49, document_analyzer.py:23-678): same constructors, nested `configs` keys and
return tuples.  The aggregation is integer box logic on the host and must give bit-exact word ->
cell / paragraph assignment and reading order.

MI355X specifics: the uint8 page is uploaded to HBM ONCE and shared by the four modules; the
det -> rec chain and the layout -> table chain still run concurrently (two Python threads, each
with its own HIP stream), as in document_analyzer.py:622-669.
"""

from __future__ import annotations

import math
import re

import numpy as np
import torch

from . import imaging
from .geometry import calc_overlap_ratio, containment_matrix, is_contained, quad_to_xyxy
from .layout_parser import LayoutParser
from .reading_order import prediction_reading_order
from .schemas import (
    DocumentAnalyzerSchema,
    FigureSchema,
    LayoutAnalyzerSchema,
    OCRSchema,
    ParagraphSchema,
)
from .deskew import check_deskew
from .figures import check_figures
from .serving import StageAnalyzer, check_jpeg_preset
from .table_structure_recognizer import TableStructureRecognizer
from .text_detector import TextDetector
from .text_recognizer import TextRecognizer

def _vis_to_host(vis):
    """What a public call returns for `vis`: the device canvas of a visualize=True chain as np.ndarray (None stays None)."""
    return vis if vis is None or isinstance(vis, np.ndarray) else vis.cpu().numpy()


_USAGE = "configs must be a dict. See the https://kotaro-kinoshita.github.io/yomitoku/module/#config"


# ---------------------------------------------------------------------------------------------- OCR
def ocr_aggregate(det_outputs, rec_outputs):
    return [
        {"points": p, "content": c, "direction": d, "det_score": ds, "rec_score": rs}
        for p, ds, c, rs, d in zip(det_outputs.points, det_outputs.scores, rec_outputs.contents, rec_outputs.scores,
                                   rec_outputs.directions)
    ]


_NO_VIS_SERVE = ("visualize=True is not supported by serve / serve_sharded: build the analyzer with "
                 "visualize=False and ask per job, serve(..., overlays=True) (__call__ and analyze_pages "
                 "draw with visualize=True)")


class OCR(StageAnalyzer):
    chains = ("ocr",)  # the page pipeline runs detect ... decode and `finish` for it: there is no layout chain to wait for

    def __init__(self, configs={}, device="cuda", visualize=False, workspace_reuse=False):
        det_kwargs = {"device": device, "visualize": visualize, "workspace_reuse": workspace_reuse}
        rec_kwargs = {"device": device, "visualize": visualize, "workspace_reuse": workspace_reuse}
        if not isinstance(configs, dict):
            raise ValueError(_USAGE)
        det_kwargs.update(configs.get("text_detector", {}))
        rec_kwargs.update(configs.get("text_recognizer", {}))
        self.detector = TextDetector(**det_kwargs)
        self.recognizer = TextRecognizer(**rec_kwargs)
        self.visualize = visualize
        self._init_chains()

    # the reference's names are `detector` / `recognizer`; the shared stage bodies and close() say text_detector / text_recognizer
    @property
    def text_detector(self):
        return self.detector

    @property
    def text_recognizer(self):
        return self.recognizer

    def _nets(self):
        return self.detector, self.recognizer

    def __call__(self, img):
        page = imaging.page_to_device(img, self.detector.device) if not isinstance(img, torch.Tensor) else img
        det_outputs, vis = self.detector._call(page, to_host=False)  # the overlay stays on the device inside the chain
        rec_outputs, vis = self.recognizer._call(page, det_outputs.points, vis=vis, to_host=False)
        return OCRSchema(words=ocr_aggregate(det_outputs, rec_outputs)), _vis_to_host(vis)

    def _stage_finish(self, wave, k):
        """Page k of the wave -> OCRSchema: what `__call__` makes of the page's detections and strings."""
        return OCRSchema(words=ocr_aggregate(wave.dets[k], wave.recs[k]))

    def _page_drawings(self, wave, k, results):
        """The one drawing of page k of a finished wave: the detection quads and the recognised strings, recorded as
        DocumentAnalyzer records its OCR picture."""
        return (self._ocr_drawing(wave, k),)

    def serve(self, sources, wave: int = 16, in_flight: int = 4, defer_full_gc: bool = True, with_source: bool = False, rec_lanes: int = 2,
              overlays: bool = False, jpeg=None, jpeg_optimize: bool = False, jpeg_subsampling=None, jpeg_grey=False,
              jpeg_bilevel=False, deskew=False, jpeg_mrc=False, jpeg_despeckle=False, jpeg_lossless=False):
        """The multi-page entry point of a text-only job (searchable PDFs, full-text indexing): host pages (uint8 H x W x 3 BGR
        arrays) and / or image file paths in, one result per page out, in page order, through the stage pipeline of
        yomitoku_amd/serving.py with the OCR chain alone - detect, boxes, crops, recognize (two lanes), decode, finish; no
        layout, tables or cells stage exists for this analyzer, neither thread nor stream.  Arguments and conventions are
        `DocumentAnalyzer.serve`'s.  A page's entry is its OCRSchema - equal to `__call__(img)[0]` - or, when the page (or
        its file) failed, the exception object; the other pages are not affected.
        `wave`, `in_flight`, `defer_full_gc`, `with_source`, `rec_lanes`: see `DocumentAnalyzer.serve`.
        `overlays`: a property of the job - True: a page's entry is (schema, ocr overlay), the picture with the detection quads
        and the recognised strings (the first of DocumentAnalyzer's two, byte for byte) as a uint8 H x W x 3 array the caller
        owns, drawn by the pipeline's render stage.
        `jpeg`: None, or a preset of the searchable PDF ("high", "middle", "low"; anything else is a ValueError before a source
        is read): a page's entry ends with its EncodedJpeg - (schema, EncodedJpeg), or (schema, ocr overlay, EncodedJpeg) -
        encoded on the device from the clean page, so that
            searchable_pdf_bytes([e[-1] for e in out], [e[0] for e in out])
        is the whole searchable-PDF job.  `jpeg_optimize`: those files with Huffman tables made for each page; a ValueError
        without `jpeg`.  `jpeg_subsampling`, `jpeg_grey`, `jpeg_bilevel` (False, "auto", "otsu", "adaptive"), `jpeg_mrc`
        (False, True or the cells), `jpeg_despeckle` (False, True, an int or the sizes), `jpeg_lossless` (False, True or the budget),
        `deskew`: as DocumentAnalyzer.serve."""
        files = check_jpeg_preset(jpeg, jpeg_optimize, jpeg_subsampling, jpeg_grey, jpeg_bilevel, jpeg_mrc, jpeg_despeckle, jpeg_lossless)  # before the pipeline is built or a source read
        deskew = check_deskew(deskew) or False
        if self.visualize:
            raise NotImplementedError(_NO_VIS_SERVE)
        return self._serve(sources, wave, in_flight, defer_full_gc, with_source, rec_lanes, overlays, files=files, deskew=deskew)


# ---------------------------------------------------------------------------------------------- layout
class LayoutAnalyzer:
    def __init__(self, configs={}, device="cuda", visualize=False, workspace_reuse=False):
        lp_kwargs = {"device": device, "visualize": visualize, "workspace_reuse": workspace_reuse}
        ts_kwargs = {"device": device, "visualize": visualize, "workspace_reuse": workspace_reuse}
        if not isinstance(configs, dict):
            raise ValueError(_USAGE)
        lp_kwargs.update(configs.get("layout_parser", {}))
        ts_kwargs.update(configs.get("table_structure_recognizer", {}))
        self.layout_parser = LayoutParser(**lp_kwargs)
        self.table_structure_recognizer = TableStructureRecognizer(**ts_kwargs)

    def __call__(self, img):
        return self._call(img)

    def _call(self, img, to_host=True):
        """`__call__`; to_host False leaves the overlay on the device (DocumentAnalyzer draws the reading order onto it)."""
        page = imaging.page_to_device(img, self.layout_parser.device) if not isinstance(img, torch.Tensor) else img
        layout_results, vis = self.layout_parser._call(page, to_host=False)
        table_boxes = [t.box for t in layout_results.tables]
        table_results, vis = self.table_structure_recognizer._call(page, table_boxes, vis=vis, to_host=False)
        results = LayoutAnalyzerSchema(paragraphs=layout_results.paragraphs, tables=table_results,
                                       figures=layout_results.figures)
        return results, _vis_to_host(vis) if to_host else vis


# ---------------------------------------------------------------------------------------------- aggregation helpers
def combine_flags(flag1, flag2):
    return [a or b for a, b in zip(flag1, flag2)]


def judge_page_direction(paragraphs):
    """'vertical' when vertical paragraphs cover more area than horizontal ones (:23-40)."""
    area = {"h": 0, "v": 0}
    for p in paragraphs:
        x1, y1, x2, y2 = p.box
        area["h" if p.direction == "horizontal" else "v"] += (x2 - x1) * (y2 - y1)
    return "vertical" if area["v"] > area["h"] else "horizontal"


def extract_paragraph_within_figure(paragraphs, figures):
    """Paragraphs at least 70 % inside a figure move into it, ordered inside the figure (:43-68)."""
    new_figures = []
    taken = [False] * len(paragraphs)
    for figure in figures:
        inside = []
        for i, paragraph in enumerate(paragraphs):
            if is_contained(figure.box, paragraph.box, threshold=0.7):
                inside.append(paragraph)
                taken[i] = True
        direction = judge_page_direction(inside)
        ordered = prediction_reading_order(inside, "left2right" if direction == "horizontal" else "right2left")
        new_figures.append(FigureSchema(box=figure.box, order=0, direction=direction,
                                        paragraphs=sorted(ordered, key=lambda p: p.order)))
    return new_figures, taken


_HIRAGANA = re.compile("^[\u3040-\u309F]+$")
_KATAKANA = re.compile("^[\u30A0-\u30FF]+$")


def _mad_threshold(sizes):
    ordered = sorted(sizes)
    n = len(ordered)
    median = ordered[n // 2]
    if median == 0:
        return None
    mad = sorted(abs(s - median) for s in sizes)[n // 2]
    if mad == 0:
        return None
    t = median - 2 * mad
    return t if t > 0 else None


def _compute_ruby_threshold(sizes, k):
    """Valley between the two dominant peaks of the log-size histogram when the bimodality is strong
    enough (sep >= k), else a median - 2 MAD fallback (:87-137)."""
    n = len(sizes)
    if n < 3:
        return None
    logs = [math.log(s) for s in sizes]
    bins = max(8, int(math.sqrt(n)))
    lo_v, hi_v = min(logs), max(logs)
    if hi_v - lo_v < 1e-9:
        return None
    width = (hi_v - lo_v) / bins
    hist = [0] * bins
    for v in logs:
        hist[min(int((v - lo_v) / width), bins - 1)] += 1
    p1 = max(range(bins), key=lambda i: hist[i])
    p2, p2_val = None, -1
    for i in range(bins):
        if abs(i - p1) >= 2 and hist[i] > p2_val:
            p2, p2_val = i, hist[i]
    if p2 is None:
        return _mad_threshold(sizes)
    lo, hi = min(p1, p2), max(p1, p2)
    if hi - lo <= 1:
        return _mad_threshold(sizes)
    valley_val = min(hist[i] for i in range(lo + 1, hi))
    candidates = [i for i in range(lo + 1, hi) if hist[i] == valley_val]
    valley = candidates[len(candidates) // 2]
    if (hist[p1] + hist[p2]) / (2 * valley_val + 1e-6) >= k:
        return math.exp(lo_v + (valley + 0.5) * width)
    return _mad_threshold(sizes)


def filter_ruby(contained_words, element_direction, ruby_threshold):
    """Drop small kana-only words (furigana) below the size threshold (:140-172)."""
    if len(contained_words) <= 1:
        return contained_words
    sizes = [math.sqrt((w.box[2] - w.box[0]) * (w.box[3] - w.box[1])) for w in contained_words]
    valid = [s for s in sizes if s > 0]
    if len(valid) < 2:
        return contained_words
    threshold = _compute_ruby_threshold(valid, ruby_threshold)
    if threshold is None:
        return contained_words
    kept = []
    for word, s in zip(contained_words, sizes):
        if 0 < s < threshold:
            text = word.contents.replace(" ", "")
            if _HIRAGANA.match(text) or _KATAKANA.match(text):
                continue
        kept.append(word)
    return kept


def extract_words_within_element(pred_words, element, ignore_ruby=False, ruby_threshold=2.0):
    """Words at least 50 % inside `element`, joined in reading order (:175-217).
    Returns (text or None, direction or None, per-word membership flags)."""
    word_boxes = [quad_to_xyxy(word.points) for word in pred_words]
    flags = containment_matrix([element.box], word_boxes, 0.5)[0].tolist()
    return _words_of_element(pred_words, word_boxes, flags, ignore_ruby, ruby_threshold)


def _words_of_element(pred_words, word_boxes, flags, ignore_ruby, ruby_threshold):
    """Second half of extract_words_within_element, given the element's membership flags (aggregate()
    computes them for all cells and paragraphs of the page in one containment_matrix call)."""
    inside = [ParagraphSchema(box=word_boxes[i], contents=pred_words[i].content, direction=pred_words[i].direction,
                              order=0, role=None) for i in np.flatnonzero(flags).tolist()]
    if not inside:
        return None, None, flags
    dirs = [w.direction for w in inside]
    element_direction = "horizontal" if dirs.count("horizontal") > dirs.count("vertical") else "vertical"
    if ignore_ruby:
        inside = filter_ruby(inside, element_direction, ruby_threshold)
        if not inside:
            return None, None, flags
    prediction_reading_order(inside, "left2right" if element_direction == "horizontal" else "right2left")
    text = "\n".join(w.contents for w in sorted(inside, key=lambda w: w.order))
    return text, element_direction, flags


def is_vertical(quad, thresh_aspect=2):
    q = np.array(quad)
    return np.linalg.norm(q[1] - q[2]) > np.linalg.norm(q[0] - q[1]) * thresh_aspect


def is_noise(quad, thresh=15):
    q = np.array(quad)
    return np.linalg.norm(q[0] - q[1]) < thresh or np.linalg.norm(q[1] - q[2]) < thresh


def recursive_update(original, new_data):
    for key, value in new_data.items():
        if isinstance(value, dict) and isinstance(original.get(key), dict):
            recursive_update(original[key], value)
        else:
            original[key] = value
    return original


# ---- split_text_across_cells (:283-423)
def _extract_words_within_table(words, table, check_list):
    horizontal, vertical = [], []
    for i, (points, score) in enumerate(zip(words.points, words.scores)):
        if is_contained(table.box, quad_to_xyxy(points), threshold=0.5):
            (vertical if is_vertical(points) else horizontal).append({"points": points, "score": score})
            check_list[i] = True
    return horizontal, vertical, check_list


def _calc_overlap_words_on_lines(lines, words):
    return [[calc_overlap_ratio(line.box, quad_to_xyxy(word["points"]))[0] for line in lines] for word in words]


def _clip_words_to_cells(overlaps, table, words, vertical):
    """Cut each word at the borders of the cells of its best-matching column (vertical text) or row."""
    new_points, new_scores = [], []
    for word, ratios in zip(words, overlaps):
        line = ratios.index(max(ratios)) + 1
        pts, score = word["points"], word["score"]
        for cell in table.cells:
            start, span = (cell.col, cell.col_span) if vertical else (cell.row, cell.row_span)
            if not (start <= line < start + span):
                continue
            _, inter = calc_overlap_ratio(cell.box, quad_to_xyxy(pts))
            if inter is None:
                continue
            x1, y1, x2, y2 = inter
            if vertical:
                cut = [[pts[0][0], max(pts[0][1], y1)], [pts[1][0], max(pts[1][1], y1)],
                       [pts[2][0], min(pts[2][1], y2)], [pts[3][0], min(pts[3][1], y2)]]
            else:
                cut = [[max(pts[0][0], x1), pts[0][1]], [min(pts[1][0], x2), pts[1][1]],
                       [min(pts[2][0], x2), pts[2][1]], [max(pts[3][0], x1), pts[3][1]]]
            if not is_noise(cut):
                new_points.append(cut)
                new_scores.append(score)
    return new_points, new_scores


def _correct_vertical_word_boxes(overlap_ratios_vertical, table, table_words_vertical):
    return _clip_words_to_cells(overlap_ratios_vertical, table, table_words_vertical, vertical=True)


def _correct_horizontal_word_boxes(overlap_ratios_horizontal, table, table_words_horizontal):
    return _clip_words_to_cells(overlap_ratios_horizontal, table, table_words_horizontal, vertical=False)


def _split_text_across_cells(results_det, results_layout):
    check_list = [False] * len(results_det.points)
    new_points, new_scores = [], []
    for table in results_layout.tables:
        horizontal, vertical, check_list = _extract_words_within_table(results_det, table, check_list)
        ph, sh = _correct_horizontal_word_boxes(_calc_overlap_words_on_lines(table.rows, horizontal), table, horizontal)
        pv, sv = _correct_vertical_word_boxes(_calc_overlap_words_on_lines(table.cols, vertical), table, vertical)
        new_points += ph + pv
        new_scores += sh + sv
    for i, used in enumerate(check_list):
        if not used:
            new_points.append(results_det.points[i])
            new_scores.append(results_det.scores[i])
    results_det.points = new_points
    results_det.scores = new_scores
    return results_det


# ---------------------------------------------------------------------------------------------- DocumentAnalyzer
class DocumentAnalyzer(StageAnalyzer):
    def __init__(self, configs={}, device="cuda", visualize=False, ignore_meta=False, reading_order="auto",
                 split_text_across_cells=False, ignore_ruby=False, ruby_threshold=2.0, workspace_reuse=False):
        # workspace_reuse: every network plans its workspace so that dead activations share bytes (include/ymk.h,
        # "workspace_reuse"; the same results from a fraction of the device memory); a module's own config entry wins
        common = {"device": device, "visualize": visualize, "workspace_reuse": workspace_reuse}
        default_configs = {
            "ocr": {"text_detector": dict(common), "text_recognizer": dict(common)},
            "layout_analyzer": {"layout_parser": dict(common), "table_structure_recognizer": dict(common)},
        }
        self.reading_order = reading_order
        if not isinstance(configs, dict):
            raise ValueError(_USAGE)
        recursive_update(default_configs, configs)
        self.text_detector = TextDetector(**default_configs["ocr"]["text_detector"])
        self.text_recognizer = TextRecognizer(**default_configs["ocr"]["text_recognizer"])
        self.layout = LayoutAnalyzer(configs=default_configs["layout_analyzer"])
        self.visualize = visualize
        self.ignore_meta = ignore_meta
        self.split_text_across_cells = split_text_across_cells
        self.ignore_ruby = ignore_ruby
        self.ruby_threshold = ruby_threshold
        # `handover`: an object with any of maps / boxes / layout_raw / table_boxes / layouts (yomitoku_amd.testing.Handover);
        # it exists so that a throughput measurement with seeded weights can feed realistic unit counts downstream without a
        # subclass that re-states the stage bodies (bench.py; tests/test_serving_gpu.py holds the hook to "identity in,
        # identical results out")
        self._init_chains()

    def _nets(self):
        return self.text_detector, self.text_recognizer, self.layout.layout_parser, self.layout.table_structure_recognizer

    # ---- aggregation (:487-601)
    def aggregate(self, ocr_res, layout_res, img=None):
        """`img` (the page, for its size): defaults to `self.img` as in the reference; the multi-page paths pass it so
        that no page's aggregation depends on shared state."""
        if img is None:
            img = self.img
        paragraphs = []
        cells = [cell for table in layout_res.tables for cell in table.cells]
        word_boxes = [quad_to_xyxy(word.points) for word in ocr_res.words]
        # word -> cell / paragraph membership for the whole page at once (same flags as the per-element form)
        member = containment_matrix([e.box for e in cells] + [p.box for p in layout_res.paragraphs], word_boxes, 0.5)
        used = np.zeros(len(ocr_res.words), dtype=bool)
        for cell, flags in zip(cells, member):
            words, _, _ = _words_of_element(ocr_res.words, word_boxes, flags, self.ignore_ruby, self.ruby_threshold)
            cell.contents = "" if words is None else words
            used |= flags
        for paragraph, flags in zip(layout_res.paragraphs, member[len(cells):]):
            words, direction, _ = _words_of_element(ocr_res.words, word_boxes, flags, self.ignore_ruby, self.ruby_threshold)
            if words is None:
                continue
            used |= flags
            paragraphs.append(ParagraphSchema(contents=words, box=paragraph.box, direction=direction, order=0,
                                              role=paragraph.role))
        for word, taken in zip(ocr_res.words, used):
            if not taken:
                paragraphs.append(ParagraphSchema(contents=word.content, box=quad_to_xyxy(word.points),
                                                  direction=word.direction, order=0, role=None))
        figures, in_figure = extract_paragraph_within_figure(paragraphs, layout_res.figures)
        paragraphs = [p for p, f in zip(paragraphs, in_figure) if not f]
        page_direction = judge_page_direction(paragraphs)
        headers = [p for p in paragraphs if p.role == "page_header" and not self.ignore_meta]
        footers = [p for p in paragraphs if p.role == "page_footer" and not self.ignore_meta]
        page_contents = [p for p in paragraphs if p.role is None or p.role == "section_headings"]
        elements = page_contents + layout_res.tables + figures
        prediction_reading_order(headers, "left2right")
        prediction_reading_order(footers, "left2right")
        if self.reading_order == "auto":
            order = "right2left" if page_direction == "vertical" else "top2bottom"
        else:
            order = self.reading_order
        prediction_reading_order(elements, order, img)
        for element in elements:
            element.order += len(headers)
        for footer in footers:
            footer.order += len(elements) + len(headers)
        return {
            "paragraphs": sorted(headers + page_contents + footers, key=lambda p: p.order),
            "tables": sorted(layout_res.tables, key=lambda t: t.order),
            "figures": sorted(figures, key=lambda f: f.order),
            "words": ocr_res.words,
        }

    def _vis_det(self, page, results_det):
        """document_analyzer.py:613-617: the analyzer's own detection overlay (default colour, no heat map) - the canvas the
        recogniser draws its strings onto.  Stays on the device."""
        if not self.visualize:
            return None
        from .utils.visualizer import det_visualizer

        return det_visualizer(page, results_det.points, to_host=False)

    def _detect_and_recognize(self, page):
        results_det, _ = self.text_detector.detect(page)
        results_rec, ocr = self.text_recognizer._call(page, results_det.points, self._vis_det(page, results_det), to_host=False)
        return results_det, results_rec, ocr

    def run(self, page):
        """(results, ocr overlay, layout overlay); with visualize=True the overlays are device canvases (`__call__` brings them
        to the host)."""
        if self.split_text_across_cells:
            f_det = self._submit("ocr", self.text_detector.detect, page)
            f_lay = self._submit("layout", self.layout._call, page, False)
            results_det, _ = f_det.result()
            results_layout, layout = f_lay.result()
            results_det = _split_text_across_cells(results_det, results_layout)
            results_rec, ocr = self.text_recognizer._call(page, results_det.points, self._vis_det(page, results_det), to_host=False)
        else:
            f_ocr = self._submit("ocr", self._detect_and_recognize, page)
            f_lay = self._submit("layout", self.layout._call, page, False)
            results_det, results_rec, ocr = f_ocr.result()
            results_layout, layout = f_lay.result()
        results_ocr = OCRSchema(words=ocr_aggregate(results_det, results_rec))
        outputs = self.aggregate(results_ocr, results_layout)
        return DocumentAnalyzerSchema(**outputs), ocr, layout

    # ---- several pages per call: device batches across pages (the per-page path above leaves an MI355X mostly idle:
    # batch-1 RT-DETR / PARSeq launches are grid-starved and every page pays its own greedy-decode loop).  The stages of
    # a wave (yomitoku_amd.serving.Wave) are separate methods: `analyze_pages` runs them as two concurrent chains,
    # `serve` as a pipeline with one thread and HIP stream per stage.
    def _stage_split(self, wave):
        wave.dets = [_split_text_across_cells(d, l) for d, l in zip(wave.dets, wave.lays)]

    def _stage_layout(self, wave):
        """One RT-DETRv2 layout forward over the pages (device half)."""
        wave.lay_raw = self._handed("layout_raw", wave, self.layout.layout_parser.forward_pages(wave.pages))

    def _stage_tables(self, wave):
        """Layout boxes on the host, then one table-structure forward over all table crops of the wave."""
        wave.lay_parsed = self.layout.layout_parser.pages_from_raw(wave.lay_raw)
        wave.lay_raw = None
        boxes = self._handed("table_boxes", wave, [[t.box for t in l.tables] for l in wave.lay_parsed])
        wave.tab_raw = self.layout.table_structure_recognizer.forward_tables(wave.pages, boxes)

    def _stage_cells(self, wave):
        """Row / column / span filters and the cell grids on the host."""
        tables = self.layout.table_structure_recognizer.tables_from_raw(wave.tab_raw, len(wave.pages))
        wave.tab_raw = None
        lays = [LayoutAnalyzerSchema(paragraphs=l.paragraphs, tables=t, figures=l.figures) for l, t in zip(wave.lay_parsed, tables)]
        wave.lays = self._handed("layouts", wave, lays)

    def _stage_finish(self, wave, k):
        """Aggregation of page k of the wave -> DocumentAnalyzerSchema."""
        results_ocr = OCRSchema(words=ocr_aggregate(wave.dets[k], wave.recs[k]))
        return DocumentAnalyzerSchema(**self.aggregate(results_ocr, wave.lays[k], img=wave.imgs[k]))

    def _page_drawings(self, wave, k, results):
        """The two drawings of page k of a finished wave, recorded for the wave renderer: what `_with_overlays` draws with
        every visualize flag on - the detection quads and the recognised strings; the layout boxes, the table cells and the
        reading order."""
        from .utils import visualizer as V

        ocr, layout = self._ocr_drawing(wave, k), V.RunOverlay()
        V._layout_commands(layout, wave.lay_parsed[k])
        for table in wave.lays[k].tables:
            V._table_commands(layout, table)
        V._page_order_commands(layout, results)
        return ocr, layout

    def analyze_pages(self, imgs, wave: int = 8):
        """`__call__` over a list of pages, `wave` pages at a time on the device.  Every page's result is what
        `__call__(img)` returns for it (pages never interact: batches are per-image independent, recogniser
        mini-batches are formed per page); what changes is how the launches are shared.  The two chains of a wave
        run concurrently on their own HIP streams, as in `run`.  Returns [(DocumentAnalyzerSchema, ocr_vis, layout_vis), ...]
        (the two images of `__call__` with visualize=True, else None).
        One wave at a time: `serve` is the throughput path (several waves in flight, failures isolated per page)."""
        out = []
        size = max(1, int(wave))
        for start in range(0, len(imgs), size):
            w = self._run_wave(imgs[start : start + size], start)
            out.extend(self._with_overlays(w, k, self._stage_finish(w, k)) for k in range(len(w)))
        return out

    def _with_overlays(self, wave, k, results):
        """(results, ocr overlay, layout overlay) of page k of a finished wave: the images `__call__` returns for the page -
        each module that was built with visualize=True draws what its own `__call__` draws, from the wave's per-page results.
        (results, None, None) when nothing visualises."""
        lp, ts = self.layout.layout_parser, self.layout.table_structure_recognizer
        page = wave.pages[k]
        ocr = self._vis_det(page, wave.dets[k])
        if self.text_recognizer.visualize:
            ocr = self.text_recognizer._visualize(page, wave.recs[k], ocr, to_host=False)
        layout = None
        if lp.visualize:
            from .utils.visualizer import layout_visualizer

            layout = layout_visualizer(wave.lay_parsed[k], page, to_host=False)
        if ts.visualize:
            layout = ts._visualize(page, wave.lays[k].tables, layout, to_host=False)
        if self.visualize:
            layout = self._vis_reading_order(page, layout, results)
        return results, _vis_to_host(ocr), _vis_to_host(layout)

    def _vis_reading_order(self, page, layout, results):
        """document_analyzer.py:675-676: order numbers and arrows on the layout overlay (on a copy of the page when the layout
        modules drew none)."""
        from .utils.visualizer import reading_order_visualizer

        return reading_order_visualizer(page if layout is None else layout, results, to_host=False)

    def serve(self, sources, wave: int = 16, in_flight: int = 4, defer_full_gc: bool = True, with_source: bool = False, rec_lanes: int = 2,
              overlays: bool = False, jpeg=None, jpeg_optimize: bool = False, jpeg_subsampling=None, jpeg_grey=False,
              jpeg_bilevel=False, deskew=False, jpeg_mrc=False, jpeg_despeckle=False, figures=None, jpeg_lossless=False):
        """The multi-page entry point: host pages (uint8 H x W x 3 BGR arrays) and / or image file paths in, one result
        per page out, in page order - the page loop of cli/main.py:105-137 as a stage pipeline on one GPU from one
        process (yomitoku_amd/serving.py): pinned staging + H2D on a copy stream, `wave` pages per device batch (16 measured best
        at 1600 x 1200: one greedy loop and forwards of equal size per wave; 8: 5 % less, 32: 3 % less), up to `in_flight` waves
        between upload and aggregation.  A page's entry is its DocumentAnalyzerSchema - equal to
        `__call__(img)[0]` - or, when the page (or its file) failed, the exception object; the other pages are not
        affected (cli/main.py:555-564).  `defer_full_gc`: postpone CPython's generation-2 garbage collections until
        the job is done (a full pass holds the GIL for 100+ ms with a few hundred results alive and stalls every stage).
        `with_source`: (source index, frame index, entry) triples, for callers that write one output per file page.
        `rec_lanes`: recogniser forwards in flight (2: a second PARSeq handle with the same weights; serving.py).
        `overlays`: a property of the job, not of the analyzer - True: a page's entry is (schema, ocr overlay, layout overlay),
        the two images `analyze_pages` returns for the page when everything was built with visualize=True (detection quads and
        recognised strings; layout boxes, table cells, reading order; no heat map), as uint8 H x W x 3 arrays the caller owns.
        They are drawn on the device by a render stage of the pipeline - text layout, per-tile culling and all canvases of a
        wave in two launches ("Overlay rasteriser") - that only the waves of such a job visit.
        `jpeg`: a property of the job too - None, or a preset of the searchable PDF ("high", "middle", "low"; anything else is
        a ValueError before a source is read): a page's entry ends with its EncodedJpeg (yomitoku_amd/jpeg.py), i.e. (schema,
        EncodedJpeg) or (schema, ocr overlay, layout overlay, EncodedJpeg) - the file `searchable_pdf_bytes` embeds as it is,
        encoded on the device in the same render stage from the clean page ("JPEG encoder").
        `jpeg_optimize`: with `jpeg`, the files are coded with Huffman tables made for each page instead of Annex K's typical
        ones (libjpeg's `optimize`): two more launches per wave, the same decoded pixels, about a third fewer bytes on scanned
        pages; the EncodedJpeg says `optimized=True`.  Without `jpeg` it is a ValueError before a source is read.
        `jpeg_subsampling`: None (4:2:0), "4:2:0", "4:2:2" or "4:4:4" - how much of the chroma the colour files keep: "4:4:4"
        keeps all of it (red seals, coloured ruling and small coloured print stay sharp; about a third more bytes on a scanned
        page), "4:2:2" its full height.  `jpeg_grey`: False, or "auto" - every page is tested on the device after the preset's
        resize, and one whose pixels all have B == G == R (a black-and-white scan loaded as B G R) is written as a grey file, a
        third of the blocks; its EncodedJpeg says `grey=True`, `subsampling=None`.  Any other value, and either option without
        `jpeg`, is a ValueError before a source is read.
        `jpeg_bilevel`: False, or "auto" - every page is tested on the device as it arrived, before the preset's resize, and a
        two-valued one (every sample 0 or 255 and B == G == R: what a 1-bit scan loads as) is written as a CCITT Group 4 file
        instead: its entry ends with an EncodedBilevel (yomitoku_amd/ccitt.py; `scale` 1.0, the full-size page, lossless) that
        `searchable_pdf_bytes` embeds as a /CCITTFaxDecode image.  Such a page ignores the preset's resize and the three options
        above; every other page goes the way it goes without the switch.  The same refusals.
        `jpeg_bilevel`: "otsu" or "adaptive" - every GREY-VALUED page (one channel, or B == G == R everywhere: a flatbed or phone
        scan of a black-and-white document, with paper noise, soft edges, a gradient of light - and a grey photograph too: the
        switch is a decision about the job, not a guess about a page) is thresholded on the device and written as a Group 4 file
        the same way; its EncodedBilevel says `method` and, for "otsu", `threshold`.  "otsu" takes one threshold per page from its
        histogram; "adaptive" calls a pixel black where it is 15 % below the mean of its window of max(h, w) // 16 pixels each
        way, which follows uneven light (tests/binarize_ref.py is the definition of both).  OCR and layout see the page as it
        arrived; only the file changes.  A colour page goes the way it goes without the switch; a two-valued page gives the file
        of "auto".
        `deskew`: False, True, or a dict with any of `max_angle` (5.0), `step` (0.1), `min_angle` (0.3), in degrees; anything
        else is a ValueError before a source is read.  Every page's skew is estimated and undone on the device behind its upload
        (yomitoku_amd/deskew.py; DESIGN.md, "Page skew"), so every network, the overlays and the page files see the corrected
        page, and a page's entry ends with its PageSkew: (schema, PageSkew), (schema, EncodedJpeg, PageSkew) and so on.  All
        coordinates of the schema are the corrected page's; `PageSkew.to_original` maps them back.
        `jpeg_mrc`: False, True, or a dict with any of `bg_cell` (2) and `fg_cell` (8), each one of 1, 2, 4, 8, 16; anything else, and
        the switch without `jpeg`, is a ValueError before a source is read.  Of the pages `jpeg_bilevel` leaves - colour or grey, a
        form with a stamp, tinted paper - every page with ink and with paper is written as a layered page (yomitoku_amd/mrc.py;
        DESIGN.md, "Layered pages"): its entry ends with an EncodedMrc - the ink mask as a lossless Group 4 file of the full-size
        page, the paper as a JPEG of one pixel per `bg_cell` x `bg_cell` pixels, the ink's colour as one per `fg_cell` x `fg_cell` -
        which `searchable_pdf_bytes` embeds as three images, the foreground painted through the mask.  Such a page is never
        resized (`scale` 1.0); `jpeg_optimize` and `jpeg_subsampling` apply to its two layer files, `jpeg_grey` does not.  A blank
        page, or one that is all ink, keeps its plain file.  OCR and layout see the page as it arrived; only the file changes.
        The dict may also hold `despeckle` (what `jpeg_despeckle` takes) and `blobs` (False, True, or a dict with `side` (128),
        2..16383, and / or `fill` (64), 1..256), both False by default: the ink filtered before it is used - specks and pinholes
        removed, and every ink component at least `side` pixels high and wide that fills `fill` / 256 of its bounding box, the dark
        part of a picture, left to the background layer (yomitoku_amd/despeckle.py: check_blobs; DESIGN.md, "Layered pages: the
        ink filtered ...").  The page's `EncodedMrc.mask.despeckled` then says what went.
        `jpeg_despeckle`: False, True (4 and 4), an int n, or a dict with `black` and / or `white` (a missing one is 0), each
        0..65535 and not both 0; anything else, the switch without `jpeg`, and the switch with `jpeg_bilevel=False` (there is no
        Group 4 file to clean) is a ValueError before a source is read.  Every page that gets a Group 4 file of its own has its
        8-connected black components of fewer than `black` pixels cleared, then its 4-connected white components of fewer than
        `white` pixels filled, on the device before it is coded (yomitoku_amd/despeckle.py; DESIGN.md, "Despeckled pages"):
        paper grain and dust cost T.6 most of a noisy page's bytes.  `EncodedBilevel.despeckled` says what went.  With
        `jpeg_bilevel="auto"` the file is then no longer lossless.  OCR and layout see the page as it arrived.
        `figures`: None / False, True, an int 1..100 (the JPEG quality), or a dict with any of `quality` (95), `subsampling`
        ("4:2:0"), `optimize` (False) and `max_side` (None, or 16..16383: a crop whose long side exceeds it is shrunk to it);
        anything else is a ValueError before a source is read.  The crops of the page's `schema.figures` - the only pixels the
        Markdown / HTML / JSON / CSV exporters write - are cut on the device from the clean page (with `deskew` the corrected
        one, whose boxes the schema holds; full size whatever the `jpeg` preset) and coded as JPEG files in the render stage
        (yomitoku_amd/figures.py; DESIGN.md, "Figure crops"): the entry gets a PageFigures behind the page file and in front of
        the PageSkew - (schema, PageFigures), (schema, ocr overlay, layout overlay, EncodedJpeg, PageFigures, PageSkew) -, one
        EncodedJpeg per figure in `schema.figures` order (None for an empty box), which `schema.to_markdown(path,
        figures=entry[...])` and the other exporters write in place of crops of a host image.
        `jpeg_lossless`: False, True, or {"budget": b} with b a positive finite number of bytes a pixel; anything else, an unknown
        key, and the switch without `jpeg`, is a ValueError before a source is read.  Every page `jpeg_bilevel` and `jpeg_mrc`
        leave - one channel or three: a rasterised PDF, a screenshot, a slide, a form, a page with drawn graphics - is written as a
        lossless file instead of a JPEG (yomitoku_amd/flate.py; DESIGN.md, "Lossless pages"): its entry ends with an
        EncodedLossless - `data`, a zlib stream of the page's PNG-filtered rows made on the device, `width`, `height`, `channels`,
        `scale` 1.0, `nbytes`, `to_png()` - which `searchable_pdf_bytes` embeds as a /FlateDecode image with /Predictor 15.  Such a
        page is never resized; `jpeg_optimize` and `jpeg_subsampling` do not apply to it, `jpeg_grey="auto"` does (`channels` 1 for
        a three-channel page that is grey); with `deskew` the file is of the corrected page.  With a budget a page goes lossless
        only where its file takes at most b bytes a pixel (in integers: nbytes * 256 <= ceil(256 b) * height * width) and gets
        exactly the JPEG of the job without the switch otherwise - a grainy scan is several times larger lossless.  OCR and layout
        see the page as it arrived; only the file changes."""
        files = check_jpeg_preset(jpeg, jpeg_optimize, jpeg_subsampling, jpeg_grey, jpeg_bilevel, jpeg_mrc, jpeg_despeckle, jpeg_lossless)  # before the pipeline is built or a source read
        deskew = check_deskew(deskew) or False
        figures = check_figures(figures)
        if self.visualize:
            raise NotImplementedError(_NO_VIS_SERVE)
        return self._serve(sources, wave, in_flight, defer_full_gc, with_source, rec_lanes, overlays, files=files, deskew=deskew, figures=figures)

    def __call__(self, img):
        self.img = img
        dev = self.text_detector.device
        page = img if isinstance(img, torch.Tensor) else imaging.page_to_device(img, dev)
        results, ocr, layout = self.run(page)
        if self.visualize:
            layout = self._vis_reading_order(page, layout, results)
        return results, _vis_to_host(ocr), _vis_to_host(layout)
