"""TableSemanticParser (reference table_semantic_parser.py:40-991): a form or a table read as grids (rows x columns with
column headers) and key-value items - the consumer of CellDetector's cells, `kv_regions` and `grid_regions`.

    parser = TableSemanticParser(configs={...}, device="cuda")
    results, _, _ = parser(img_bgr_uint8)          # TableSemanticParserSchema
    results.to_dict() / .to_structured() / .to_simple() / .to_csv(outdir)
    results, vis_layout, vis_ocr = parser(img_bgr_uint8, overlays=True)   # + the reference's two pictures, uint8 H x W x 3

Same constructor keys (`table_detector`, `table_cell_parser`, `text_detector`, `text_recognizer`), same `__call__`
arguments and the same result for the same model outputs.  What differs from the reference:

  * the pictures are a property of the CALL, as in `DocumentAnalyzer.serve(overlays=True)`: `parser(img, overlays=True)` and
    `parse_pages(imgs, overlays=True)` return the reference's layout picture (tables and paragraphs boxed and labelled, cells
    tinted by role, key -> value arrows, grid boxes, grid graphs) and its OCR picture, drawn on the device from the page that was
    uploaded for the networks (utils/visualizer.py; the page itself is never drawn on).  The constructor's `visualize` defaults
    to False (the reference: True) and True still raises NotImplementedError;
  * the page is uploaded once and the device page is shared by the four modules; the text chain (DBNet -> PARSeq) and the table
    chain (RT-DETRv2 table detector -> RT-DETRv2 cell detector) run side by side on two HIP streams, like the two chains of
    DocumentAnalyzer (the reference runs the two detectors side by side and the rest in sequence; the results are the same);
  * `parse_pages(imgs)`: several pages through shared forwards, one wave at a time;
  * `serve(sources)`: the throughput path - the parser as the analyzer of the page pipeline (serving.py): several waves in
    flight, the host stages on threads of their own, a failing page isolated; `template`, `grid_only`, `kv_only` and `overlays`
    per job.  `distributed.ShardedServer` / `serve_sharded` take a `make_analyzer` that returns a parser;
  * `aggregate` assigns words to cells from one words x cells overlap matrix instead of a double loop (same assignment).

Everything after the four networks is host logic on at most a few hundred boxes per table (`semantic_stage`): no kernel.
Not restated: the helpers of the reference's module that nothing on its call path uses
(`_weakly_cluster_nodes_with_graph`, `is_grid_cluster`, `_get_cluster_nodes`, `drop_single_out_edge_by_type`, `replace_edge_type`).
"""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import imaging
from .document_analyzer import _USAGE, ocr_aggregate
from .geometry import is_contained, quad_to_xyxy
from .grid_parser import parse_grid_from_bottom_up
from .kv_parser import parse_kv_items
from .layout_parser import LayoutParser
from .reading_order import prediction_reading_order
from .schemas import Element, OCRSchema, ParagraphSchema
from .serving import StageAnalyzer
from .table_cell_detector import CellDetector
from .table_semantic_schemas import TableSemanticContentsSchema, TableSemanticParserSchema
from .text_detector import TextDetector
from .text_recognizer import TextRecognizer

_NO_VIS = ("the constructor's visualize flag is not supported (visualize=False only): ask for the pictures per call, "
           "parser(img, overlays=True) / parse_pages(imgs, overlays=True)")
_VALUE_ROLES = ("cell", "header", "empty")


def _split_nodes_with_role(cells):
    """{"header": [...], "cell": [...], "empty": [...]} (+ any further role met), each in the order given."""
    nodes = {"header": [], "cell": [], "empty": []}
    for cell in cells:
        nodes.setdefault(cell.role, []).append(cell)
    return nodes


def get_cell_by_id(cells, cell_id):
    return next((cell for cell in cells if cell.id == cell_id), None)


def _region_cell_ids(region, cells, threshold=0.5):
    """Ids of the cells more than `threshold` inside the region."""
    return {cell.id for cell in cells if is_contained(region.box, cell.box, threshold=threshold)}


def _resolve_overlapping_regions(grid_regions, kv_regions, value_cells, conflict_ratio_th=0.5):
    """The model may predict a grid twice, or a kv region and a grid over the same cells.  Two regions conflict when the cells
    they share are at least `conflict_ratio_th` of the cells of the one holding fewer.  Among conflicting grids the higher
    score stays; between a grid and a kv region the one holding more cells stays, the grid among equals.
    Returns (grids kept, kv regions kept), each in the order given."""
    grid_cells = [_region_cell_ids(g, value_cells) for g in grid_regions]
    kv_cells = [_region_cell_ids(k, value_cells) for k in kv_regions]

    def conflict(a, b):
        fewer = min(len(a), len(b))
        return bool(fewer) and len(a & b) / fewer >= conflict_ratio_th

    kept, drop_grid, drop_kv = [], set(), set()
    for gi in sorted(range(len(grid_regions)), key=lambda i: getattr(grid_regions[i], "score", 1.0), reverse=True):
        if any(conflict(grid_cells[gi], grid_cells[gj]) for gj in kept):
            drop_grid.add(gi)
        else:
            kept.append(gi)
    for gi in range(len(grid_regions)):
        for ki in range(len(kv_regions)):
            if gi in drop_grid or ki in drop_kv:
                continue
            if grid_cells[gi] & kv_cells[ki] and conflict(grid_cells[gi], kv_cells[ki]):
                if len(grid_cells[gi]) >= len(kv_cells[ki]):
                    drop_kv.add(ki)
                else:
                    drop_grid.add(gi)
    return ([g for i, g in enumerate(grid_regions) if i not in drop_grid], [k for i, k in enumerate(kv_regions) if i not in drop_kv])


def _gap_valley_tol(coords, min_tol=8.0):
    """The gap above which two sorted coordinates belong to different rows, from the coordinates themselves: offsets inside a
    row are a few px, the row pitch tens of px, so the sorted gaps (with `min_tol` put in front as the reference gap, which lets
    a single gap be judged too) jump once - the threshold is the middle of the largest RATIO jump (the last one among equals),
    as far from both populations as can be.  `min_tol` when no gap exceeds it."""
    coords = sorted(coords)
    gaps = sorted(b - a for a, b in zip(coords, coords[1:]))
    if not gaps or gaps[-1] <= min_tol:
        return min_tol
    gaps = [min_tol] + gaps
    best, best_ratio = 0, 0.0
    for i in range(len(gaps) - 1):
        ratio = (gaps[i + 1] + 1) / (gaps[i] + 1)
        if ratio >= best_ratio:
            best, best_ratio = i, ratio
    return (gaps[best] + gaps[best + 1]) / 2


def _cluster_centers(coords, tol):
    """Means of the runs of the sorted coordinates, a run ending where the next coordinate is more than `tol` away."""
    coords = sorted(coords)
    runs = [[coords[0]]]
    for v in coords[1:]:
        if v - runs[-1][-1] > tol:
            runs.append([v])
        else:
            runs[-1].append(v)
    return [sum(run) / len(run) for run in runs]


def _nearest_index(value, centers):
    return min(range(len(centers)), key=lambda i: abs(centers[i] - value))


def sort_cells(cells):
    """Cells in reading order with position ids: value cells `r<row>c<col>`, group cells `grp<k>`.  Returns (cells, {old id:
    new id}); the cells' ids are rewritten in place.

    The row is the cluster of the cell's top edge among the table's value cells (so cells outside any grid get one too); the
    column is the cell's ordinal from the left INSIDE its row - not a cluster of x over the table, which has no valleys in dense
    forms whose rows are divided differently.  Unlike running numbers such ids do not move when a cell is missed or added
    elsewhere, and they survive jitter and a shifted scan."""
    cells = list(cells)
    if len(cells) == 0:
        return cells, {}
    min_height = min(cell.box[3] - cell.box[1] for cell in cells)
    values = sorted((c for c in cells if c.role in _VALUE_ROLES), key=lambda c: (c.box[1] // min_height, c.box[0]))
    groups = sorted((c for c in cells if c.role == "group"), key=lambda c: (c.box[1], c.box[0]))
    remap = {}

    def rename(cell, new_id):
        remap[cell.id] = new_id
        cell.id = new_id

    if values:
        tops = [c.box[1] for c in values]
        centers = _cluster_centers(tops, _gap_valley_tol(tops))
        rows = {}
        for cell in values:
            rows.setdefault(_nearest_index(cell.box[1], centers), []).append(cell)
        for row, members in rows.items():
            members.sort(key=lambda c: c.box[0])
            for col, cell in enumerate(members):
                rename(cell, f"r{row}c{col}")
    for k, cell in enumerate(groups):
        rename(cell, f"grp{k}")
    return values + groups, remap


def _sort_elements(elements, prefix="t"):
    """Top to bottom in bands of the smallest element height, left to right inside a band; ids `<prefix><k>`."""
    if len(elements) == 0:
        return elements
    min_height = min(e.box[3] - e.box[1] for e in elements)
    elements = sorted(elements, key=lambda e: (e.box[1] // min_height, e.box[0]))
    for k, element in enumerate(elements):
        element.id = f"{prefix}{k}"
    return elements


def _assign_ids(table_information):
    """Grids g<k>, kv items kv<k>, cells by position (sort_cells) - and every reference to a cell follows."""
    for k, grid in enumerate(table_information["grids"]):
        grid.id = f"g{k}"
    for k, kv in enumerate(table_information["kv_items"]):
        kv.id = f"kv{k}"
    cells, remap = sort_cells(table_information["cells"].values())
    table_information["cells"] = {cell.id: cell for cell in cells}

    def moved(ids):
        return [remap[i] if i is not None else None for i in ids]

    for kv in table_information["kv_items"]:
        kv.key = moved(kv.key)
        kv.value = remap[kv.value]
    for grid in table_information["grids"]:
        data, headers = [moved(row) for row in grid.data], [moved(col) for col in grid.col_headers]
        grid.data, grid.col_headers = data, headers


def overlap_ratio_matrix(boxes_a, boxes_b):
    """[len(a)][len(b)] float64: calc_overlap_ratio(a_i, b_j)[0] - the share of b_j that a_i covers - for every pair at once,
    with the scalar form's integer truncation and the same float64 quotient."""
    if len(boxes_a) == 0 or len(boxes_b) == 0:
        return np.zeros((len(boxes_a), len(boxes_b)), dtype=np.float64)
    raw_b = np.asarray(boxes_b, dtype=np.float64).reshape(-1, 4)
    a = np.trunc(np.asarray(boxes_a, dtype=np.float64).reshape(-1, 4)).astype(np.int64)
    b = np.trunc(raw_b).astype(np.int64)
    w = np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])
    h = np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])
    hit = (w > 0) & (h > 0)
    area_b = (raw_b[:, 2] - raw_b[:, 0]) * (raw_b[:, 3] - raw_b[:, 1])
    if np.any(hit & (area_b[None, :] == 0)):
        raise ZeroDivisionError("division by zero")  # what the scalar form does for a degenerate box
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (w * h) / area_b[None, :]
    return np.where(hit, ratio, 0.0)


def _owned_host_image(canvas):
    """A device canvas as an array the caller owns: one D2H copy into a freshly allocated array."""
    out = np.empty(tuple(canvas.shape), dtype=np.uint8)
    torch.from_numpy(out).copy_(canvas)
    return out


class TableSemanticParser(StageAnalyzer):
    merge_same_column_values = False  # True: grid columns under the same innermost header cell become one column
    visualize = False

    def __init__(self, configs={}, device="cuda", visualize=False, workspace_reuse=False):
        if not isinstance(configs, dict):
            raise ValueError(_USAGE)
        if visualize:
            raise NotImplementedError(_NO_VIS)
        common = {"device": device, "visualize": visualize, "workspace_reuse": workspace_reuse}
        kwargs = {name: {**common, **configs.get(name, {})} for name in ("table_detector", "table_cell_parser", "text_detector", "text_recognizer")}
        self.layout_parser = LayoutParser(**kwargs["table_detector"])
        self.cell_detector = CellDetector(**kwargs["table_cell_parser"])
        self.text_detector = TextDetector(**kwargs["text_detector"])
        self.text_recognizer = TextRecognizer(**kwargs["text_recognizer"])
        self.visualize = visualize
        self.merge_same_column_values = False
        # `handover`: None, or an object whose `tables(page index, [Element])` sees - and may replace - the table boxes that the
        # table detector hands to the cell detector (measurements and tests with seeded weights, whose detections are noise)
        self._init_chains()

    def _nets(self):
        return self.text_detector, self.text_recognizer, self.layout_parser, self.cell_detector

    # ---- words into cells
    def aggregate(self, ocr_res, cells, overlap_th=0.2):
        """Every word goes to the ONE non-group cell that covers most of it (the first among equals), if that is at least
        `overlap_th` of the word; a cell's contents are its words in reading order (right to left when its vertical words
        outnumber the horizontal ones), joined without separator.  Cells without words get ""."""
        cells = list(cells)
        words = ocr_res.words
        word_boxes = [quad_to_xyxy(word.points) for word in words]
        ratio = overlap_ratio_matrix([c.box for c in cells], word_boxes).T  # words x cells
        if ratio.size:
            ratio[:, [c.role == "group" for c in cells]] = 0.0
            best = ratio.argmax(axis=1)
            best_ratio = ratio[np.arange(len(words)), best]
            taken = (best_ratio > 0) & ~(best_ratio < overlap_th)
        else:
            best, taken = np.zeros(len(words), dtype=np.int64), np.zeros(len(words), dtype=bool)
        words_of = [[] for _ in cells]
        for i in np.flatnonzero(taken).tolist():
            words_of[best[i]].append(ParagraphSchema(box=word_boxes[i], contents=words[i].content, direction=words[i].direction,
                                                     order=0, role=None))
        for cell, contained in zip(cells, words_of):
            if not contained:
                cell.contents = ""
                continue
            dirs = [w.direction for w in contained]
            horizontal = dirs.count("horizontal") >= dirs.count("vertical")
            prediction_reading_order(contained, "left2right" if horizontal else "right2left")
            text = "\n".join(w.contents for w in sorted(contained, key=lambda w: w.order))
            cell.contents = text.replace("\n", "").strip()

    def replace_table_to_paragraphs(self, tables, paragraphs):
        """A "table" with fewer than two cell / header cells is a paragraph: it is appended to `paragraphs` (in place).
        Returns the tables that stay."""
        kept = []
        for table in tables:
            if sum(cell.role in ("cell", "header") for cell in table.cells) < 2:
                paragraphs.append(Element(id=None, box=table.box, contents="", score=1.0, role=None))
            else:
                kept.append(table)
        return kept

    # ---- the four networks
    def _handed_tables(self, k, tables):
        fn = getattr(self.handover, "tables", None) if self.handover is not None else None
        return tables if fn is None else fn(k, tables)

    def _detect_and_recognize(self, page):
        results_det, _ = self.text_detector(page)
        results_rec, _ = self.text_recognizer(page, results_det.points)
        return results_det, results_rec

    def _tables_and_cells(self, page):
        results_layout, _ = self.layout_parser(page)
        return results_layout, self.cell_detector(page, self._handed_tables(0, list(results_layout.tables)))

    def run_models(self, img):
        """(OCRSchema, [TableDetectorSchema], [Element] paragraphs) of a page: one upload, two chains side by side."""
        dev = self.text_detector.device
        page = img if isinstance(img, torch.Tensor) else imaging.page_to_device(img, dev)
        f_ocr = self._submit("ocr", self._detect_and_recognize, page)
        f_tab = self._submit("layout", self._tables_and_cells, page)
        results_det, results_rec = f_ocr.result()
        results_layout, results_table = f_tab.result()
        return self._hand_over(results_det, results_rec, results_layout, results_table)

    def _hand_over(self, results_det, results_rec, results_layout, results_table):
        paragraphs = results_layout.paragraphs
        results_table = self.replace_table_to_paragraphs(results_table, paragraphs)
        return OCRSchema(words=ocr_aggregate(results_det, results_rec)), results_table, paragraphs

    # ---- everything after the networks
    def _parse_table(self, table, cells, grid_only, kv_only, dags=None):
        """(grids, kv items, {id: cell} the items refer to) of one detected table; `cells`: its cells by id.  `dags`: a list
        that every parsed grid's graph is appended to."""
        value_cells = [c for c in table.cells if c.role in _VALUE_ROLES]
        grid_regions = [] if kv_only else list(table.grid_regions)
        kv_regions = [] if grid_only else list(table.kv_regions)
        grid_regions, kv_regions = _resolve_overlapping_regions(grid_regions, kv_regions, value_cells)
        grids, kv_items, used = [], [], {}
        claimed = set()
        for region in grid_regions:  # rows and columns inside every grid region
            region_cells = [c for c in value_cells if is_contained(region.box, c.box, threshold=0.5)]
            if len(region_cells) == 0:
                continue
            result = parse_grid_from_bottom_up(cells, _split_nodes_with_role(region_cells), self.merge_same_column_values)
            if result is None:
                continue
            grids.append(result[0])
            used.update(result[1])
            if dags is not None:
                dags.append(result[2])
            claimed.update(c.id for c in region_cells)
        remaining = [c for c in value_cells if c.id not in claimed]  # what no grid claimed is read as key-value items
        if remaining:
            for k, region in enumerate(kv_regions):
                region.id = f"kvr{k}"
            items, _, kv_cells = parse_kv_items(_split_nodes_with_role(remaining), cells, kv_regions)
            kv_items.extend(items)
            used.update(kv_cells)
        return grids, kv_items, used

    def semantic_stage(self, results_ocr, results_table, paragraphs, template=None, grid_only=False, kv_only=False, dags=None):
        """`run_models`' results -> TableSemanticParserSchema: words into cells and paragraphs, grids and kv items per table
        (or, with `template`, the template's), ids by position.  `dags`: a list that the graph of every parsed grid is appended
        to, in table order (what dag_visualizer draws; the kv graph is not handed out, as in the reference)."""
        for table in results_table:
            self.aggregate(results_ocr, table.cells)
        self.aggregate(results_ocr, paragraphs)
        tables = []
        for k, table in enumerate(results_table):
            cells = {cell.id: cell for cell in table.cells}
            info = {"id": f"t{k}", "box": table.box, "cells": {}, "style": "border", "kv_items": [], "grids": []}
            if template is None:
                info["grids"], info["kv_items"], used = self._parse_table(table, cells, grid_only, kv_only, dags)
                info["cells"].update(used)
            for cell in cells.values():
                info["cells"].setdefault(cell.id, cell)
            info["kv_items"] = sorted(info["kv_items"], key=lambda kv: info["cells"][kv.value].box[1])
            info["grids"] = sorted(info["grids"], key=lambda g: g.box[1])
            _assign_ids(info)
            tables.append(TableSemanticContentsSchema(**info))
        results = TableSemanticParserSchema(tables=_sort_elements(tables, prefix="t"), paragraphs=_sort_elements(paragraphs, prefix="p"),
                                            words=results_ocr.words)
        if template is not None:
            results.load_template_json(template)
        return results

    # ---- overlays=True: the reference's two pictures, per call
    def _drawings(self, results, dags, recorder):
        """(layout drawing, ocr drawing) of one page's results, recorded on two `recorder()`s."""
        from .utils import visualizer as V

        layout, ocr = recorder(), recorder()
        V._semantic_layout_commands(layout, results, dags)
        cfg = self.text_recognizer._cfg.visualize
        V._semantic_ocr_commands(ocr, results, V.load_font(cfg.font, cfg.font_size), cfg.font_size, tuple(cfg.color[::-1]))
        return layout, ocr

    def __call__(self, img, template=None, id=None, grid_only=False, kv_only=False, overlays=False):
        """`img`: uint8 H x W x 3 BGR page.  `template`: path of a template JSON (save_template_json) whose kv items and grids
        replace the parsed ones; `grid_only` / `kv_only`: ignore the predicted kv / grid regions; `id`: accepted and unused, as in
        the reference.  Returns (TableSemanticParserSchema, None, None); with `overlays=True` (TableSemanticParserSchema, layout
        picture, OCR picture), two uint8 H x W x 3 arrays the caller owns, each one launch over a device copy of the page."""
        if self.visualize:
            raise NotImplementedError(_NO_VIS)
        if not overlays:
            results_ocr, results_table, paragraphs = self.run_models(img)
            return self.semantic_stage(results_ocr, results_table, paragraphs, template, grid_only, kv_only), None, None
        from .utils import visualizer as V

        page = img if isinstance(img, torch.Tensor) else imaging.page_to_device(img, self.text_detector.device)
        dags = []
        results = self.semantic_stage(*self.run_models(page), template, grid_only, kv_only, dags=dags)
        with torch.cuda.device(page.device):
            layout, ocr = self._drawings(results, dags, V.Overlay)
            vis_layout, vis_ocr = layout.render(page), ocr.render(page)  # each a clone of the page: the D2H below is the only copy out
            return results, _owned_host_image(vis_layout), _owned_host_image(vis_ocr)

    # ---- several pages per call
    def parse_pages(self, imgs, wave: int = 8, template=None, grid_only=False, kv_only=False, overlays=False):
        """`__call__` over a list of pages, `wave` pages at a time on the device, through the stage methods `serve` runs (the two
        chains of a wave side by side, then `finish` per page): DBNet and the table detector run over the pages of a wave,
        PARSeq over the lines of all its pages, the cell detector over the tables of all its pages in chunks of
        CellDetector.MAX_TABLES_PER_FORWARD.  Pages never interact, so every page's result is what `__call__` returns for it.
        `handover.tables(k, ...)` sees a page under its index in `imgs`, as in `serve` (not its index in the wave).
        Returns [TableSemanticParserSchema], in page order; with `overlays=True` [(TableSemanticParserSchema, layout picture,
        OCR picture)]: all canvases of a wave, two per page, are drawn by the wave renderer (utils/visualizer.py: render_wave)."""
        if self.visualize:
            raise NotImplementedError(_NO_VIS)
        job = SimpleNamespace(options={"template": template, "grid_only": grid_only, "kv_only": kv_only}, overlays=bool(overlays))
        out = []
        size = max(1, int(wave))
        pinned = [None]  # the pinned buffer the canvases come back through: this call's, reused by its waves
        for start in range(0, len(imgs), size):
            w = self._run_wave(imgs[start : start + size], start, job)
            results = [self._stage_finish(w, k) for k in range(len(w))]
            if overlays:
                with torch.cuda.device(w.pages[0].device):
                    images = self._stage_render(w, results, pinned)
                for k, pictures in enumerate(images):
                    if isinstance(pictures, BaseException):
                        raise pictures
                    results[k] = (results[k],) + pictures
            out.extend(results)
        return out

    # ---- the stage protocol of the page pipeline (serving.py: StageAnalyzer, which holds the OCR chain).  The table chain
    # ends in the cell detector's two halves; `finish` is what `__call__` does after the networks.
    def _stage_layout(self, wave):
        """One RT-DETRv2 table-detector forward over the pages (device half)."""
        wave.lay_raw = self.layout_parser.forward_pages(wave.pages)

    def _stage_tables(self, wave):
        """Table boxes on the host (shown to the hand-over under the page's position in the job), then the cell detector's
        forwards over all table crops of the wave."""
        wave.lay_parsed = self.layout_parser.pages_from_raw(wave.lay_raw)
        wave.lay_raw = None
        tables = [self._handed_tables(idx, list(l.tables)) for idx, l in zip(wave.ids, wave.lay_parsed)]
        wave.tab_raw = self.cell_detector.forward_tables(wave.pages, tables)

    def _stage_cells(self, wave):
        """The cell detector's box logic on the host: per page its [TableDetectorSchema]."""
        wave.lays = self.cell_detector.tables_from_raw(wave.tab_raw, len(wave.pages))
        wave.tab_raw = None

    def _stage_finish(self, wave, k):
        """Page k of the wave -> TableSemanticParserSchema, with the job's template / grid_only / kv_only: what `__call__` does
        after the networks.  An overlays job keeps the page's grid graphs on the wave for the render stage."""
        job = wave.job
        options = getattr(job, "options", None) or {}
        dags = [] if getattr(job, "overlays", False) else None
        handed = self._hand_over(wave.dets[k], wave.recs[k], wave.lay_parsed[k], wave.lays[k])
        results = self.semantic_stage(*handed, options.get("template"), options.get("grid_only", False), options.get("kv_only", False), dags=dags)
        if dags is not None:
            if wave.dags is None:
                wave.dags = [None] * len(wave)
            wave.dags[k] = dags
        return results

    def _page_drawings(self, wave, k, results):
        """(layout drawing, ocr drawing) of page k - the order `__call__` returns the pictures in -, from the grid graphs that
        `finish` kept on the wave."""
        from .utils.visualizer import RunOverlay

        return self._drawings(results, wave.dags[k], RunOverlay)

    def serve(self, sources, wave: int = 16, in_flight: int = 4, defer_full_gc: bool = True, with_source: bool = False, rec_lanes: int = 2,
              overlays: bool = False, template=None, grid_only=False, kv_only=False, deskew=False):
        """The multi-page entry point, as `DocumentAnalyzer.serve`: host pages (uint8 H x W x 3 BGR arrays) and / or image file
        paths in, one entry per page out, in page order, through the stage pipeline of yomitoku_amd/serving.py - `wave` pages
        per device batch, up to `in_flight` waves between upload and the semantic stage, every host stage (table boxes, the
        cell detector's box logic, the semantic stage) on a thread of its own, so that the networks of the next waves run
        while this wave's cells and grids are worked out.  A page's entry is its TableSemanticParserSchema - equal to
        `__call__(img, template, grid_only=..., kv_only=...)[0]` - or, when the page (or its file) failed, the exception
        object; the other pages are not affected.  `with_source`: (source index, frame index, entry) triples.  `overlays`:
        a page's entry is (schema, layout picture, OCR picture), the two pictures of `__call__(img, overlays=True)` as uint8
        H x W x 3 arrays the caller owns, drawn by the pipeline's render stage; a failed page's entry stays the exception.
        `template`, `grid_only`, `kv_only`, `overlays` are properties of the JOB: they travel with it and the next job starts
        without them.  `defer_full_gc`, `rec_lanes`, `deskew` (the entry ends with the page's PageSkew): see
        `DocumentAnalyzer.serve`."""
        from .deskew import check_deskew

        check_deskew(deskew)  # before the pipeline is built or a source read
        if self.visualize:
            raise NotImplementedError(_NO_VIS)
        options = {"template": template, "grid_only": bool(grid_only), "kv_only": bool(kv_only)}
        return self._serve(sources, wave, in_flight, defer_full_gc, with_source, rec_lanes, overlays, options, deskew=deskew)
