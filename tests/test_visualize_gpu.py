"""visualize=True through the product classes: every module and orchestrator returns the image the standalone
yomitoku_amd.utils.visualizer function draws from the schema it returns, and the schema it returns with visualize=False.
Seeded weights and the lite recogniser, as tests/test_pipeline_gpu.py builds them; one 640 x 600 synthetic page (about the
smallest the page generator lays a table on)."""
import contextlib
from types import SimpleNamespace

import numpy as np
import pytest

from tests import overlay_ref as ref

pytestmark = pytest.mark.gpu

CONFIGS = {
    "ocr": {
        "text_detector": {"from_pretrained": False},
        "text_recognizer": {"model_name": "parseq-tiny-dynw-v4", "from_pretrained": False, "dynamic_width": True, "batch_bucketing": True},
    },
    "layout_analyzer": {"layout_parser": {"from_pretrained": False}, "table_structure_recognizer": {"from_pretrained": False}},
}


@pytest.fixture(scope="module")
def page():
    from yomitoku_amd.utils.synth import synthetic_page_with_truth

    return synthetic_page_with_truth(3, 640, 600)


@pytest.fixture(scope="module")
def analyzer(dev):
    from yomitoku_amd import DocumentAnalyzer
    from yomitoku_amd.utils.synth import dbnet_state_dict, parseq_state_dict
    from yomitoku_amd.utils.synth_rtdetr import rtdetr_state_dict

    an = DocumentAnalyzer(configs=CONFIGS, device="cuda:0", visualize=True)
    an.text_detector.model.load_state_dict(dbnet_state_dict(1234, out_bias=-2.0))
    an.text_recognizer.model.load_state_dict(parseq_state_dict(1235, eos_bias=6.0))
    an.layout.layout_parser.model.load_state_dict(rtdetr_state_dict(1240, num_classes=6, score_bias=-2.0))
    an.layout.table_structure_recognizer.model.load_state_dict(rtdetr_state_dict(1243, num_classes=3, score_bias=-1.0))
    # Seeded weights score low, so the thresholds are set where the layout and table stages keep a FEW boxes and every overlay has
    # content.  Layout: the seeded net's scores on these pages lie between 0.17 and 0.52, all of class 0; 0.4888 sits in a gap of
    # the sorted scores of both pages (0.4878 | 0.4903 on the 640 x 600 page, 0.4859 | 0.4898 on the 600 x 640 one) and keeps five
    # and nine boxes - at 0.05 it keeps 200 overlapping "tables" per page.  Table net: seed 1243 as in
    # tests/test_baseline_configs_gpu.py (1241 fires on columns only, so every table would be dropped for lack of rows); its one
    # row scores 0.41 and its columns 0.42 .. 0.62, all far above 0.05.
    an.layout.layout_parser.thresh_score = 0.4888
    an.layout.table_structure_recognizer.thresh_score = 0.05
    yield an
    an.close()


@contextlib.contextmanager
def visualize(flag, *objects):
    old = [o.visualize for o in objects]
    for o in objects:
        o.visualize = flag
    try:
        yield
    finally:
        for o, v in zip(objects, old):
            o.visualize = v


def _is_image_of(vis, img):
    assert isinstance(vis, np.ndarray) and vis.dtype == np.uint8 and vis.shape == img.shape


def _rec_like(words):
    return SimpleNamespace(contents=[w.content for w in words], points=[w.points for w in words], directions=[w.direction for w in words])


def _rec_overlay(module, canvas, outputs):
    from yomitoku_amd.utils.visualizer import rec_visualizer

    cfg = module._cfg.visualize
    return rec_visualizer(canvas, outputs, font_path=cfg.font, font_size=cfg.font_size, font_color=tuple(cfg.color[::-1]))


def test_text_detector(analyzer, page):
    from yomitoku_amd.utils.visualizer import det_visualizer

    img, det = page[0], analyzer.text_detector
    before = img.copy()
    results, vis = det(img)
    _is_image_of(vis, img)
    with visualize(False, det):
        plain, none = det(img)
    assert none is None and plain.model_dump() == results.model_dump()
    print("detector quads:", len(results.points))
    assert len(results.points) > 0
    assert np.array_equal(vis, det_visualizer(img, results.points, line_color=tuple(det._cfg.visualize.color[::-1])))
    assert not np.array_equal(vis, img) and np.array_equal(img, before)
    # the drawing is what the rules say: closed polylines of thickness 1 in the configured colour
    cmds = [[0, *det._cfg.visualize.color[::-1], 255, *q[k], *q[(k + 1) % 4], 1, 0, 0, 0, 0, 0, 0] for q in results.points for k in range(4)]
    assert np.array_equal(vis, ref.draw_reference(img, cmds, within_reach=True))


def test_text_detector_heatmap(analyzer, page):
    """visualize.heatmap: the probability map is blended under the quads - every pixel the blend must change has changed."""
    img, det = page[0], analyzer.text_detector
    det._cfg.visualize.heatmap = True
    try:
        results, vis = det(img)
        prob = det.model(det.preprocess(img))["binary"][0, 0].cpu().numpy()
    finally:
        det._cfg.visualize.heatmap = False
    heat = ref.heatmap_reference(img, prob)
    cmds = [[0, *det._cfg.visualize.color[::-1], 255, *q[k], *q[(k + 1) % 4], 1, 0, 0, 0, 0, 0, 0] for q in results.points for k in range(4)]
    assert np.array_equal(vis, ref.draw_reference(heat, cmds, within_reach=True))
    must_change = (heat != img).any(-1)
    assert must_change.mean() > 0.5
    assert (vis[must_change] != img[must_change]).any(-1).mean() > 0.99  # all but the few pixels a line happens to restore


def test_text_recognizer(analyzer, page):
    img, quads, rec = page[0], page[1][:12], analyzer.text_recognizer
    results, vis = rec(img, quads)
    _is_image_of(vis, img)
    with visualize(False, rec):
        plain, none = rec(img, quads)
    assert none is None and plain.model_dump() == results.model_dump()
    print("recognised:", results.contents[:4])
    assert np.array_equal(vis, _rec_overlay(rec, img, results))
    assert not np.array_equal(vis, img)
    # `vis` given: the strings are drawn onto it, and it is not modified
    canvas = np.full_like(img, 90)
    _, onto = rec(img, quads, vis=canvas)
    assert np.array_equal(onto, _rec_overlay(rec, canvas, results)) and np.all(canvas == 90)


def test_layout_parser_and_table_structure_recognizer(analyzer, page):
    from yomitoku_amd.utils.visualizer import layout_visualizer, table_visualizer

    img, tables = page[0], page[2]
    lp, ts = analyzer.layout.layout_parser, analyzer.layout.table_structure_recognizer
    results, vis = lp(img)
    _is_image_of(vis, img)
    with visualize(False, lp):
        plain, none = lp(img)
    assert none is None and plain.model_dump() == results.model_dump()
    counts = {k: len(v) for k, v in results.model_dump().items()}
    print("layout elements:", counts)
    assert sum(counts.values()) > 0
    assert np.array_equal(vis, layout_visualizer(results, img)) and not np.array_equal(vis, img)

    out, tvis = ts(img, tables)
    _is_image_of(tvis, img)
    with visualize(False, ts):
        plain, none = ts(img, tables)
    assert none is None and [t.model_dump() for t in plain] == [t.model_dump() for t in out]
    print("tables:", [(t.n_row, t.n_col) for t in out])
    assert len(out) > 0 and sum(len(t.cells) for t in out) > 0
    want = img
    for table in out:  # the reference's loop: one table_visualizer call per table
        want = table_visualizer(want, table)
    assert np.array_equal(tvis, want) and not np.array_equal(tvis, img)
    # chained: drawn onto the layout overlay
    _, both = ts(img, tables, vis=vis)
    want = vis
    for table in out:
        want = table_visualizer(want, table)
    assert np.array_equal(both, want)


def test_ocr(dev, page):
    from yomitoku_amd.document_analyzer import OCR
    from yomitoku_amd.utils.synth import dbnet_state_dict, parseq_state_dict
    from yomitoku_amd.utils.visualizer import det_visualizer

    img = page[0]
    ocr = OCR(configs=CONFIGS["ocr"], device="cuda:0", visualize=True)
    ocr.detector.model.load_state_dict(dbnet_state_dict(1234, out_bias=-2.0))
    ocr.recognizer.model.load_state_dict(parseq_state_dict(1235, eos_bias=6.0))
    results, vis = ocr(img)
    _is_image_of(vis, img)
    with visualize(False, ocr.detector, ocr.recognizer):
        plain, none = ocr(img)
    assert none is None and plain.model_dump() == results.model_dump()
    assert len(results.words) > 0
    under = det_visualizer(img, [w.points for w in results.words], line_color=tuple(ocr.detector._cfg.visualize.color[::-1]))
    assert np.array_equal(vis, _rec_overlay(ocr.recognizer, under, _rec_like(results.words)))
    for module in (ocr.detector, ocr.recognizer):
        module.model.close()


def test_layout_analyzer(analyzer, page):
    from yomitoku_amd.utils.visualizer import layout_visualizer, table_visualizer

    img, layout = page[0], analyzer.layout
    results, vis = layout(img)
    _is_image_of(vis, img)
    with visualize(False, layout.layout_parser, layout.table_structure_recognizer):
        plain, none = layout(img)
        parsed, _ = layout.layout_parser(img)
    assert none is None and plain.model_dump() == results.model_dump()
    want = layout_visualizer(parsed, img)
    for table in results.tables:
        want = table_visualizer(want, table)
    assert np.array_equal(vis, want) and not np.array_equal(vis, img)


def _modules(an):
    return an, an.text_detector, an.text_recognizer, an.layout.layout_parser, an.layout.table_structure_recognizer


def _expected_analyzer_images(an, img, results):
    from yomitoku_amd.utils.visualizer import det_visualizer, reading_order_visualizer

    ocr = _rec_overlay(an.text_recognizer, det_visualizer(img, [w.points for w in results.words]), _rec_like(results.words))
    _, layout = an.layout(img)
    return ocr, reading_order_visualizer(layout, results)


def test_document_analyzer(analyzer, page):
    img = page[0]
    results, ocr, layout = analyzer(img)
    _is_image_of(ocr, img)
    _is_image_of(layout, img)
    with visualize(False, *_modules(analyzer)):
        plain, no_ocr, no_layout = analyzer(img)
    assert no_ocr is None and no_layout is None and plain.model_dump() == results.model_dump()
    want_ocr, want_layout = _expected_analyzer_images(analyzer, img, results)
    assert np.array_equal(ocr, want_ocr) and np.array_equal(layout, want_layout)
    orders = len(results.paragraphs) + len(results.tables) + len(results.figures)
    print("words:", len(results.words), "ordered elements:", orders)
    assert orders > 0 and not np.array_equal(layout, analyzer.layout(img)[1]), "the reading order is drawn over the layout overlay"


def test_analyze_pages_images_equal_per_page_calls(analyzer, page):
    """A wave shares its forwards among the pages, so scores may differ from the per-page call in their last bits
    (tests/test_pipeline_gpu.py::test_analyze_pages_equals_per_page_calls); boxes, strings and orders - all that is drawn - are
    the same, and so are the images."""
    from tests.test_pipeline_gpu import _assert_same_schema
    from yomitoku_amd.utils.synth import synthetic_page_with_truth

    imgs = [page[0], synthetic_page_with_truth(5, 600, 640)[0], page[0]]
    singles = [analyzer(img) for img in imgs]
    multi = analyzer.analyze_pages(imgs, wave=2)
    assert len(multi) == 3
    for img, (r1, ocr1, lay1), (r2, ocr2, lay2) in zip(imgs, singles, multi):
        _is_image_of(ocr2, img)
        _is_image_of(lay2, img)
        _assert_same_schema(r1.model_dump(), r2.model_dump())  # what is drawn is the same; a difference here is not the overlay's
        print("tables:", [(t.n_row, t.n_col, len(t.cells)) for t in r2.tables], "differing pixels:",
              int((ocr1 != ocr2).any(-1).sum()), int((lay1 != lay2).any(-1).sum()))
        assert np.array_equal(ocr1, ocr2) and np.array_equal(lay1, lay2)
    with visualize(False, *_modules(analyzer)):
        for _, ocr, lay in analyzer.analyze_pages(imgs[:1]):
            assert ocr is None and lay is None


def test_serve_still_refuses(analyzer, page):
    with pytest.raises(NotImplementedError, match="serve"):
        analyzer.serve([page[0]])
