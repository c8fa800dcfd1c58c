"""DocumentAnalyzer.serve(overlays=True): the triples of the render stage against analyze_pages with every visualize flag on.
The analyzer, its seeds, thresholds and pages are those of tests/test_visualize_gpu.py."""
import numpy as np
import pytest

from tests.test_serving_gpu import COUNTERS
from tests.test_visualize_gpu import CONFIGS, _modules, visualize

pytestmark = pytest.mark.gpu


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
    an.layout.layout_parser.thresh_score = 0.4888  # tests/test_visualize_gpu.py says why
    an.layout.table_structure_recognizer.thresh_score = 0.05
    yield an
    an.close()


def test_serve_overlays_equal_analyze_pages(analyzer):
    import threading

    from yomitoku_amd import _lib
    from yomitoku_amd.utils.synth import synthetic_page_with_truth

    page = synthetic_page_with_truth(3, 640, 600)[0]
    imgs = [page, synthetic_page_with_truth(5, 600, 640)[0], page]
    before = [img.copy() for img in imgs]
    want = analyzer.analyze_pages(imgs, wave=2)  # every flag on
    counters = {k: _lib.stat(k) for k in COUNTERS}
    with visualize(False, *_modules(analyzer)):
        plain = analyzer.serve(imgs, wave=2)
        assert not [t for t in threading.enumerate() if t.name == "ymk-render"]
        got = analyzer.serve(imgs, wave=2, overlays=True)
        after = analyzer.serve(imgs, wave=2)
        tagged = analyzer.serve(imgs[:1], wave=2, overlays=True, with_source=True)
    assert len(got) == 3 and all(isinstance(e, tuple) and len(e) == 3 for e in got)
    for k, (img, (schema, ocr, lay), (w_schema, w_ocr, w_lay)) in enumerate(zip(imgs, got, want)):
        assert schema.model_dump() == plain[k].model_dump() == after[k].model_dump()
        for vis, w_vis, name in ((ocr, w_ocr, "ocr"), (lay, w_lay, "layout")):
            assert isinstance(vis, np.ndarray) and vis.dtype == np.uint8 and vis.shape == img.shape and vis.flags.owndata
            print(f"page {k} {name}: differing pixels {int((vis != w_vis).any(-1).sum())}, drawn {int((vis != img).any(-1).sum())}")
            assert np.array_equal(vis, w_vis)
            assert not np.array_equal(vis, img)
        print(f"page {k}: words {len(schema.words)}, tables {[(t.n_row, t.n_col) for t in schema.tables]}")
        assert len(schema.words) > 0
    assert any(len(s.tables) > 0 for s, _, _ in got)
    assert all(not isinstance(e, tuple) for e in after)
    assert tagged[0][:2] == (0, 0) and np.array_equal(tagged[0][2][1], got[0][1]) and np.array_equal(tagged[0][2][2], got[0][2])
    assert all(np.array_equal(a, b) for a, b in zip(imgs, before))
    after_counters = {k: _lib.stat(k) for k in COUNTERS}  # no forward allocated, built or waited: the render stage is not in them
    assert after_counters == counters, {k: after_counters[k] - counters[k] for k in COUNTERS}
