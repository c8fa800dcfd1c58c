"""TableSemanticParser on the MI355X with seeded weights: the WIRING of the page path - one upload, the device page handed to
the four modules, the two chains on their own HIP streams, the cell detector's crops cut from the device page - not the
arithmetic of the nets (tests/test_dbnet_gpu.py, test_rtdetr_gpu.py, test_parseq_gpu.py, test_cells_gpu.py hold that) and not the
host logic (tests/test_table_semantic_golden.py)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# Seeded random weights detect noise: if the table detector finds no table on the page there is nothing for the cell detector
# and the semantic stage to do, and the test would compare two empty results.  Then these two boxes (300 x 200 and 200 x 300 px,
# inside the 842 x 596 / 596 x 842 page) are put in at the layout hand-over - on BOTH sides of every comparison.
FIXED_TABLES = ([30, 40, 330, 240], [350, 250, 550, 550])


class _FixedTables:
    def tables(self, k, tables):
        from yomitoku_amd.schemas import Element

        return [Element(id=None, box=list(b), score=1.0, role=None, contents=None) for b in FIXED_TABLES]


@pytest.fixture(scope="module")
def page():
    from yomitoku_amd.data.functions import load_image

    (img,) = load_image(os.path.join(os.path.dirname(__file__), "golden", "test_page.jpg"))
    assert min(img.shape[:2]) >= 550
    return img


@pytest.fixture(scope="module")
def parser(dev, page):
    from yomitoku_amd import TableSemanticParser
    from yomitoku_amd.utils.synth import dbnet_state_dict, parseq_state_dict
    from yomitoku_amd.utils.synth_rtdetr import rtdetr_state_dict

    configs = {"table_detector": {"from_pretrained": False}, "table_cell_parser": {"from_pretrained": False},
               "text_detector": {"from_pretrained": False},
               "text_recognizer": {"model_name": "parseq-tiny-dynw-v4", "from_pretrained": False, "dynamic_width": True, "batch_bucketing": True}}
    p = TableSemanticParser(configs=configs, device="cuda:0")
    # the seeds of tests/test_baseline_configs_gpu.py (a detector that finds text boxes on this page), test_pipeline_gpu.py and
    # test_cells_gpu.py (a cell detector that finds cells in a crop)
    p.text_detector.model.load_state_dict(dbnet_state_dict(8, out_bias=-1.5))
    p.text_recognizer.model.load_state_dict(parseq_state_dict(1235, eos_bias=6.0))
    p.layout_parser.model.load_state_dict(rtdetr_state_dict(1240, num_classes=6, score_bias=-2.0))
    p.cell_detector.model.load_state_dict(rtdetr_state_dict(1243, num_classes=6, eval_size=(960, 960), enc_score_gain=12.0, score_bias=-3.0,
                                                            score_gain=2.0))
    if not p.layout_parser(page)[0].tables:
        p.handover = _FixedTables()
    yield p
    p.close()


def _one_after_another(p, img):
    """The four modules called in sequence by the test, each uploading the host page itself, then the CPU semantic stage."""
    det, _ = p.text_detector(img)
    lay, _ = p.layout_parser(img)
    tables = p.cell_detector(img, p._handed_tables(0, list(lay.tables)))
    rec, _ = p.text_recognizer(img, det.points)
    return p.semantic_stage(*p._hand_over(det, rec, lay, tables))


@pytest.fixture(scope="module")
def single(parser, page):
    """`__call__` on the page, once for both tests."""
    got, vis_layout, vis_ocr = parser(page)
    assert vis_layout is None and vis_ocr is None
    return got


def test_call_equals_the_modules_called_one_after_another(parser, page, single):
    from yomitoku_amd.schemas import TableSemanticParserSchema

    got = single
    assert isinstance(got, TableSemanticParserSchema)
    want = _one_after_another(parser, page)
    assert got.model_dump() == want.model_dump()
    n_cells = sum(len(t.cells) for t in got.tables)
    print("tables", len(got.tables), "cells", n_cells, "kv items", sum(len(t.kv_items) for t in got.tables),
          "grids", sum(len(t.grids) for t in got.tables), "paragraphs", len(got.paragraphs), "words", len(got.words),
          "fixed tables" if parser.handover is not None else "detected tables")
    assert len(got.words) > 0 and len(got.tables) > 0 and n_cells > 0
    assert set(got.to_dict()) == {t.id for t in got.tables} and len(got.to_simple().tables) == len(got.tables)


def test_parse_pages_equals_per_page_calls(parser, page, single):
    """The comparison tests/test_pipeline_gpu.py::test_analyze_pages_equals_per_page_calls applies: same structure, strings and
    integers, scores to 1e-4 (a forward over more crops may pick another tile shape: logits differ in their last bits)."""
    from tests.test_pipeline_gpu import _assert_same_schema

    flipped = np.ascontiguousarray(page[:, ::-1])
    singles = [single.model_dump(), parser(flipped)[0].model_dump()]
    multi = parser.parse_pages([page, flipped])
    assert len(multi) == 2
    for one, many in zip(singles, multi):
        _assert_same_schema(one, many.model_dump())
    assert parser.parse_pages([]) == []


@pytest.mark.parametrize("overlays", [False, True], ids=["plain", "overlays"])
def test_parse_pages_across_chunk_boundaries(parser, page, overlays):
    """Three pages with wave=2: two chunks, the second ragged - the smallest input whose pages' indices in the call differ from
    their indices in the wave (the stage methods run over a Wave per chunk; `finish` and the renderer index it by position).
    Every entry is the per-page `__call__`'s, to the tolerances above; the pictures are equal byte for byte (an integer
    rasteriser over the same integer boxes and strings)."""
    from tests.test_pipeline_gpu import _assert_same_schema

    flipped = np.ascontiguousarray(page[:, ::-1])
    want = [parser(img, overlays=overlays) for img in (page, flipped)]
    multi = parser.parse_pages([page, flipped, page], wave=2, overlays=overlays)
    assert len(multi) == 3
    for (one, vis_layout, vis_ocr), many in zip(want + want[:1], multi):
        if overlays:
            many, many_layout, many_ocr = many
            assert many_layout.shape == page.shape and many_layout.dtype == np.uint8
            assert np.array_equal(many_layout, vis_layout) and np.array_equal(many_ocr, vis_ocr)
        _assert_same_schema(one.model_dump(), many.model_dump())
    if overlays:
        assert not np.array_equal(multi[0][1], multi[1][1]) and not np.array_equal(multi[0][1], page)  # something was drawn
