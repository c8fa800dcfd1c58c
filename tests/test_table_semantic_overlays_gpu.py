"""TableSemanticParser's per-call pictures on the MI355X with seeded weights: `parser(img, overlays=True)` and
`parse_pages(imgs, overlays=True)` return what the calls without the keyword return, plus two images that equal the NumPy
restatement of the drawing rules (tests/overlay_layer_ref.py) applied to the page with the commands rebuilt on the host from the
returned results and the grid graphs `semantic_stage` handed out.  The set-up is that of tests/test_table_semantic_gpu.py."""
import os

import numpy as np
import pytest
import torch

from tests import overlay_layer_ref as lref

pytestmark = pytest.mark.gpu

# Seeded random weights detect noise: if the table detector finds no table on the page, these two boxes (inside the 842 x 596 /
# 596 x 842 page) are put in at the layout hand-over, as tests/test_table_semantic_gpu.py does.
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
    p.text_detector.model.load_state_dict(dbnet_state_dict(8, out_bias=-1.5))
    p.text_recognizer.model.load_state_dict(parseq_state_dict(1235, eos_bias=6.0))
    p.layout_parser.model.load_state_dict(rtdetr_state_dict(1240, num_classes=6, score_bias=-2.0))
    p.cell_detector.model.load_state_dict(rtdetr_state_dict(1243, num_classes=6, eval_size=(960, 960), enc_score_gain=12.0, score_bias=-3.0,
                                                            score_gain=2.0))
    if not p.layout_parser(page)[0].tables:
        p.handover = _FixedTables()
    # the graphs of every semantic_stage call, in call order: the list the parser passes as `dags` is kept
    p.graphs = []
    stage = p.semantic_stage

    def recording_stage(*args, **kwargs):
        if kwargs.get("dags") is not None:
            p.graphs.append(kwargs["dags"])
        return stage(*args, **kwargs)

    p.semantic_stage = recording_stage
    yield p
    p.close()


def _expected(parser, img, results, dags):
    """The two pictures from the rules: the drawings recorded again from `results` and `dags`, built on the host (text laid out
    by Overlay.text, no binning needed) and applied by the restatement."""
    from yomitoku_amd.utils import visualizer as V

    h, w = img.shape[:2]
    out = []
    for ov in parser._drawings(results, dags, V.Overlay):
        data = ov.build(h, w, tile=32)
        out.append((lref.draw_reference(img, data["cmds"], data["atlas"], within_reach=True), data["cmds"]))
    return out


def _same(got, want, what):
    bad = np.argwhere((got != want).any(-1))
    assert np.array_equal(got, want), f"{what}: {len(bad)} pixels differ, first at (y, x) = {bad[0].tolist()}"


def _check_images(parser, img, results, dags, vis_layout, vis_ocr, what):
    from yomitoku_amd.utils import visualizer as V

    (want_layout, layout_cmds), (want_ocr, ocr_cmds) = _expected(parser, img, results, dags)
    for vis in (vis_layout, vis_ocr):
        assert isinstance(vis, np.ndarray) and vis.dtype == np.uint8 and vis.shape == img.shape and vis.flags.owndata and vis.flags.writeable
        assert not np.array_equal(vis, img)
    _same(vis_layout, want_layout, f"{what}: layout picture")
    _same(vis_ocr, want_ocr, f"{what}: ocr picture")
    kinds = layout_cmds[:, 0]
    n_tables = len(results.tables)
    assert (kinds == V.FLUSH).sum() == n_tables and (kinds == (V.BOX | V.TO_LAYER)).sum() > 0  # one tint flush per table
    assert (ocr_cmds[:, 0] == V.SEG).sum() == 4 * len(results.words)
    return layout_cmds


@pytest.fixture(scope="module")
def single(parser, page):
    got, vis_layout, vis_ocr = parser(page)
    assert vis_layout is None and vis_ocr is None
    return got


def test_call_with_overlays(parser, page, single):
    before = page.copy()
    page_dev = torch.from_numpy(np.ascontiguousarray(page)).to("cuda:0")
    parser.graphs.clear()
    got, vis_layout, vis_ocr = parser(page_dev, overlays=True)
    assert got.model_dump() == single.model_dump()
    n_cells = sum(len(t.cells) for t in got.tables)
    assert len(got.words) > 0 and len(got.tables) > 0 and n_cells > 0  # something to draw
    assert len(parser.graphs) == 1
    cmds = _check_images(parser, page, got, parser.graphs[0], vis_layout, vis_ocr, "device page")
    print("tables", len(got.tables), "cells", n_cells, "kv items", sum(len(t.kv_items) for t in got.tables), "grids",
          sum(len(t.grids) for t in got.tables), "graphs", len(parser.graphs[0]), "words", len(got.words), "layout commands", len(cmds))
    assert np.array_equal(page_dev.cpu().numpy(), before)  # the page the networks read is never drawn on


def test_parse_pages_with_overlays(parser, page, single):
    from tests.test_pipeline_gpu import _assert_same_schema

    flipped = np.ascontiguousarray(page[:, ::-1])
    singles = [single.model_dump(), parser(flipped)[0].model_dump()]
    parser.graphs.clear()
    before = page.copy()
    multi = parser.parse_pages([page, flipped], overlays=True)  # host pages: a strided view and a contiguous array
    assert len(multi) == 2 and len(parser.graphs) == 2
    assert np.array_equal(page, before) and np.array_equal(flipped, before[:, ::-1])
    for img, one, (results, vis_layout, vis_ocr), dags in zip((page, flipped), singles, multi, parser.graphs):
        _assert_same_schema(one, results.model_dump())
        _check_images(parser, img, results, dags, vis_layout, vis_ocr, "wave")  # each against ITS OWN results
    assert not np.array_equal(multi[0][1], multi[1][1])
    assert parser.parse_pages([], overlays=True) == []
