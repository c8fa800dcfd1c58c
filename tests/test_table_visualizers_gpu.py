"""The four public table visualisers of yomitoku_amd/utils/visualizer.py - cell_detector_visualizer, cell_id_visualizer,
kv_items_visualizer, dag_visualizer - run on the MI355X on the tiny table of tests/test_overlay_layer.py, with host and with
device pages: each image equals the NumPy restatement (tests/overlay_layer_ref.py) applied to a hand-written command list, and
the input image is never drawn on."""
import numpy as np
import pytest
import torch

from tests import overlay_layer_ref as lref
from tests.test_overlay_layer import L, _tiny_table, box, flush, outline, seg
from yomitoku_amd.utils import visualizer as V

pytestmark = pytest.mark.gpu

GREEN, RED = (0, 255, 0), (255, 0, 0)
HEADER, CELL, HOLE, GROUP = (0, 255, 0), (255, 128, 0), (200, 200, 200), (255, 255, 0)


def _page(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _same(got, want, what):
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == want.shape, what
    bad = np.argwhere((got != want).any(-1))
    assert np.array_equal(got, want), f"{what}: {len(bad)} pixels differ, first at (y, x) = {bad[0].tolist()}"


def _both_ways(dev, fn, page, want, what):
    """`fn(img, to_host)` with a host page and with a device page, to the host and left on the device: always `want`, and the
    page stays what it was."""
    assert not np.array_equal(want, page), what
    before = page.copy()
    page_dev = torch.from_numpy(page).to(dev)
    _same(fn(page, True), want, f"{what}, host page")
    _same(fn(page_dev, True), want, f"{what}, device page")
    canvas = fn(page_dev, False)
    assert isinstance(canvas, torch.Tensor) and canvas.is_cuda and canvas.data_ptr() != page_dev.data_ptr()
    _same(canvas.cpu().numpy(), want, f"{what}, left on the device")
    assert np.array_equal(page, before) and np.array_equal(page_dev.cpu().numpy(), before), f"{what}: the input was drawn on"


def test_cell_detector_visualizer(dev):
    table = _tiny_table()
    cells = list(table.cells.values())
    page1, page2 = _page(100, 110, 1), _page(100, 110, 2)
    tint = [box((10, 10, 50, 50), color=HEADER, flag=L), box((50, 10, 90, 50), color=CELL, flag=L), box((10, 50, 50, 90), color=CELL, flag=L),
            flush((10, 10, 90, 90), 77, keep255=1),
            outline((10, 10, 50, 50), 2, HEADER), outline((50, 10, 90, 50), 2, CELL), outline((10, 50, 50, 90), 2, CELL),
            outline((60, 60, 80, 80), 2, HOLE)]
    want1 = lref.draw_reference(page1, tint)
    want2 = lref.draw_reference(page2, [outline((5, 5, 95, 95), 2, GROUP)])
    _both_ways(dev, lambda img, host: V.cell_detector_visualizer(img, page2, cells, to_host=host)[0], page1, want1, "first image")
    _both_ways(dev, lambda img, host: V.cell_detector_visualizer(page1, img, cells, to_host=host)[1], page2, want2, "second image")
    out1, out2 = V.cell_detector_visualizer(page1, torch.from_numpy(page2).to(dev), iter(cells))  # any iterable, mixed pages
    _same(out1, want1, "pair: first")
    _same(out2, want2, "pair: second")
    # the tint is composited once: on the border column the two cells share, and inside the header where channel 1 is 255
    p = page1.astype(np.int64)
    assert out1[30, 30, 1] == p[30, 30, 1] and out1[30, 30, 0] == (p[30, 30, 0] * 178 + 127) // 255
    assert out1[30, 50, 0] == 255  # the outlines are drawn over the tint, opaque
    assert out1[30, 47, 0] == (p[30, 47, 0] * 178 + 127) // 255 and out1[30, 53, 0] == p[30, 53, 0]  # header left of it, cell (255, 128, 0) right
    # no group cell: the second image is an empty drawing, a plain copy
    out1, out2 = V.cell_detector_visualizer(page1, page2, [c for c in cells if c.role != "group"])
    _same(out1, want1, "no group: first")
    assert np.array_equal(out2, page2) and out2 is not page2


def test_kv_items_visualizer(dev):
    table = _tiny_table()
    table.cells["r0c1"].box = [110, 20, 150, 120]  # the value spans rows: the arrow stays horizontal at the shared band's middle
    page = _page(130, 170, 3)
    # (30, 35) -> (130, 35): 100 px, tip min(0.2, 12 / 100) * 100 = 12 px, its strokes 8.49 px on either axis
    want = lref.draw_reference(page, [seg(30, 35, 130, 35, 2, GREEN), seg(122, 27, 130, 35, 2, GREEN), seg(122, 43, 130, 35, 2, GREEN)])
    _both_ways(dev, lambda img, host: V.kv_items_visualizer(table, img, to_host=host), page, want, "kv arrows")
    table.kv_items = []
    assert np.array_equal(V.kv_items_visualizer(table, page), page)


def test_dag_visualizer(dev):
    from yomitoku_amd.utils.graph import OrderedDiGraph

    dag = OrderedDiGraph()
    dag.add_node("a", bbox=(10, 10, 50, 50))
    dag.add_node("b", bbox=(110, 20, 150, 80))
    dag.add_node("c", bbox=(20, 110, 80, 150))
    for u, v, d in (("a", "b", "R"), ("b", "a", "L"), ("a", "c", "D"), ("c", "a", "U")):
        dag.add_edge(u, v, dir=d)
    page = _page(160, 160, 4)
    want = lref.draw_reference(page, [seg(30, 35, 130, 35, 2, GREEN), seg(122, 27, 130, 35, 2, GREEN), seg(122, 43, 130, 35, 2, GREEN),
                                      seg(35, 30, 35, 130, 2, RED), seg(43, 122, 35, 130, 2, RED), seg(27, 122, 35, 130, 2, RED)])
    _both_ways(dev, lambda img, host: V.dag_visualizer(dag, img, to_host=host), page, want, "grid graph")


def _chips(tables, font_size, h, w):
    """cell_id_visualizer's drawing from its rule, written out: per non-group cell with an id the glyphs of the id are placed
    once at the origin to measure their box; the chip is that box plus the pad on every side with its corner at the cell's
    corner + (2, 2); the glyphs go inside it, pad from its edges.  Returns the launch data of the whole drawing."""
    font = V.load_font(None, font_size)
    pad = max(2, font_size // 5)
    ov = V.Overlay()
    for table in tables:
        for cell in (table.cells.values() if isinstance(table.cells, dict) else table.cells):
            if cell.role == "group" or cell.id is None:
                continue
            probe = V.Overlay()
            probe.text((0, 0), cell.id, font, (0, 0, 0))
            g = np.asarray(probe.build(h, w, tile=32)["cmds"])
            left, top = int(g[:, 5].min()), int(g[:, 6].min())
            right, bottom = int((g[:, 5] + g[:, 7]).max()), int((g[:, 6] + g[:, 8]).max())
            bx, by = cell.box[0] + 2, cell.box[1] + 2
            ov.rounded_fill((bx, by, bx + right - left + 2 * pad, by + bottom - top + 2 * pad), pad, (40, 40, 40), alpha=200)
            ov.text((bx + pad - left, by + pad - top), cell.id, font, (255, 255, 255))
    return ov.build(h, w, tile=32)


def test_cell_id_visualizer(dev):
    from types import SimpleNamespace

    table = _tiny_table()
    table.cells["r1c0"].id = None
    as_list = SimpleNamespace(cells=[SimpleNamespace(id="r9c9", box=[100, 60, 140, 90], role="empty")])
    tables = [table, as_list]
    # the default size is max(14, width // 75): 14 on a narrow page, 16 on one 1200 px wide (pad = radius = 2 and 3)
    for (h, w), size in (((100, 150), 14), ((100, 1200), 16)):
        page = _page(h, w, 5)
        data = _chips(tables, size, h, w)
        kinds = data["cmds"][:, 0]
        assert (kinds == V.RBOX).sum() == 4 and (data["cmds"][kinds == V.RBOX, 9] == max(2, size // 5)).all()
        assert data["cmds"][0, 5:7].tolist() == [12, 12] and (kinds == V.GLYPH).sum() == len("r0c0" "r0c1" "x0" "r9c9")
        want = lref.draw_reference(page, data["cmds"], data["atlas"], within_reach=True)
        _both_ways(dev, lambda img, host: V.cell_id_visualizer(img, tables, None, to_host=host), page, want, f"default size on a {w} px page")
        _same(V.cell_id_visualizer(page, tables, None, font_size=size), want, "the same size given")
        if size == 14:
            other = _chips(tables, 20, h, w)
            _same(V.cell_id_visualizer(page, tables, None, font_size=20), lref.draw_reference(page, other["cmds"], other["atlas"], within_reach=True),
                  "font_size=20")
    # the chip is blended at 200 / 255 over the page, straight onto the canvas
    page = _page(100, 150, 5)
    got = V.cell_id_visualizer(page, tables, None)
    assert got[13, 20].tolist() == ((40 * 200 + page[13, 20].astype(np.int64) * 55 + 127) // 255).tolist()  # in the pad above the glyphs
    assert got[12, 12].tolist() == page[12, 12].tolist()  # the rounded corner is not covered
