"""Host half of the table overlays (yomitoku_amd/utils/visualizer.py): the layer, the flush and the rounded box in the command
builder and the binning, the four table visualisers' command lists, and the per-call switch of TableSemanticParser - against the
NumPy restatement of the rules in tests/overlay_layer_ref.py.  No GPU: nothing here launches."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import overlay_layer_ref as lref
from tests import overlay_ref as ref
from tests.test_overlay_plan import _random_overlay, _tiles_of_bbox
from yomitoku_amd.utils import visualizer as vz

L = vz.TO_LAYER


def seg(x0, y0, x1, y1, t, color, a=255, flag=0):
    return [vz.SEG | flag, *color, a, x0, y0, x1, y1, t, 0, 0, 0, 0, 0, 0]


def box(outer, inner=(1, 1, 0, 0), color=(255, 0, 255), a=255, flag=0):
    return [vz.BOX | flag, *color, a, *outer, *inner, 0, 0, 0]


def outline(b, t, color):
    g, s = t // 2, (t + 1) // 2
    return box((b[0] - g, b[1] - g, b[2] + g, b[3] + g), (b[0] + s, b[1] + s, b[2] - s, b[3] - s), color)


def rbox(b, r, color, a=255, flag=0):
    return [vz.RBOX | flag, *color, a, *b, r, 0, 0, 0, 0, 0, 0]


def flush(b, a, keep255=0, flag=0):
    return [vz.FLUSH | flag, 0, 0, 0, a, *b, keep255, 0, 0, 0, 0, 0, 0]


def _page(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _cmds(ov, h=100, w=100):
    return ov.build(h, w, tile=32)["cmds"].tolist()


# ------------------------------------------------------------------------------------------------------ the two restatements
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_new_reference_equals_the_old_one_without_new_kinds(seed):
    h, w = 45, 70
    data = _random_overlay(seed, h, w).build(h, w, tile=8)
    page = _page(h, w, 50 + seed)
    want = ref.draw_reference(page, data["cmds"], data["atlas"])
    assert np.array_equal(lref.draw_reference(page, data["cmds"], data["atlas"]), want)
    assert np.array_equal(lref.draw_by_tiles(page, data["cmds"], data["atlas"], data["tile_offsets"], data["tile_cmds"], 8), want)
    for cmd in data["cmds"]:
        got = lref.box_of(cmd)
        assert got == tuple(int(v[0]) for v in vz.command_bounds(cmd[None]))


# ------------------------------------------------------------------------------------------------------------------ binning
def _layered_overlay(seed, h, w, n=36):
    """Canvas and layer commands of every kind interleaved, flushes in between (some with nothing painted, some with keep255),
    and layer commands after the last flush."""
    rng = np.random.default_rng(seed)
    ov = vz.Overlay()
    font = vz.load_font(None, 12)

    def pt():
        return int(rng.integers(-12, w + 12)), int(rng.integers(-12, h + 12))

    def one():
        kind = int(rng.integers(0, 5))
        color = tuple(int(v) for v in rng.choice([0, 128, 255, int(rng.integers(0, 256))], 3))
        alpha = int(rng.choice([77, 255, 255, int(rng.integers(1, 255))]))
        if kind == 0:
            ov.segment(pt(), pt(), color, int(rng.integers(1, 7)), alpha)
        elif kind == 1:
            ov.rectangle(pt() + pt(), color, int(rng.integers(1, 6)), alpha)
        elif kind == 2:
            ov.fill(pt() + pt(), color, alpha)
        elif kind == 3:
            ov.text(pt(), "Ab3", font, color)
        else:
            ov.rounded_fill(pt() + pt(), int(rng.integers(0, 12)), color, alpha)

    for i in range(n):
        if i % 3 == 0:
            one()
        else:
            with ov.layer():
                one()
        if i % 7 == 6:
            ov.flush(int(rng.choice([77, 255, 140])), keep255=bool(i % 2))
        if i % 14 == 13:
            ov.flush(255)  # right after a flush: nothing pending, nothing emitted
    return ov


@pytest.mark.parametrize("h,w,tile", [(37, 53, 32), (64, 32, 32), (130, 67, 32), (45, 70, 8), (1, 40, 32), (40, 1, 32)])
def test_binned_render_equals_sequential_render(h, w, tile):
    ov = _layered_overlay(h + w, h, w)
    data = ov.build(h, w, tile=tile)
    cmds, atlas, offsets, lists = data["cmds"], data["atlas"], data["tile_offsets"], data["tile_cmds"]
    kinds = cmds[:, 0] & 0xFF
    assert len(cmds) == len(ov) and set(kinds.tolist()) == {0, 1, 2, 3, 4}
    assert ((cmds[:, 0] & L) != 0).sum() >= 10 and not (cmds[kinds == vz.FLUSH, 0] & L).any()
    listed = [set() for _ in range(len(cmds))]
    for t in range(len(offsets) - 1):
        for i in lists[offsets[t] : offsets[t + 1]]:
            listed[int(i)].add(t)
    for i, cmd in enumerate(cmds):
        assert listed[i] == _tiles_of_bbox(*lref.box_of(cmd), h, w, tile), f"command {i}: {cmd.tolist()}"
    page = _page(h, w, 100 + h)
    whole = lref.draw_reference(page, cmds, atlas)
    assert np.array_equal(whole, lref.draw_by_tiles(page, cmds, atlas, offsets, lists, tile))
    assert np.array_equal(whole, lref.draw_reference(page, cmds, atlas, within_reach=True))
    assert not np.array_equal(whole, page)
    # the layer matters: the same records with the flag stripped draw another picture
    plain = cmds.copy()
    plain[:, 0] &= 0xFF
    assert not np.array_equal(whole, lref.draw_reference(page, plain, atlas))


def test_flush_box_is_the_union_of_the_layer_commands_since_the_last_flush():
    ov = vz.Overlay()
    font = vz.load_font(None, 12)
    ov.fill((0, 0, 99, 99), (1, 2, 3))  # on the canvas: not part of any flush box
    ov.flush(200)
    assert len(ov) == 1  # nothing in the layer: nothing emitted
    with ov.layer():
        ov.fill((30, 40, 50, 60), (9, 9, 9))
        ov.segment((10, 45), (20, 70), (9, 9, 9), 5)   # reaches (5 + 1) // 2 = 3 beyond its end points
        ov.rounded_fill((35, 20, 45, 30), 4, (9, 9, 9))
        ov.text((60, 50), "Ag", font, (9, 9, 9))
        ov.flush(77, keep255=True)                      # inside the context: still a plain record
    ov.rectangle((0, 0, 5, 5), (4, 4, 4), 1)
    with ov.layer():
        ov.fill((-50, 70, 20000, 75), (8, 8, 8))
    ov.flush(255)
    ov.flush(255)
    with ov.layer():
        ov.fill((1, 1, 2, 2), (7, 7, 7))  # never flushed: recorded, dropped by the kernel at the end of each tile
    cmds = np.asarray(_cmds(ov))
    kinds, flagged = cmds[:, 0] & 0xFF, (cmds[:, 0] & L) != 0
    first, second = np.flatnonzero(kinds == vz.FLUSH)
    assert (kinds == vz.FLUSH).sum() == 2 and not flagged[[first, second]].any()
    assert flagged[1:first].all() and first >= 5 and not flagged[first + 1] and flagged[-1]
    x0, y0, x1, y1 = (v[1:first] for v in vz.command_bounds(cmds))
    assert cmds[first, 5:10].tolist() == [int(x0.min()), int(y0.min()), int(x1.max()), int(y1.max()), 1]
    assert cmds[first, 5:7].tolist() == [7, 20] and cmds[first, 4] == 77
    assert cmds[first, 7] == cmds[first - 1, 5] + cmds[first - 1, 7] - 1  # the right edge is the last glyph's last column
    # only what came after the first flush, clipped into the coordinate range like every box
    assert cmds[second, 4:10].tolist() == [255, -50, 70, 16383, 75, 0]


def test_clamping_knows_the_new_kinds():
    for recorder in (vz.Overlay, vz.RunOverlay):
        ov = recorder()
        with ov.layer():
            ov.rounded_fill((-30000, 5, 30000, 40000), 50000, (300, -4, 7), alpha=999)
            ov.rectangle((-30000, 5, 30000, 9), (1, 2, 3), 2)
        ov.flush(400, keep255=True)
        ov.rounded_fill((1, 2, 3, 4), -5, (1, 1, 1))
        got = ov._clamped().tolist()
        assert got[0] == rbox((-16383, 5, 16383, 16383), 16383, (255, 0, 7), 255, L)
        assert got[1][0] == vz.BOX | L and got[1][5:9] == [-16383, 4, 16383, 10]
        assert got[2] == flush((-16383, 4, 16383, 16383), 255, 1)
        assert got[3] == rbox((1, 2, 3, 4), 0, (1, 1, 1))
        x0, y0, x1, y1 = vz.command_bounds(np.asarray(got))
        assert [int(v[2]) for v in (x0, y0, x1, y1)] == [-16383, 4, 16383, 16383]
    ov = vz.RunOverlay()
    with ov.layer(), pytest.raises(NotImplementedError):
        ov.text((0, 0), "a", vz.load_font(None, 12), (1, 2, 3))
    # a word 0 with a stray bit has no bounds and is listed in no tile
    stray = np.asarray([box((0, 0, 9, 9)), box((0, 0, 9, 9)), box((0, 0, 9, 9))])
    stray[0, 0], stray[1, 0] = vz.BOX | 0x200, -1
    assert [lref.box_of(c) for c in stray] == [None, None, (0, 0, 9, 9)]
    offsets, lists = vz.bin_commands(stray, 20, 20, 32)
    assert lists.tolist() == [2]


# ------------------------------------------------------------------------------------------------------------- rounded boxes
def _mask(cmd, h=40, w=40):
    return lref.rbox_coverage(cmd, (0, h, 0, w)) > 0


def test_rounded_box_coverage():
    # r = 0: the filled box
    assert np.array_equal(_mask(rbox((5, 6, 30, 20), 0, (1, 1, 1))), ref.coverage(box((5, 6, 30, 20)), None, (0, 40, 0, 40)) > 0)
    # r beyond half the shorter side is clamped to it: (20 - 6) // 2 = 7
    assert np.array_equal(_mask(rbox((5, 6, 30, 20), 1000, (1, 1, 1))), _mask(rbox((5, 6, 30, 20), 7, (1, 1, 1))))
    assert not np.array_equal(_mask(rbox((5, 6, 30, 20), 7, (1, 1, 1))), _mask(rbox((5, 6, 30, 20), 6, (1, 1, 1))))
    # the corner rule by hand, r = 3 on a 10 x 10 box at the origin: the corner circle is centred on (3, 3)
    m = _mask(rbox((0, 0, 9, 9), 3, (1, 1, 1)))
    assert m[:4, :4].astype(int).tolist() == [[0, 0, 0, 1], [0, 1, 1, 1], [0, 1, 1, 1], [1, 1, 1, 1]]
    assert np.array_equal(m[:10, :10], m[:10, :10][::-1, ::-1]) and np.array_equal(m[:10, :10], m[:10, :10].T) and not m[10:].any()
    assert m[3:7, :10].all() and m[:10, 3:7].all()
    # a 1 x 1 box is one pixel whatever r says; an inverted box is nothing
    one = _mask(rbox((7, 8, 7, 8), 5, (1, 1, 1)))
    assert one.sum() == 1 and one[8, 7]
    assert not _mask(rbox((9, 9, 3, 3), 2, (1, 1, 1))).any()
    # through the builder: corners in any order, the alpha in word 4
    ov = vz.Overlay()
    ov.rounded_fill((30, 20, 5, 6), 4, (1, 2, 3), alpha=200)
    assert _cmds(ov) == [rbox((5, 6, 30, 20), 4, (1, 2, 3), 200)]
    page = _page(40, 40, 3)
    got = lref.draw_reference(page, _cmds(ov))
    want = ref.blend(page.astype(np.int64), (1, 2, 3), np.where(_mask(rbox((5, 6, 30, 20), 4, (1, 1, 1))), 200, 0))
    assert np.array_equal(got, want.astype(np.uint8))


# ----------------------------------------------------------------------------------------------------------- tint semantics
def test_overlapping_cells_are_tinted_once():
    page = _page(30, 40, 4)
    a, b = (2, 3, 20, 15), (12, 9, 35, 25)  # overlap: x 12..20, y 9..15
    cmds = [box(a, color=(255, 128, 0), flag=L), box(b, color=(0, 255, 0), flag=L), flush((2, 3, 35, 25), 77)]
    got = lref.draw_reference(page, cmds).astype(np.int64)
    p = page.astype(np.int64)
    once = lambda colour: (np.asarray(colour) * 77 + p * 178 + 127) // 255  # noqa: E731
    assert np.array_equal(got[9:16, 12:21], once((0, 255, 0))[9:16, 12:21])      # the later colour, blended ONCE
    assert np.array_equal(got[3:9, 2:21], once((255, 128, 0))[3:9, 2:21])
    assert np.array_equal(got[16:26, 12:36], once((0, 255, 0))[16:26, 12:36])
    assert np.array_equal(got[26:], p[26:]) and np.array_equal(got[:, :2], p[:, :2])
    twice = ref.draw_reference(page, [box(a, color=(255, 128, 0), a=77), box(b, color=(0, 255, 0), a=77)])
    assert not np.array_equal(got[9:16, 12:21], twice[9:16, 12:21])             # what sequential alpha boxes would do
    # keep255: a channel whose tint is exactly 255 keeps the page's byte - per channel
    kept = lref.draw_reference(page, cmds[:2] + [flush((2, 3, 35, 25), 77, keep255=1)]).astype(np.int64)
    assert np.array_equal(kept[3:9, 2:21, 0], p[3:9, 2:21, 0]) and np.array_equal(kept[3:9, 2:21, 1:], once((255, 128, 0))[3:9, 2:21, 1:])
    assert np.array_equal(kept[9:16, 12:21, 1], p[9:16, 12:21, 1]) and np.array_equal(kept[9:16, 12:21, 0], once((0, 255, 0))[9:16, 12:21, 0])
    # a partly transparent second cell blends INSIDE the layer: colour towards the new one, coverage towards 255
    soft = lref.draw_reference(page, [box(a, color=(200, 100, 0), a=100, flag=L), box(a, color=(0, 50, 250), a=128, flag=L),
                                      flush(a, 255)]).astype(np.int64)
    colour = [(0 * 128 + 200 * 127 + 127) // 255, (50 * 128 + 100 * 127 + 127) // 255, (250 * 128 + 0 * 127 + 127) // 255]
    cov = (255 * 128 + 100 * 127 + 127) // 255
    assert np.array_equal(soft[5, 5], (np.asarray(colour) * cov + p[5, 5] * (255 - cov) + 127) // 255)


def test_a_layer_is_flushed_once_or_dropped():
    page = _page(30, 40, 5)
    paint = [box((2, 3, 20, 15), color=(10, 20, 30), flag=L), seg(0, 0, 39, 29, 3, (200, 0, 0), flag=L)]
    assert np.array_equal(lref.draw_reference(page, paint), page)                       # no flush: the page is unchanged
    once = lref.draw_reference(page, paint + [flush((0, 0, 39, 29), 200)])
    assert not np.array_equal(once, page)
    assert np.array_equal(lref.draw_reference(page, paint + [flush((0, 0, 39, 29), 200)] * 2), once)  # the second draws nothing
    assert np.array_equal(lref.draw_reference(page, paint + [flush((0, 0, 39, 29), 200, flag=L)]), page)  # a flagged FLUSH
    # a flush box smaller than what was painted: the rest stays in the layer for the next flush
    part = lref.draw_reference(page, paint + [flush((0, 0, 10, 29), 200)])
    assert np.array_equal(part[:, :11], once[:, :11]) and np.array_equal(part[:, 11:], page[:, 11:])
    assert np.array_equal(lref.draw_reference(page, paint + [flush((0, 0, 10, 29), 200), flush((0, 0, 39, 29), 200)]), once)


# ------------------------------------------------------------------------------------------------- the four public builders
def _cell(cid, b, role):
    return SimpleNamespace(id=cid, box=list(b), role=role, contents="")


def _tiny_table():
    cells = [_cell("r0c0", (10, 10, 50, 50), "header"), _cell("r0c1", (50, 10, 90, 50), "cell"), _cell("r1c0", (10, 50, 50, 90), "cell"),
             _cell("grp0", (5, 5, 95, 95), "group"), _cell("x0", (60, 60, 80, 80), "hole")]
    kv = SimpleNamespace(id="kv0", key=["r0c0", "gone"], value="r0c1")
    return SimpleNamespace(id="t0", box=[5, 5, 95, 95], cells={c.id: c for c in cells}, kv_items=[kv], grids=[])


def _recorded(fn, *args):
    ov = vz.Overlay()
    fn(ov, *args)
    return _cmds(ov, 200, 200)


def test_cell_detector_visualizer_commands():
    table = _tiny_table()
    ov1, ov2 = vz.Overlay(), vz.Overlay()
    vz._cell_commands(ov1, table.cells.values(), ov2)
    header, cell, hole = (0, 255, 0), (255, 128, 0), (200, 200, 200)
    assert _cmds(ov1, 200, 200) == [
        box((10, 10, 50, 50), color=header, flag=L), box((50, 10, 90, 50), color=cell, flag=L), box((10, 50, 50, 90), color=cell, flag=L),
        flush((10, 10, 90, 90), 77, keep255=1),
        outline((10, 10, 50, 50), 2, header), outline((50, 10, 90, 50), 2, cell), outline((10, 50, 50, 90), 2, cell),
        outline((60, 60, 80, 80), 2, hole)]
    assert _cmds(ov2, 200, 200) == [outline((5, 5, 95, 95), 2, (255, 255, 0))]
    # the shared border column x = 50 and the shared row y = 50 carry ONE tint: the later cell's
    page = np.full((100, 100, 3), 200, np.uint8)
    got = lref.draw_reference(page, _cmds(ov1, 100, 100)[:4])
    assert got[30, 50].tolist() == [200, (128 * 77 + 200 * 178 + 127) // 255, (0 * 77 + 200 * 178 + 127) // 255]
    assert got[50, 30].tolist() == got[30, 50].tolist() and got[30, 30].tolist() == [(200 * 178 + 127) // 255, 200, (200 * 178 + 127) // 255]


def test_kv_items_visualizer_commands():
    green = (0, 255, 0)
    # (30, 30) -> (70, 30): the centres already share the band's middle; 40 px long, tip min(0.2, 12 / 40) * 40 = 8 px
    assert _recorded(vz._kv_commands, _tiny_table()) == [
        seg(30, 30, 70, 30, 2, green), seg(64, 24, 70, 30, 2, green), seg(64, 36, 70, 30, 2, green)]
    # a value cell that spans two rows: the arrow stays horizontal, in the middle of the rows the two cells share
    table = _tiny_table()
    table.cells["r0c1"].box = [110, 20, 150, 120]
    assert _recorded(vz._kv_commands, table)[0] == seg(30, 35, 130, 35, 2, green)
    # a chain of two keys, the second below the first (same centre column): a vertical link, then a horizontal one
    table = _tiny_table()
    table.kv_items[0].key = ["r0c0", "r1c0"]
    table.cells["r0c1"].box = [50, 50, 90, 90]
    got = _recorded(vz._kv_commands, table)
    assert [c[5:9] for c in got[::3]] == [[30, 30, 30, 70], [30, 70, 70, 70]] and len(got) == 6
    table.kv_items[0].value = "gone"
    assert len(_recorded(vz._kv_commands, table)) == 3
    table.kv_items[0].key = "r0c0"  # a single key given as a string, value missing: no link
    assert _recorded(vz._kv_commands, table) == []


def test_dag_visualizer_commands():
    from yomitoku_amd.utils.graph import OrderedDiGraph

    dag = OrderedDiGraph()
    dag.add_node("a", bbox=(10, 10, 50, 50))
    dag.add_node("b", bbox=(110, 20, 150, 80))
    dag.add_node("c", bbox=(20, 110, 80, 150))
    dag.add_edge("a", "b", dir="R")
    dag.add_edge("b", "a", dir="L")
    dag.add_edge("a", "c", dir="D")
    dag.add_edge("c", "a", dir="U")
    green, other = (0, 255, 0), (255, 0, 0)
    # R: y moves to the middle of the shared rows 20..50; D: x to the middle of the shared columns 20..50.  Both are 100 px
    # long: tip min(0.2, 12 / 100) * 100 = 12 px, its strokes end at 12 / sqrt 2 = 8.49 px from the head on either axis
    assert _recorded(vz._dag_commands, dag) == [
        seg(30, 35, 130, 35, 2, green), seg(122, 27, 130, 35, 2, green), seg(122, 43, 130, 35, 2, green),
        seg(35, 30, 35, 130, 2, other), seg(43, 122, 35, 130, 2, other), seg(27, 122, 35, 130, 2, other)]
    lone = OrderedDiGraph()
    lone.add_node("a", bbox=(10, 10, 50, 50))
    lone.add_node("b", bbox=(110, 60, 150, 80))  # an R edge without shared rows is drawn centre to centre
    lone.add_edge("a", "b", dir="R")
    assert _recorded(vz._dag_commands, lone)[0] == seg(30, 30, 130, 70, 2, green)


def test_cell_id_visualizer_commands():
    table = _tiny_table()
    table.cells["r1c0"].id = None
    font = vz.load_font(None, 14)
    as_list = SimpleNamespace(cells=list(table.cells.values()))
    got = _recorded(vz._cell_id_commands, [table, as_list], font, 14)
    assert got[: len(got) // 2] == [c[:5] + [v for v in c[5:]] for c in got[len(got) // 2 :]]  # dict or list: the same drawing
    got = got[: len(got) // 2]
    chips = [i for i, c in enumerate(got) if c[0] == vz.RBOX]
    assert len(chips) == 3 and chips[0] == 0  # header, cell and hole; not the group, not the cell without id
    for k, (i, cell) in enumerate(zip(chips, (table.cells["r0c0"], table.cells["r0c1"], table.cells["x0"]))):
        glyphs = got[i + 1 : chips[k + 1] if k + 1 < len(chips) else len(got)]
        assert len(glyphs) == len(cell.id) and all(g[:5] == [vz.GLYPH, 255, 255, 255, 255] for g in glyphs)
        chip = got[i]
        assert chip[:5] == [vz.RBOX, 40, 40, 40, 200] and chip[5:7] == [cell.box[0] + 2, cell.box[1] + 2] and chip[9] == 2  # pad = radius = max(2, 14 // 5)
        left, top = min(g[5] for g in glyphs), min(g[6] for g in glyphs)
        right, bottom = max(g[5] + g[7] for g in glyphs), max(g[6] + g[8] for g in glyphs)
        assert [left - 2, top - 2, right + 2, bottom + 2] == chip[5:9]  # the placed glyphs' box plus the pad on every side
    assert vz.text_box(font, " ") == (0, 0, 0, 0) and vz.text_box(font, "") == (0, 0, 0, 0)


def test_semantic_layout_order():
    """Tables, then paragraphs; per table tint, flush, outlines, kv arrows, grid boxes; the graphs last."""
    from yomitoku_amd.utils.graph import OrderedDiGraph

    table = _tiny_table()
    table.grids = [SimpleNamespace(box=[10, 10, 90, 50])]
    para = SimpleNamespace(id="p0", box=[100, 120, 180, 150])
    dag = OrderedDiGraph()
    dag.add_node("a", bbox=(10, 10, 50, 50))
    dag.add_node("b", bbox=(50, 10, 90, 50))
    dag.add_edge("a", "b", dir="R")
    results = SimpleNamespace(tables=[table], paragraphs=[para], words=[])
    got = _recorded(vz._semantic_layout_commands, results, [dag])
    n_t, n_p = len("Table: t0") - 1, len("Paragraph: p0") - 1  # a space has no glyph
    assert got[0] == outline((5, 5, 95, 95), 2, (0, 255, 0)) and all(g[:4] == [vz.GLYPH, 255, 0, 0] for g in got[1 : 1 + n_t])
    at = 1 + n_t
    assert got[at] == outline((100, 120, 180, 150), 2, (0, 255, 0))
    at += 1 + n_p
    kinds = [c[0] for c in got[at:]]
    assert kinds == [vz.BOX | L] * 3 + [vz.FLUSH] + [vz.BOX] * 4 + [vz.SEG] * 3 + [vz.BOX] + [vz.SEG] * 3
    assert got[at + 11] == outline((10, 10, 90, 50), 3, (255, 0, 0))
    font = vz.load_font(None, 19)
    assert min(g[6] + g[8] for g in got[1 : 1 + n_t]) <= 5 - 10 and got[1][5] >= 5  # the label sits on a baseline 10 px above the box
    assert max(g[6] + g[8] for g in got[1 : 1 + n_t]) <= 5 - 10 + font[0].getmetrics()[1] + 1


def test_semantic_ocr_commands():
    """Per word: its quad as four segments of t = 1 in green, then its text - a horizontal word from quad[0] + (0, -size), a
    vertical one from quad[0] + (-size, 0) running down - in the recogniser's colour; words follow one another."""
    font = vz.load_font(None, 12)
    words = [SimpleNamespace(points=[[10.7, 40.2], [60, 40], [60, 55], [10, 55]], content="Ab", direction="horizontal"),
             SimpleNamespace(points=[[80, 20], [95, 20], [95, 70], [80, 70]], content="xy", direction="vertical"),
             SimpleNamespace(points=[[1, 2], [3, 2], [3, 4], [1, 4]], content="", direction="horizontal")]
    got = _recorded(vz._semantic_ocr_commands, SimpleNamespace(words=words), font, 12, (255, 0, 9))
    green = (0, 255, 0)
    quads = [[(10, 40), (60, 40), (60, 55), (10, 55)], [(80, 20), (95, 20), (95, 70), (80, 70)], [(1, 2), (3, 2), (3, 4), (1, 4)]]
    text = vz.Overlay()
    text.text((10, 28), "Ab", font, (255, 0, 9))
    text.text((68, 20), "xy", font, (255, 0, 9), direction="vertical")
    glyphs = _cmds(text, 200, 200)
    assert len(glyphs) == 4 and glyphs[3][6] - glyphs[2][6] in range(6, 19)  # the second vertical character a font size further down
    want = [seg(*q[k], *q[(k + 1) % 4], 1, green) for k in range(4) for q in quads[:1]] + glyphs[:2]
    want += [seg(*quads[1][k], *quads[1][(k + 1) % 4], 1, green) for k in range(4)] + glyphs[2:]
    want += [seg(*quads[2][k], *quads[2][(k + 1) % 4], 1, green) for k in range(4)]
    strip = lambda cmds: [c[:9] + c[10:] if c[0] == vz.GLYPH else c for c in cmds]  # noqa: E731 - word 9 is the atlas offset of THAT drawing
    assert strip(got) == strip(want)
    assert [c[9] for c in got if c[0] == vz.GLYPH] == sorted(c[9] for c in got if c[0] == vz.GLYPH)


# ---------------------------------------------------------------------------------------------------------------------- API
def test_cell_detector_accepts_visualize():
    from yomitoku_amd.table_cell_detector import CellDetector

    det = CellDetector.__new__(CellDetector)
    det.visualize = True
    det._cfg = SimpleNamespace(data=SimpleNamespace(img_size=(960, 960)))
    assert det(np.zeros((8, 8, 3), np.uint8), []) == []
    assert det.detect_pages([], []) == []


def test_table_semantic_parser_draws_per_call():
    import inspect

    from yomitoku_amd import TableSemanticParser

    with pytest.raises(NotImplementedError, match="visualize=False only.*overlays=True"):
        TableSemanticParser(visualize=True)
    parser = TableSemanticParser.__new__(TableSemanticParser)
    assert parser.parse_pages([], overlays=True) == [] and parser.parse_pages([]) == []
    for fn in (TableSemanticParser.__call__, TableSemanticParser.parse_pages):
        assert inspect.signature(fn).parameters["overlays"].default is False
    assert inspect.signature(TableSemanticParser.semantic_stage).parameters["dags"].default is None
    for name in ("cell_detector_visualizer", "cell_id_visualizer", "kv_items_visualizer", "dag_visualizer"):
        assert inspect.signature(getattr(vz, name)).parameters["to_host"].default is True


def test_semantic_stage_hands_out_the_grid_graphs():
    """A 2 x 2 grid of cells under one grid region: `dags` collects its graph, and the results do not depend on the keyword."""
    from yomitoku_amd.schemas import CellSchema, OCRSchema, RegionSchema, TableDetectorSchema
    from yomitoku_amd.table_semantic_parser import TableSemanticParser

    def table():
        cells = [CellSchema(id=f"c{k}", box=[10 + 100 * (k % 2), 10 + 40 * (k // 2), 110 + 100 * (k % 2), 50 + 40 * (k // 2)],
                            role="header" if k < 2 else "cell", contents=None, row=None, col=None, row_span=None, col_span=None) for k in range(4)]
        return TableDetectorSchema(id=None, box=[10, 10, 210, 90], role=None, cells=cells, kv_regions=[],
                                   grid_regions=[RegionSchema(id=None, box=[5, 5, 215, 95], role="grid", score=0.9)])

    parser = TableSemanticParser.__new__(TableSemanticParser)
    dags = []
    with_graphs = parser.semantic_stage(OCRSchema(words=[]), [table()], [], dags=dags)
    without = parser.semantic_stage(OCRSchema(words=[]), [table()], [])
    assert with_graphs.model_dump() == without.model_dump()
    assert len(dags) == sum(len(t.grids) for t in with_graphs.tables) == 1
    dirs = sorted(d["dir"] for _, _, d in dags[0].edges())
    assert "R" in dirs and "D" in dirs and all("bbox" in dags[0].nodes[n] for n in dags[0].nodes)
    assert any(c[0] == vz.SEG for c in _recorded(vz._dag_commands, dags[0]))
