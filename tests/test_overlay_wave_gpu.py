"""ymk_overlay_layout and ymk_draw_overlay_pages (yomitoku_amd/csrc/ymk_overlay.hip): the layout and the bounds as integers
against tests/overlay_wave_ref.py, the canvases bit for bit against tests/overlay_ref.py and against the per-page path
(Overlay.render: host binning + ymk_draw_overlay).  Every case is a few thousand pixels."""
import numpy as np
import pytest
import torch

from tests import overlay_ref as ref
from tests import overlay_wave_ref as wref
from tests.test_overlay_gpu import _boxes, _glyphs, _page, _segments, box, glyph, seg
from tests.test_overlay_wave import TEXT_CASES, _draw_both
from yomitoku_amd.utils import visualizer as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def consts(dev):
    from yomitoku_amd import _lib

    lib = _lib.load()
    return int(lib.ymk_overlay_tile()), int(lib.ymk_overlay_chunk()), int(lib.ymk_overlay_cull_pass())


def _launch(pages, cmd_lists, tile, atlas=None, runs=None, codes=None, glyphs=None):
    """One wave: `pages` (host arrays) with `cmd_lists[i]` drawn over page i.  Returns (canvases, launch dict)."""
    sizes = [p.shape[:2] for p in pages]
    table, nbytes, _ = wref.pack(sizes, [len(c) for c in cmd_lists], tile)
    buf = np.full(nbytes + 64, 171, dtype=np.uint8)  # padding between and after the canvases must come back untouched
    keep = np.ones(len(buf), bool)
    for (off, h, w, *_), p in zip(table.tolist(), pages):
        buf[off : off + h * w * 3] = p.reshape(-1)
        keep[off : off + h * w * 3] = False
    cmds = np.concatenate([np.asarray(c, dtype=np.int32).reshape(-1, 16) for c in cmd_lists])
    buf_dev = torch.from_numpy(buf).to("cuda:0")
    out = V.launch_wave(buf_dev, cmds, table, runs, codes, glyphs, atlas)
    got = buf_dev.cpu().numpy()
    assert (got[keep] == 171).all(), "bytes outside the canvases were written"
    out["table"] = table
    return [got[off : off + h * w * 3].reshape(h, w, 3) for off, h, w, *_ in table.tolist()], out


def _same(got, want, what=""):
    bad = np.argwhere((got != want).any(-1))
    assert np.array_equal(got, want), f"{what}: {len(bad)} pixels differ, first at (y, x) = {bad[0].tolist()}"


# ------------------------------------------------------------------------------------------------------------ layout kernel
def _glyph_table(rng, n=40):
    """Random glyph entries; some without pixels (w or h 0), offsets into a random atlas."""
    table, at = [], 0
    for g in range(n):
        w, h = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        if g % 7 == 3:
            w = 0
        if g % 11 == 5:
            h = 0
        table.append((at, w, h, int(rng.integers(-3, 4)), int(rng.integers(-3, 9)), int(rng.integers(0, 14))))
        at += w * h
    return np.asarray(table, np.int32), rng.integers(1, 256, at, dtype=np.uint8)


def _text_slots(n, colour=(250, 10, 20)):
    rec = np.zeros((n, 16), np.int32)
    rec[:, 0], rec[:, 1:4], rec[:, 4] = 2, colour, 255
    return rec


def test_layout_runs_of_every_length_in_one_launch(consts):
    tile, _, _ = consts
    rng = np.random.default_rng(1)
    glyphs, atlas = _glyph_table(rng)
    lengths = [1, 63, 64, 300, 65, 128, 2]  # the 300 is horizontal: its pen runs into the clamp
    cmds = [np.asarray([box((0, 0, 5, 5))], np.int32)]
    runs, codes, slot = [], [], 1
    for i, n in enumerate(lengths):
        ids = rng.integers(0, len(glyphs), n)
        if n >= 63:
            ids[[5, n - 1]] = (len(glyphs), -1)  # ids outside the table: records that draw nothing and advance by 0
            ids[7] = 1 << 20
        vertical = i % 3 == 1
        pen = (16000, -20) if n == 300 else (int(rng.integers(-30, 60)), int(rng.integers(-30, 60)))  # 300: runs into the clamp
        runs.append((slot, len(codes), n, *pen, int(vertical), 11 if vertical else 0, 0))
        codes += ids.tolist()
        cmds.append(_text_slots(n))
        slot += n
    cmds.append(np.asarray([seg(1, 1, 30, 30, 2)], np.int32))
    total = slot + 1
    spare = _text_slots(4, (1, 2, 3))  # slots that only bad runs point at: they keep what the host wrote
    cmds.append(spare)
    bad_runs = [(total, 0, 5, 0, 0, 0, 0, 0),             # slots run past the array
                (total + 4, 0, 1, 0, 0, 0, 0, 0),         # first slot past the array
                (total, len(codes) - 2, 3, 0, 0, 0, 0, 0),  # codes run past the array
                (-1, 0, 2, 0, 0, 0, 0, 0), (total, -1, 2, 0, 0, 0, 0, 0), (total, 0, -3, 0, 0, 0, 0, 0), (total, 0, 0, 0, 0, 0, 0, 0),
                (2**31 - 2, 0, 4, 0, 0, 0, 0, 0), (total, 2**31 - 2, 4, 0, 0, 0, 0, 0)]
    runs = np.asarray(runs + bad_runs, np.int32)
    cmds = np.concatenate(cmds)
    page = _page(70, 90, 2)
    (got,), out = _launch([page], [cmds], tile, atlas=atlas, runs=runs, codes=np.asarray(codes, np.int32), glyphs=glyphs)
    want = wref.layout_reference(cmds, runs, codes, glyphs)
    laid = out["cmds_dev"].cpu().numpy()
    assert np.array_equal(laid, want)
    assert np.array_equal(laid[total:], spare) and (want[:, 0] == -1).sum() >= 3 * 4
    assert (np.abs(want[want[:, 0] == 2][:, 5]) == wref.M).any()
    assert np.array_equal(out["bounds_dev"].cpu().numpy(), wref.bounds_reference(want, out["table"]))
    _same(got, ref.draw_reference(page, want[want[:, 0] >= 0], atlas), "laid-out text")
    assert not np.array_equal(got, page)


@pytest.mark.parametrize("case", list(TEXT_CASES))
def test_layout_of_recorded_text(consts, case):
    """The cases of tests/test_overlay_wave.py through the recorder, the glyph store's device tensors and the kernels."""
    store = V.GlyphStore()
    want, data = _draw_both(case, store)
    page = _page(70, 90, 3)
    buf = torch.from_numpy(np.ascontiguousarray(page)).to("cuda:0").reshape(-1)
    out = V.draw_wave(buf, [_recorded(case)], [(70, 90)], store=store)
    glyphs, atlas = store.host()
    laid = wref.layout_reference(data["cmds"], data["runs"], data["codes"], glyphs)
    assert np.array_equal(out["cmds_dev"].cpu().numpy(), laid)
    assert np.array_equal(out["bounds_dev"].cpu().numpy(), wref.bounds_reference(laid, data["table"]))
    got = buf.cpu().numpy().reshape(70, 90, 3)
    _same(got, ref.draw_reference(page, want["cmds"], want["atlas"]), case)  # what Overlay's records draw


def _recorded(case):
    fonts = V.load_font(None, 12), V.load_font(None, 24)
    ov = V.RunOverlay()
    ov.rectangle((2, 2, 50, 40), (1, 2, 3), 2)
    for xy, string, fi, direction, anchor in TEXT_CASES[case]:
        ov.text(xy, string, fonts[fi], (10 * fi, 200, 30), direction=direction, anchor=anchor)
    ov.segment((0, 0), (9, 9), (9, 9, 9), 3)
    return ov


# -------------------------------------------------------------------------------------------------------------- draw kernel
def _mixed(h, w, colour=None):
    glyphs, atlas = _glyphs(h, w)
    parts = [_segments(h, w), _boxes(h, w), glyphs]
    cmds = [list(p[i]) for i in range(max(map(len, parts))) for p in parts if i < len(p)]
    if colour is not None:
        for c in cmds:
            c[1:4] = colour
            if c[0] != 2:
                c[4] = 255
    return cmds, atlas


def test_canvases_of_differing_sizes_in_one_launch(consts):
    tile, _, _ = consts
    sizes = [(1, 1), (1, 70), (33, 31), (40, 40), (100, 130)]
    pages = [_page(h, w, 20 + i) % 200 for i, (h, w) in enumerate(sizes)]  # no page byte above 199
    lists = []
    for i, (h, w) in enumerate(sizes):
        cmds, atlas = _mixed(h, w, colour=(250, 251, 252) if i == 2 else None)  # one atlas layout for all: _glyphs is size-blind
        if i != 2:
            for c in cmds:
                c[1:4] = [v % 200 for v in c[1:4]]
        lists.append([] if i == 3 else cmds)
    got, out = _launch(pages, lists, tile, atlas=atlas)
    for i, (g, p, cmds) in enumerate(zip(got, pages, lists)):
        _same(g, ref.draw_reference(p, cmds, atlas) if cmds else p, f"canvas {i}")
    assert np.array_equal(got[3], pages[3])  # zero commands: untouched
    assert (got[2] == (250, 251, 252)).all(-1).any()
    for i in (0, 1, 3, 4):  # canvas 2's colour on no other canvas
        assert not (got[i] >= 250).any()
    bounds = out["bounds_dev"].cpu().numpy()
    assert np.array_equal(bounds, wref.bounds_reference(np.concatenate([np.asarray(c).reshape(-1, 16) for c in lists]), out["table"]))


def test_long_lists_and_several_cull_passes(consts):
    tile, chunk, cull = consts
    rng = np.random.default_rng(6)

    def tiny(i, ox, oy):
        x, y = ox + int(rng.integers(2, tile - 4)), oy + int(rng.integers(2, tile - 4))
        colour = tuple(int(v) for v in rng.integers(0, 256, 3))
        if i % 3 == 0:
            return seg(x, y, x + int(rng.integers(0, 3)), y + int(rng.integers(0, 3)), int(rng.integers(1, 4)), colour, int(rng.integers(60, 256)))
        return box((x, y, x + 2, y + 2), color=colour, a=int(rng.integers(60, 256)))

    # (a) one tile hit by every one of 2 * cull + 50 > 3 * chunk commands: more hits than the LDS ring holds at once
    dense = [tiny(i, tile, 0) for i in range(2 * cull + 50)]
    # (b) more commands than two cull passes, nearly all of them elsewhere: tile (0, 0) is hit by the first and the last
    #     command only (they overlap: the order decides), tile (1, 1) by a few from the middle passes
    sparse = [tiny(i, 2 * tile, tile) for i in range(2 * cull + 40)]
    sparse[0] = box((3, 3, 20, 20), color=(255, 0, 0))
    sparse[-1] = box((10, 10, 28, 28), color=(0, 0, 255), a=140)
    for k in (cull - 1, cull, cull + 1, 2 * cull - 1, 2 * cull):
        sparse[k] = tiny(k, tile, tile)
    sparse[5] = seg(-90, -50, -20, -60, 6)  # wholly outside
    pages = [_page(2 * tile + 5, 3 * tile - 1, 7), _page(2 * tile + 5, 3 * tile - 1, 8)]
    got, _ = _launch(pages, [dense, sparse], tile)
    _same(got[0], ref.draw_reference(pages[0], dense, within_reach=True), "dense")
    _same(got[1], ref.draw_reference(pages[1], sparse, within_reach=True), "sparse")
    assert np.array_equal(got[0][tile:], pages[0][tile:]) and np.array_equal(got[0][:, :tile], pages[0][:, :tile])
    assert got[1][15, 15].tolist() != [255, 0, 0] and got[1][5, 5].tolist() == [255, 0, 0]


def test_order_decides_and_canvases_of_one_page_differ(consts):
    tile, _, _ = consts
    page = _page(37, 53, 5)
    a = box((5, 5, 30, 25), color=(255, 0, 0))
    b = seg(0, 0, 52, 36, 5, color=(0, 0, 255))
    (ab, ba, none), _ = _launch([page, page, page], [[a, b], [b, a], [seg(-9, -9, -5, -5, 2)]], tile)
    _same(ab, ref.draw_reference(page, [a, b]))
    _same(ba, ref.draw_reference(page, [b, a]))
    assert ab[15, 22].tolist() == [0, 0, 255] and ba[15, 22].tolist() == [255, 0, 0]
    assert np.array_equal(none, page)


def _random_drawing(ov, h, w, seed):
    rng = np.random.default_rng(seed)
    small, large = V.load_font(None, 12), V.load_font(None, 24)
    words = ["Ag 1", "[2, 3] (1x2)", "paragraphs", "17", "W i d e", "éü", ""]
    ov.fill((0, 0, w - 1, h // 3), (10, 20, 30), alpha=90)
    for i in range(14):
        x0, x1 = sorted(int(v) for v in rng.integers(-20, w + 20, 2))
        y0, y1 = sorted(int(v) for v in rng.integers(-20, h + 20, 2))
        colour = tuple(int(v) for v in rng.integers(0, 256, 3))
        ov.rectangle((x0, y0, x1, y1), colour, int(rng.integers(1, 4)))
        ov.text((x0, y0), words[i % len(words)], small if i % 2 else large, colour, direction="vertical" if i % 5 == 4 else "horizontal",
                anchor="ls" if i % 3 else "la")
        ov.arrow((x0, y1), (x1, y0), colour, 2, tip=float(rng.integers(0, 12)))
        ov.polyline(rng.integers(0, max(h, w), (2, 4, 2)), True, colour, 1)
    return ov


def test_wave_equals_the_per_page_path(dev):
    """The same drawings through Overlay.render (host layout, host binning, ymk_draw_overlay) and through the wave."""
    sizes = [(100, 130), (70, 45), (33, 31)]
    pages = [torch.from_numpy(_page(h, w, 30 + i)).to("cuda:0") for i, (h, w) in enumerate(sizes)]
    before = [p.cpu().numpy() for p in pages]
    want = [_random_drawing(V.Overlay(), h, w, 40 + i).render(p).cpu().numpy() for i, ((h, w), p) in enumerate(zip(sizes, pages))]
    slot = [None]
    got = V.render_wave(pages, [_random_drawing(V.RunOverlay(), h, w, 40 + i) for i, (h, w) in enumerate(sizes)], slot)
    for i, (g, w_, b) in enumerate(zip(got, want, before)):
        _same(g, w_, f"page {i}")
        assert not np.array_equal(g, b) and g.flags.owndata and g.flags.writeable
    assert all(np.array_equal(p.cpu().numpy(), b) for p, b in zip(pages, before))  # the pages are never drawn on
    # the slot's pinned buffer is reused; the arrays of the first call are the caller's and stay what they were
    pinned = slot[0]
    again = V.render_wave(pages[1:2] * 2, [V.RunOverlay(), _random_drawing(V.RunOverlay(), 70, 45, 99)], slot)  # a smaller wave
    assert slot[0] is pinned and np.array_equal(again[0], before[1]) and not np.array_equal(again[1], before[1])
    _same(got[0], want[0], "first call's array after the second call")
