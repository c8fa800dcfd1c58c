"""The host half of serve(overlays=True) without a GPU: the run recorder and the wave builder of
yomitoku_amd/utils/visualizer.py against the per-page Overlay (whose records the existing renderer draws), through the
restatement of the device's layout and bounds rules in tests/overlay_wave_ref.py."""
import numpy as np
import pytest

from tests import overlay_wave_ref as wref
from yomitoku_amd.utils import visualizer as V

TILE = 32  # build_wave only numbers tiles with it; the library's value is checked on the GPU


@pytest.fixture(autouse=True)
def _tile(monkeypatch):
    monkeypatch.setattr(V, "overlay_tile", lambda: TILE)


def _fonts():
    return V.load_font(None, 12), V.load_font(None, 24)


# name -> [(xy, string, font index, direction, anchor)]
TEXT_CASES = {
    "horizontal": [((5, 7), "Agjy12", 0, "horizontal", "la")],
    "vertical": [((40, 3), "Tate", 1, "vertical", "la")],
    "anchor_ls": [((9, 60), "[1, 2] (1x1)", 0, "horizontal", "ls")],
    "space": [((3, 3), "a b  c", 0, "horizontal", "la")],
    "spaces_only": [((3, 3), "   ", 0, "horizontal", "la")],
    "empty": [((3, 3), "", 0, "horizontal", "la"), ((4, 30), "x", 0, "horizontal", "la")],
    "non_bmp": [((3, 3), "a\U0001F600b\U00020000", 1, "horizontal", "la")],
    "twice": [((3, 3), "same string", 0, "horizontal", "la"), ((3, 40), "same string", 0, "horizontal", "la")],
    "clamp": [((16370, -16390), "push right", 1, "horizontal", "la"), ((-16400, 16300), "down", 1, "vertical", "la"),
              ((40000, 5), "gone", 0, "horizontal", "ls")],
    "two_fonts": [((3, 3), "small", 0, "horizontal", "la"), ((3, 30), "LARGE", 1, "vertical", "ls")],
}


def _draw_both(case, store):
    fonts = _fonts()
    old, new = V.Overlay(), V.RunOverlay()
    for ov in (old, new):
        ov.rectangle((2, 2, 50, 40), (1, 2, 3), 2)  # text slots do not start at record 0
        for xy, string, fi, direction, anchor in TEXT_CASES[case]:
            ov.text(xy, string, fonts[fi], (10 * fi, 200, 30), direction=direction, anchor=anchor)
        ov.segment((0, 0), (9, 9), (9, 9, 9), 3)
    want = old.build(70, 90, tile=TILE)
    data = V.build_wave([new], [(70, 90)], store=store)
    return want, data


def _assert_same_glyphs(want, data, store):
    glyphs, atlas = store.host()
    got = wref.layout_reference(data["cmds"], data["runs"], data["codes"], glyphs)
    got = got[got[:, 0] != -1]  # the records of characters without pixels draw nothing; Overlay never makes them
    ref = want["cmds"].astype(np.int64)
    assert got.shape == ref.shape
    cols = [c for c in range(16) if c != 9]
    assert np.array_equal(got[:, cols], ref[:, cols])
    for g, r in zip(got[got[:, 0] == V.GLYPH], ref[ref[:, 0] == V.GLYPH]):  # word 9: another atlas, the same mask bytes
        size = int(g[7] * g[8])
        assert size > 0 and np.array_equal(atlas[g[9] : g[9] + size], want["atlas"][r[9] : r[9] + size])
    return got


@pytest.mark.parametrize("case", list(TEXT_CASES))
def test_layout_rule_gives_the_records_overlay_builds(case):
    store = V.GlyphStore()  # fresh: every code point of the drawing takes the slow path once
    want, data = _draw_both(case, store)
    assert len(data["codes"]) == sum(len(t[1]) for t in TEXT_CASES[case]) == int(data["runs"][:, 2].sum())
    assert len(data["runs"]) == sum(1 for t in TEXT_CASES[case] if t[1])  # the empty string records nothing
    got = _assert_same_glyphs(want, data, store)
    if case == "clamp":
        xy = got[got[:, 0] == V.GLYPH][:, 5:7]
        assert (np.abs(xy) == wref.M).any() and (np.abs(xy) <= wref.M).all()
    if case == "spaces_only":
        assert not (got[:, 0] == V.GLYPH).any()


def test_known_glyphs_keep_their_ids_and_offsets():
    store = V.GlyphStore()
    font = V.load_font(None, 12)
    first = store.ids(font, [ord(c) for c in "hello"])
    table, atlas = store.host()
    n = store.n_glyphs
    assert n == 4 and first[2] == first[3]
    again = store.ids(font, [ord(c) for c in "hello"])  # the fast path: nothing is added
    assert np.array_equal(first, again) and store.n_glyphs == n
    more = store.ids(font, [ord(c) for c in "hello world"])  # new code points are appended, nothing moves
    table2, atlas2 = store.host()
    assert np.array_equal(more[:5], first) and store.n_glyphs > n
    assert np.array_equal(table2[:n], table) and np.array_equal(atlas2[: len(atlas)], atlas)
    other = store.ids(V.load_font(None, 24), [ord("h")])  # another font: its own glyph
    assert other[0] not in set(more.tolist())
    # second drawing through the same store: all of it on the fast path, the same records
    want, data = _draw_both("twice", store)
    grown = store.n_glyphs
    _assert_same_glyphs(want, data, store)
    want, data = _draw_both("twice", store)
    assert store.n_glyphs == grown
    _assert_same_glyphs(want, data, store)


def _mixed_commands(h, w, seed):
    rng = np.random.default_rng(seed)
    ov = V.Overlay()
    for _ in range(12):
        x0, x1 = sorted(int(v) for v in rng.integers(-40, w + 40, 2))
        y0, y1 = sorted(int(v) for v in rng.integers(-40, h + 40, 2))
        ov.segment((x0, y1), (x1, y0), (1, 2, 3), int(rng.integers(0, 7)))
        ov.rectangle((x0, y0, x1, y1), (4, 5, 6), int(rng.integers(1, 5)))
        ov.fill((x0, y0, x1, y1), (7, 8, 9), 100)
        ov.text((x0, y0), "Ag 1", V.load_font(None, 12), (0, 0, 255))
    # wholly outside, on every side, and at the coordinate bounds
    ov.segment((-30, -30), (-5, -9), (0, 0, 0), 5)
    ov.segment((w + 5, 3), (w + 50, 9), (0, 0, 0), 4)
    ov.fill((3, h + 2, 9, h + 30), (0, 0, 0))
    ov.fill((-wref.M, -wref.M, -1, wref.M), (0, 0, 0))
    ov.segment((-wref.M, -wref.M), (wref.M, wref.M), (0, 0, 0), wref.M)
    ov.text((w, 5), "off", V.load_font(None, 12), (0, 0, 255))
    ov.text((5, -40), "off", V.load_font(None, 12), (0, 0, 255))
    return ov.build(h, w, tile=TILE)["cmds"]


@pytest.mark.parametrize("size", [(1, 1), (33, 31), (100, 130)])
def test_bounds_rule_is_command_bounds_clipped_to_the_canvas(size):
    h, w = size
    cmds = _mixed_commands(h, w, 3)
    table, _, _ = wref.pack([size], [len(cmds)], TILE)
    got = wref.bounds_reference(cmds, table).astype(np.int64)
    x0, y0, x1, y1 = V.command_bounds(cmds)
    x0, y0, x1, y1 = np.maximum(x0, 0), np.maximum(y0, 0), np.minimum(x1, w - 1), np.minimum(y1, h - 1)
    valid = (x0 <= x1) & (y0 <= y1)
    assert valid.any() and (~valid).any()
    assert np.array_equal(got[:, 0] <= got[:, 2], valid)
    assert np.array_equal(got[valid], np.stack([x0, y0, x1, y1], axis=1)[valid])
    assert (got[~valid] == (1, 1, 0, 0)).all()
    # culling by that box is bin_commands' predicate: per tile the same commands, in the same order
    offsets, lists = V.bin_commands(cmds, h, w, TILE)
    tiles_x = -(-w // TILE)
    for t in range(len(offsets) - 1):
        ty, tx = divmod(t, tiles_x)
        hit = (got[:, 0] <= got[:, 2]) & (got[:, 0] <= tx * TILE + TILE - 1) & (got[:, 2] >= tx * TILE) \
            & (got[:, 1] <= ty * TILE + TILE - 1) & (got[:, 3] >= ty * TILE)
        assert np.array_equal(np.flatnonzero(hit), lists[offsets[t] : offsets[t + 1]])


def test_build_wave_numbers_canvases_commands_and_tiles():
    font = V.load_font(None, 12)
    a, b, c = V.RunOverlay(), V.RunOverlay(), V.RunOverlay()
    a.text((1, 1), "ab", font, (1, 1, 1))
    a.fill((0, 0, 3, 3), (2, 2, 2))
    c.rectangle((0, 0, 9, 9), (3, 3, 3), 1)
    c.text((1, 1), "xyz", font, (4, 4, 4), direction="vertical")
    data = V.build_wave([a, b, c], [(33, 31), (1, 70), (100, 130)], store=V.GlyphStore())
    assert data["table"].tolist() == [[0, 33, 31, 0, 3, 0], [3072, 1, 70, 3, 0, 2], [3296, 100, 130, 3, 4, 5]]
    assert data["tiles"] == 2 + 3 + 20 and data["bytes"] == 3296 + 39008
    assert data["runs"].tolist() == [[0, 0, 2, 1, 1, 0, 12, 0], [4, 2, 3, 1, 1, 1, 12, 0]]
    assert data["cmds"][:, 0].tolist() == [2, 2, 1, 1, 2, 2, 2] and data["cmds"][4:, 1:5].tolist() == [[4, 4, 4, 255]] * 3
    with pytest.raises(NotImplementedError):
        a.glyph(0, 0, np.zeros((2, 2), np.uint8), (0, 0, 0))
