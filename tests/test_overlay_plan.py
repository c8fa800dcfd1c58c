"""Host half of visualize=True (yomitoku_amd/utils/visualizer.py): the command builder, the per-tile binning and the jet table,
against the NumPy restatement of the drawing rules in tests/overlay_ref.py.  No GPU: nothing here launches."""
import logging

import numpy as np
import pytest

from tests import overlay_ref as ref
from yomitoku_amd.utils import visualizer as vz


def _random_overlay(seed, h, w, n=40):
    """A drawing of every primitive through the builder: on, across and off the canvas."""
    rng = np.random.default_rng(seed)
    ov = vz.Overlay()
    font = vz.load_font(None, 12)

    def pt():
        return int(rng.integers(-20, w + 20)), int(rng.integers(-20, h + 20))

    for _ in range(n):
        kind = int(rng.integers(0, 6))
        color = tuple(int(v) for v in rng.integers(0, 256, 3))
        alpha = int(rng.choice([0, 77, 255, int(rng.integers(1, 255))]))
        if kind == 0:
            ov.segment(pt(), pt(), color, int(rng.integers(0, 7)), alpha)
        elif kind == 1:
            ov.rectangle(pt() + pt(), color, int(rng.integers(1, 6)), alpha)
        elif kind == 2:
            ov.fill(pt() + pt(), color, alpha)
        elif kind == 3:
            ov.text(pt(), "Ab3", font, color, direction="vertical" if rng.integers(0, 2) else "horizontal")
        elif kind == 4:
            ov.arrow(pt(), pt(), color, 2, tip=float(rng.integers(0, 12)))
        else:
            ov.polyline([pt(), pt(), pt()], bool(rng.integers(0, 2)), color, int(rng.integers(1, 4)), alpha)
    return ov


def _tiles_of_bbox(x0, y0, x1, y1, h, w, tile):
    """Row-major ids of the tiles an inclusive bounding box touches, pixel by pixel of its clipped corners."""
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
    if x0 > x1 or y0 > y1:
        return set()
    tiles_x = -(-w // tile)
    return {ty * tiles_x + tx for ty in range(y0 // tile, y1 // tile + 1) for tx in range(x0 // tile, x1 // tile + 1)}


def _bbox(cmd):
    c = [int(v) for v in cmd]
    if c[0] == vz.SEG:
        pad = (c[9] + 1) // 2
        return min(c[5], c[7]) - pad, min(c[6], c[8]) - pad, max(c[5], c[7]) + pad, max(c[6], c[8]) + pad
    if c[0] == vz.BOX:
        return c[5], c[6], c[7], c[8]
    return c[5], c[6], c[5] + c[7] - 1, c[6] + c[8] - 1


@pytest.mark.parametrize("h,w,tile", [(37, 53, 32), (64, 32, 32), (130, 67, 32), (45, 70, 8), (1, 40, 32), (40, 1, 16)])
@pytest.mark.parametrize("seed", [0, 1])
def test_binned_render_equals_sequential_render(h, w, tile, seed):
    ov = _random_overlay(seed, h, w)
    data = ov.build(h, w, tile=tile)
    cmds, atlas, offsets, lists = data["cmds"], data["atlas"], data["tile_offsets"], data["tile_cmds"]
    assert cmds.dtype == np.int32 and cmds.shape[1] == 16 and len(cmds) == len(ov)
    n_tiles = -(-h // tile) * -(-w // tile)
    assert len(offsets) == n_tiles + 1 and offsets[0] == 0 and offsets[-1] == len(lists)
    assert np.all(np.diff(offsets) >= 0)
    # every command sits in exactly the tiles its bounding box touches, and every list ascends
    listed = [set() for _ in range(len(cmds))]
    for t in range(n_tiles):
        lst = lists[offsets[t] : offsets[t + 1]]
        assert np.all(np.diff(lst) > 0), f"tile {t}: list not strictly ascending"
        for i in lst:
            listed[int(i)].add(t)
    for i, cmd in enumerate(cmds):
        assert listed[i] == _tiles_of_bbox(*_bbox(cmd), h, w, tile), f"command {i}: {cmd.tolist()}"
    page = np.random.default_rng(100 + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    whole = ref.draw_reference(page, cmds, atlas)
    tiled = ref.draw_by_tiles(page, cmds, atlas, offsets, lists, tile)
    assert np.array_equal(whole, tiled)
    assert not np.array_equal(whole, page)


def test_quads_become_four_segments_each():
    quads = np.random.default_rng(0).integers(0, 100, (7, 4, 2))
    ov = vz.Overlay()
    ov.polyline(quads, True, (0, 255, 0), 1)
    cmds = ov.build(100, 100, tile=32)["cmds"]
    assert len(cmds) == 28 and np.all(cmds[:, 0] == vz.SEG) and np.all(cmds[:, 9] == 1)
    assert np.all(cmds[:, 1:5] == (0, 255, 0, 255))
    for q in range(7):
        for k in range(4):
            assert cmds[4 * q + k, 5:9].tolist() == quads[q, k].tolist() + quads[q, (k + 1) % 4].tolist()
    open_ov = vz.Overlay()
    open_ov.polyline(quads[0], False, (1, 2, 3))
    assert len(open_ov) == 3


@pytest.mark.parametrize("t", [1, 2, 3, 5])
def test_outline_boxes_follow_the_thickness_rule(t):
    ov = vz.Overlay()
    ov.rectangle((10, 20, 50, 70), (9, 8, 7), t, alpha=77)
    (cmd,) = ov.build(100, 100, tile=32)["cmds"]
    assert cmd[0] == vz.BOX and cmd[1:5].tolist() == [9, 8, 7, 77]
    assert cmd[5:9].tolist() == [10 - t // 2, 20 - t // 2, 50 + t // 2, 70 + t // 2]
    assert cmd[9:13].tolist() == [10 + (t + 1) // 2, 20 + (t + 1) // 2, 50 - (t + 1) // 2, 70 - (t + 1) // 2]


def test_filled_rectangle_has_an_empty_inner_box():
    ov = vz.Overlay()
    ov.fill((50, 70, 10, 20), (1, 2, 3), alpha=128)  # corners in any order, as cv2.rectangle takes them
    (cmd,) = ov.build(100, 100, tile=32)["cmds"]
    assert cmd[5:9].tolist() == [10, 20, 50, 70] and cmd[9] > cmd[11] and cmd[4] == 128


def test_arrow_tips():
    ov = vz.Overlay()
    ov.arrow((5, 5), (5, 5), (0, 0, 255), 2, tip=10)
    assert len(ov) == 1  # a zero-length arrow has no tip
    ov = vz.Overlay()
    ov.arrow((0, 0), (100, 0), (0, 0, 255), 2, tip=10)
    cmds = ov.build(50, 200, tile=32)["cmds"]
    assert len(cmds) == 3 and np.all(cmds[:, 9] == 2)
    assert cmds[0, 5:9].tolist() == [0, 0, 100, 0]
    # +-45 degrees around the reversed direction: 10 / sqrt 2 = 7.07 -> 7
    assert cmds[1, 5:9].tolist() == [93, -7, 100, 0]
    assert cmds[2, 5:9].tolist() == [93, 7, 100, 0]


def test_coordinates_clamp():
    ov = vz.Overlay()
    ov.segment((-50000, 3), (70000, 99999), (1, 1, 1), thickness=1 << 20)
    ov.rectangle((-40000, -40000, 40000, 40000), (1, 1, 1), 2)
    ov.fill((-40000, 5, 40000, 6), (1, 1, 1))
    ov.glyph(99999, -99999, np.full((2, 2), 255, np.uint8), (1, 1, 1))
    cmds = ov.build(64, 64, tile=32)["cmds"]
    assert cmds[0, 5:10].tolist() == [-16383, 3, 16383, 16383, 16383]
    assert cmds[1, 5:13].tolist() == [-16383, -16383, 16383, 16383, -16383, -16383, 16383, 16383]
    assert cmds[2, 5:9].tolist() == [-16383, 5, 16383, 6]
    assert cmds[3, 5:7].tolist() == [16383, -16383]
    assert np.abs(cmds[:, 5:9]).max() <= 16383


def test_text_layout_horizontal_and_vertical():
    font, key = vz.load_font(None, 12)
    text = "Ag 1"
    ov = vz.Overlay()
    end = ov.text((30, 40), text, (font, key), (255, 0, 0))
    data = ov.build(100, 200, tile=32)
    cmds, atlas = data["cmds"], data["atlas"]
    pen, k = 30, 0
    for ch in text:
        mask = font.getmask(ch, mode="L")
        gw, gh = mask.size
        if gw and gh:
            ox, oy = font.getbbox(ch)[:2]
            assert cmds[k, 0] == vz.GLYPH and cmds[k, 5:9].tolist() == [pen + ox, 40 + oy, gw, gh]
            assert cmds[k, 10] == gw
            got = atlas[cmds[k, 9] : cmds[k, 9] + gw * gh].reshape(gh, gw)
            assert np.array_equal(got, np.frombuffer(bytes(mask), np.uint8).reshape(gh, gw))
            k += 1
        pen += round(font.getlength(ch))
    assert k == len(cmds) == 3 and end == (pen, 40)  # the space advances the pen and draws nothing
    # vertical: the pen moves down by the font size, one glyph per character
    ov = vz.Overlay()
    ov.text((30, 40), "AgA", (font, key), (255, 0, 0), direction="vertical")
    data = ov.build(200, 100, tile=32)
    cmds = data["cmds"]
    for k, ch in enumerate("AgA"):
        ox, oy = font.getbbox(ch)[:2]
        assert cmds[k, 5:7].tolist() == [30 + ox, 40 + 12 * k + oy]
    assert cmds[0, 9] == cmds[2, 9], "a glyph used twice is packed once"
    # baseline anchor (cv2.putText's origin): the line's top is the ascent above the point
    ov = vz.Overlay()
    ov.text((30, 40), "A", (font, key), (255, 0, 0), anchor="ls")
    assert ov.build(100, 100, tile=32)["cmds"][0, 6] == 40 - font.getmetrics()[0] + font.getbbox("A")[1]


def test_missing_font_falls_back_and_warns_once(monkeypatch, caplog):
    monkeypatch.setattr(vz, "_font_warned", False)
    with caplog.at_level(logging.WARNING, logger="yomitoku_amd.utils.visualizer"):
        f1, k1 = vz.load_font("/no/such/font.ttf", 18)
        f2, k2 = vz.load_font("/no/such/other.ttf", 18)
        vz.load_font(None, 18)  # asking for the built-in font is not a fallback
    assert len([r for r in caplog.records if "not found" in r.getMessage()]) == 1
    assert k1 == k2 == (None, 18) and f1 is f2 and f1.getmask("A", mode="L").size[0] > 0


def test_jet_table_is_pinned_to_its_formula():
    jet = vz.jet_table()
    assert jet.dtype == np.uint8 and jet.shape == (256, 3)
    assert np.array_equal(jet, ref.jet_reference())
    assert jet[0].tolist() == [128, 0, 0] and jet[255].tolist() == [0, 0, 128]  # 127.5 rounds to the even 128
    assert jet[:, 1].max() == 255 and int(jet[:, 1].argmax()) in range(96, 160)


def test_restatement_blend_end_points():
    """a = 255 overwrites, a = 0 leaves the pixel, anything else is the rounded mix."""
    page = np.full((4, 4, 3), 200, np.uint8)
    box = lambda a: [vz.BOX, 10, 20, 30, a, 0, 0, 3, 3, 1, 1, 0, 0, 0, 0, 0]  # noqa: E731
    assert np.all(ref.draw_reference(page, [box(255)]) == (10, 20, 30))
    assert np.array_equal(ref.draw_reference(page, [box(0)]), page)
    assert np.all(ref.draw_reference(page, [box(77)])[0, 0] == [(c * 77 + 200 * 178 + 127) // 255 for c in (10, 20, 30)])
