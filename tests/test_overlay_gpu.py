"""ymk_draw_overlay and ymk_heatmap_blend (yomitoku_amd/csrc/ymk_overlay.hip) against the NumPy restatement of the drawing
rules in tests/overlay_ref.py: bit-exact, every case a few thousand pixels."""
import numpy as np
import pytest
import torch

from tests import overlay_ref as ref

pytestmark = pytest.mark.gpu

SEG, BOX, GLYPH = 0, 1, 2
M = 16383


def seg(x0, y0, x1, y1, t, color=(0, 255, 0), a=255):
    return [SEG, *color, a, x0, y0, x1, y1, t, 0, 0, 0, 0, 0, 0]


def box(outer, inner=(1, 1, 0, 0), color=(255, 0, 255), a=255):
    return [BOX, *color, a, *outer, *inner, 0, 0, 0]


def glyph(x, y, w, h, offset, pitch, color=(255, 0, 0)):
    return [GLYPH, *color, 0, x, y, w, h, offset, pitch, 0, 0, 0, 0, 0]


@pytest.fixture(scope="module")
def tile():
    from yomitoku_amd import _lib

    lib = _lib.load()
    return int(lib.ymk_overlay_tile()), int(lib.ymk_overlay_chunk())


def _page(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _draw(page, cmds, atlas=None):
    from yomitoku_amd.utils.visualizer import draw_commands

    canvas = torch.from_numpy(page).to("cuda:0")
    out = draw_commands(canvas, np.asarray(cmds, dtype=np.int32).reshape(-1, 16), atlas)
    assert out is canvas
    return canvas.cpu().numpy()


def _check(page, cmds, atlas=None):
    got = _draw(page, cmds, atlas)
    want = ref.draw_reference(page, cmds, atlas)
    bad = np.argwhere((got != want).any(-1))
    assert np.array_equal(got, want), f"{len(bad)} pixels differ, first at (y, x) = {bad[0].tolist()}"
    return got


def _canvases(t):
    return {"37x53": (37, 53), "one_tile": (t, t), "2tile_x_tile": (2 * t, t), "130x67": (130, 67), "row": (1, 40), "column": (40, 1)}


CANVAS_NAMES = ["37x53", "one_tile", "2tile_x_tile", "130x67", "row", "column"]


def _segments(h, w):
    cx, cy = w // 2, h // 2
    out = []
    shapes = [(cx, cy, cx, cy),                      # degenerate: P0 = P1
              (2, cy, w - 3, cy),                    # horizontal
              (cx, 1, cx, h - 2),                    # vertical
              (1, 1, min(h, w) - 2, min(h, w) - 2),  # 45 degrees
              (cx - 3, 0, cx + 3, h - 1),            # steep
              (0, cy - 2, w - 1, cy + 2),            # shallow
              (-9, cy + 3, cx, -7),                  # partly off the canvas
              (w + 5, -20, w + 40, -3),              # wholly off
              (-30, h + 10, -2, h + 4)]
    for k, s in enumerate(shapes):
        for t in (1, 2, 5, 0):
            out.append(seg(*s, t, color=(40 * k % 256, 255 - 20 * k, 17 * t), a=255 if (k + t) % 3 else 150))
    # end points at the coordinate bounds: the products of the coverage test reach 2^62
    out += [seg(-M, -M, M, M, 3, (1, 2, 3)), seg(-M, M, M, -M + h, 2, (200, 100, 50), 90), seg(M, cy, -M, cy + 1, 5, (9, 99, 199)),
            seg(-M, -M, -M, -M, 7), seg(cx, -M, cx + 1, M, 1, (255, 255, 0)), seg(M, M, M - 1, M - 3, 4)]
    return out


def _boxes(h, w):
    return [box((3, 2, w - 4, h - 3), (5, 4, w - 6, h - 5), a=255),          # an outline
            box((w // 3, h // 3, 2 * w // 3, 2 * h // 3), a=77),              # filled, blended
            box((1, 1, w // 2, h // 2), (0, 0, w, h), color=(1, 2, 3)),       # inner larger than outer: nothing
            box((-10, -10, 6, 5), (-12, 2, 3, 9), color=(0, 0, 255), a=77),   # across the corner, inner cuts a part
            box((0, 0, w - 1, h - 1), color=(9, 9, 9), a=0),                  # alpha 0 changes nothing
            box((w - 3, h - 2, w + 50, h + 50), (w - 1, 3, w - 2, 2), color=(0, 200, 0)),  # inverted inner = no hole
            box((-M, h // 2, M, h // 2), color=(250, 250, 0), a=200)]         # one row, from bound to bound


def _glyphs(h, w):
    """(commands, atlas): one 7 x 5 mask stored with pitch 9 (pitch > width) and one tight 3 x 3 mask, blitted inside the
    canvas and over each of its four edges."""
    rng = np.random.default_rng(5)
    wide = rng.integers(0, 256, (5, 9), dtype=np.uint8)
    wide[0, 0], wide[1, 1], wide[2, 2] = 255, 0, 128
    small = rng.integers(1, 256, (3, 3), dtype=np.uint8)
    atlas = np.concatenate([np.zeros(4, np.uint8), wide.reshape(-1), small.reshape(-1)])
    g = lambda x, y, c=(255, 0, 0): glyph(x, y, 7, 5, 4, 9, c)  # noqa: E731
    cmds = [g(w // 2 - 3, h // 2 - 2), g(-3, h // 2 - 2, (0, 255, 0)), g(w - 4, h // 2 - 1, (0, 0, 255)), g(w // 2 - 1, -2, (255, 255, 0)),
            g(w // 2 - 2, h - 3, (0, 255, 255)), g(-3, -2, (7, 7, 7)), g(w + 1, 0), g(0, h),
            glyph(1, 1, 3, 3, 4 + 45, 3, (128, 64, 32)), glyph(w - 2, h - 2, 3, 3, 4 + 45, 3, (32, 64, 128))]
    return cmds, atlas


@pytest.mark.parametrize("name", CANVAS_NAMES)
def test_segments_match_the_restatement(dev, tile, name):
    h, w = _canvases(tile[0])[name]
    got = _check(_page(h, w, 1), _segments(h, w))
    assert not np.array_equal(got, _page(h, w, 1))


@pytest.mark.parametrize("name", CANVAS_NAMES)
def test_boxes_match_the_restatement(dev, tile, name):
    h, w = _canvases(tile[0])[name]
    _check(_page(h, w, 2), _boxes(h, w))


@pytest.mark.parametrize("name", CANVAS_NAMES)
def test_glyphs_match_the_restatement(dev, tile, name):
    h, w = _canvases(tile[0])[name]
    cmds, atlas = _glyphs(h, w)
    _check(_page(h, w, 3), cmds, atlas)


@pytest.mark.parametrize("name", CANVAS_NAMES)
def test_mixed_drawing_matches_the_restatement(dev, tile, name):
    """All three primitives interleaved, so that later commands blend over earlier ones of another kind."""
    h, w = _canvases(tile[0])[name]
    glyphs, atlas = _glyphs(h, w)
    parts = [_segments(h, w), _boxes(h, w), glyphs]
    cmds = [p[i] for i in range(max(map(len, parts))) for p in parts if i < len(p)]
    _check(_page(h, w, 4), cmds, atlas)


def test_command_order_decides(dev, tile):
    page = _page(37, 53, 5)
    a = box((5, 5, 30, 25), color=(255, 0, 0))
    b = seg(0, 0, 52, 36, 5, color=(0, 0, 255))
    ab, ba = _check(page, [a, b]), _check(page, [b, a])
    assert not np.array_equal(ab, ba)
    assert ab[15, 22].tolist() == [0, 0, 255] and ba[15, 22].tolist() == [255, 0, 0]


def test_list_longer_than_the_lds_chunk(dev, tile):
    """One tile whose list spans more than three LDS chunks of tiny, overlapping, partly transparent commands: a dropped,
    repeated or reordered command changes the blend."""
    t, chunk = tile
    n = 3 * chunk + 7
    rng = np.random.default_rng(6)
    cmds = []
    for i in range(n):
        x, y = int(rng.integers(2, t - 4)), int(rng.integers(2, t - 4))  # with its reach (<= 2 + 1 px) inside the tile
        color = tuple(int(v) for v in rng.integers(0, 256, 3))
        if i % 3 == 0:
            cmds.append(seg(x, y, x + int(rng.integers(0, 3)), y + int(rng.integers(0, 3)), int(rng.integers(1, 4)), color, int(rng.integers(60, 256))))
        else:
            cmds.append(box((x, y, x + 2, y + 2), color=color, a=int(rng.integers(60, 256))))
    _check(_page(t, t, 6), cmds)
    # the same list in a canvas of several tiles: only that tile's list is long
    shifted = [c[:5] + [v + t for v in c[5:9]] + c[9:] for c in cmds]  # end points / outer box; the boxes have no hole
    page = _page(2 * t + 5, 3 * t - 1, 7)
    got = _check(page, shifted)
    assert np.array_equal(got[:t], page[:t]) and np.array_equal(got[:, :t], page[:, :t])


def test_zero_commands_and_empty_tiles_leave_the_page(dev, tile):
    t, _ = tile
    page = _page(3 * t, 3 * t, 8)
    assert np.array_equal(_draw(page, np.zeros((0, 16), np.int32)), page)
    cmds = [box((t + 2, t + 3, 2 * t - 4, 2 * t - 2), color=(1, 2, 3), a=200), seg(t + 1, t + 1, 2 * t - 2, 2 * t - 2, 2)]
    got = _check(page, cmds)
    untouched = np.ones((3 * t, 3 * t), bool)
    untouched[t : 2 * t, t : 2 * t] = False
    assert np.array_equal(got[untouched], page[untouched])
    assert not np.array_equal(got[t : 2 * t, t : 2 * t], page[t : 2 * t, t : 2 * t])
    # commands that lie wholly off the canvas: every list is empty
    assert np.array_equal(_draw(page, [seg(-50, -50, -10, -20, 5), box((3 * t, 0, 4 * t, 10))]), page)


def test_render_leaves_the_page_alone(dev):
    from yomitoku_amd.utils.visualizer import Overlay, load_font

    page = _page(130, 67, 9)
    page_dev = torch.from_numpy(page).to("cuda:0")
    ov = Overlay()
    ov.fill((0, 0, 66, 129), (0, 0, 0), alpha=128)
    ov.rectangle((5, 5, 60, 100), (0, 255, 0), 3)
    ov.text((8, 20), "Ag1", load_font(None, 24), (255, 0, 0))
    ov.arrow((10, 120), (60, 60), (0, 0, 255), 2, tip=10)
    canvas = ov.render(page_dev)
    assert canvas.is_cuda and canvas.data_ptr() != page_dev.data_ptr()
    assert np.array_equal(page_dev.cpu().numpy(), page)
    data = ov.build(130, 67)
    want = ref.draw_reference(page, data["cmds"], data["atlas"])
    assert np.array_equal(ov.to_host(), want) and not np.array_equal(want, page)
    assert np.array_equal(Overlay().render(page_dev).cpu().numpy(), page)  # an empty drawing: a plain copy
    host = ov.render(page)  # a host page is uploaded, drawn on the device, and stays what it was
    assert np.array_equal(host.cpu().numpy(), want) and np.array_equal(page, _page(130, 67, 9))


HEAT_CASES = {
    "5x7_onto_37x53": ((5, 7), (37, 53)),
    "identity": ((37, 53), (37, 53)),
    "1x1_map": ((1, 1), (37, 53)),
    "downscale": ((130, 67), (37, 53)),
    "onto_a_row": ((5, 7), (1, 40)),
}


@pytest.mark.parametrize("name", list(HEAT_CASES))
def test_heatmap_matches_the_restatement(dev, name):
    from yomitoku_amd.utils.visualizer import Overlay

    (mh, mw), (h, w) = HEAT_CASES[name]
    rng = np.random.default_rng(10)
    prob = rng.uniform(-0.3, 1.3, (mh, mw)).astype(np.float32)  # values below 0 and above 1 are clamped
    prob.flat[0] = 1.0
    if prob.size > 3:
        prob.flat[1:4] = (0.0, -2.0, 7.5)
    page = _page(h, w, 11)
    ov = Overlay()
    ov.heatmap(torch.from_numpy(prob).to("cuda:0")[None])  # 1 x H x W, as preds["binary"][0]
    got = ov.render(torch.from_numpy(page).to("cuda:0")).cpu().numpy()
    want = ref.heatmap_reference(page, prob)
    assert np.array_equal(got, want)
    assert (got != page).any(-1).mean() > 0.9
    # the heat map first, the commands over it
    ov.rectangle((2, 0, w - 3, h - 1), (0, 255, 0), 1)
    got = ov.render(page).cpu().numpy()
    assert np.array_equal(got, ref.draw_reference(want, ov.build(h, w)["cmds"]))
