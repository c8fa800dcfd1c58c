"""The layer, the flush and the rounded box in ymk_draw_overlay, ymk_draw_overlay_pages and ymk_overlay_layout's bounds
(yomitoku_amd/csrc/ymk_overlay.hip) against the NumPy restatement of the rules in tests/overlay_layer_ref.py: bit-exact, every
case a few thousand pixels."""
import numpy as np
import pytest
import torch

from tests import overlay_layer_ref as lref
from tests.test_overlay_gpu import _glyphs, _page, glyph
from tests.test_overlay_layer import L, box, flush, rbox, seg
from yomitoku_amd.utils import visualizer as V

pytestmark = pytest.mark.gpu

M = 16383
CANVASES = {"37x53": (37, 53), "70x45": (70, 45), "row": (1, 40), "column": (40, 1)}


@pytest.fixture(scope="module")
def consts(dev):
    from yomitoku_amd import _lib

    lib = _lib.load()
    return int(lib.ymk_overlay_tile()), int(lib.ymk_overlay_chunk())


def _draw(page, cmds, atlas=None):
    canvas = torch.from_numpy(page).to("cuda:0")
    V.draw_commands(canvas, np.asarray(cmds, dtype=np.int32).reshape(-1, 16), atlas)
    return canvas.cpu().numpy()


def _same(got, want, what=""):
    bad = np.argwhere((got != want).any(-1))
    assert np.array_equal(got, want), f"{what}: {len(bad)} pixels differ, first at (y, x) = {bad[0].tolist()}"


def _check(page, cmds, atlas=None):
    got = _draw(page, cmds, atlas)
    _same(got, lref.draw_reference(page, cmds, atlas))
    return got


def _rboxes(h, w, flag=0):
    return [rbox((26, 26, 40, 40), 6, (255, 0, 0), flag=flag),             # all four corners around the tile corner (32, 32)
            rbox((20, 29, 50, 35), 3, (0, 255, 0), 140, flag),             # corners left and right of x = 32, the box across y = 32
            rbox((29, 3, 35, 60), 100, (0, 0, 255), 200, flag),            # r clamped to (35 - 29) / 2: round ends on x = 32
            rbox((2, 2, 12, 9), 0, (9, 99, 199), flag=flag),               # r = 0: a plain box
            rbox((3, 12, 3, 12), 7, (255, 255, 0), flag=flag),             # one pixel
            rbox((-10, -10, 8, 8), 5, (0, 255, 255), 90, flag),            # partly off the canvas
            rbox((w - 6, h - 5, w + 9, h + 8), 4, (255, 0, 255), flag=flag),
            rbox((w + 5, 0, w + 30, 10), 3, (1, 2, 3), flag=flag),         # wholly off
            rbox((0, -40, w - 1, -3), 9, (1, 2, 3), flag=flag),
            rbox((-M, -M, M, M), M, (60, 70, 80), 30, flag),               # the coordinate bounds: a disc of radius 16383 around (0, 0)
            rbox((-M, h // 2, M, h // 2 + 4), 2, (250, 250, 0), 120, flag),  # from bound to bound: no corner on the canvas
            rbox((M - 5, M - 5, M, M), 2, (1, 2, 3), flag=flag),
            rbox((12, 9, 2, 2), 3, (1, 2, 3), flag=flag)]                  # inverted: nothing


@pytest.mark.parametrize("name", list(CANVASES))
def test_rounded_boxes_match_the_restatement(consts, name):
    h, w = CANVASES[name]
    page = _page(h, w, 21)
    got = _check(page, _rboxes(h, w))
    assert not np.array_equal(got, page)


@pytest.mark.parametrize("name", list(CANVASES))
def test_layer_records_of_every_kind(consts, name):
    """SEG, BOX, GLYPH (partial coverage from the atlas) and RBOX painted into the layer over one another, canvas records
    in between, then one flush: every pixel is composited once, with the coverage the layer accumulated."""
    h, w = CANVASES[name]
    glyphs, atlas = _glyphs(h, w)
    layer = [c[:] for c in glyphs]
    for c in layer:
        c[0] |= L
    layer += [seg(0, 0, w - 1, h - 1, 5, (255, 128, 0), 255, L), seg(w - 1, 0, 0, h - 1, 3, (0, 128, 255), 100, L),
              box((3, 2, w - 4, h - 3), (8, 6, w - 9, h - 7), (255, 0, 255), 200, L), box((w // 3, h // 3, w // 2 + 4, h // 2 + 4), color=(0, 255, 0), flag=L)]
    layer += _rboxes(h, w, L)[:9]
    canvas = [seg(2, h // 2, w - 3, h // 2, 2, (10, 20, 30)), box((1, 1, w // 2, h // 2), color=(200, 200, 0), a=77), glyph(w // 2, h // 2, 7, 5, 4, 9)]
    cmds = [p[i] for i in range(len(layer)) for p in (layer, canvas) if i < len(p)]  # interleaved
    page = _page(h, w, 22)
    for alpha, keep in ((77, 1), (255, 0)):
        got = _check(page, cmds + [flush((-5, -5, w + 5, h + 5), alpha, keep)], atlas)
        assert not np.array_equal(got, _check(page, cmds, atlas))  # without the flush only the canvas records show
    _same(_draw(page, cmds, atlas), lref.draw_reference(page, canvas, atlas), "no flush at all")


@pytest.mark.parametrize("name", list(CANVASES))
def test_flush_boxes(consts, name):
    h, w = CANVASES[name]
    page = _page(h, w, 23)
    paint = [box((0, 0, w - 1, h - 1), color=(255, 128, 0), flag=L), rbox((4, 4, 44, 44), 8, (0, 255, 0), 180, L)]
    small = flush((w // 4, h // 4, w // 4 + 20, h // 4 + 20), 77, 1)
    part = _check(page, paint + [small])                                    # a flush box smaller than what was painted
    y, x = min(h // 4 + 21, h), min(w // 4 + 21, w)
    assert np.array_equal(part[y:], page[y:]) and np.array_equal(part[:, x:], page[:, x:]) and not np.array_equal(part, page)
    whole = _check(page, paint + [flush((0, 0, w, h), 77, 1)])
    _same(_check(page, paint + [small, flush((0, 0, w, h), 77, 1)]), whole, "the rest at the next flush")
    _same(_check(page, paint + [flush((0, 0, w, h), 77, 1)] * 2), whole, "a second flush draws nothing")
    empty = [box((0, 0, 3, 0), color=(1, 2, 3), flag=L), flush((w // 2 + 1, 1, w + 9, h + 9), 255), flush((-9, -9, -1, -1), 255)]
    assert np.array_equal(_check(page, empty), page)  # flushes with no painted pixel in their box
    assert np.array_equal(_check(page, paint), page)                         # no flush at all: a tile's layer is dropped
    # a canvas record under and over the flush keeps its place in the order
    order = [box((2, 0, 30, 30), color=(0, 0, 255))] + paint + [flush((0, 0, w, h), 128), seg(0, 0, w, h, 3, (255, 255, 255), 100)]
    _check(page, order)


@pytest.mark.parametrize("name", list(CANVASES))
def test_stray_bits_and_flagged_flush_draw_nothing(consts, name):
    h, w = CANVASES[name]
    page = _page(h, w, 24)
    full = (0, 0, w - 1, h - 1)
    bad = [box(full), box(full, flag=L), seg(0, 0, w, h, 9, (1, 2, 3)), rbox(full, 2, (1, 2, 3)), flush(full, 255)]
    for c, bits in zip(bad, (0x200, 0x400, 0x10000, 1 << 30, 0x200)):
        c[0] |= bits
    minus = box(full)
    minus[0] = -1
    unknown = box(full)
    unknown[0] = 5
    cmds = bad + [minus, unknown, box(full, color=(9, 9, 9), flag=L), flush(full, 255, flag=L)]
    assert np.array_equal(_check(page, cmds), page)
    _check(page, cmds + [flush(full, 255)])  # the plain flush after them shows the one record that did paint the layer


def test_layer_survives_the_chunks_of_a_long_list(consts):
    """One tile with more than three LDS chunks: the layer is painted before the first chunk boundary and flushed after the
    last, with canvas and layer records in every chunk between."""
    tile, chunk = consts
    n = max(3 * chunk + 20, 200)
    rng = np.random.default_rng(25)
    cmds = [box((2, 2, tile - 3, tile - 3), color=(255, 128, 0), flag=L), rbox((4, 4, 20, 20), 5, (0, 255, 0), 150, L)]
    for i in range(n):
        x, y = int(rng.integers(2, tile - 4)), int(rng.integers(2, tile - 4))
        color = tuple(int(v) for v in rng.integers(0, 256, 3))
        flag = L if i % 4 == 1 else 0
        if i % 3 == 0:
            cmds.append(seg(x, y, x + int(rng.integers(0, 3)), y + int(rng.integers(0, 3)), int(rng.integers(1, 4)), color, int(rng.integers(60, 256)), flag))
        else:
            cmds.append(box((x, y, x + 2, y + 2), color=color, a=int(rng.integers(60, 256)), flag=flag))
    cmds.append(flush((0, 0, tile - 1, tile - 1), 77, 1))
    assert len(cmds) > 3 * chunk and len(cmds) >= 200
    page = _page(tile, tile, 26)
    got = _check(page, cmds)
    assert not np.array_equal(got, _check(page, cmds[:-1]))
    # the same list in the middle tile of a larger canvas: the other tiles are not touched
    shifted = [c[:5] + [v + tile for v in c[5:9]] + c[9:] for c in cmds]
    big = _page(2 * tile + 5, 3 * tile - 1, 27)
    got = _check(big, shifted)
    assert np.array_equal(got[:tile], big[:tile]) and np.array_equal(got[:, :tile], big[:, :tile])


# ---------------------------------------------------------------------------------------------------------------- the wave
def _wave_drawing(h, w, seed):
    rng = np.random.default_rng(seed)
    glyphs, atlas = _glyphs(h, w)
    cmds = []
    for i in range(30):
        x0, x1 = sorted(int(v) for v in rng.integers(-15, w + 15, 2))
        y0, y1 = sorted(int(v) for v in rng.integers(-15, h + 15, 2))
        color = tuple(int(v) for v in rng.choice([0, 128, 255, 37], 3))
        alpha = int(rng.choice([77, 255, 180]))
        flag = L if i % 3 else 0
        kind = i % 5
        if kind == 0:
            cmds.append(seg(x0, y0, x1, y1, int(rng.integers(1, 6)), color, alpha, flag))
        elif kind == 1:
            cmds.append(box((x0, y0, x1, y1), color=color, a=alpha, flag=flag))
        elif kind == 2:
            g = list(glyphs[i % len(glyphs)])
            g[0] |= flag
            cmds.append(g)
        else:
            cmds.append(rbox((x0, y0, x1, y1), int(rng.integers(0, 15)), color, alpha, flag))
        if i % 8 == 7:
            cmds.append(flush((min(x0, 3), min(y0, 3), w - 4, h - 4), int(rng.choice([77, 255])), i % 16 == 7))
    stray = box((0, 0, w, h))
    stray[0] = -1
    return cmds + [stray, rbox((-M, -M, M, M), 40, (5, 6, 7), 20), flush((-M, -M, M, M), 200)], atlas


def test_wave_equals_the_single_canvas_kernel_and_the_restatement(consts):
    from tests import overlay_wave_ref as wref

    tile, _ = consts
    sizes = [(33, 31), (1, 70), (100, 130)]
    pages = [_page(h, w, 30 + i) for i, (h, w) in enumerate(sizes)]
    lists, atlas = [], None
    for i, (h, w) in enumerate(sizes):
        cmds, atlas = _wave_drawing(h, w, 40 + i)  # one atlas layout for all: _glyphs is size-blind
        lists.append(cmds)
    table, nbytes, _ = wref.pack(sizes, [len(c) for c in lists], tile)
    buf = np.full(nbytes + 64, 171, dtype=np.uint8)
    for (off, h, w, *_), p in zip(table.tolist(), pages):
        buf[off : off + h * w * 3] = p.reshape(-1)
    all_cmds = np.concatenate([np.asarray(c, dtype=np.int32).reshape(-1, 16) for c in lists])
    buf_dev = torch.from_numpy(buf).to("cuda:0")
    out = V.launch_wave(buf_dev, all_cmds, table, atlas=atlas)
    got = buf_dev.cpu().numpy()
    for i, ((off, h, w, *_), page, cmds) in enumerate(zip(table.tolist(), pages, lists)):
        canvas = got[off : off + h * w * 3].reshape(h, w, 3)
        _same(canvas, lref.draw_reference(page, cmds, atlas), f"canvas {i} against the restatement")
        _same(canvas, _draw(page, cmds, atlas), f"canvas {i} against ymk_draw_overlay")
        assert not np.array_equal(canvas, page)
    # the device's bounds: the restatement's, and the host's command_bounds clipped to each canvas
    bounds = out["bounds_dev"].cpu().numpy()
    assert np.array_equal(bounds, lref.bounds_reference(all_cmds, table))
    for _, h, w, first, count, _ in table.tolist():
        x0, y0, x1, y1 = V.command_bounds(all_cmds[first : first + count])
        x0, y0, x1, y1 = np.maximum(x0, 0), np.maximum(y0, 0), np.minimum(x1, w - 1), np.minimum(y1, h - 1)
        dead = (x0 > x1) | (y0 > y1)
        want = np.where(dead[:, None], np.asarray([1, 1, 0, 0]), np.stack([x0, y0, x1, y1], axis=1))
        assert np.array_equal(bounds[first : first + count], want)
    assert (all_cmds[:, 0] & 0xFF == V.FLUSH).sum() >= 9 and (bounds[all_cmds[:, 0] == -1] == (1, 1, 0, 0)).all()
