"""NumPy restatement of the overlay drawing rules (include/ymk.h, DESIGN.md "Overlay rasteriser"): the yardstick of
tests/test_overlay_plan.py and tests/test_overlay_gpu.py.  Written from the rules, one command after the other over the whole
canvas; it shares no code with yomitoku_amd.utils.visualizer.

Arithmetic: the rules are stated as `4 c <= T`.  They are evaluated in that form, in Python integers (object arrays) whenever a
coordinate is large enough for an int64 product to overflow, in int64 otherwise."""
import numpy as np

WORDS = 16
K_SEG, K_BOX, K_GLYPH = 0, 1, 2


def _grid(region, dtype):
    y0, y1, x0, x1 = region
    py, px = np.mgrid[y0:y1, x0:x1]
    return px.astype(dtype), py.astype(dtype)


def coverage(cmd, atlas, region):
    """uint8-valued alpha (int64 array) of one command over the pixels of region = (y0, y1, x0, x1), half open."""
    c = [int(v) for v in cmd]
    kind = c[0]
    big = max(abs(v) for v in c[5:13]) > 2000
    px, py = _grid(region, object if big and kind == K_SEG else np.int64)
    shape = px.shape
    if kind == K_SEG:
        x0, y0, x1, y1, t = c[5:10]
        dx, dy = x1 - x0, y1 - y0
        l2 = dx * dx + dy * dy
        qx, qy = px - x0, py - y0
        u = qx * dx + qy * dy
        near0 = 4 * (qx * qx + qy * qy) <= t * t
        near1 = 4 * ((px - x1) * (px - x1) + (py - y1) * (py - y1)) <= t * t
        cross = qx * dy - qy * dx
        body = 4 * (cross * cross) <= t * t * l2
        if l2 == 0:
            inside = near0
        else:
            inside = np.where(u <= 0, near0, np.where(u >= l2, near1, body))
        return np.where(inside.astype(bool), c[4], 0).astype(np.int64)
    if kind == K_BOX:
        ox1, oy1, ox2, oy2, ix1, iy1, ix2, iy2 = c[5:13]
        outer = (px >= ox1) & (px <= ox2) & (py >= oy1) & (py <= oy2)
        inner = (px >= ix1) & (px <= ix2) & (py >= iy1) & (py <= iy2)  # empty when ix1 > ix2
        return np.where(outer & ~inner, c[4], 0).astype(np.int64)
    if kind == K_GLYPH:
        x, y, w, h, off, pitch = c[5:11]
        inside = (px >= x) & (px < x + w) & (py >= y) & (py < y + h)
        idx = off + (py - y) * pitch + (px - x)
        out = np.zeros(shape, dtype=np.int64)
        if inside.any():
            out[inside] = np.asarray(atlas, dtype=np.int64)[idx[inside]]
        return out
    raise ValueError(f"unknown command kind {kind}")


def blend(dst, colour, a):
    """dst = (colour * a + dst * (255 - a) + 127) / 255, integer division; dst int64 [...][3], a int64 [...]."""
    a = a[..., None]
    return (np.asarray(colour, dtype=np.int64) * a + dst * (255 - a) + 127) // 255


def reach(cmd):
    """(y0, y1, x0, x1), half open: a rectangle outside of which the command covers no pixel - a segment cannot reach further
    than t from its end points' bounding box, a box or a glyph not beyond its own rectangle."""
    c = [int(v) for v in cmd]
    if c[0] == K_SEG:
        return min(c[6], c[8]) - c[9], max(c[6], c[8]) + c[9] + 1, min(c[5], c[7]) - c[9], max(c[5], c[7]) + c[9] + 1
    if c[0] == K_BOX:
        return c[6], c[8] + 1, c[5], c[7] + 1
    return c[6], c[6] + c[8], c[5], c[5] + c[7]


def draw_reference(canvas, cmds, atlas=None, region=None, order=None, within_reach=False):
    """Apply `cmds` (int [n][16]) one after the other - or the commands `order` lists, in that order - to a copy of `canvas`
    (uint8 H x W x 3), over the whole canvas or over region = (y0, y1, x0, x1) only.  within_reach: evaluate each command
    only inside `reach(cmd)` (the same image; for page-sized canvases with hundreds of commands)."""
    out = np.array(canvas, dtype=np.int64)
    h, w = out.shape[:2]
    region = (0, h, 0, w) if region is None else region
    y0, y1, x0, x1 = region
    cmds = np.asarray(cmds).reshape(-1, WORDS)
    atlas = np.zeros(0, np.uint8) if atlas is None else atlas
    whole = region
    for i in (range(len(cmds)) if order is None else order):
        if within_reach:
            r = reach(cmds[i])
            y0, y1, x0, x1 = region = (max(whole[0], r[0]), min(whole[1], r[1]), max(whole[2], r[2]), min(whole[3], r[3]))
            if y0 >= y1 or x0 >= x1:
                continue
        a = coverage(cmds[i], atlas, region)
        view = out[y0:y1, x0:x1]
        view[...] = np.where((a > 0)[..., None], blend(view, cmds[i][1:4], a), view)
    return out.astype(np.uint8)


def draw_by_tiles(canvas, cmds, atlas, tile_offsets, tile_cmds, tile):
    """The same drawing tile by tile from per-tile CSR lists: each tile applies ITS list, in list order."""
    out = np.array(canvas, dtype=np.uint8)
    h, w = out.shape[:2]
    tiles_x = -(-w // tile)
    for t in range(len(tile_offsets) - 1):
        lst = [int(v) for v in tile_cmds[tile_offsets[t] : tile_offsets[t + 1]]]
        if not lst:
            continue
        ty, tx = divmod(t, tiles_x)
        region = (ty * tile, min(h, (ty + 1) * tile), tx * tile, min(w, (tx + 1) * tile))
        out = draw_reference(out, cmds, atlas, region=region, order=lst)
    return out


def jet_reference():
    """uint8 [256][3] (B, G, R) from the formula, one entry at a time; Python's round() rounds half to even."""
    table = np.zeros((256, 3), dtype=np.uint8)
    for v in range(256):
        s = v / 255
        r = min(max(1.5 - abs(4 * s - 3), 0.0), 1.0)
        g = min(max(1.5 - abs(4 * s - 2), 0.0), 1.0)
        b = min(max(1.5 - abs(4 * s - 1), 0.0), 1.0)
        table[v] = (round(b * 255), round(g * 255), round(r * 255))
    return table


def heatmap_reference(canvas, prob, jet=None):
    """det_visualizer(vis_heatmap=True) in integers, as include/ymk.h states it."""
    jet = jet_reference() if jet is None else jet
    canvas = np.asarray(canvas)
    h, w = canvas.shape[:2]
    p = np.clip(np.asarray(prob, dtype=np.float32), np.float32(0), np.float32(1))
    m = (p * np.float32(255)).astype(np.uint8).astype(np.int64)  # float32 product, truncated
    mh, mw = m.shape

    def taps(d, dn, sn):
        X = ((2 * d + 1) * sn * 1024) // (2 * dn) - 512
        X = np.clip(X, 0, (sn - 1) * 1024)
        i0 = X >> 10
        return i0, np.minimum(i0 + 1, sn - 1), X & 1023

    x0, x1, fx = taps(np.arange(w, dtype=np.int64), w, mw)
    y0, y1, fy = taps(np.arange(h, dtype=np.int64), h, mh)
    fx, fy = fx[None, :], fy[:, None]
    v = (m[y0][:, x0] * (1024 - fx) * (1024 - fy) + m[y0][:, x1] * fx * (1024 - fy) + m[y1][:, x0] * (1024 - fx) * fy
         + m[y1][:, x1] * fx * fy + (1 << 19)) >> 20
    return ((canvas.astype(np.int64) + jet[v].astype(np.int64) + 1) >> 1).astype(np.uint8)
