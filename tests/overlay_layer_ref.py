"""NumPy restatement of the overlay drawing rules WITH the layer (include/ymk.h, DESIGN.md "Overlay rasteriser", "Layer"):
rounded boxes, records directed into the layer, and the flush that composites the layer once.  The yardstick of
tests/test_overlay_layer.py, tests/test_overlay_layer_gpu.py and tests/test_table_semantic_overlays_gpu.py.  The three old
kinds are evaluated by tests/overlay_ref.py (which stays the yardstick of the old tests); everything else is written here from
the rules, one command after the other over the whole canvas, and shares no code with yomitoku_amd.utils.visualizer."""
import numpy as np

from tests import overlay_ref as old

WORDS = 16
K_SEG, K_BOX, K_GLYPH, K_RBOX, K_FLUSH = 0, 1, 2, 3, 4
KIND_MASK, TO_LAYER = 0xFF, 0x100


def split_word0(word0):
    """(kind, flagged) of a record's word 0; (None, False) for a word with a bit outside 0x1ff (-1 among them): draws nothing."""
    word0 = int(word0)
    if word0 & ~(KIND_MASK | TO_LAYER):
        return None, False
    return word0 & KIND_MASK, bool(word0 & TO_LAYER)


def rbox_coverage(cmd, region):
    """Alpha (int64 array) of a rounded box over region = (y0, y1, x0, x1), half open."""
    c = [int(v) for v in cmd]
    x1, y1, x2, y2, r = c[5:10]
    px, py = old._grid(region, np.int64)
    if x2 < x1 or y2 < y1:
        return np.zeros(px.shape, dtype=np.int64)
    r = max(min(r, (x2 - x1) // 2, (y2 - y1) // 2), 0)
    cx, cy = np.clip(px, x1 + r, x2 - r), np.clip(py, y1 + r, y2 - r)
    inside = (px >= x1) & (px <= x2) & (py >= y1) & (py <= y2) & ((px - cx) ** 2 + (py - cy) ** 2 <= r * r)
    return np.where(inside, c[4], 0).astype(np.int64)


def coverage(kind, cmd, atlas, region):
    if kind in (K_SEG, K_BOX, K_GLYPH):
        plain = [int(v) for v in cmd]
        plain[0] = kind
        return old.coverage(plain, atlas, region)
    if kind == K_RBOX:
        return rbox_coverage(cmd, region)
    y0, y1, x0, x1 = region
    return np.zeros((y1 - y0, x1 - x0), dtype=np.int64)  # an unknown kind draws nothing


def blend1(dst, colour, a):
    return (colour * a + dst * (255 - a) + 127) // 255


def reach(cmd):
    """(y0, y1, x0, x1), half open: a rectangle outside of which the record neither covers nor flushes a pixel."""
    c = [int(v) for v in cmd]
    kind, _ = split_word0(c[0])
    if kind in (K_SEG, K_BOX, K_GLYPH):
        return old.reach([kind] + c[1:])
    if kind in (K_RBOX, K_FLUSH):
        return c[6], c[8] + 1, c[5], c[7] + 1
    return 0, 0, 0, 0


def draw_reference(canvas, cmds, atlas=None, region=None, order=None, within_reach=False):
    """Apply `cmds` (int [n][16]) one after the other - or the commands `order` lists, in that order - to a copy of `canvas`
    (uint8 H x W x 3), over the whole canvas or over region = (y0, y1, x0, x1) only.  The layer starts empty and what is left in
    it at the end is dropped.  within_reach: evaluate each command only inside `reach(cmd)` (the same image; for page-sized
    canvases with hundreds of commands)."""
    out = np.array(canvas, dtype=np.int64)
    h, w = out.shape[:2]
    whole = (0, h, 0, w) if region is None else region
    cmds = np.asarray(cmds).reshape(-1, WORDS)
    atlas = np.zeros(0, np.uint8) if atlas is None else atlas
    layer_colour = np.zeros((h, w, 3), dtype=np.int64)
    layer_cov = np.zeros((h, w), dtype=np.int64)
    for i in (range(len(cmds)) if order is None else order):
        c = [int(v) for v in cmds[i]]
        kind, flagged = split_word0(c[0])
        if kind is None:
            continue
        region = whole
        if within_reach:
            r = reach(c)
            region = (max(whole[0], r[0]), min(whole[1], r[1]), max(whole[2], r[2]), min(whole[3], r[3]))
        y0, y1, x0, x1 = region
        if y0 >= y1 or x0 >= x1:
            continue
        view, colour, cov = out[y0:y1, x0:x1], layer_colour[y0:y1, x0:x1], layer_cov[y0:y1, x0:x1]
        if kind == K_FLUSH:
            if flagged:
                continue
            px, py = old._grid(region, np.int64)
            alpha, keep255 = c[4], c[9] != 0
            inside = (px >= c[5]) & (px <= c[7]) & (py >= c[6]) & (py <= c[8])
            e = (cov * alpha + 127) // 255
            for ch in range(3):
                hit = inside & (cov > 0)
                if keep255:
                    hit = hit & (colour[..., ch] != 255)
                view[..., ch] = np.where(hit, blend1(view[..., ch], colour[..., ch], e), view[..., ch])
            cov[inside] = 0
            continue
        a = coverage(kind, c, atlas, region)
        hit = a > 0
        if not flagged:
            view[...] = np.where(hit[..., None], old.blend(view, c[1:4], a), view)
            continue
        first = hit & (cov == 0)
        again = hit & (cov > 0)
        for ch in range(3):
            colour[..., ch] = np.where(first, c[1 + ch], np.where(again, blend1(colour[..., ch], c[1 + ch], a), colour[..., ch]))
        cov[...] = np.where(first, a, np.where(again, blend1(cov, 255, a), cov))
    return out.astype(np.uint8)


def draw_by_tiles(canvas, cmds, atlas, tile_offsets, tile_cmds, tile):
    """The same drawing tile by tile from per-tile CSR lists: each tile applies ITS list, in list order, with its own layer."""
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


def box_of(cmd):
    """Inclusive (x0, y0, x1, y1) of one record - a flagged record has the bounds of its kind - None for one that draws nothing."""
    c = [int(v) for v in cmd]
    kind, _ = split_word0(c[0])
    if kind == K_SEG:
        pad = (c[9] + 1) // 2
        return min(c[5], c[7]) - pad, min(c[6], c[8]) - pad, max(c[5], c[7]) + pad, max(c[6], c[8]) + pad
    if kind in (K_BOX, K_RBOX, K_FLUSH):
        return c[5], c[6], c[7], c[8]
    if kind == K_GLYPH:
        return c[5], c[6], c[5] + c[7] - 1, c[6] + c[8] - 1
    return None


def bounds_reference(cmds, table):
    """int16 [n][4]: per command of every canvas of `table` (int [c][6]: byte offset, h, w, first command, count, first tile)
    its box clipped to the canvas, (1, 1, 0, 0) when nothing is left; zeros for commands no canvas names."""
    cmds = np.asarray(cmds, dtype=np.int64).reshape(-1, WORDS)
    out = np.zeros((len(cmds), 4), dtype=np.int16)
    for _, h, w, first, count, _ in np.asarray(table, dtype=np.int64).reshape(-1, 6).tolist():
        for k in range(first, first + count):
            b = box_of(cmds[k])
            if b is not None:
                b = (max(b[0], 0), max(b[1], 0), min(b[2], w - 1), min(b[3], h - 1))
            out[k] = b if b is not None and b[0] <= b[2] and b[1] <= b[3] else (1, 1, 0, 0)
    return out
