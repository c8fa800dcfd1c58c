"""NumPy / plain-Python restatement of what ymk_overlay_layout computes (include/ymk.h: text runs -> GLYPH records, and every
command's bounding box clipped to its canvas): the yardstick of tests/test_overlay_wave.py and tests/test_overlay_wave_gpu.py.
Written from the rules, one character and one command at a time; it shares no code with yomitoku_amd.utils.visualizer."""
import numpy as np

WORDS = 16
K_SEG, K_BOX, K_GLYPH = 0, 1, 2
M = 16383


def _clamp(v):
    return min(max(int(v), -M), M)


def layout_reference(cmds, runs, codes, glyphs):
    """`cmds` (int [n][16], the text slots reserved with kind and colour) after the layout rule has been applied to `runs`
    (int [r][8]: first slot, first code, count, pen x, pen y, vertical, step, 0), `codes` (glyph ids) and `glyphs`
    (int [g][6]: atlas offset, w, h, x offset, y offset, advance)."""
    out = np.array(cmds, dtype=np.int64).reshape(-1, WORDS)
    codes = [int(c) for c in np.asarray(codes).reshape(-1)]
    glyphs = np.asarray(glyphs, dtype=np.int64).reshape(-1, 6)
    for run in np.asarray(runs, dtype=np.int64).reshape(-1, 8).tolist():
        slot0, code0, count, pen_x, pen_y, vertical, step = run[:7]
        if count <= 0 or slot0 < 0 or code0 < 0 or slot0 + count > len(out) or code0 + count > len(codes):
            continue  # a run outside the arrays is skipped
        advanced = 0
        for i in range(count):
            gid = codes[code0 + i]
            known = 0 <= gid < len(glyphs)
            off, w, h, ox, oy, adv = glyphs[gid].tolist() if known else (0, 0, 0, 0, 0, 0)
            x, y = (pen_x, pen_y + i * step) if vertical else (pen_x + advanced, pen_y)
            rec = out[slot0 + i]
            if known and w > 0 and h > 0:
                rec[5:11] = (_clamp(x + ox), _clamp(y + oy), w, h, off, w)
            else:
                rec[0] = -1
                rec[5:11] = 0
            advanced += adv
    return out


def box_of(cmd):
    """Inclusive (x0, y0, x1, y1) of one record, None for a kind that draws nothing."""
    c = [int(v) for v in cmd]
    if c[0] == K_SEG:
        pad = (c[9] + 1) // 2
        return min(c[5], c[7]) - pad, min(c[6], c[8]) - pad, max(c[5], c[7]) + pad, max(c[6], c[8]) + pad
    if c[0] == K_BOX:
        return c[5], c[6], c[7], c[8]
    if c[0] == K_GLYPH:
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


def pack(sizes, counts, tile):
    """(table int64 [c][6], total bytes, total tiles) for canvases of `sizes` with `counts` commands each, packed on 16-byte
    boundaries."""
    table, at, first, tiles = [], 0, 0, 0
    for (h, w), n in zip(sizes, counts):
        table.append((at, h, w, first, n, tiles))
        at += -(-(h * w * 3) // 16) * 16
        first += n
        tiles += -(-h // tile) * -(-w // tile)
    return np.asarray(table, dtype=np.int64).reshape(-1, 6), at, tiles
