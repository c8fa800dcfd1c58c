"""visualize=True: the reference's overlays (utils/visualizer.py:11-295, table_semantic_parser.py:308-620) drawn on the device.

The reference draws with OpenCV and Pillow on host copies of the page.  Here a drawing is an ordered list of fixed-size int32
commands - thick segments, boxes with an optional hole, glyph blits - that ONE launch of ymk_draw_overlay applies to a device
copy of the page (include/ymk.h has the record layout and the exact pixel rules, DESIGN.md "Overlay rasteriser" the design).
The host's share is building the list, packing the glyph masks Pillow rasterises into an atlas, and binning the commands by
bounding box into per-tile lists; all of it travels to the device as one staged blob.  The page the networks read is never
drawn on: `Overlay.render` clones it.

The overlays are equivalent in content to the reference's (same elements, colours, thicknesses, label strings, anchor
points), not byte-identical: OpenCV's Hershey font and Bresenham rules are replaced by the rules of include/ymk.h and by
Pillow glyphs.  Colour tuples are applied to the canvas's channels in the order given, as cv2 and ImageDraw do.

`DocumentAnalyzer.serve(overlays=True)` draws the same content another way (the second half of this file): text is recorded
as runs and laid out by ymk_overlay_layout, and ymk_draw_overlay_pages culls per tile and draws all canvases of a wave of pages
in one launch - no per-character loop and no binning on the host.  The CONTENT of each drawing is written once, in the
`_xxx_commands(ov, ...)` helpers, for both recorders (Overlay, RunOverlay).

The table-semantic parser's drawings (`cell_detector_visualizer`, `cell_id_visualizer`, `kv_items_visualizer`, `dag_visualizer`)
need two things more: a tint that is composited ONCE however many cells cover a pixel - commands recorded inside
`with ov.layer():` paint a per-pixel layer, `ov.flush(alpha)` blends it over the canvas - and a rounded filled box.

The nine functions keep the reference's names and arguments and return np.ndarray; `img` may also be a device tensor, and
`to_host=False` (not in the reference) returns the device canvas instead, which is how the modules chain overlays without a
round trip through the host.
"""

from __future__ import annotations

import contextlib
import logging
import os
import threading

import numpy as np

logger = logging.getLogger(__name__)

CMD_WORDS = 16  # YMK_OVERLAY_CMD_WORDS
SEG, BOX, GLYPH, RBOX, FLUSH = 0, 1, 2, 3, 4  # YMK_OVERLAY_SEG / _BOX / _GLYPH / _RBOX / _FLUSH
KIND_MASK, TO_LAYER = 0xFF, 0x100  # YMK_OVERLAY_KIND_MASK / _TO_LAYER: word 0 = kind | flag
COORD_MAX = 16383

# constants.py:9-32
PALETTE = [
    [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [128, 0, 0], [0, 128, 0], [0, 0, 128],
    [255, 128, 0], [0, 255, 128], [128, 0, 255], [128, 255, 0], [0, 128, 255], [255, 0, 128], [255, 128, 128], [128, 255, 128],
    [128, 128, 255], [255, 255, 128], [255, 128, 255], [128, 255, 255], [128, 128, 128],
]


def overlay_tile() -> int:
    """Edge of the rasteriser's canvas tiles (include/ymk.h: ymk_overlay_tile)."""
    from .. import _lib

    return int(_lib.load().ymk_overlay_tile())


def jet_table() -> np.ndarray:
    """uint8 [256][3] (B, G, R): r, g, b = clip(1.5 - |4 s - 3|, 0, 1), clip(1.5 - |4 s - 2|, 0, 1), clip(1.5 - |4 s - 1|, 0, 1)
    at s = v / 255 in float64, scaled to 0..255 and rounded half to even."""
    s = np.arange(256, dtype=np.float64) / 255.0
    r = np.clip(1.5 - np.abs(4.0 * s - 3.0), 0.0, 1.0)
    g = np.clip(1.5 - np.abs(4.0 * s - 2.0), 0.0, 1.0)
    b = np.clip(1.5 - np.abs(4.0 * s - 1.0), 0.0, 1.0)
    return np.rint(np.stack([b, g, r], axis=1) * 255.0).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- binning
def _kinds(word0):
    """The kind in word 0 without the layer flag; -1 for a word with a bit outside 0x1ff (a record that draws nothing)."""
    word0 = np.asarray(word0, dtype=np.int64)
    return np.where((word0 & ~(KIND_MASK | TO_LAYER)) != 0, -1, word0 & KIND_MASK)


def command_bounds(cmds: np.ndarray):
    """Inclusive bounding box (x0, y0, x1, y1; int64 arrays) of every command; x1 < x0 for one that covers nothing."""
    c = np.asarray(cmds, dtype=np.int64).reshape(-1, CMD_WORDS)
    kind = _kinds(c[:, 0])  # a record directed into the layer has the bounds of its kind
    pad = (c[:, 9] + 1) // 2  # a segment reaches t / 2 from its axis
    seg = (np.minimum(c[:, 5], c[:, 7]) - pad, np.minimum(c[:, 6], c[:, 8]) - pad,
           np.maximum(c[:, 5], c[:, 7]) + pad, np.maximum(c[:, 6], c[:, 8]) + pad)
    box = (c[:, 5], c[:, 6], c[:, 7], c[:, 8])
    glyph = (c[:, 5], c[:, 6], c[:, 5] + c[:, 7] - 1, c[:, 6] + c[:, 8] - 1)
    none = (np.ones_like(kind), np.ones_like(kind), np.zeros_like(kind), np.zeros_like(kind))
    boxed = (kind == BOX) | (kind == RBOX) | (kind == FLUSH)
    return tuple(np.where(kind == SEG, s, np.where(boxed, b, np.where(kind == GLYPH, g, e)))
                 for s, b, g, e in zip(seg, box, glyph, none))


def bin_commands(cmds: np.ndarray, h: int, w: int, tile: int):
    """Per-tile command lists in CSR form: (tile_offsets int32 [tiles + 1], tile_cmds int32 [n_list]).  Tiles are row-major,
    ceil(w / tile) per row; a command is listed in every tile its bounding box (clipped to the canvas) touches, and every
    list is in ascending command order."""
    tiles_x, tiles_y = -(-int(w) // tile), -(-int(h) // tile)
    x0, y0, x1, y1 = command_bounds(cmds)
    x0, y0 = np.maximum(x0, 0), np.maximum(y0, 0)
    x1, y1 = np.minimum(x1, int(w) - 1), np.minimum(y1, int(h) - 1)
    valid = (x0 <= x1) & (y0 <= y1)
    tx0, ty0 = x0 // tile, y0 // tile
    nx = np.where(valid, x1 // tile - tx0 + 1, 0)
    ny = np.where(valid, y1 // tile - ty0 + 1, 0)
    count = nx * ny
    total = int(count.sum())
    offsets = np.zeros(tiles_x * tiles_y + 1, dtype=np.int32)
    if total == 0:
        return offsets, np.zeros(0, dtype=np.int32)
    ids = np.repeat(np.arange(len(count), dtype=np.int64), count)
    k = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(count) - count, count)
    nxr = np.repeat(nx, count)
    tiles = (np.repeat(ty0, count) + k // nxr) * tiles_x + np.repeat(tx0, count) + k % nxr
    order = np.argsort(tiles, kind="stable")  # stable: inside a tile the commands keep their order
    offsets[1:] = np.cumsum(np.bincount(tiles, minlength=tiles_x * tiles_y))
    return offsets, ids[order].astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ fonts
_FONTS = {}
_GLYPHS = {}
_font_lock = threading.Lock()
_font_warned = False


def load_font(path, size: int):
    """(font, cache key).  `path` when that file exists; otherwise Pillow's built-in scalable font.  Asking for a file that
    is not there is reported once per process: glyphs outside the built-in font's coverage render as boxes."""
    global _font_warned
    from PIL import ImageFont

    size = int(size)
    name = path if path and os.path.isfile(path) else None
    if path and name is None:
        with _font_lock:
            if not _font_warned:
                _font_warned = True
                logger.warning("font file %s not found: text overlays use Pillow's built-in font, characters outside its "
                               "coverage render as boxes (set visualize.font to a TrueType file)", path)
    key = (name, size)
    with _font_lock:
        font = _FONTS.get(key)
        if font is None:
            font = _FONTS[key] = ImageFont.truetype(name, size) if name else ImageFont.load_default(size)
    return font, key


def glyph_of(font, key, ch: str):
    """(mask uint8 [h][w], x offset, y offset, advance) of one character, cached per (font file, size, character): the mask is
    font.getmask(ch, mode="L"), placed at the pen position plus font.getbbox(ch)[:2]; the pen advances by
    round(font.getlength(ch))."""
    gkey = (key, ch)
    got = _GLYPHS.get(gkey)
    if got is None:
        core = font.getmask(ch, mode="L")
        gw, gh = core.size
        mask = np.frombuffer(bytes(core), dtype=np.uint8).reshape(gh, gw).copy() if gw > 0 and gh > 0 else np.zeros((0, 0), np.uint8)
        ox, oy = font.getbbox(ch)[:2]
        got = _GLYPHS[gkey] = (mask, int(ox), int(oy), int(round(font.getlength(ch))))
    return got


# ---------------------------------------------------------------------------------------------------------------- builder
def _to_device_page(img, device=None):
    """(uint8 H x W x 3 device tensor, whether it is already a private copy)."""
    import torch

    if isinstance(img, torch.Tensor):
        if img.dtype != torch.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("overlay: the page must be a uint8 H x W x 3 tensor")
        if not img.is_cuda:
            return img.contiguous().to(device or "cuda"), True
        return img, False
    arr = np.ascontiguousarray(img)
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError("overlay: the page must be a uint8 H x W x 3 array")
    return torch.from_numpy(arr).to(device or "cuda"), True


def device_page(img, device=None):
    """`img` (host array or tensor) as a uint8 H x W x 3 tensor on `device`; a device tensor is returned as it is."""
    return _to_device_page(img, device)[0]


def to_host(canvas):
    """Device canvas (or an array) -> np.ndarray."""
    if canvas is None or isinstance(canvas, np.ndarray):
        return canvas
    return canvas.cpu().numpy()


class Overlay:
    """An ordered drawing.  Every method appends commands; `render(page)` applies them, in order, to a device copy of the
    page (the heat map, if one was set, is blended first) and returns the device canvas; `to_host()` gives the array."""

    def __init__(self):
        self._chunks = []     # int64 [k][CMD_WORDS] blocks in drawing order; glyph records hold a mask index in word 9
        self._masks = []      # glyph masks of this drawing, each once
        self._mask_index = {}
        self._chars = {}      # (font key, character) -> (mask index or -1, x offset, y offset, advance, width, height)
        self._heatmap = None
        self._flag = 0        # TO_LAYER inside `with ov.layer():`
        self._pending = []    # the blocks pushed into the layer since the last flush
        self.canvas = None

    def __len__(self):
        return sum(len(c) for c in self._chunks)

    # ---- the layer
    @contextlib.contextmanager
    def layer(self):
        """Everything pushed inside `with ov.layer():` paints the layer instead of the canvas (include/ymk.h); `flush`
        composites what was painted over the canvas once."""
        before, self._flag = self._flag, TO_LAYER
        try:
            yield self
        finally:
            self._flag = before

    def flush(self, alpha, keep255=False):
        """ONE FLUSH record over the union of the bounds of the layer commands since the previous flush (nothing when there
        are none): the layer is blended over the canvas at `alpha`, each pixel once however many commands painted it.
        keep255: a channel whose layer colour is exactly 255 keeps the canvas's byte."""
        pending, self._pending = self._pending, []
        if not pending:
            return
        x0, y0, x1, y1 = command_bounds(np.concatenate(pending, axis=0))
        live = (x0 <= x1) & (y0 <= y1)
        if not live.any():
            return
        before, self._flag = self._flag, 0  # the flush itself is never directed into the layer
        try:
            self._push(FLUSH, (0, 0, 0), alpha, [[int(x0[live].min()), int(y0[live].min()), int(x1[live].max()), int(y1[live].max()),
                                                   int(bool(keep255))]])
        finally:
            self._flag = before

    # ---- primitives
    def _push(self, kind, color, alpha, params):
        params = np.asarray(params, dtype=np.int64).reshape(-1, np.shape(params)[-1])
        rec = np.zeros((len(params), CMD_WORDS), dtype=np.int64)
        rec[:, 0] = kind | self._flag
        rec[:, 1:4] = np.asarray(color, dtype=np.int64).reshape(-1, 3)  # clamped with the coordinates, once, in build()
        rec[:, 4] = min(max(int(alpha), 0), 255)
        rec[:, 5 : 5 + params.shape[1]] = params
        if len(rec):
            self._chunks.append(rec)
            if self._flag:
                self._pending.append(rec)

    def segment(self, p0, p1, color, thickness=1, alpha=255):
        """Thick segment(s) with round caps; p0, p1: (x, y) or arrays [k][2]."""
        p0 = np.asarray(p0, dtype=np.int64).reshape(-1, 2)
        p1 = np.asarray(p1, dtype=np.int64).reshape(-1, 2)
        t = np.full((len(p0), 1), int(thickness), dtype=np.int64)
        self._push(SEG, color, alpha, np.concatenate([p0, p1, t], axis=1))

    def polyline(self, points, closed, color, thickness=1, alpha=255):
        """points: [k][2], or [n][k][2] for n polylines of k vertices each (n quads, closed: 4 n segments)."""
        pts = np.asarray(points, dtype=np.int64)
        if pts.size == 0:
            return
        pts = pts.reshape((-1,) + pts.shape[-2:])
        nxt = np.roll(pts, -1, axis=1)
        if not closed:
            pts, nxt = pts[:, :-1], nxt[:, :-1]
        self.segment(pts.reshape(-1, 2), nxt.reshape(-1, 2), color, thickness, alpha)

    def rectangle(self, box, color, thickness=1, alpha=255):
        """Outline of thickness t around (x1, y1, x2, y2): the outer box grows by t // 2, the hole shrinks by (t + 1) // 2.
        thickness < 0 fills, as in cv2.rectangle."""
        if int(thickness) < 0:
            return self.fill(box, color, alpha)
        b = np.asarray(box, dtype=np.int64).reshape(-1, 4)
        x1, x2 = np.minimum(b[:, 0], b[:, 2]), np.maximum(b[:, 0], b[:, 2])
        y1, y2 = np.minimum(b[:, 1], b[:, 3]), np.maximum(b[:, 1], b[:, 3])
        t = int(thickness)
        g, s = t // 2, (t + 1) // 2
        rec = np.stack([x1 - g, y1 - g, x2 + g, y2 + g, x1 + s, y1 + s, x2 - s, y2 - s], axis=1)
        self._push(BOX, color, alpha, rec)

    def fill(self, box, color, alpha=255):
        """Filled rectangle(s) (x1, y1, x2, y2), both corners included, blended with `alpha`."""
        b = np.asarray(box, dtype=np.int64).reshape(-1, 4)
        x1, x2 = np.minimum(b[:, 0], b[:, 2]), np.maximum(b[:, 0], b[:, 2])
        y1, y2 = np.minimum(b[:, 1], b[:, 3]), np.maximum(b[:, 1], b[:, 3])
        outer = np.stack([x1, y1, x2, y2], axis=1)
        hole = np.tile(np.array([1, 1, 0, 0], dtype=np.int64), (len(outer), 1))  # ix1 > ix2: no hole
        self._push(BOX, color, alpha, np.concatenate([outer, hole], axis=1))

    def rounded_fill(self, box, radius, color, alpha=255):
        """Filled rectangle(s) (x1, y1, x2, y2), both corners included, with corners of `radius` (clamped to half the shorter
        side by the rule of include/ymk.h), blended with `alpha`."""
        b = np.asarray(box, dtype=np.int64).reshape(-1, 4)
        x1, x2 = np.minimum(b[:, 0], b[:, 2]), np.maximum(b[:, 0], b[:, 2])
        y1, y2 = np.minimum(b[:, 1], b[:, 3]), np.maximum(b[:, 1], b[:, 3])
        self._push(RBOX, color, alpha, np.stack([x1, y1, x2, y2, np.full_like(x1, int(radius))], axis=1))

    def arrow(self, p0, p1, color, thickness=1, tip=10.0, alpha=255):
        """cv2.arrowedLine: the shaft, then two strokes of length `tip` (pixels) from p1 at +-45 degrees around the reversed
        direction, their far ends rounded half to even.  A zero-length arrow (or tip <= 0) has no tip."""
        x0, y0 = int(p0[0]), int(p0[1])
        x1, y1 = int(p1[0]), int(p1[1])
        self.segment((x0, y0), (x1, y1), color, thickness, alpha)
        if (x0, y0) == (x1, y1) or not tip > 0:
            return
        angle = np.arctan2(float(y0 - y1), float(x0 - x1))
        for side in (np.pi / 4, -np.pi / 4):
            px = int(np.rint(x1 + tip * np.cos(angle + side)))
            py = int(np.rint(y1 + tip * np.sin(angle + side)))
            self.segment((px, py), (x1, y1), color, thickness, alpha)

    def glyph(self, x, y, mask, color, key=None):
        """Blit one uint8 coverage mask [h][w] with its top-left corner at (x, y).  `key`: masks with equal keys are packed once."""
        key = id(mask) if key is None else key
        idx = self._mask_index.get(key)
        if idx is None:
            idx = self._mask_index[key] = len(self._masks)
            self._masks.append(np.ascontiguousarray(mask, dtype=np.uint8))
        gh, gw = self._masks[idx].shape
        self._push(GLYPH, color, 255, [[int(x), int(y), gw, gh, idx, gw]])

    def text(self, xy, string, font, color, direction="horizontal", anchor="la"):
        """One glyph per character from the pen position xy: the pen moves right by round(font.getlength(ch)), or - direction
        "vertical" - down by the font size.  anchor "la": xy is the top-left of the line (ImageDraw.text's default); "ls": xy
        lies on the baseline (cv2.putText's origin).  `font`: what load_font returned."""
        font, fkey = font
        pen_x, pen_y = int(xy[0]), int(xy[1])
        if anchor == "ls":
            pen_y -= int(font.getmetrics()[0])
        vertical, step = direction == "vertical", int(font.size)
        chars, rows = self._chars, []
        for ch in string:
            entry = chars.get((fkey, ch))
            if entry is None:  # first use in this drawing: pack the mask
                mask, ox, oy, advance = glyph_of(font, fkey, ch)
                idx = -1
                if mask.size:
                    idx = len(self._masks)
                    self._masks.append(mask)
                entry = chars[(fkey, ch)] = (idx, ox, oy, advance, mask.shape[1], mask.shape[0])
            idx, ox, oy, advance, gw, gh = entry
            if idx >= 0:
                rows.append((pen_x + ox, pen_y + oy, gw, gh, idx, gw))
            if vertical:
                pen_y += step
            else:
                pen_x += advance
        if rows:
            self._push(GLYPH, color, 255, rows)
        return pen_x, pen_y

    def heatmap(self, prob):
        """The detector's probability map (2-D, torch or numpy, any size), blended over the page before the commands."""
        self._heatmap = prob

    # ---- build + launch
    def _clamped(self):
        """The recorded commands, int64 [n][16]: every coordinate clipped into [-16383, 16383] (the range the kernel's 64-bit
        products are sized for), colours into 0..255."""
        cmds = np.concatenate(self._chunks, axis=0) if self._chunks else np.zeros((0, CMD_WORDS), dtype=np.int64)
        kind = _kinds(cmds[:, 0:1])  # with or without the layer flag
        words = np.arange(CMD_WORDS)[None, :]
        coord = ((kind == SEG) & (words >= 5) & (words <= 8)) | ((kind == BOX) & (words >= 5) & (words <= 12)) \
            | ((kind == GLYPH) & (words >= 5) & (words <= 6)) | (((kind == RBOX) | (kind == FLUSH)) & (words >= 5) & (words <= 8))
        cmds = np.where(coord, np.clip(cmds, -COORD_MAX, COORD_MAX), cmds)
        cmds[:, 1:4] = np.clip(cmds[:, 1:4], 0, 255)
        length = (kind[:, 0] == SEG) | (kind[:, 0] == RBOX)  # word 9 of both is a length (thickness, radius), not a coordinate
        cmds[length, 9] = np.clip(cmds[length, 9], 0, COORD_MAX)
        return cmds

    def build(self, h: int, w: int, tile=None):
        """The launch's host data: {"cmds": int32 [n][16], "atlas": uint8 [bytes], "tile_offsets", "tile_cmds"}."""
        tile = overlay_tile() if tile is None else int(tile)
        cmds = self._clamped()
        sizes = np.array([m.size for m in self._masks], dtype=np.int64)
        starts = np.cumsum(sizes) - sizes
        atlas = np.concatenate([m.reshape(-1) for m in self._masks]) if self._masks else np.zeros(0, dtype=np.uint8)
        is_glyph = _kinds(cmds[:, 0]) == GLYPH
        if is_glyph.any():
            cmds[is_glyph, 9] = starts[cmds[is_glyph, 9]]
        offsets, lists = bin_commands(cmds, h, w, tile)
        return {"cmds": cmds.astype(np.int32), "atlas": atlas, "tile_offsets": offsets, "tile_cmds": lists}

    def render(self, page, device=None):
        canvas, private = _to_device_page(page, device)
        if not private:
            canvas = canvas.clone()
        h, w = int(canvas.shape[0]), int(canvas.shape[1])
        data = self.build(h, w)
        self.canvas = draw_commands(canvas, data["cmds"], data["atlas"], heatmap=self._heatmap,
                                    lists=(data["tile_offsets"], data["tile_cmds"]))
        return self.canvas

    def to_host(self):
        return to_host(self.canvas)


def stage_commands(canvas, cmds, atlas=None, heatmap=None, lists=None):
    """Upload what the launches of one drawing read - commands (int32 [n][16], include/ymk.h), per-tile lists (binned here unless
    given), atlas and, with a heat map, the jet table - as ONE blob on the current stream.  Returns the launch arguments for
    `launch_staged`; the dict keeps the device buffers alive."""
    import torch

    from .. import _lib

    if not (isinstance(canvas, torch.Tensor) and canvas.is_cuda and canvas.dtype == torch.uint8 and canvas.is_contiguous()
            and canvas.ndim == 3 and canvas.shape[2] == 3):
        raise ValueError("overlay: canvas must be a contiguous uint8 H x W x 3 device tensor")
    h, w = int(canvas.shape[0]), int(canvas.shape[1])
    tile = int(_lib.load().ymk_overlay_tile())
    cmds = np.ascontiguousarray(np.asarray(cmds, dtype=np.int32).reshape(-1, CMD_WORDS))
    atlas = np.zeros(0, dtype=np.uint8) if atlas is None else np.ascontiguousarray(atlas, dtype=np.uint8).reshape(-1)
    offsets, tile_cmds = lists if lists is not None else bin_commands(cmds, h, w, tile)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    tile_cmds = np.ascontiguousarray(tile_cmds, dtype=np.int32)
    if len(offsets) != -(-h // tile) * -(-w // tile) + 1 or int(offsets[-1]) != len(tile_cmds):
        raise ValueError("overlay: the per-tile lists do not match the canvas")
    parts = [cmds.view(np.uint8).reshape(-1), offsets.view(np.uint8), tile_cmds.view(np.uint8), atlas]
    if heatmap is not None:
        parts.append(jet_table().reshape(-1))
    starts, size = [], 0
    for part in parts:  # every section starts on a 16-byte boundary
        starts.append(size)
        size += -(-part.size // 16) * 16
    blob = np.zeros(max(size, 16), dtype=np.uint8)
    for start, part in zip(starts, parts):
        blob[start : start + part.size] = part
    staged = {"h": h, "w": w, "n": len(cmds), "n_list": len(tile_cmds), "atlas_bytes": int(atlas.size), "prob": None}
    with torch.cuda.device(canvas.device):
        blob_dev = staged["blob"] = torch.from_numpy(blob).to(canvas.device)  # one H2D copy, ordered before the launches
        base = blob_dev.data_ptr()
        staged.update(cmds=base + starts[0], offsets=base + starts[1], lists=base + starts[2], atlas=base + starts[3] if atlas.size else None)
        if heatmap is not None:
            prob = heatmap if isinstance(heatmap, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(heatmap, dtype=np.float32))
            prob = prob.detach().to(device=canvas.device, dtype=torch.float32)
            staged["prob"] = prob.reshape(prob.shape[-2], prob.shape[-1]).contiguous()
            staged["jet"] = base + starts[4]
    return staged


def launch_staged(canvas, staged):
    """At most two launches on the current stream, IN PLACE on `canvas`: ymk_heatmap_blend, then ymk_draw_overlay."""
    import torch

    from .. import _lib

    lib = _lib.load()
    with torch.cuda.device(canvas.device):
        stream = _lib.current_stream_ptr()
        prob = staged["prob"]
        if prob is not None:
            _lib.check(lib.ymk_heatmap_blend(canvas.data_ptr(), staged["h"], staged["w"], prob.data_ptr(), int(prob.shape[0]),
                                             int(prob.shape[1]), staged["jet"], stream), "ymk_heatmap_blend")
        if staged["n"] and staged["n_list"]:
            _lib.check(lib.ymk_draw_overlay(canvas.data_ptr(), staged["h"], staged["w"], staged["cmds"], staged["n"], staged["offsets"],
                                            staged["lists"], staged["n_list"], staged["atlas"], staged["atlas_bytes"], stream),
                       "ymk_draw_overlay")
    return canvas


def draw_commands(canvas, cmds, atlas=None, heatmap=None, lists=None):
    """Apply a raw command array to `canvas` - a contiguous uint8 H x W x 3 device tensor - in place on the current stream."""
    return launch_staged(canvas, stage_commands(canvas, cmds, atlas, heatmap, lists))


# ------------------------------------------------------------------------------------------ the reference's five functions
def _finish(overlay, img, to_host_flag):
    canvas = overlay.render(img)
    return to_host(canvas) if to_host_flag else canvas


def det_visualizer(img, quads, preds=None, vis_heatmap=False, line_color=(0, 255, 0), to_host=True):
    """utils/visualizer.py:81-96: the optional heat map of preds["binary"], then every quad as a closed polyline, t = 1."""
    ov = Overlay()
    if vis_heatmap:
        binary = preds["binary"] if isinstance(preds, dict) else preds
        ov.heatmap(binary[0] if binary.ndim == 4 else binary)
    _det_commands(ov, quads, line_color)
    return _finish(ov, img, to_host)


def _det_commands(ov, quads, line_color=(0, 255, 0)):
    ov.polyline(np.asarray(quads, dtype=np.int64).reshape(-1, 4, 2), True, line_color, 1)


def rec_visualizer(img, outputs, font_path, font_size=12, font_color=(255, 0, 0), to_host=True):
    """utils/visualizer.py:207-250: every recognised line next to its quad - horizontal lines start at quad[0] + (0, -font_size),
    vertical lines at quad[0] + (-font_size, 0) and run downwards."""
    ov = Overlay()
    _rec_commands(ov, outputs, load_font(font_path, font_size), font_size, font_color)
    return _finish(ov, img, to_host)


def _rec_commands(ov, outputs, font, font_size, font_color):
    for pred, quad, direction in zip(outputs.contents, outputs.points, outputs.directions):
        x, y = int(quad[0][0]), int(quad[0][1])
        if direction == "vertical":
            ov.text((x - font_size, y), pred, font, font_color, direction="vertical")
        else:
            ov.text((x, y - font_size), pred, font, font_color)


def layout_visualizer(results, img, to_host=True):
    """utils/visualizer.py:99-125: per category the PALETTE colour, an outline of t = 2 and the label `category(role)` in the
    built-in font at 12 px with its baseline at (x1, y1)."""
    ov = Overlay()
    _layout_commands(ov, results)
    return _finish(ov, img, to_host)


def _layout_commands(ov, results):
    font = load_font(None, 12)
    for idx, (category, preds) in enumerate(results.model_dump().items()):
        color = PALETTE[idx % len(PALETTE)]
        for element in preds:
            role = element.get("role")
            x1, y1, x2, y2 = (int(v) for v in element["box"])
            ov.rectangle((x1, y1, x2, y2), color, 2)
            ov.text((x1, y1), category + ("" if role is None else f"({role})"), font, color, anchor="ls")


def table_visualizer(img, table, to_host=True):
    """utils/visualizer.py:128-152: cell outlines in (255, 0, 255), t = 2, labelled "[row, col] (RxC)" in (255, 0, 0)."""
    ov = Overlay()
    _table_commands(ov, table)
    return _finish(ov, img, to_host)


def _table_commands(ov, table):
    font = load_font(None, 12)
    for cell in table.cells:
        x1, y1, x2, y2 = (int(v) for v in cell.box)
        ov.rectangle((x1, y1, x2, y2), (255, 0, 255), 2)
        ov.text((x1, y1), f"[{cell.row}, {cell.col}] ({cell.row_span}x{cell.col_span})", font, (255, 0, 0), anchor="ls")


def tables_visualizer(img, tables, to_host=True):
    """table_visualizer for every table of a page in one launch (what TableStructureRecognizer's loop over tables draws)."""
    ov = Overlay()
    for table in tables:
        _table_commands(ov, table)
    return _finish(ov, img, to_host)


def _reading_order_commands(ov, elements, line_color, tip_size):
    font = load_font(None, 24)
    prev = None
    for i, element in enumerate(elements):
        x1, y1, x2, y2 = element.box
        cur = (x1 + (x2 - x1) / 2, y1 + (y2 - y1) / 2)
        ov.text((int(cur[0]), int(cur[1])), str(i), font, (0, 200, 0), anchor="ls")
        if prev is not None:
            length = float(np.linalg.norm(np.array(cur) - np.array(prev)))
            p0, p1 = (int(prev[0]), int(prev[1])), (int(cur[0]), int(cur[1]))
            # cv2.arrowedLine scales tipLength = tip_size / length by the length of the INTEGER end points
            tip = float(np.hypot(p0[0] - p1[0], p0[1] - p1[1])) * tip_size / length if length > 0 else 0.0
            ov.arrow(p0, p1, line_color, 2, tip=tip)
        prev = cur


def reading_order_visualizer(img, results, line_color=(0, 0, 255), tip_size=10, visualize_figure_letter=False, to_host=True):
    """utils/visualizer.py:11-78: the order number of every paragraph, table and figure at its centre (24 px) and an arrow of
    t = 2 from each element's centre to the next one's."""
    ov = Overlay()
    _page_order_commands(ov, results, line_color, tip_size, visualize_figure_letter)
    return _finish(ov, img, to_host)


def _page_order_commands(ov, results, line_color=(0, 0, 255), tip_size=10, visualize_figure_letter=False):
    elements = sorted(results.paragraphs + results.tables + results.figures, key=lambda e: e.order)
    _reading_order_commands(ov, elements, line_color, tip_size)
    if visualize_figure_letter:
        for figure in results.figures:
            _reading_order_commands(ov, figure.paragraphs, (0, 255, 0), 5)


# --------------------------------------------------------------------------------- the table-semantic parser's drawings
CELL_COLORS = {"cell": (255, 128, 0), "empty": (255, 0, 255), "header": (0, 255, 0), "group": (255, 255, 0)}
UNKNOWN_ROLE_COLOR = (200, 200, 200)
TINTED_ROLES = ("cell", "empty", "header")


def _cell_commands(ov, cells, groups=None):
    """cell_detector_visualizer's first image on `ov` (and, with `groups`, its second on that recorder): the cell / empty /
    header boxes go opaquely into the layer - a later cell overwrites an earlier one where they overlap or share a border row -
    and ONE flush blends the layer over the page at 77 / 255, leaving the channels whose tint is 255 alone (the reference
    compares its fill image with 255 per channel).  Then the outlines, t = 2, in the role's colour."""
    cells = list(cells)
    with ov.layer():
        for cell in cells:
            if cell.role in TINTED_ROLES:
                ov.fill([int(v) for v in cell.box], CELL_COLORS[cell.role])
    ov.flush(77, keep255=True)
    for cell in cells:
        target = groups if cell.role == "group" else ov
        if target is not None:
            target.rectangle([int(v) for v in cell.box], CELL_COLORS.get(cell.role, UNKNOWN_ROLE_COLOR), 2)


def cell_detector_visualizer(img1, img2, cells, to_host=True):
    """utils/visualizer.py:155-204: (img1 with the cells tinted by role and outlined, img2 with the outlines of the group cells)."""
    cells = list(cells)
    ov1, ov2 = Overlay(), Overlay()
    _cell_commands(ov1, cells, ov2)
    return _finish(ov1, img1, to_host), _finish(ov2, img2, to_host)


def _link_commands(ov, box_u, box_v, direction, color):
    """One arrow of t = 2 from box_u to box_v, centre to centre - but on the axis ACROSS the contact both ends move to the
    middle of the band the two boxes share, so a link to a spanning cell stays horizontal / vertical.  direction "R" / "D":
    the contact is known; None: a horizontal link when the boxes share rows and their centres differ in x (compared as
    integers), else a vertical one when they share columns.  The tip is min(0.2, 12 / length) of the arrow's length, the ratio
    taken from the exact centres and applied, as cv2.arrowedLine does, to the length between the integer end points."""
    cx1, cy1 = (box_u[0] + box_u[2]) / 2, (box_u[1] + box_u[3]) / 2
    cx2, cy2 = (box_v[0] + box_v[2]) / 2, (box_v[1] + box_v[3]) / 2
    y_lo, y_hi = max(box_u[1], box_v[1]), min(box_u[3], box_v[3])
    x_lo, x_hi = max(box_u[0], box_v[0]), min(box_u[2], box_v[2])
    if direction is None:
        direction = "R" if y_lo < y_hi and int(cx1) != int(cx2) else "D"
    if direction == "R" and y_lo < y_hi:
        cy1 = cy2 = (y_lo + y_hi) / 2
    elif direction == "D" and x_lo < x_hi:
        cx1 = cx2 = (x_lo + x_hi) / 2
    length = max(1.0, float(np.hypot(cx2 - cx1, cy2 - cy1)))
    p0, p1 = (int(cx1), int(cy1)), (int(cx2), int(cy2))
    ov.arrow(p0, p1, color, 2, tip=min(0.2, 12.0 / length) * float(np.hypot(p1[0] - p0[0], p1[1] - p0[1])))


def _kv_commands(ov, table):
    cells = table.cells
    for kv in table.kv_items:
        keys = [kv.key] if isinstance(kv.key, str) else list(kv.key)
        chain = [k for k in keys if k in cells] + ([kv.value] if kv.value in cells else [])
        for u, v in zip(chain, chain[1:]):
            _link_commands(ov, cells[u].box, cells[v].box, None, (0, 255, 0))


def kv_items_visualizer(table, img, to_host=True):
    """table_semantic_parser.py:537-577: every kv item's chain key[0] -> ... -> value as green arrows between the cells."""
    ov = Overlay()
    _kv_commands(ov, table)
    return _finish(ov, img, to_host)


def _dag_commands(ov, dag):
    for u, v, attrs in dag.edges():  # OrderedDiGraph: (u, v, attributes)
        if attrs["dir"] in ("L", "U"):
            continue
        right = attrs["dir"] == "R"
        _link_commands(ov, dag.nodes[u]["bbox"], dag.nodes[v]["bbox"], "R" if right else "D", (0, 255, 0) if right else (255, 0, 0))


def dag_visualizer(dag, img, to_host=True):
    """table_semantic_parser.py:580-620: the grid graph's R edges (0, 255, 0) and D edges (255, 0, 0); L and U are their mirrors."""
    ov = Overlay()
    _dag_commands(ov, dag)
    return _finish(ov, img, to_host)


def text_box(font, string):
    """(left, top, right, bottom), right and bottom excluded, of `string` drawn horizontally with the pen at (0, 0) under the
    text rule above: the union of the placed glyph boxes; (0, 0, 0, 0) for a string without pixels."""
    font_obj, fkey = font
    pen, boxes = 0, []
    for ch in string:
        mask, ox, oy, advance = glyph_of(font_obj, fkey, ch)
        if mask.size:
            boxes.append((pen + ox, oy, pen + ox + mask.shape[1], oy + mask.shape[0]))
        pen += advance
    if not boxes:
        return 0, 0, 0, 0
    return min(b[0] for b in boxes), min(b[1] for b in boxes), max(b[2] for b in boxes), max(b[3] for b in boxes)


def _cell_id_commands(ov, tables, font, font_size):
    pad = radius = max(2, font_size // 5)
    for table in tables:
        cells = table.cells.values() if isinstance(table.cells, dict) else table.cells
        for cell in cells:
            if cell.role == "group" or cell.id is None:
                continue
            label = str(cell.id)
            left, top, right, bottom = text_box(font, label)
            bx, by = int(cell.box[0]) + 2, int(cell.box[1]) + 2
            ov.rounded_fill((bx, by, bx + right - left + 2 * pad, by + bottom - top + 2 * pad), radius, (40, 40, 40), alpha=200)
            ov.text((bx + pad - left, by + pad - top), label, font, (255, 255, 255))


def cell_id_visualizer(img, tables, font_path, font_size=None, to_host=True):
    """utils/visualizer.py:254-295: the id of every non-group cell as a chip - a rounded dark box at alpha 200 with the id in
    white - at the cell's top-left corner + (2, 2)."""
    page = device_page(img)
    font_size = max(14, int(page.shape[1]) // 75) if font_size is None else int(font_size)
    ov = Overlay()
    _cell_id_commands(ov, tables, load_font(font_path, font_size), font_size)
    return _finish(ov, page, to_host)


def _semantic_layout_commands(ov, results, dags=()):
    """TableSemanticParser's layout image (table_semantic_parser.py:795-830, :986-989): tables, then paragraphs, boxed in green
    with their id; per table the tinted cells (a flush of its own), its kv arrows and its grid boxes; the grid graphs."""
    font = load_font(None, 19)  # cv2.putText at scale 0.8
    for prefix, elements in (("Table", results.tables), ("Paragraph", results.paragraphs)):
        for element in elements:
            x1, y1, x2, y2 = (int(v) for v in element.box)
            ov.rectangle((x1, y1, x2, y2), (0, 255, 0), 2)
            ov.text((x1, y1 - 10), f"{prefix}: {element.id}", font, (255, 0, 0), anchor="ls")
    for table in results.tables:
        _cell_commands(ov, table.cells.values())
        _kv_commands(ov, table)
        for grid in table.grids:
            ov.rectangle([int(v) for v in grid.box], (255, 0, 0), 3)
    for dag in dags:
        _dag_commands(ov, dag)


def _semantic_ocr_commands(ov, results, font, font_size, font_color):
    """TableSemanticParser's OCR image (table_semantic_parser.py:335-387): per word its quad, closed, in green, then its text
    placed as rec_visualizer places a line."""
    for word in results.words:
        quad = np.asarray(word.points).astype(np.int32)
        ov.polyline(quad.reshape(4, 2), True, (0, 255, 0), 1)
        x, y = int(quad[0][0]), int(quad[0][1])
        if word.direction == "vertical":
            ov.text((x - font_size, y), word.content, font, font_color, direction="vertical")
        else:
            ov.text((x, y - font_size), word.content, font, font_color)


# ------------------------------------------------------------------------------- a wave of canvases (serve(overlays=True))
# The per-page path above spends its time on the host: a Python loop per character and a sort over the per-tile lists
# (DESIGN.md "Overlay rasteriser").  Here the host records text as RUNS and reserves one command slot per character;
# ymk_overlay_layout places the glyphs and computes every command's clipped bounding box, ymk_draw_overlay_pages culls per
# tile and draws all canvases of a wave in one launch (include/ymk.h).
RUN_WORDS, GLYPH_WORDS, CANVAS_WORDS = 8, 6, 6  # YMK_OVERLAY_RUN_WORDS / _GLYPH_WORDS / _CANVAS_WORDS
PEN_MAX = 1 << 30  # pens are int32 on the device; a pen this far out has left the clamp range for good


class GlyphStore:
    """Glyph table and atlas of every font drawn through the wave path: glyph id -> (atlas offset, w, h, x offset, y offset,
    advance), ids and offsets handed out once and never moved (append-only).  The host mirror serves the code point -> glyph id
    lookup (`ids`: one searchsorted per font; a code point seen for the first time goes through `glyph_of`); `tensors` keeps a
    device copy up to date.  A device tensor is only ever appended to past what earlier launches can reference, and replaced -
    never resized - when it is full, so a wave in flight stays valid as long as it holds the tensors it launched with."""

    def __init__(self):
        self._lock = threading.Lock()
        self._fonts = {}                                    # font key -> (sorted code points int64, glyph ids int32)
        self._table = np.zeros((256, GLYPH_WORDS), np.int32)
        self._atlas = np.zeros(1 << 16, np.uint8)
        self.n_glyphs = 0
        self.atlas_bytes = 0
        self._dev = {}                                      # device -> [table tensor, rows uploaded, atlas tensor, bytes uploaded]

    @staticmethod
    def _lookup(entry, codes):
        cps, gids = entry
        if len(cps) == 0:
            return np.full(len(codes), -1, np.int32), np.zeros(len(codes), bool)
        pos = np.minimum(np.searchsorted(cps, codes), len(cps) - 1)
        return gids[pos], cps[pos] == codes

    def ids(self, font, codes):
        """Glyph ids (int32) of the code points `codes` (integer array) in `font` (what load_font returned)."""
        font_obj, fkey = font
        codes = np.asarray(codes, dtype=np.int64)
        with self._lock:
            entry = self._fonts.get(fkey) or (np.zeros(0, np.int64), np.zeros(0, np.int32))
            gids, hit = self._lookup(entry, codes)
            if not hit.all():
                entry = self._fonts[fkey] = self._append(font_obj, fkey, entry, np.unique(codes[~hit]))
                gids, hit = self._lookup(entry, codes)
            return gids

    def _append(self, font_obj, fkey, entry, missing):
        """Slow path: rasterise the code points `missing` (sorted, unique) and append them to the table and the atlas."""
        new_ids = []
        for cp in missing.tolist():
            mask, ox, oy, advance = glyph_of(font_obj, fkey, chr(cp))
            gh, gw = mask.shape
            if self.n_glyphs == len(self._table):
                self._table = np.concatenate([self._table, np.zeros_like(self._table)])
            while self.atlas_bytes + mask.size > len(self._atlas):
                self._atlas = np.concatenate([self._atlas, np.zeros_like(self._atlas)])
            self._table[self.n_glyphs] = (self.atlas_bytes, gw, gh, ox, oy, advance)
            self._atlas[self.atlas_bytes : self.atlas_bytes + mask.size] = mask.reshape(-1)
            new_ids.append(self.n_glyphs)
            self.n_glyphs += 1
            self.atlas_bytes += mask.size
        cps = np.concatenate([entry[0], missing])
        gids = np.concatenate([entry[1], np.asarray(new_ids, np.int32)])
        order = np.argsort(cps, kind="stable")
        return cps[order], gids[order]

    def host(self):
        """(glyph table int32 [n][6], atlas uint8 [bytes]) as they stand."""
        with self._lock:
            return self._table[: self.n_glyphs].copy(), self._atlas[: self.atlas_bytes].copy()

    def tensors(self, device):
        """(table tensor, n_glyphs, atlas tensor, atlas_bytes) on `device`, holding everything `ids` has handed out so far."""
        import torch

        device = torch.device(device)
        with self._lock:
            st = self._dev.get(device)
            if st is None:
                st = self._dev[device] = [None, 0, None, 0]
            if st[1] < self.n_glyphs or st[3] < self.atlas_bytes or st[0] is None:
                with torch.cuda.device(device):
                    if st[0] is None or st[0].shape[0] < self.n_glyphs:  # full: a new tensor; the old one lives on with its waves
                        st[0], st[1] = torch.zeros((len(self._table), GLYPH_WORDS), dtype=torch.int32, device=device), 0
                    if st[2] is None or st[2].shape[0] < self.atlas_bytes:
                        st[2], st[3] = torch.zeros(len(self._atlas), dtype=torch.uint8, device=device), 0
                    if st[1] < self.n_glyphs:
                        st[0][st[1] : self.n_glyphs].copy_(torch.from_numpy(self._table[st[1] : self.n_glyphs].copy()))
                    if st[3] < self.atlas_bytes:
                        st[2][st[3] : self.atlas_bytes].copy_(torch.from_numpy(self._atlas[st[3] : self.atlas_bytes].copy()))
                    st[1], st[3] = self.n_glyphs, self.atlas_bytes
                    torch.cuda.current_stream().synchronize()  # rare (a glyph seen for the first time): visible to every stream
            return st[0], st[1], st[2], st[3]


_STORE = GlyphStore()


def glyph_store() -> GlyphStore:
    """The process's glyph store."""
    return _STORE


class RunOverlay(Overlay):
    """Overlay's drawing methods for the wave path.  `text` records a RUN - first slot, pen, direction, font, string - and
    reserves one GLYPH slot per character; the records of those slots (kind, colour) are written for all runs at once when the
    wave is built (np.repeat), and the device lays the characters out.  A single rectangle is recorded as plain integers.
    There is no per-character work on the host and no array is made per call.  `text` returns None (the pen's end is only
    known on the device); `glyph` and `heatmap` are not part of the wave path."""

    def __init__(self):
        super().__init__()
        self._n = 0
        self._at = []     # first slot of every block of self._chunks
        self._boxes = []  # (slot, r, g, b, alpha, eight BOX words) of rectangles given as four numbers
        self._runs = []   # (first slot, count, pen x, pen y, vertical, step, font, string, colour)

    def _push(self, kind, color, alpha, params):
        before = len(self._chunks)
        super()._push(kind, color, alpha, params)
        if len(self._chunks) > before:
            self._at.append(self._n)
            self._n += len(self._chunks[-1])

    def __len__(self):
        return self._n

    def glyph(self, *args, **kwargs):
        raise NotImplementedError("RunOverlay draws text through runs; free-standing masks go through Overlay")

    def heatmap(self, prob):
        raise NotImplementedError("the wave path draws no heat map")

    def render(self, page, device=None):
        raise NotImplementedError("a RunOverlay is drawn with its wave: render_wave / draw_wave")

    def build(self, h, w, tile=None):
        raise NotImplementedError("a RunOverlay is built with its wave: build_wave")

    def rectangle(self, box, color, thickness=1, alpha=255):
        if int(thickness) < 0 or np.ndim(box) != 1 or np.ndim(color) != 1 or self._flag:
            return super().rectangle(box, color, thickness, alpha)
        xa, ya, xb, yb = (int(v) for v in box)  # Overlay.rectangle for one box, in plain integers
        x1, x2, y1, y2 = min(xa, xb), max(xa, xb), min(ya, yb), max(ya, yb)
        t = int(thickness)
        g, s = t // 2, (t + 1) // 2
        self._boxes.append((self._n, int(color[0]), int(color[1]), int(color[2]), min(max(int(alpha), 0), 255),
                            x1 - g, y1 - g, x2 + g, y2 + g, x1 + s, y1 + s, x2 - s, y2 - s))
        self._n += 1

    def text(self, xy, string, font, color, direction="horizontal", anchor="la"):
        n = len(string)
        if n == 0:
            return None
        if self._flag:  # flush needs the bounds of what was painted; a run's are only known on the device
            raise NotImplementedError("RunOverlay: text cannot be directed into the layer")
        font_obj = font[0]
        pen_x, pen_y = int(xy[0]), int(xy[1])
        if anchor == "ls":
            pen_y -= int(font_obj.getmetrics()[0])
        self._runs.append((self._n, n, min(max(pen_x, -PEN_MAX), PEN_MAX), min(max(pen_y, -PEN_MAX), PEN_MAX),
                           direction == "vertical", int(font_obj.size), font, string, color))
        self._n += n
        return None

    def _clamped(self):
        """The records of this drawing, int64 [n][16], clamped as Overlay's; the text slots carry kind, colour and alpha."""
        self._chunks, blocks, at = [], self._chunks, self._at
        try:
            if self._boxes:
                boxes = np.asarray(self._boxes, dtype=np.int64)
                rec = np.zeros((len(boxes), CMD_WORDS), dtype=np.int64)
                rec[:, 0] = BOX
                rec[:, 1:13] = boxes[:, 1:]
                blocks, at = blocks + [rec], at + [boxes[:, 0]]
            self._chunks = blocks
            drawn = super()._clamped()  # every block that is not text, in the order of `blocks`
        finally:
            self._chunks = self._chunks[: len(self._at)]
        out = np.zeros((self._n, CMD_WORDS), dtype=np.int64)
        if len(drawn):
            out[np.concatenate([np.arange(len(b)) + a if np.ndim(a) == 0 else a for b, a in zip(blocks, at)])] = drawn
        if self._runs:
            first = np.asarray([r[0] for r in self._runs], dtype=np.int64)
            counts = np.asarray([r[1] for r in self._runs], dtype=np.int64)
            colours = np.clip(np.asarray([r[8] for r in self._runs], dtype=np.int64).reshape(-1, 3), 0, 255)
            slots = np.repeat(first - (np.cumsum(counts) - counts), counts) + np.arange(int(counts.sum()))
            out[slots, 0] = GLYPH
            out[slots, 1:4] = np.repeat(colours, counts, axis=0)
            out[slots, 4] = 255
        return out


def build_wave(drawings, sizes, offsets=None, store=None):
    """Host data of one wave: `drawings` - one RunOverlay per canvas - on canvases of `sizes` [(h, w)] that start at byte
    `offsets` of the canvas buffer (default: packed, each on a 16-byte boundary).
    {"cmds" int32 [n][16], "table" int64 [canvases][6], "runs" int32 [runs][8], "codes" int32 [characters], "tiles", "bytes"}."""
    store = _STORE if store is None else store
    tile = overlay_tile()
    table = np.zeros((len(drawings), CANVAS_WORDS), dtype=np.int64)
    parts, runs, strings, fonts, font_of_run = [], [], [], {}, []
    first = tiles = at = 0
    for ci, (ov, (h, w)) in enumerate(zip(drawings, sizes)):
        h, w = int(h), int(w)
        if offsets is None:
            off, at = at, at + -(-(h * w * 3) // 16) * 16
        else:
            off = int(offsets[ci])
            at = max(at, off + h * w * 3)
        table[ci] = (off, h, w, first, len(ov), tiles)
        if len(ov):
            parts.append(ov._clamped())
        for slot, n, pen_x, pen_y, vertical, step, font, string, _ in ov._runs:
            runs.append((first + slot, 0, n, pen_x, pen_y, int(vertical), step, 0))
            strings.append(string)
            font_of_run.append(fonts.setdefault(font[1], (len(fonts), font))[0])
        first += len(ov)
        tiles += -(-h // tile) * -(-w // tile)
    cmds = np.concatenate(parts, axis=0).astype(np.int32) if parts else np.zeros((0, CMD_WORDS), dtype=np.int32)
    runs = np.asarray(runs, dtype=np.int32).reshape(-1, RUN_WORDS)
    # every string of the wave as code points in one pass; glyph ids by one sorted lookup per font
    points = np.frombuffer("".join(strings).encode("utf-32-le", "surrogatepass"), dtype="<u4").astype(np.int64)
    codes = np.zeros(len(points), dtype=np.int32)
    if len(runs):
        counts = runs[:, 2].astype(np.int64)
        runs[:, 1] = np.cumsum(counts) - counts
        which = np.repeat(np.asarray(font_of_run, dtype=np.int64), counts)
        for fi, font in fonts.values():
            sel = which == fi
            codes[sel] = store.ids(font, points[sel])
    return {"cmds": cmds, "table": table, "runs": runs, "codes": codes, "tiles": tiles, "bytes": at}


def launch_wave(canvas_buf, cmds, table, runs=None, codes=None, glyphs=None, atlas=None):
    """Two library calls on the current stream, in place on `canvas_buf` (a contiguous 1-D uint8 device tensor that holds the
    canvases `table` describes): ymk_overlay_layout, ymk_draw_overlay_pages.  cmds / table / runs / codes: host arrays as
    build_wave returns them, uploaded as ONE blob; glyphs / atlas: the glyph table and the atlas, device tensors (GlyphStore.
    tensors) or host arrays (uploaded with the blob).  Returns a dict that keeps every device buffer of the launches alive
    ("cmds_dev" int32 [n][16] and "bounds_dev" int16 [n][4] are what the layout call wrote)."""
    import torch

    from .. import _lib

    lib = _lib.load()
    if not (isinstance(canvas_buf, torch.Tensor) and canvas_buf.is_cuda and canvas_buf.dtype == torch.uint8 and canvas_buf.ndim == 1
            and canvas_buf.is_contiguous()):
        raise ValueError("overlay: the canvas buffer must be a contiguous 1-D uint8 device tensor")
    tile = int(lib.ymk_overlay_tile())
    cmds = np.ascontiguousarray(np.asarray(cmds, dtype=np.int32).reshape(-1, CMD_WORDS))
    table = np.ascontiguousarray(np.asarray(table, dtype=np.int64).reshape(-1, CANVAS_WORDS))
    runs = np.zeros((0, RUN_WORDS), np.int32) if runs is None else np.ascontiguousarray(np.asarray(runs, dtype=np.int32).reshape(-1, RUN_WORDS))
    codes = np.zeros(0, np.int32) if codes is None else np.ascontiguousarray(codes, dtype=np.int32).reshape(-1)
    total_tiles = 0
    for off, h, w, first, count, tile0 in table.tolist():  # the kernels ignore an entry that does not fit; here it is a caller's bug
        if not (0 < h <= COORD_MAX and 0 < w <= COORD_MAX and 0 <= off and off + h * w * 3 <= canvas_buf.numel()
                and 0 <= first and 0 <= count and first + count <= len(cmds) and tile0 == total_tiles):
            raise ValueError("overlay: the canvas table does not match the canvas buffer, the commands or the tile numbering")
        total_tiles += -(-h // tile) * -(-w // tile)
    host = {"cmds": cmds, "table": table, "runs": runs, "codes": codes}
    dev_glyphs = isinstance(glyphs, torch.Tensor)
    if not dev_glyphs:
        host["glyphs"] = np.zeros((0, GLYPH_WORDS), np.int32) if glyphs is None else np.ascontiguousarray(np.asarray(glyphs, dtype=np.int32).reshape(-1, GLYPH_WORDS))
        host["atlas"] = np.zeros(0, np.uint8) if atlas is None else np.ascontiguousarray(atlas, dtype=np.uint8).reshape(-1)
    starts, size = {}, 0
    for name, part in host.items():  # every section starts on a 16-byte boundary
        starts[name] = size
        size += -(-part.nbytes // 16) * 16
    blob = np.zeros(max(size, 16), dtype=np.uint8)
    for name, part in host.items():
        blob[starts[name] : starts[name] + part.nbytes] = part.view(np.uint8).reshape(-1)
    out = {"n": len(cmds), "tiles": total_tiles}
    with torch.cuda.device(canvas_buf.device):
        blob_dev = out["blob"] = torch.from_numpy(blob).to(canvas_buf.device)  # one H2D copy, ordered before the launches
        base = blob_dev.data_ptr()
        if dev_glyphs:
            out["glyphs"], out["atlas"] = glyphs, atlas
            n_glyphs, atlas_bytes = int(glyphs.shape[0]), int(atlas.numel()) if atlas is not None else 0
            glyphs_ptr, atlas_ptr = glyphs.data_ptr(), atlas.data_ptr() if atlas_bytes else None
        else:
            n_glyphs, atlas_bytes = len(host["glyphs"]), int(host["atlas"].size)
            glyphs_ptr, atlas_ptr = base + starts["glyphs"], base + starts["atlas"] if atlas_bytes else None
        n = len(cmds)
        out["cmds_dev"] = blob_dev[starts["cmds"] : starts["cmds"] + cmds.nbytes].view(torch.int32).view(-1, CMD_WORDS)
        bounds = out["bounds_dev"] = torch.zeros((n, 4), dtype=torch.int16, device=canvas_buf.device)
        stream = _lib.current_stream_ptr()
        # the two calls' arguments up to the stream (tools/overlay_timing.py times each call on its own)
        out["layout_args"] = (base + starts["cmds"], n, bounds.data_ptr(), base + starts["runs"], len(runs), base + starts["codes"],
                              len(codes), glyphs_ptr, n_glyphs, base + starts["table"], len(table))
        out["draw_args"] = (canvas_buf.data_ptr(), canvas_buf.numel(), base + starts["table"], len(table), total_tiles,
                            base + starts["cmds"], n, bounds.data_ptr(), atlas_ptr, atlas_bytes)
        if n:
            _lib.check(lib.ymk_overlay_layout(*out["layout_args"], stream), "ymk_overlay_layout")
            _lib.check(lib.ymk_draw_overlay_pages(*out["draw_args"], stream), "ymk_draw_overlay_pages")
    return out


def draw_wave(canvas_buf, drawings, sizes, offsets=None, store=None):
    """`drawings` (one RunOverlay per canvas) onto the canvases of `sizes` inside `canvas_buf`, in place on the current stream."""
    store = _STORE if store is None else store
    data = build_wave(drawings, sizes, offsets, store)
    glyphs, n_glyphs, atlas, atlas_bytes = store.tensors(canvas_buf.device)  # after build_wave: it may have added glyphs
    out = launch_wave(canvas_buf, data["cmds"], data["table"], data["runs"], data["codes"], glyphs[:n_glyphs], atlas[:atlas_bytes])
    out["store"] = (glyphs, atlas)
    return out


def render_wave(pages, drawings, pinned=None, store=None):
    """One canvas per entry of `pages` (uint8 H x W x 3 device tensors; a page may appear several times, it is never drawn
    on) with the RunOverlay of the same index drawn over it: one batched clone into a canvas buffer, one blob upload, the
    two launches, one copy of all canvases to pinned memory, one wait for the stream.  Returns owned np.ndarrays.
    `pinned`: a one-element list the caller keeps per wave slot; its pinned buffer is reused while it is large enough."""
    import torch

    sizes = [(int(p.shape[0]), int(p.shape[1])) for p in pages]
    for p in pages:
        if not (p.is_cuda and p.dtype == torch.uint8 and p.ndim == 3 and p.shape[2] == 3):
            raise ValueError("overlay: a page must be a uint8 H x W x 3 device tensor")
    data_bytes = [h * w * 3 for h, w in sizes]
    offsets = np.cumsum([0] + [-(-b // 16) * 16 for b in data_bytes])
    total = int(offsets[-1])
    device = pages[0].device
    with torch.cuda.device(device):
        buf = torch.empty(max(total, 16), dtype=torch.uint8, device=device)
        views = [buf[int(o) : int(o) + b].view(h, w, 3) for o, b, (h, w) in zip(offsets, data_bytes, sizes)]
        torch._foreach_copy_(views, [p.contiguous() for p in pages])
        staged = draw_wave(buf, drawings, sizes, offsets[:-1], store)
        pinned = [None] if pinned is None else pinned
        if pinned[0] is None or pinned[0].numel() < buf.numel():
            pinned[0] = torch.empty(buf.numel(), dtype=torch.uint8, pin_memory=True)
        host = pinned[0][: buf.numel()]
        host.copy_(buf, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        del staged
        arr = host.numpy()
        return [arr[int(o) : int(o) + b].reshape(h, w, 3).copy() for o, b, (h, w) in zip(offsets, data_bytes, sizes)]
