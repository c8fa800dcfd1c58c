"""visualize=True: the reference's overlays (utils/visualizer.py:11-250) drawn on the device.

The reference draws with OpenCV and Pillow on host copies of the page.  Here a drawing is an ordered list of fixed-size int32
commands - thick segments, boxes with an optional hole, glyph blits - that ONE launch of ymk_draw_overlay applies to a device
copy of the page (include/ymk.h has the record layout and the exact pixel rules, DESIGN.md "Overlay rasteriser" the design).
The host's share is building the list, packing the glyph masks Pillow rasterises into an atlas, and binning the commands by
bounding box into per-tile lists; all of it travels to the device as one staged blob.  The page the networks read is never
drawn on: `Overlay.render` clones it.

The overlays are equivalent in content to the reference's (same elements, colours, thicknesses, label strings, anchor
points), not byte-identical: OpenCV's Hershey font and Bresenham rules are replaced by the rules of include/ymk.h and by
Pillow glyphs.  Colour tuples are applied to the canvas's channels in the order given, as cv2 and ImageDraw do.

The five functions keep the reference's names and arguments and return np.ndarray; `img` may also be a device tensor, and
`to_host=False` (not in the reference) returns the device canvas instead, which is how the modules chain overlays without a
round trip through the host.
"""

from __future__ import annotations

import logging
import os
import threading

import numpy as np

logger = logging.getLogger(__name__)

CMD_WORDS = 16  # YMK_OVERLAY_CMD_WORDS
SEG, BOX, GLYPH = 0, 1, 2  # YMK_OVERLAY_SEG / _BOX / _GLYPH
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
def command_bounds(cmds: np.ndarray):
    """Inclusive bounding box (x0, y0, x1, y1; int64 arrays) of every command; x1 < x0 for one that covers nothing."""
    c = np.asarray(cmds, dtype=np.int64).reshape(-1, CMD_WORDS)
    kind = c[:, 0]
    pad = (c[:, 9] + 1) // 2  # a segment reaches t / 2 from its axis
    seg = (np.minimum(c[:, 5], c[:, 7]) - pad, np.minimum(c[:, 6], c[:, 8]) - pad,
           np.maximum(c[:, 5], c[:, 7]) + pad, np.maximum(c[:, 6], c[:, 8]) + pad)
    box = (c[:, 5], c[:, 6], c[:, 7], c[:, 8])
    glyph = (c[:, 5], c[:, 6], c[:, 5] + c[:, 7] - 1, c[:, 6] + c[:, 8] - 1)
    none = (np.ones_like(kind), np.ones_like(kind), np.zeros_like(kind), np.zeros_like(kind))
    return tuple(np.where(kind == SEG, s, np.where(kind == BOX, b, np.where(kind == GLYPH, g, e)))
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
        self.canvas = None

    def __len__(self):
        return sum(len(c) for c in self._chunks)

    # ---- primitives
    def _push(self, kind, color, alpha, params):
        params = np.asarray(params, dtype=np.int64).reshape(-1, np.shape(params)[-1])
        rec = np.zeros((len(params), CMD_WORDS), dtype=np.int64)
        rec[:, 0] = kind
        rec[:, 1:4] = np.asarray(color, dtype=np.int64).reshape(-1, 3)  # clamped with the coordinates, once, in build()
        rec[:, 4] = min(max(int(alpha), 0), 255)
        rec[:, 5 : 5 + params.shape[1]] = params
        if len(rec):
            self._chunks.append(rec)

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
    def build(self, h: int, w: int, tile=None):
        """The launch's host data: {"cmds": int32 [n][16], "atlas": uint8 [bytes], "tile_offsets", "tile_cmds"}."""
        tile = overlay_tile() if tile is None else int(tile)
        cmds = np.concatenate(self._chunks, axis=0) if self._chunks else np.zeros((0, CMD_WORDS), dtype=np.int64)
        # every coordinate into [-16383, 16383] (the range the kernel's 64-bit products are sized for), colours into 0..255
        kind = cmds[:, 0:1]
        words = np.arange(CMD_WORDS)[None, :]
        coord = ((kind == SEG) & (words >= 5) & (words <= 8)) | ((kind == BOX) & (words >= 5) & (words <= 12)) \
            | ((kind == GLYPH) & (words >= 5) & (words <= 6))
        cmds = np.where(coord, np.clip(cmds, -COORD_MAX, COORD_MAX), cmds)
        cmds[:, 1:4] = np.clip(cmds[:, 1:4], 0, 255)
        seg_t = cmds[:, 0] == SEG
        cmds[seg_t, 9] = np.clip(cmds[seg_t, 9], 0, COORD_MAX)
        sizes = np.array([m.size for m in self._masks], dtype=np.int64)
        starts = np.cumsum(sizes) - sizes
        atlas = np.concatenate([m.reshape(-1) for m in self._masks]) if self._masks else np.zeros(0, dtype=np.uint8)
        is_glyph = cmds[:, 0] == GLYPH
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
    ov.polyline(np.asarray(quads, dtype=np.int64).reshape(-1, 4, 2), True, line_color, 1)
    return _finish(ov, img, to_host)


def rec_visualizer(img, outputs, font_path, font_size=12, font_color=(255, 0, 0), to_host=True):
    """utils/visualizer.py:207-250: every recognised line next to its quad - horizontal lines start at quad[0] + (0, -font_size),
    vertical lines at quad[0] + (-font_size, 0) and run downwards."""
    ov = Overlay()
    font = load_font(font_path, font_size)
    for pred, quad, direction in zip(outputs.contents, outputs.points, outputs.directions):
        x, y = int(quad[0][0]), int(quad[0][1])
        if direction == "vertical":
            ov.text((x - font_size, y), pred, font, font_color, direction="vertical")
        else:
            ov.text((x, y - font_size), pred, font, font_color)
    return _finish(ov, img, to_host)


def layout_visualizer(results, img, to_host=True):
    """utils/visualizer.py:99-125: per category the PALETTE colour, an outline of t = 2 and the label `category(role)` in the
    built-in font at 12 px with its baseline at (x1, y1)."""
    ov = Overlay()
    font = load_font(None, 12)
    for idx, (category, preds) in enumerate(results.model_dump().items()):
        color = PALETTE[idx % len(PALETTE)]
        for element in preds:
            role = element.get("role")
            x1, y1, x2, y2 = (int(v) for v in element["box"])
            ov.rectangle((x1, y1, x2, y2), color, 2)
            ov.text((x1, y1), category + ("" if role is None else f"({role})"), font, color, anchor="ls")
    return _finish(ov, img, to_host)


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
    elements = sorted(results.paragraphs + results.tables + results.figures, key=lambda e: e.order)
    _reading_order_commands(ov, elements, line_color, tip_size)
    if visualize_figure_letter:
        for figure in results.figures:
            _reading_order_commands(ov, figure.paragraphs, (0, 255, 0), 5)
    return _finish(ov, img, to_host)
