"""The crops of a page's figures, cut and JPEG-coded on the device: the only pixels the exporters (yomitoku_amd/export.py) write.

    made = crop_figure_files(pages, [[f.box for f in schema.figures] for schema in schemas])    # one PageFigures per page
    schema.to_markdown("out/page.md", figures=made[0])                                          # the files, as they are

`DocumentAnalyzer.serve(sources, figures=True)` hands a PageFigures back next to every page's schema; its render stage calls
`crop_figure_files` on the wave's clean (with `deskew`: corrected) pages with the wave slot's scratch.

The rule is the exporters' slice (`_save_figures`: `img[y1:y2, x1:x2]` of `map(int, box)`), restated in `figure_rects`: `int()`
of every coordinate, which truncates toward zero, clamped to the page; a box that leaves nothing has no file.  tests/figures_ref.py
is the definition.  All crops of a call are cut by one launch (yomitoku_amd/csrc/ymk_crop.hip: ymk_crop_u8) into one scratch
buffer, every crop at a multiple of 16 bytes; with `max_side` the crops whose long side exceeds it are shrunk by one launch of
the presets' resample (jpeg.resize_pages); the encoder (jpeg.launch_encode) takes the crops as pages like any other.  The host
sees one copy of the files' lengths and one of their bytes, both through pinned memory.  There is no host fallback.

The defaults - quality 95, 4:2:0, Annex K tables, no resize - are what the reference's `cv2.imencode(".jpg")` and this project's
`save_image` use: a file from here decodes to the pixels of the file the `img=` path of the exporters writes
(tests/test_figures_host.py)."""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, imaging
from . import jpeg as J
from .devpages import MAX_SIDE, addr_words, entered, gather_files, grown, to_pinned

CROP_WORDS = 16  # YMK_CROP_U8_WORDS
CAPACITY_ROOM = 2048  # a crop's file may take 2 x its raw bytes + this: the header alone is ~620 bytes, noise at quality 100 / 4:4:4 1.4 x raw
# the scratch keys of this module (a scratch dict belongs to one stream at a time; the encoder's and the gather's keys are theirs)
CROPS, PIN_LENGTHS = "fig_crops", "fig_pin_lengths"


@dataclass(frozen=True)
class FigureOptions:
    """What a job wants of its figure files: the checked form of `figures=...` (`check_figures`)."""

    quality: int = 95
    subsampling: str = "4:2:0"
    optimize: bool = False
    max_side: Optional[int] = None  # a crop whose long side exceeds it is shrunk to it


def check_figures(figures) -> Optional[FigureOptions]:
    """`figures` of a serve() call or of `crop_figure_files`: None / False (-> None), True (the defaults), an int 1..100 (the
    quality) or a dict with any of `quality`, `subsampling` (one of jpeg.SUBSAMPLINGS), `optimize` (a bool) and `max_side`
    (None, or 16..16383) -> the job's FigureOptions; a FigureOptions passes.  Anything else is a ValueError."""
    if figures is None or figures is False:
        return None
    if figures is True:  # a bool is an int: True means the defaults, not quality 1
        return FigureOptions()
    if isinstance(figures, FigureOptions):
        figures = {"quality": figures.quality, "subsampling": figures.subsampling, "optimize": figures.optimize, "max_side": figures.max_side}
    elif isinstance(figures, (int, np.integer)):
        figures = {"quality": int(figures)}
    if not isinstance(figures, dict):
        raise ValueError(f"figures is None, False, True, a quality 1..100 or a dict of quality / subsampling / optimize / max_side, got {figures!r}")
    unknown = sorted(str(k) for k in figures if k not in ("quality", "subsampling", "optimize", "max_side"))
    if unknown:
        raise ValueError(f"unknown figures option(s) {unknown}: quality, subsampling, optimize, max_side")
    quality = figures.get("quality", 95)
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError(f"figures quality is an int 1..100, got {quality!r}")
    subsampling = figures.get("subsampling", "4:2:0")
    if not isinstance(subsampling, str) or subsampling not in J.SUBSAMPLINGS:
        raise ValueError(f"unknown figures subsampling {subsampling!r}: one of {sorted(J.SUBSAMPLINGS)}")
    optimize = figures.get("optimize", False)
    if not isinstance(optimize, bool):
        raise ValueError(f"figures optimize is a bool, got {optimize!r}")
    max_side = figures.get("max_side", None)
    if max_side is not None and (isinstance(max_side, bool) or not isinstance(max_side, (int, np.integer)) or not 16 <= max_side <= MAX_SIDE):
        raise ValueError(f"figures max_side is None or an int 16..{MAX_SIDE}, got {max_side!r}")
    return FigureOptions(int(quality), subsampling, optimize, None if max_side is None else int(max_side))


def figure_rects(boxes: Sequence, h: int, w: int) -> List[Optional[Tuple[int, int, int, int]]]:
    """Per box (x1, y1, x2, y2 as numbers) the rectangle the exporters cut, (x1, y1, x2, y2) in pixels, or None where nothing
    is left: `int()` of every coordinate - toward zero -, clamped to [0, w] / [0, h]; empty is x2 <= x1 or y2 <= y1.  For a box
    inside the page (layout_parser.RTDETRPostProcessor clamps its boxes) that is exactly `img[y1:y2, x1:x2]`."""
    out = []
    for box in boxes:
        x1, y1, x2, y2 = (int(v) for v in box)
        x1, x2 = min(max(x1, 0), w), min(max(x2, 0), w)
        y1, y2 = min(max(y1, 0), h), min(max(y2, 0), h)
        out.append(None if x2 <= x1 or y2 <= y1 else (x1, y1, x2, y2))
    return out


@dataclass
class PageFigures:
    """The figure files of one page: `files[i]` belongs to `schema.figures[i]` - its EncodedJpeg, None where the box left nothing
    of the page, or the YmkError of a crop whose file did not fit; `rects[i]` is the rectangle it was cut at (None likewise)."""

    files: tuple = ()
    rects: tuple = ()

    def __len__(self):
        return len(self.files)

    def __iter__(self):
        return iter(self.files)


def _page_shape(page):
    """(h, w) of something that is a page as devpages.as_device_page takes it - without touching the device; else its ValueError."""
    if isinstance(page, torch.Tensor):
        dtype, shape = page.dtype, tuple(page.shape)
        ok = dtype == torch.uint8
    else:
        arr = np.asarray(page)
        dtype, shape = arr.dtype, arr.shape
        ok = dtype == np.uint8
    if not ok or not (len(shape) == 2 or (len(shape) == 3 and shape[2] == 3)):
        raise ValueError(f"a page is uint8 H x W x 3 (B G R) or H x W, got {dtype} {tuple(shape)}")
    if min(shape[:2]) < 1 or max(shape[:2]) > MAX_SIDE:
        raise ValueError(f"a page has 1..{MAX_SIDE} pixels on a side, got {tuple(shape[:2])}")
    return int(shape[0]), int(shape[1])


def launch_crops(devs: Sequence[torch.Tensor], rects_per_page: Sequence[Sequence], scratch: dict) -> List[torch.Tensor]:
    """Launch the cut of every rectangle (x1, y1, x2, y2; inside its page) of contiguous uint8 device pages on the current
    stream: one ymk_crop_u8 launch into scratch[CROPS], every crop at a multiple of 16 bytes.  -> the crops, page by page and
    in order, as [ch][cw][3] / [ch][cw] views of that buffer.  Waits for nothing."""
    recs, at, chunk = [], 0, 0
    for dev, rects in zip(devs, rects_per_page):
        h, w = int(dev.shape[0]), int(dev.shape[1])
        c = 1 if dev.dim() == 2 else 3
        for x1, y1, x2, y2 in rects:
            rec = np.zeros(CROP_WORDS, np.int32)
            rec[0:2] = addr_words(dev.data_ptr())
            rec[2:9] = (h, w, c, x1, y1, x2 - x1, y2 - y1)
            rec[11] = chunk
            recs.append((rec, at, (y2 - y1, x2 - x1) if c == 1 else (y2 - y1, x2 - x1, 3)))
            chunks = -(-((y2 - y1) * (x2 - x1) * c) // 16)
            at, chunk = at + 16 * chunks, chunk + chunks
    if not recs:
        return []
    device = devs[0].device
    buf = grown(scratch, CROPS, at, torch.uint8, device)
    base = buf.data_ptr()
    for rec, off, _ in recs:
        rec[9:11] = addr_words(base + off)
    blob = np.concatenate([rec for rec, _, _ in recs])
    blob_dev = imaging._stage_blob(blob, device)
    _lib.check(_lib.load().ymk_crop_u8(blob_dev.data_ptr(), blob.size, len(recs), chunk, _lib.current_stream_ptr()), "ymk_crop_u8")
    return [buf[off : off + int(np.prod(shape))].view(shape) for _, off, shape in recs]


def crop_figure_files(pages: Sequence, boxes_per_page: Sequence[Sequence], figures: Union[bool, int, dict, FigureOptions] = True,
                      stream=None, scratch: Optional[dict] = None) -> list:
    """One PageFigures per page, in order - or the exception of a page that is no page (not uint8, not H x W x 3 / H x W) or
    whose boxes are no boxes.  pages: device tensors and / or host arrays; boxes_per_page: per page the boxes of its figures
    (`[f.box for f in schema.figures]`); figures: what `check_figures` takes (True: quality 95, 4:2:0).  stream: the torch stream
    to launch on (default: the current one); scratch: a dict the caller keeps between calls to reuse the device and pinned
    buffers (serve: one per wave slot).
    The launches: one cut of all crops of the call (ymk_crop_u8), with `max_side` one resample of the crops whose long side
    exceeds it (to max(int(h * s), 1) x max(int(w * s), 1), as the page presets do it; `EncodedJpeg.scale` records s), the
    encoder's three (five with `optimize`).  Two waits: one for the files' lengths, one inside the gather of their bytes.  A
    file may take twice its crop's raw bytes plus 2048; a crop whose file does not fit has the YmkError in its slot.  A
    one-channel page gives grey files.  A page without figures gives an empty PageFigures; a call without a crop queues
    nothing, waits for nothing and needs no device."""
    opts = check_figures(figures)
    if opts is None:
        raise ValueError("crop_figure_files needs figure options: True, a quality or a dict (check_figures), got None / False")
    if len(boxes_per_page) != len(pages):
        raise ValueError(f"{len(pages)} pages and the boxes of {len(boxes_per_page)}")
    scratch = {} if scratch is None else scratch
    out: list = [None] * len(pages)
    rects: list = [None] * len(pages)
    for k, (page, boxes) in enumerate(zip(pages, boxes_per_page)):
        try:
            rects[k] = figure_rects(boxes, *_page_shape(page))
        except Exception as exc:  # noqa: BLE001 - only this page fails
            out[k] = exc
    todo = [k for k in range(len(pages)) if rects[k] is not None and any(r is not None for r in rects[k])]
    files = {k: [None] * len(rects[k]) for k in range(len(pages)) if rects[k] is not None}
    with entered([pages[k] for k in todo], stream, "crop_figure_files needs") as (_, live, devs, entered_out):
        for j, k in enumerate(todo):
            if isinstance(entered_out[j], BaseException):
                out[k], rects[k] = entered_out[j], None
        live = [todo[j] for j in live]
        if live:
            slots = [(k, i) for k in live for i, r in enumerate(rects[k]) if r is not None]
            crops = launch_crops(devs, [[r for r in rects[k] if r is not None] for k in live], scratch)
            scales = [1.0] * len(crops)
            if opts.max_side is not None:
                large = [i for i, c in enumerate(crops) if max(int(c.shape[0]), int(c.shape[1])) > opts.max_side]
                sizes = []
                for i in large:
                    h, w = int(crops[i].shape[0]), int(crops[i].shape[1])
                    scales[i] = opts.max_side / max(w, h)
                    sizes.append((max(int(h * scales[i]), 1), max(int(w * scales[i]), 1)))
                if large:
                    for i, small in zip(large, J.resize_pages([crops[i] for i in large], sizes)):
                        crops[i] = small
            caps = [2 * c.numel() + CAPACITY_ROOM for c in crops]
            colour = J.SUBSAMPLINGS[opts.subsampling]
            jpegs, offsets, lengths = J.launch_encode(crops, opts.quality, caps, opts.optimize, [0 if c.dim() == 2 else colour for c in crops], scratch)
            pin = to_pinned(scratch, PIN_LENGTHS, lengths, len(crops))
            torch.cuda.current_stream().synchronize()
            sizes = pin[: len(crops)].tolist()
            datas = gather_files([(jpegs, offsets[i], sizes[i]) for i in range(len(crops))], scratch)
            for (k, i), crop, cap, scale, data in zip(slots, crops, caps, scales, datas):
                if data is None:
                    files[k][i] = _lib.YmkError(f"figure {i} of page {k}: the JPEG file does not fit its capacity of {cap} bytes")
                else:
                    one = crop.dim() == 2
                    files[k][i] = J.EncodedJpeg(data, int(crop.shape[1]), int(crop.shape[0]), one, float(scale), opts.optimize,
                                                None if one else opts.subsampling)
    for k in range(len(pages)):
        if rects[k] is not None:
            out[k] = PageFigures(tuple(files[k]), tuple(rects[k]))
    return out
