"""Layered pages (mixed raster content): a colour or grey scan of a text page as a lossless ink mask and two small pictures.

    encoded = encode_mrc_pages(pages, "high")                         # device tensors or host arrays, uint8 H x W x 3 (B G R) or H x W
    encode_jpeg_pages(pages, "high", mrc={"bg_cell": 2, "fg_cell": 8})  # the same switch on the JPEG entry
    flag, mask, foreground, background = separate_pages(pages)[0]     # the separation alone, device tensors
    analyzer.serve(sources, jpeg="high", jpeg_mrc=True)               # a page's entry ends with its EncodedMrc

One JPEG of a text page spends its bytes on stroke edges and rings round every character.  A layered page has three parts
("Layered pages"; the definition is tests/mrc_ref.py, which the device equals bit for bit;
yomitoku_amd/csrc/ymk_mrc.hip):

  - the mask: the page's ink at full size - the luminance plane under the binariser's "adaptive" rule, the ink of the page-skew
    step - as a Group 4 file (yomitoku_amd/ccitt.py), lossless;
  - the background: the paper with the ink lifted out of it, one value per cell of `bg_cell` pixels a side: the mean of the
    cell's pixels outside the ink dilated by 3 x 3, which keeps anti-aliased stroke edges out of the paper;
  - the foreground: the ink's colour, one value per cell of `fg_cell` pixels: the mean of the cell's ink pixels.

A cell without such pixels is filled by pull-push with binary weights, so both pictures are smooth where nothing is known and the
JPEG encoder (yomitoku_amd/jpeg.py, unchanged) finds little to code.  A PDF draws the background and paints the foreground
through the mask (utils/searchable_pdf.py).  A page without ink, or without paper once the ink is dilated, has flag 0 and stays the
plain file it is without the switch.  Like a two-valued page a layered page is never resized: the preset gives the quality.
There is no host fallback.

    encode_jpeg_pages(pages, "high", mrc={"despeckle": True, "blobs": {"side": 48}})  # the ink filtered before it is used
    analyzer.serve(sources, jpeg="high", jpeg_mrc={"despeckle": True, "blobs": True})

The ink is the adaptive rule's as it is unless the dict asks for the ink filter (yomitoku_amd/despeckle.py; tests/ink_filter_ref.py
is the definition; DESIGN.md, "Layered pages: the ink filtered ..."): "despeckle" - False, True, an int or sizes, as
`check_despeckle` takes them - removes the specks and pinholes the mask's file pays for; "blobs" - False, True or a dict with
`side` and / or `fill`, as `check_blobs` takes them - sends every ink component that is large and fills its box, the dark part of
a picture, back to the paper, where it is a picture in the background layer and not a stencil over a mean colour.  The filter runs
on the device between the ink and the cells; the page's `EncodedMrc.mask.despeckled` is its `InkFiltered`.  A page whose ink is
all removed has flag 0.  Without the two keys every launch and byte is what it was.

Out: JBIG2 and JPEG 2000 layers, a choice of cells or of the filter's parameters per page, picture regions from the layout model,
smoothing of the fills, `serve_sharded`.
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import ClassVar, List, Optional, Sequence

import numpy as np

CELLS = (1, 2, 4, 8, 16)
DEFAULTS = {"bg_cell": 2, "fg_cell": 8}
FILTERS = ("despeckle", "blobs")  # the ink filter's keys: on only where asked for
PAGE_WORDS = 16  # YMK_MRC_PAGE_WORDS
LAYER_ROOM = 2048  # a layer's file may take its raw bytes and this: the header fits a tiny layer


def check_mrc(mrc=False) -> Optional[dict]:
    """`mrc` of a call: False -> None; True -> the defaults; a dict with any of bg_cell, fg_cell, each one of 1, 2, 4, 8, 16 -> the
    defaults with those.  The dict may also hold "despeckle" (what yomitoku_amd/despeckle.py's check_despeckle takes) and "blobs"
    (what its check_blobs takes), both False by default: the ink filter of the mask.  One that is on is in the result under its
    key, as that function's dict; without either the result is the cells alone.  Anything else is a ValueError."""
    from .despeckle import check_blobs, check_despeckle

    if mrc is False:
        return None
    if mrc is True:
        return dict(DEFAULTS)
    if not isinstance(mrc, dict) or any(k not in DEFAULTS and k not in FILTERS for k in mrc):
        raise ValueError(f"unknown jpeg mrc {mrc!r}: False, True or a dict with any of {sorted(DEFAULTS) + list(FILTERS)}")
    out = dict(DEFAULTS)
    for key, value in mrc.items():
        if key in FILTERS:
            continue
        if isinstance(value, bool) or not isinstance(value, int) or value not in CELLS:
            raise ValueError(f"jpeg mrc[{key!r}] is one of {CELLS}, got {value!r}")
        out[key] = int(value)
    for key, check in (("despeckle", check_despeckle), ("blobs", check_blobs)):
        checked = check(mrc.get(key, False))
        if checked is not None:
            out[key] = checked
    return out


@dataclass
class EncodedMrc:
    """One page in three files.  mask: an EncodedBilevel (method "adaptive") of the full-size page, 1 = ink; background,
    foreground: EncodedJpegs of ceil(h / cell) x ceil(w / cell) pixels.  `scale` is 1.0: a layered page is never resized."""

    mask: "EncodedBilevel"  # noqa: F821 - yomitoku_amd/ccitt.py
    background: "EncodedJpeg"  # noqa: F821 - yomitoku_amd/jpeg.py
    foreground: "EncodedJpeg"  # noqa: F821
    width: int
    height: int
    scale: float = 1.0
    bg_cell: int = DEFAULTS["bg_cell"]
    fg_cell: int = DEFAULTS["fg_cell"]
    mrc: ClassVar[bool] = True  # what utils/searchable_pdf.py recognises the object by

    @property
    def nbytes(self) -> int:
        return len(self.mask.data) + len(self.background.data) + len(self.foreground.data)


def scratch_sizes(shapes: Sequence, bg_cell: int, fg_cell: int):
    """((bytes of the planes, the summed-area tables, the packed rows, the pyramids, the layers, the flags), per page (word 5 of
    its record, the byte offsets of its foreground and background in the layers)) of pages of `shapes` = (h, w) or (h, w, 3)."""
    from . import _lib
    from .devpages import shape_args

    n = len(shapes)
    sizes, places = (ctypes.c_int64 * 6)(), (ctypes.c_int64 * max(1, 3 * n))()
    _lib.check(_lib.load().ymk_mrc_scratch_bytes(*shape_args(shapes, channels=True), n, bg_cell, fg_cell, sizes, places), "ymk_mrc_scratch_bytes")
    return tuple(int(v) for v in sizes), [tuple(int(places[3 * k + i]) for i in range(3)) for k in range(n)]


def page_table(pages: Sequence, packed_at: Sequence[int], places: Sequence) -> np.ndarray:
    """int32 [n][16]: the page table of include/ymk.h ("Layered pages") - the planes and summed-area tables one page behind the
    other, the packed rows at `packed_at`, pyramids and layers at `places`."""
    from .devpages import addr_words

    rec = np.zeros((len(pages), PAGE_WORDS), np.int32)
    luma = sat = 0
    for k, p in enumerate(pages):
        h, w, ch = int(p.shape[0]), int(p.shape[1]), 1 if p.dim() == 2 else 3
        rec[k, 0:2] = addr_words(p.data_ptr())
        rec[k, 2:5] = (h, w, ch)
        rec[k, 5] = places[k][0]
        rec[k, 6:8] = addr_words(int(packed_at[k]))
        if ch == 3:
            rec[k, 8:10] = addr_words(luma)
            luma += -(-(h * w) // 16) * 16
        rec[k, 11:13] = addr_words(places[k][1])
        rec[k, 14:16] = addr_words(sat)
        sat += h * w
    return rec


def pack_mask(mask, device):
    """A bool H x W mask (array or tensor, True = ink) as the packed rows of include/ymk.h on `device`: int32 [H][ceil(W / 32)],
    the leftmost pixel of a word in its bit 31."""
    import torch

    m = torch.as_tensor(np.asarray(mask, bool) if not isinstance(mask, torch.Tensor) else mask).to(device=device, dtype=torch.int64)
    h, w = int(m.shape[0]), int(m.shape[1])
    rw = -(-w // 32)
    bits = torch.zeros((h, rw * 32), dtype=torch.int64, device=device)
    bits[:, :w] = m
    words = (bits.view(h, rw, 32) << torch.arange(31, -1, -1, dtype=torch.int64, device=device)).sum(-1)
    return torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32)


class _Separated:
    """The launches of one call.  `pages`, `packed`, `packed_at`, `packed_bytes`: what ccitt.launch_encode reads of a finished
    test - the masks are coded by the Group 4 launches as they are.  `layers`: the buffer of the layer images; `pin`: the flags
    on their way to pinned memory; `buffers`: what the stages wrote, for the tests."""

    def __init__(self, pages, params, packed, packed_at, packed_bytes, layers, places, pin, buffers, ink_filter=None):
        self.pages, self.params, self.packed, self.packed_at, self.packed_bytes = pages, params, packed, packed_at, packed_bytes
        self.layers, self.places, self.pin, self.buffers, self.ink_filter = layers, places, pin, buffers, ink_filter

    def flags(self) -> List[int]:
        """Per page 1 (layered), 0 (no ink, or no paper: no layers) or -1 (no page) - once the stream has been waited for."""
        return self.pin[: len(self.pages)].tolist()

    def filtered(self) -> list:
        """Per page the InkFiltered of its mask (yomitoku_amd/despeckle.py), or None where the ink filter did not run - once
        the stream has been waited for.  The six counts lie behind the flags and the planes' table in `pin`."""
        from .despeckle import filter_result

        n = len(self.pages)
        if self.ink_filter is None:
            return [None] * n
        at = n * (1 + PAGE_WORDS)
        return [filter_result(self.ink_filter, six) for six in self.pin[at : at + 6 * n].view(n, 6).tolist()]

    def _layer(self, j: int, at: int, cell: int):
        p = self.pages[j]
        H0, W0 = -(-int(p.shape[0]) // cell), -(-int(p.shape[1]) // cell)
        shape = (H0, W0) if p.dim() == 2 else (H0, W0, 3)
        return self.layers[at : at + int(np.prod(shape))].view(shape)

    def foreground(self, j: int):
        """The foreground layer of page j, uint8 [H0][W0] or [H0][W0][3]: a view of `layers`, written where the flag is 1."""
        return self._layer(j, self.places[j][1], self.params["fg_cell"])

    def background(self, j: int):
        return self._layer(j, self.places[j][2], self.params["bg_cell"])

    def mask_rows(self, j: int):
        """The packed ink of page j, int32 [h][ceil(w / 32)]: a view of `packed`."""
        h, rw = int(self.pages[j].shape[0]), -(-int(self.pages[j].shape[1]) // 32)
        return self.packed[self.packed_at[j] : self.packed_at[j] + h * rw].view(h, rw)


class _Ink:
    """What despeckle.launch_filter reads of a test: the pages (their shapes) and where their packed ink lies."""

    def __init__(self, pages, packed, packed_at, packed_bytes):
        self.pages, self.packed, self.packed_at, self.packed_bytes = pages, packed, packed_at, packed_bytes


def launch(pages: Sequence, params: dict, scratch: dict, masks: Optional[Sequence] = None, packed=None, layers=None,
           edit_table=None) -> _Separated:
    """Queue the separation of device pages (uint8 H x W x 3 or H x W, contiguous) on the current stream: luminance and ink (the
    page-skew step's two calls; with `masks` - per page a bool H x W array or tensor - those are packed in their place), cells,
    pull, flags and push, and the copy of the flags to pinned memory.  Waits for nothing.  With "despeckle" or "blobs" in
    `params` the ink filter (yomitoku_amd/despeckle.py: launch_filter) is queued between the ink and the cells, in place on the
    packed rows - the ink then comes from ymk_dsk_luma and ymk_bin_adaptive_pack called here, and ymk_mrc_pages takes it as the
    caller's -, and its six counts a page go to pinned memory behind the flags, in the same copy; without them the call is the
    one it was.  scratch: the device and pinned buffers,
    kept between calls - but the layers are a fresh tensor per call, which the returned object holds.  packed: (buffer, word
    offsets per page, bytes) of packed rows the ink is to be written to (default: scratch's, one page behind the other); layers: a
    caller's uint8 buffer for the layer images (the tests' poisoned one); edit_table: a function that may change the int32 [n][16]
    page table before it is staged (the tests' malformed record)."""
    import torch

    from . import _lib, imaging
    from . import despeckle as specks
    from .devpages import LUMA_PLANE, PACKED_ROWS, SUMMED_AREA, grown, to_pinned

    lib, device, n = _lib.load(), pages[0].device, len(pages)
    assert lib.ymk_mrc_page_words() == PAGE_WORDS
    bg_cell, fg_cell = int(params["bg_cell"]), int(params["fg_cell"])
    (luma_b, sat_b, packed_b, pyr_b, layers_b, _), places = scratch_sizes([tuple(p.shape) for p in pages], bg_cell, fg_cell)
    if packed is None:
        packed_at, at = [], 0
        for p in pages:
            packed_at.append(at)
            at += int(p.shape[0]) * (-(-int(p.shape[1]) // 32))
        packed_dev = grown(scratch, PACKED_ROWS, packed_b // 4, torch.int32, device)
    else:
        packed_dev, packed_at, packed_b = packed
    rec = page_table(pages, packed_at, places)
    if edit_table is not None:
        edit_table(rec)
    pyr = grown(scratch, "mrc_pyramids", pyr_b // 4, torch.int32, device)
    if layers is None:
        layers = torch.empty(max(layers_b, 16), dtype=torch.uint8, device=device)
    ink_filter = None
    if any(key in params for key in FILTERS):
        ink_filter = specks.filter_params(params.get("despeckle"), params.get("blobs"))
    # the flags, then the planes' table, then - the ink filter - its six counts a page
    answer = grown(scratch, "mrc_answer", n * (1 + PAGE_WORDS + (6 if ink_filter else 0)), torch.int32, device)
    luma = sat = None
    if masks is None:
        luma = grown(scratch, LUMA_PLANE, max(luma_b, 16), torch.uint8, device)
        sat = grown(scratch, SUMMED_AREA, sat_b // 4, torch.int32, device)
    else:
        for j, m in enumerate(masks):
            rows = pack_mask(m, device).reshape(-1)
            packed_dev[packed_at[j] : packed_at[j] + rows.numel()].copy_(rows)
    blob_dev = imaging._stage_blob(rec.reshape(-1), device)
    max_h, max_w, stream = max(int(p.shape[0]) for p in pages), max(int(p.shape[1]) for p in pages), _lib.current_stream_ptr()
    planes = None if masks is not None else answer.data_ptr() + 4 * n
    if ink_filter is not None:
        # the ink by the two entries ymk_mrc_pages would call, the filter in place on the packed rows, then the separation of
        # what is the caller's ink now.  A caller's masks are filtered like the pages' own ink.
        if planes is not None:
            _lib.check(lib.ymk_dsk_luma(blob_dev.data_ptr(), rec.size, n, max_h * max_w, luma.data_ptr(), luma_b, packed_b, sat_b, planes, stream),
                       "ymk_dsk_luma")
            _lib.check(lib.ymk_bin_adaptive_pack(planes, n * PAGE_WORDS, n, max_h, max_w, sat.data_ptr(), sat_b, packed_dev.data_ptr(), packed_b,
                                                 stream), "ymk_bin_adaptive_pack")
            planes = None
        ink = _Ink(pages, packed_dev, packed_at, packed_b)
        specks.launch_filter(ink, list(range(n)), ink_filter, scratch, counts=answer[n * (1 + PAGE_WORDS) : n * (7 + PAGE_WORDS)])
    _lib.check(lib.ymk_mrc_pages(blob_dev.data_ptr(), rec.size, n, max_h, max_w,
                                 bg_cell, fg_cell, None if luma is None else luma.data_ptr(), luma_b, None if sat is None else sat.data_ptr(), sat_b,
                                 packed_dev.data_ptr(), packed_b, planes, pyr.data_ptr(), pyr_b,
                                 layers.data_ptr(), layers_b, answer.data_ptr(), stream), "ymk_mrc_pages")
    pin = to_pinned(scratch, "mrc_pin_flags", answer, n * (1 + PAGE_WORDS + 6) if ink_filter else n)
    buffers = {"pyramids": pyr, "flags": answer, "blob": blob_dev, "sizes": (luma_b, sat_b, packed_b, pyr_b, layers_b)}
    return _Separated(list(pages), dict(params), packed_dev, list(packed_at), packed_b, layers, places, pin, buffers, ink_filter)


def separate_pages(pages: Sequence, mrc=True, masks: Optional[Sequence] = None, stream=None, scratch: Optional[dict] = None) -> list:
    """One entry per page, in order: (flag, the packed mask, the foreground layer, the background layer) as device tensors - flag 1:
    int32 [h][ceil(w / 32)] (1 = ink, the leftmost pixel of a word in bit 31) and uint8 [ceil(h / fg_cell)][ceil(w / fg_cell)]
    (x 3 for a colour page), likewise bg_cell; flag 0 (no ink, or no paper outside the dilated ink): the layers are None -, or the
    exception that page raised (not uint8, not H x W x 3 / H x W).  pages: device tensors and / or host arrays; mrc: True or the
    dict `check_mrc` takes - with "despeckle" or "blobs" in it the mask returned, and the layers, are those of the filtered ink, and
    a page whose ink is all removed has flag 0; masks: per page a bool H x W ink mask to use instead of the adaptive one (filtered
    like it), or None for all; stream: the
    torch stream to launch on (default: the current one); scratch: a dict the caller keeps between calls.  One wait, for the flags."""
    import torch

    from .devpages import entered

    params = check_mrc(mrc)
    if params is None:
        raise ValueError("mrc=False: there is nothing to separate")
    if masks is not None and len(masks) != len(pages):
        raise ValueError(f"{len(masks)} masks for {len(pages)} pages")

    def mask_fits(k, page, dev):
        if masks is not None and tuple(np.shape(masks[k])) != tuple(dev.shape[:2]):
            raise ValueError(f"a mask has its page's H x W, got {tuple(np.shape(masks[k]))} for {tuple(page.shape[:2])}")

    scratch = {} if scratch is None else scratch
    with entered(pages, stream, "layered pages need", mask_fits) as (_, live, devs, out):
        if live:
            done = launch(devs, params, scratch, None if masks is None else [masks[k] for k in live])
            torch.cuda.current_stream().synchronize()
            for j, (k, flag) in enumerate(zip(live, done.flags())):
                rows = done.mask_rows(j).clone()
                out[k] = (flag, rows, done.foreground(j), done.background(j)) if flag == 1 else (flag, rows, None, None)
    return out


def encode_mrc_pages(pages: Sequence, image_quality: str = "high", mrc=True, stream=None, scratch: Optional[dict] = None,
                     optimize: bool = False, subsampling: str = "4:2:0") -> list:
    """One entry per page, in order: its EncodedMrc; the EncodedJpeg `encode_jpeg_pages` gives it where its flag is 0; or the
    exception that page raised.  The stand-alone form of `encode_jpeg_pages(..., mrc=mrc)`, whose arguments these are."""
    from .jpeg import encode_jpeg_pages

    if check_mrc(mrc) is None:
        raise ValueError("mrc=False: encode_jpeg_pages writes plain files")
    return encode_jpeg_pages(pages, image_quality, stream, scratch, optimize=optimize, subsampling=subsampling, mrc=mrc)
