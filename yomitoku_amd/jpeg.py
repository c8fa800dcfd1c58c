"""Baseline JPEG files of pages that are already on the device: what a searchable PDF embeds (utils/searchable_pdf.py).

    encoded = encode_jpeg_pages(pages, "high")          # device tensors or host arrays, uint8 H x W x 3 (B G R) or H x W
    searchable_pdf_bytes(encoded, docs)                 # an EncodedJpeg is embedded as it is

`DocumentAnalyzer.serve(sources, jpeg="high")` hands an EncodedJpeg back next to every page's schema; its render stage calls
`encode_jpeg_pages` on the wave's clean pages with the wave slot's scratch.

The whole file is made on the device (yomitoku_amd/csrc/ymk_jpeg.hip; DESIGN.md, "JPEG encoder"): colour conversion, 4:2:0
chroma, DCT and quantiser in one launch, the Huffman coding of every restart interval (one MCU row) in a second, header +
intervals + restart markers laid out per page in a third.  The presets are the searchable PDF's (`IMAGE_QUALITY_PRESETS`): a
page whose long side exceeds the preset's is first shrunk with Pillow's Lanczos resample, restated on the device
(ymk_pil_resize_u8), to int(w * scale) x int(h * scale) as the host path does.  The host sees one copy of the files' lengths and
one of their bytes, both through pinned memory.  There is no host fallback: a page the device cannot encode is an exception.

`optimize=True` (serve: `jpeg_optimize=True`) codes the same coefficients with Huffman tables made for each page - libjpeg's
`optimize` rule, byte for byte Pillow's `save(..., optimize=True, restart_marker_rows=1)` wherever the plain file is Pillow's:
two more launches (the page's symbol histograms, then its tables), the same pixels when decoded, a smaller file.

`subsampling="4:2:2"` / `"4:4:4"` (serve: `jpeg_subsampling=`) keeps the chroma of colour pages at full height / at full size -
libjpeg's sampling 2x1 / 1x1, what Pillow calls `subsampling=1` / `0`: red seals, coloured ruling and small coloured print stay
sharp, the file grows.  `grey="auto"` (serve: `jpeg_grey="auto"`) tests every three-channel page on the device after the
preset's resize - one more launch and one wait for its answer - and writes a page all of whose pixels have B == G == R as the
one-component file of that plane, a third of the blocks: `EncodedJpeg.grey` is True and `subsampling` None.  The definition of
the modes is tests/jpeg_modes_ref.py; the defaults write the bytes they always wrote.

`bilevel="auto"` (serve: `jpeg_bilevel="auto"`) tests every page on the device as it arrived and gives a two-valued one - every
sample 0 or 255, B == G == R - a CCITT Group 4 file, an `EncodedBilevel` of yomitoku_amd/ccitt.py, in place of the EncodedJpeg.
`bilevel="otsu"` / `"adaptive"` thresholds every grey-valued page on the device instead - a scan with paper noise, soft edges
or a gradient of light, but a grey photograph too - and codes the result the same way.

`mrc=True` (serve: `jpeg_mrc=True`) writes every remaining page that has ink and paper as a layered page, an `EncodedMrc` of
yomitoku_amd/mrc.py: its ink mask as a Group 4 file and two low-resolution pictures - the paper, the ink's colour - as JPEG files
from this encoder, which takes the layers as pages like any other.

The options are checked in one place, `page_files`, which makes a `PageFiles` of them (serve: `check_jpeg_preset`, the job's
`wave.job.files`); `encode_page_files(pages, files)` is the worker behind every entry, the list of its phases: sort the pages,
make up the JPEG batch, launch JPEG, launch Group 4, one wait and one gather.

`despeckle=True` (serve: `jpeg_despeckle=True`) removes the specks and pinholes of fewer than 4 pixels from every page that gets a
Group 4 file, on the device, before it is coded (yomitoku_amd/despeckle.py); `EncodedBilevel.despeckled` says what went.

`lossless=True` (serve: `jpeg_lossless=True`) writes every page `bilevel` and `mrc` leave as a lossless file, an `EncodedLossless`
of yomitoku_amd/flate.py - a zlib stream of the page's PNG-filtered rows, never resized - in place of the EncodedJpeg;
`lossless={"budget": b}` only where that file takes at most b bytes a pixel: a page over the budget gets the JPEG it gets
without the switch.
"""

from __future__ import annotations

import ctypes
import functools
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib, ccitt, flate, imaging
from . import despeckle as specks
from . import mrc as layered
from .devpages import addr_words, entered, gather_files, grown, shape_args, to_pinned
from .devpages import addr_words as _addr_words  # noqa: F401 - tools/jpeg_serve_timing.py takes it from here
from .utils.searchable_pdf import IMAGE_QUALITY_PRESETS

PAGE_WORDS, RESIZE_WORDS = 16, 16  # YMK_JPEG_PAGE_WORDS, YMK_PIL_RESIZE_U8_WORDS
SUBSAMPLINGS = {"4:2:0": 0, "4:2:2": 1, "4:4:4": 2}  # word 15 of a page's record: YMK_JPEG_MODE_420 / _422 / _444
MODE_GREY = 4  # YMK_JPEG_MODE_GREY: channel 0 of a three-channel page as a one-component file
_SAMPLING = {0: (2, 2), 1: (2, 1), 2: (1, 1)}  # mode -> the luminance sampling factors (hs, vs)


@dataclass
class EncodedJpeg:
    """One page as a JFIF file.  `scale`: what the preset shrank the page by (1.0: not at all) - the factor a PDF writer applies
    to the page's word coordinates."""

    data: bytes
    width: int
    height: int
    grey: bool
    scale: float = 1.0
    optimized: bool = False  # coded with the page's own Huffman tables
    subsampling: Optional[str] = "4:2:0"  # of a colour file; None: a grey file has no chroma


def jpeg_preset(image_quality: str) -> dict:
    """The preset of that name; an unknown name is a ValueError (the host path of searchable_pdf_bytes falls back to "high")."""
    try:
        return IMAGE_QUALITY_PRESETS[image_quality]
    except (KeyError, TypeError):
        raise ValueError(f"unknown jpeg preset {image_quality!r}: one of {sorted(IMAGE_QUALITY_PRESETS)}") from None


def check_modes(subsampling="4:2:0", grey=False) -> int:
    """The mode of a call's colour pages; a `subsampling` that is not one of SUBSAMPLINGS, or a `grey` that is neither False
    nor "auto", is a ValueError."""
    if not isinstance(subsampling, str) or subsampling not in SUBSAMPLINGS:
        raise ValueError(f"unknown jpeg subsampling {subsampling!r}: one of {sorted(SUBSAMPLINGS)}")
    if grey is not False and grey != "auto":
        raise ValueError(f"unknown jpeg grey {grey!r}: False or 'auto'")
    return SUBSAMPLINGS[subsampling]


def _geometry(h: int, w: int, channels: int, mode: int):
    """(tiles of the coefficient stage, blocks, restart intervals) of a page in `mode`."""
    if channels == 1 or mode == MODE_GREY:
        hs, vs, per, tile = 1, 1, 1, 8 if channels == 1 else 16
    else:
        (hs, vs), tile = _SAMPLING[mode], 16
        per = hs * vs + 2
    mw, mh = -(-w // (8 * hs)), -(-h // (8 * vs))
    return (-(-w // tile)) * (-(-h // tile)), mw * mh * per, mh


@functools.lru_cache(maxsize=256)
def _header(h: int, w: int, channels: int, quality: int, mode: int = 0) -> bytes:
    buf = (ctypes.c_ubyte * 1024)()
    n = _lib.load().ymk_jpeg_header_mode(h, w, channels, mode, quality, buf, len(buf))
    if n < 0:
        _lib.check(1, "ymk_jpeg_header_mode")
    return bytes(buf[:n])


@functools.lru_cache(maxsize=256)
def _header_opt(h: int, w: int, channels: int, quality: int, mode: int = 0):
    """(the header without its DHT segments, the bytes of it before their place)."""
    buf, split = (ctypes.c_ubyte * 1024)(), ctypes.c_int(0)
    n = _lib.load().ymk_jpeg_header_opt_mode(h, w, channels, mode, quality, buf, len(buf), ctypes.byref(split))
    if n < 0:
        _lib.check(1, "ymk_jpeg_header_opt_mode")
    return bytes(buf[:n]), int(split.value)


@functools.lru_cache(maxsize=16)
def _quant_words(quality: int) -> np.ndarray:
    out = (ctypes.c_int * 128)()
    _lib.check(_lib.load().ymk_jpeg_quant_tables(quality, out), "ymk_jpeg_quant_tables")
    return np.frombuffer(out, dtype=np.int32).copy()


def scratch_sizes(shapes: Sequence, optimize: bool = False, modes: Optional[Sequence[int]] = None) -> tuple:
    """(tiles - the MCUs of 4:2:0 and grey pages -, blocks, intervals, coefficient bytes, stream bytes, interval-record bytes) of
    pages of `shapes` = (h, w, channels) and `modes` (word 15 of their records; default 0 each); optimize: the stream bytes of
    that path, and behind the six the bytes of the histograms, the code tables and the DHT records."""
    n = len(shapes)
    sizes = (ctypes.c_int64 * (9 if optimize else 6))()
    name = "ymk_jpeg_scratch_bytes_opt_mode" if optimize else "ymk_jpeg_scratch_bytes_mode"
    _lib.check(getattr(_lib.load(), name)(*shape_args(shapes, channels=True),
                                          None if modes is None else (ctypes.c_int * max(1, n))(*[int(m) for m in modes]), n, sizes), name)
    return tuple(int(v) for v in sizes)


@functools.lru_cache(maxsize=64)
def _lanczos(in_size: int, out_size: int):
    return imaging.pil_lanczos_coeffs(in_size, out_size)  # ~10 ms of host time per new (in, out) pair: the pages of a job share theirs


def page_table(pages: Sequence[torch.Tensor], quality: int, capacities: Optional[Sequence[int]] = None, optimize: bool = False,
               modes: Optional[Sequence[int]] = None):
    """(int32 words of the page table of include/ymk.h, per page the byte offset of its file in the output, the output's bytes).
    capacities: bytes per page's file; default the page's raw byte count.  optimize: the table of the *_opt entries - headers
    without DHT segments, word 14 the place the device puts the page's own.  modes: word 15 per page - 0 (default), a value of
    SUBSAMPLINGS or MODE_GREY for a three-channel page, 0 for a grey one."""
    n = len(pages)
    rec = np.zeros((n, PAGE_WORDS), np.int32)
    shapes = [(int(p.shape[0]), int(p.shape[1]), 1 if p.dim() == 2 else 3) for p in pages]
    modes = [0] * n if modes is None else [int(m) for m in modes]
    rec[:, 15] = modes
    if optimize:
        split = [_header_opt(h, w, ch, quality, m) for (h, w, ch), m in zip(shapes, modes)]
        headers, rec[:, 14] = [s[0] for s in split], [s[1] for s in split]
    else:
        headers = [_header(h, w, ch, quality, m) for (h, w, ch), m in zip(shapes, modes)]
    at = n * PAGE_WORDS * 4  # byte offset of the first header
    mcu = blk = iv = 0
    out_at, offsets = 0, []
    for k, p in enumerate(pages):
        h, w = int(p.shape[0]), int(p.shape[1])
        ch = 1 if p.dim() == 2 else 3
        tiles, blocks, rows = _geometry(h, w, ch, modes[k])
        cap = int(capacities[k]) if capacities is not None else h * w * ch
        rec[k, 0:2] = addr_words(p.data_ptr())
        rec[k, 2:8] = (h, w, ch, mcu, blk, iv)
        rec[k, 8:10] = addr_words(out_at)
        rec[k, 10:13] = (cap, at, len(headers[k]))
        offsets.append(out_at)
        mcu, blk, iv = mcu + tiles, blk + blocks, iv + rows
        at += -(-len(headers[k]) // 4) * 4
        out_at += -(-cap // 16) * 16
    rec[:, 13] = at // 4  # one quality per call: one pair of tables behind the headers
    blob = np.zeros(at // 4 + 128, np.int32)
    blob[: n * PAGE_WORDS] = rec.reshape(-1)
    raw = blob.view(np.uint8)
    for k in range(n):
        raw[rec[k, 11] : rec[k, 11] + len(headers[k])] = np.frombuffer(headers[k], np.uint8)
    blob[at // 4 :] = _quant_words(quality)
    return blob, offsets, out_at


def resize_pages(pages: Sequence[torch.Tensor], sizes: Sequence) -> List[torch.Tensor]:
    """Pillow's `resize((ow, oh), LANCZOS)` of uint8 device pages (H x W x 3 or H x W), all in one launch on the current
    stream; sizes: (oh, ow) per page."""
    dev = pages[0].device
    outs, tables, recs = [], [], np.zeros((len(pages), RESIZE_WORDS), np.int32)
    at = len(pages) * RESIZE_WORDS
    for k, (p, (oh, ow)) in enumerate(zip(pages, sizes)):
        h, w = int(p.shape[0]), int(p.shape[1])
        ch = 1 if p.dim() == 2 else 3
        out = torch.empty((oh, ow) if ch == 1 else (oh, ow, 3), dtype=torch.uint8, device=dev)
        xb, xk, ksx = _lanczos(w, ow)
        yb, yk, ksy = _lanczos(h, oh)
        recs[k, 0:2] = addr_words(p.data_ptr())
        recs[k, 2:9] = (h, w, ch, oh, ow, ksx, ksy)
        for j, t in enumerate((xb, xk, yb, yk)):
            recs[k, 9 + j] = at
            tables.append(t.reshape(-1))
            at += t.size
        recs[k, 13:15] = addr_words(out.data_ptr())
        outs.append(out)
    blob = np.concatenate([recs.reshape(-1)] + tables).astype(np.int32, copy=False)
    blob_dev = imaging._stage_blob(blob, dev)
    _lib.check(_lib.load().ymk_pil_resize_u8(blob_dev.data_ptr(), blob.size, len(pages), max(s[0] for s in sizes),
                                             max(s[1] for s in sizes), _lib.current_stream_ptr()), "ymk_pil_resize_u8")
    return outs


def _grey_launch(pages: Sequence[torch.Tensor], scratch: dict):
    """Launch the grey test of the three-channel pages among `pages` on the current stream and the copy of its answer to
    pinned memory; waits for nothing.  -> (their indices, the pinned answer), or None where there is no such page."""
    cand = [k for k, p in enumerate(pages) if p.dim() == 3]
    if not cand:
        return None
    device = pages[cand[0]].device
    rec = np.zeros((len(cand), PAGE_WORDS), np.int32)
    for j, k in enumerate(cand):
        rec[j, 0:2] = addr_words(pages[k].data_ptr())
        rec[j, 2:5] = (int(pages[k].shape[0]), int(pages[k].shape[1]), 3)
    blob_dev = imaging._stage_blob(rec.reshape(-1), device)
    diff = grown(scratch, "grey", len(cand), torch.int32, device)
    _lib.check(_lib.load().ymk_jpeg_pages_grey(blob_dev.data_ptr(), rec.size, len(cand), max(int(pages[k].shape[0]) * int(pages[k].shape[1]) for k in cand),
                                               diff.data_ptr(), _lib.current_stream_ptr()), "ymk_jpeg_pages_grey")
    return cand, to_pinned(scratch, "pin_grey", diff, len(cand))


def _grey_answers(n: int, launched) -> List[bool]:
    """Per page of the `n` a `_grey_launch` was given whether it is a grey-valued three-channel page - once the stream has been
    waited for."""
    out = [False] * n
    if launched is not None:
        cand, pin = launched
        for k, v in zip(cand, pin[: len(cand)].tolist()):
            out[k] = v == 0
    return out


def grey_pages(pages: Sequence[torch.Tensor], scratch: Optional[dict] = None) -> List[bool]:
    """Per device page (uint8 H x W x 3 or H x W, contiguous): whether it is a three-channel page all of whose pixels have
    B == G == R.  One launch over all three-channel pages on the current stream (ymk_jpeg_pages_grey), then one wait for its
    answer, read through pinned memory."""
    launched = _grey_launch(pages, {} if scratch is None else scratch)
    if launched is not None:
        torch.cuda.current_stream().synchronize()
    return _grey_answers(len(pages), launched)


@dataclass(frozen=True)
class PageFiles:
    """What a job wants of its page files: the checked form of `encode_jpeg_pages`' and `serve`'s seven options (`page_files`)."""

    preset: str  # a name of IMAGE_QUALITY_PRESETS
    optimize: bool
    subsampling: str  # "4:2:0" | "4:2:2" | "4:4:4"
    grey: Union[bool, str]  # False | "auto"
    bilevel: Union[bool, str]  # False | "auto" | "otsu" | "adaptive"
    mrc: Optional[dict]  # None, or check_mrc's full dict
    despeckle: Optional[dict] = None  # None, or check_despeckle's {"black": n, "white": n}
    lossless: Optional[dict] = None  # None, or check_lossless's {"budget256": None or the budget in 1/256 byte a pixel}


def page_files(preset, optimize=False, subsampling="4:2:0", grey=False, bilevel=False, mrc=False, serve=False,
               despeckle=False, lossless=False) -> Optional[PageFiles]:
    """The PageFiles of a call's options - the one place they are checked; every refusal is a ValueError.  serve: the reading of
    the `serve()` entries - `preset` None: no page files (-> None), which every other option then has to agree with by
    standing at its default; `subsampling` None: 4:2:0."""
    given = subsampling
    if serve:
        if preset is not None and (not isinstance(preset, str) or preset not in IMAGE_QUALITY_PRESETS):
            raise ValueError(f"unknown jpeg preset {preset!r}: None or one of {sorted(IMAGE_QUALITY_PRESETS)}")
        if optimize and preset is None:
            raise ValueError("jpeg_optimize=True needs jpeg=...: there is no JPEG file to optimise")
        subsampling = "4:2:0" if given is None else given
    else:
        jpeg_preset(preset)
    check_modes(subsampling, grey)
    if preset is None and given is not None:
        raise ValueError(f"jpeg_subsampling={given!r} needs jpeg=...: there is no JPEG file to write that way")
    if preset is None and grey is not False:
        raise ValueError(f"jpeg_grey={grey!r} needs jpeg=...: there is no JPEG file to write that way")
    if ccitt.check_bilevel(bilevel) and preset is None:
        raise ValueError(f"jpeg_bilevel={bilevel!r} needs jpeg=...: there are no page files to write that way")
    cells = layered.check_mrc(mrc)
    if cells is not None and preset is None:
        raise ValueError(f"jpeg_mrc={mrc!r} needs jpeg=...: there are no page files to write that way")
    clean = specks.check_despeckle(despeckle)
    if clean is not None and preset is None:
        raise ValueError(f"jpeg_despeckle={despeckle!r} needs jpeg=...: there are no page files to write that way")
    if clean is not None and bilevel is False:
        raise ValueError(f"jpeg_despeckle={despeckle!r} needs jpeg_bilevel=...: there is no Group 4 file to clean")
    flat = flate.check_lossless(lossless)
    if flat is not None and preset is None:
        raise ValueError(f"jpeg_lossless={lossless!r} needs jpeg=...: there are no page files to write that way")
    return None if preset is None else PageFiles(preset, bool(optimize), subsampling, grey, bilevel, cells, clean, flat)


def check_jpeg_preset(jpeg, jpeg_optimize=False, jpeg_subsampling=None, jpeg_grey=False, jpeg_bilevel=False, jpeg_mrc=False,
                      jpeg_despeckle=False, jpeg_lossless=False):
    """`jpeg` of a serve() call: None (-> None) or a preset name of the searchable PDF (-> the job's PageFiles); anything else is
    a ValueError - raised by the public entry points before a source is read.  `jpeg_optimize`, `jpeg_subsampling` (None, "4:2:0",
    "4:2:2", "4:4:4"), `jpeg_grey` (False, "auto"), `jpeg_bilevel` (False, "auto", "otsu", "adaptive") and `jpeg_mrc` (False, True
    or a dict of cells: yomitoku_amd/mrc.py, check_mrc) ask for something of those files: a value that is none of these is a
    ValueError, and so is any of the five without `jpeg`.  `jpeg_despeckle` (False, True, an int or a dict of sizes:
    yomitoku_amd/despeckle.py, check_despeckle) cleans the Group 4 files' bits: a value that is none of these, the switch without
    `jpeg`, and the switch with `jpeg_bilevel=False` - there is no Group 4 file to clean - are ValueErrors.  `jpeg_lossless` (False,
    True or {"budget": bytes per pixel}: yomitoku_amd/flate.py, check_lossless) writes the pages the other switches leave as lossless
    files: any other value, an unknown key, a budget that is no positive finite number, and the switch without `jpeg` are ValueErrors."""
    return page_files(jpeg, jpeg_optimize, jpeg_subsampling, jpeg_grey, jpeg_bilevel, jpeg_mrc, serve=True, despeckle=jpeg_despeckle,
                      lossless=jpeg_lossless)


def launch_encode(pages: Sequence[torch.Tensor], quality: int, capacities: Optional[Sequence[int]], optimize: bool,
                  modes: Sequence[int], scratch: dict):
    """Launch the coding of device pages on the current stream (ymk_jpeg_encode_pages, or - optimize - ymk_jpeg_encode_pages_opt).
    modes: word 15 per page.  -> (the buffer of the files, per page its byte offset there, the files' lengths on the device)."""
    lib, device, n = _lib.load(), pages[0].device, len(pages)
    if not any(modes):
        modes = None  # the defaults: the table and the sizes of every call before there were modes
    blob, offsets, out_bytes = page_table(pages, quality, capacities, optimize, modes)
    sized = scratch_sizes([(int(p.shape[0]), int(p.shape[1]), 1 if p.dim() == 2 else 3) for p in pages], optimize, modes)
    mcus, blocks, intervals, coef_b, stream_b, iv_b = sized[:6]
    coef = grown(scratch, "coef", coef_b // 2, torch.int16, device)
    bits = grown(scratch, "stream", stream_b // 4, torch.int32, device)
    ivals = grown(scratch, "intervals", iv_b // 4, torch.int32, device)
    files = grown(scratch, "out", out_bytes, torch.uint8, device)
    lengths = grown(scratch, "lengths", n, torch.int32, device)
    blob_dev = imaging._stage_blob(blob, device)
    if optimize:
        hist = grown(scratch, "hist", sized[6] // 4, torch.int32, device)
        tables = grown(scratch, "tables", sized[7] // 4, torch.int32, device)
        dht = grown(scratch, "dht", sized[8] // 4, torch.int32, device)
        _lib.check(lib.ymk_jpeg_encode_pages_opt(blob_dev.data_ptr(), blob.size, n, mcus, blocks, intervals, coef.data_ptr(),
                                                 hist.data_ptr(), tables.data_ptr(), dht.data_ptr(), bits.data_ptr(), stream_b,
                                                 ivals.data_ptr(), files.data_ptr(), out_bytes, lengths.data_ptr(),
                                                 _lib.current_stream_ptr()), "ymk_jpeg_encode_pages_opt")
    else:
        _lib.check(lib.ymk_jpeg_encode_pages(blob_dev.data_ptr(), blob.size, n, mcus, blocks, intervals, coef.data_ptr(),
                                             bits.data_ptr(), stream_b, ivals.data_ptr(), files.data_ptr(), out_bytes,
                                             lengths.data_ptr(), _lib.current_stream_ptr()), "ymk_jpeg_encode_pages")
    return files, offsets, lengths


@dataclass
class _Page:
    """One live page of a call on its way to its entry."""

    k: int  # its index in the call
    dev: torch.Tensor  # on the device; the resized page once the preset has shrunk it
    large: bool  # its long side exceeds the preset's
    kind: str = "jpeg"  # what it becomes: "jpeg" | "group4" | "layered" | "lossless"
    scale: float = 1.0
    threshold: Optional[int] = None  # Otsu's, of a thresholded page
    despeckled: Optional[object] = None  # of a despeckled Group 4 page its Despeckled; of a layered page with a filtered mask its InkFiltered
    layer: Optional[int] = None  # a layered page's place in the separation
    jpeg_at: Optional[int] = None  # its place in the JPEG batch; a layered page: its foreground's, the background follows
    g4_at: Optional[int] = None  # its - or its mask's - place in the Group 4 batch
    flat_at: Optional[int] = None  # its place among the pages the lossless coder was given


def _sort(batch: List[_Page], files: PageFiles, scratch: dict):
    """Phase 1: say of every page what it becomes.  -> (the bilevel test or None, the separation or None, the grey test where it
    was launched early or None).  One wait with `bilevel`, one with `mrc`."""
    devs = [p.dev for p in batch]
    test = sep = early_grey = None
    if files.bilevel is not False:
        # on the pages as they arrived: the preset's resample would leave a two-valued page grey-valued.  Where no page can be
        # resized the grey test sees the same pixels before and after that step: it is launched here and shares the wait
        # "otsu" / "adaptive": the launches that threshold every page in place of the test; two-valued is then "grey-valued"
        test = ccitt.start_test(devs, scratch) if files.bilevel == "auto" else ccitt.start_binarize(devs, scratch, files.bilevel)
        if files.grey == "auto" and not any(p.large for p in batch):
            early_grey = _grey_launch(devs, scratch)
        torch.cuda.current_stream().synchronize()
        thresholds = test.thresholds() if files.bilevel != "auto" else [None] * len(batch)
        for p, two, threshold in zip(batch, test.answers(), thresholds):
            if two:
                p.kind, p.threshold = "group4", threshold
    cand = [j for j, p in enumerate(batch) if p.kind == "jpeg"]
    if files.mrc is not None and cand:
        # with `bilevel` the ink goes where the test packed these pages' rows, which nothing reads any more: one buffer of
        # packed rows for the one set of Group 4 launches
        shared = None if test is None else (test.packed, [test.packed_at[j] for j in cand], test.packed_bytes)
        sep = layered.launch([devs[j] for j in cand], files.mrc, scratch, packed=shared)
        torch.cuda.current_stream().synchronize()
        for i, (j, flag, filtered) in enumerate(zip(cand, sep.flags(), sep.filtered())):
            if flag == 1:
                batch[j].kind, batch[j].layer, batch[j].despeckled = "layered", i, filtered  # the mask's InkFiltered, or None
    return test, sep, early_grey


def _jpeg_batch(batch: List[_Page], files: PageFiles, long_side, sep, early_grey, capacities, scratch: dict):
    """Phase 2: -> (the pages of the JPEG launches, their capacities or None, per page whether it is written as a grey file): the
    pages that stay JPEG, shrunk to the preset and tested for grey, then the two layers of every layered page."""
    todo = []
    for p in batch:
        h, w = int(p.dev.shape[0]), int(p.dev.shape[1])
        if p.kind == "jpeg" and p.large:
            p.scale = long_side / max(w, h)
            todo.append((p, (max(int(h * p.scale), 1), max(int(w * p.scale), 1))))
    if todo:
        for (p, _), small in zip(todo, resize_pages([p.dev for p, _ in todo], [s for _, s in todo])):
            p.dev = small
    plain = [p for p in batch if p.kind == "jpeg"]  # all of them without `bilevel` and `mrc`
    jdevs = [p.dev for p in plain]
    caps = None if capacities is None else [int(capacities[p.k]) for p in plain]
    if early_grey is not None:
        as_grey = [g for p, g in zip(batch, _grey_answers(len(batch), early_grey)) if p.kind == "jpeg"]
    else:
        as_grey = grey_pages(jdevs, scratch) if files.grey == "auto" and jdevs else [False] * len(jdevs)
    for i, p in enumerate(plain):
        p.jpeg_at = i
    lay = [p for p in batch if p.kind == "layered"]
    if lay:  # behind the plain pages the two layers of every layered page, foreground first: pages like any other
        if caps is None:
            caps = [d.numel() for d in jdevs]
        for p in lay:
            p.jpeg_at = len(jdevs)
            jdevs += [sep.foreground(p.layer), sep.background(p.layer)]
        caps += [d.numel() + layered.LAYER_ROOM for d in jdevs[len(plain):]]
        as_grey = list(as_grey) + [False] * (len(jdevs) - len(plain))
    return jdevs, caps, as_grey


def _group4_batch(batch: List[_Page], test, sep):
    """Phase 4's pages: -> (what holds their packed rows, their indices there): the two-valued pages, then the masks."""
    two = [j for j, p in enumerate(batch) if p.kind == "group4"]
    lay = [j for j, p in enumerate(batch) if p.kind == "layered"]
    for i, j in enumerate(two + lay):
        batch[j].g4_at = i
    # with `bilevel` the masks lie in the test's buffer, at their pages' places
    return (test, two + lay) if test is not None else (sep, [batch[j].layer for j in lay])


def _lossless_batch(batch: List[_Page], files: PageFiles, scratch: dict):
    """Phase 1c: the pages the sort left become lossless files - all of them, or, with a budget, those whose file fits it: the
    first phase of the coder, ONE wait for the files' sizes, the rest for the pages that go on; a page over the budget stays
    "jpeg".  `grey="auto"`: the device test runs in front, and the kernels read its answer - no wait of its own.
    -> the coding, or None where no page was left."""
    cand = [p for p in batch if p.kind == "jpeg"]
    if not cand:
        return None
    coding, keep = flate.launch([p.dev for p in cand], scratch, files.lossless["budget256"], grey=files.grey == "auto")
    for i, (p, go) in enumerate(zip(cand, keep)):
        if go:
            p.kind, p.flat_at = "lossless", i
    return coding


def _entries(batch: List[_Page], files: PageFiles, out: list, jdevs, caps, as_grey, sizes, datas, flat=None):
    """Phase 5's end: every live page's entry into `out`, from the files' bytes - the JPEG batch's, then the Group 4 batch's, then
    the lossless pages' (`flat`: (the first of them in `datas`, per page its channels))."""
    def jpeg_entry(i, k, scale, what="the JPEG file"):
        d = jdevs[i]
        if sizes[i] < 0:
            cap = caps[i] if caps is not None else d.numel()
            return _lib.YmkError(f"page {k}: {what} does not fit its capacity of {cap} bytes")
        one = d.dim() == 2 or as_grey[i]
        return EncodedJpeg(datas[i], int(d.shape[1]), int(d.shape[0]), one, float(scale), bool(files.optimize), None if one else files.subsampling)

    for p in batch:
        if p.kind == "jpeg":
            out[p.k] = jpeg_entry(p.jpeg_at, p.k, p.scale)
        elif p.kind == "group4":
            out[p.k] = ccitt.bilevel_entry(p.dev, datas[len(jdevs) + p.g4_at], p.k, files.bilevel, p.threshold, p.despeckled)
        elif p.kind == "lossless":
            out[p.k] = flate.lossless_entry(p.dev, datas[flat[0] + p.flat_at], flat[1][p.flat_at], p.k)
        else:
            parts = [ccitt.bilevel_entry(p.dev, datas[len(jdevs) + p.g4_at], p.k, "adaptive", None, p.despeckled),
                     jpeg_entry(p.jpeg_at, p.k, 1.0, "the foreground's file"), jpeg_entry(p.jpeg_at + 1, p.k, 1.0, "the background's file")]
            failed = [e for e in parts if isinstance(e, BaseException)]
            out[p.k] = failed[0] if failed else layered.EncodedMrc(parts[0], parts[2], parts[1], int(p.dev.shape[1]), int(p.dev.shape[0]), 1.0,
                                                                  files.mrc["bg_cell"], files.mrc["fg_cell"])


def encode_page_files(pages: Sequence, files: PageFiles, stream=None, scratch: Optional[dict] = None,
                      capacities: Optional[Sequence[int]] = None) -> list:
    """`encode_jpeg_pages` with its options as a PageFiles (serve: the job's): one entry per page, in order.  `files.despeckle`
    cleans every page of kind "group4", the "auto" pages included: the switch is the caller's decision about the job, and "auto"
    with it is no longer lossless."""
    preset = IMAGE_QUALITY_PRESETS[files.preset]
    quality, long_side = int(preset["jpeg_quality"]), preset["max_long_side"]
    scratch = {} if scratch is None else scratch
    with entered(pages, stream, "encode_jpeg_pages needs") as (_, live, devs, out):
        if not live:
            return out
        batch = [_Page(k, dev, long_side is not None and max(int(dev.shape[0]), int(dev.shape[1])) > long_side) for k, dev in zip(live, devs)]
        # 1. sort: `bilevel`'s test (and the grey test, where no page is resized) and its wait; `mrc`'s separation and its wait
        test, sep, early_grey = _sort(batch, files, scratch)
        # 1b. `despeckle`: the Group 4 pages' bits cleaned in place, behind the wait that says which they are; no wait of its own
        two = [j for j, p in enumerate(batch) if p.kind == "group4"] if files.despeckle is not None else []
        if two:
            cc_pin = to_pinned(scratch, "cc_pin_counts", specks.launch(test, two, files.despeckle, scratch), 4 * len(two))
        # 1c. `lossless`: the pages that are left go to the lossless coder; with a budget one wait for the sizes, else none
        coding = _lossless_batch(batch, files, scratch) if files.lossless is not None else None
        # 2. the JPEG batch: resize, the grey test (its own wait unless it ran early), the layers behind the plain pages
        jdevs, caps, as_grey = _jpeg_batch(batch, files, long_side, sep, early_grey, capacities, scratch)
        # 3. launch JPEG; the lengths go to the host first (one small copy), the bytes, packed on the device, in the gather
        if jdevs:
            colour = SUBSAMPLINGS[files.subsampling]
            modes = [0 if d.dim() == 2 else (MODE_GREY if g else colour) for d, g in zip(jdevs, as_grey)]
            jpegs, offsets, lengths = launch_encode(jdevs, quality, caps, files.optimize, modes, scratch)
            pin_len = to_pinned(scratch, "pin_lengths", lengths, len(jdevs))
        # 4. launch Group 4 behind the JPEG stages: the two-valued pages, then the masks
        coded, which = _group4_batch(batch, test, sep)
        if which:
            g4s, g4_offsets, g4_lengths = ccitt.launch_encode(coded, which, scratch)
            g4_pin = to_pinned(scratch, "g4_pin_lengths", g4_lengths, len(which))
        # 5. one wait for the lengths, one gather of the bytes (its own wait), the entries
        torch.cuda.current_stream().synchronize()
        sizes = pin_len[: len(jdevs)].tolist() if jdevs else []
        for j, four in zip(two, cc_pin[: 4 * len(two)].view(-1, 4).tolist() if two else []):
            batch[j].despeckled = specks.result(files.despeckle, four)
        parts = [(jpegs, offsets[i], sizes[i]) for i in range(len(jdevs))]
        if which:
            parts += [(g4s, g4_offsets[i], n) for i, n in enumerate(g4_pin[: len(which)].tolist())]
        flat = None
        if coding is not None:
            answers, went = coding.answers(), {p.flat_at for p in batch if p.kind == "lossless"}
            flat = (len(parts), [ch for _, ch in answers])
            parts += [(coding.out, coding.offsets[i], n if i in went else -1) for i, (n, _) in enumerate(answers)]
        _entries(batch, files, out, jdevs, caps, as_grey, sizes, gather_files(parts, scratch), flat)
    return out


def encode_jpeg_pages(pages: Sequence, image_quality: str = "high", stream=None, scratch: Optional[dict] = None,
                      capacities: Optional[Sequence[int]] = None, optimize: bool = False, subsampling: str = "4:2:0",
                      grey=False, bilevel=False, mrc=False, despeckle=False, lossless=False) -> list:
    """One entry per page, in order: its EncodedJpeg, or the exception that page raised (not uint8, not H x W x 3 / H x W; a
    file larger than its capacity - default: the page's raw byte count).  pages: device tensors and / or host arrays.
    stream: the torch stream to launch on (default: the current one).  scratch: a dict the caller keeps between calls to reuse
    the device and pinned buffers (serve: one per wave slot); capacities: bytes allowed per page's file - the default cannot
    hold the ~620-byte header (~330 grey) plus the scan of a page below roughly 15 x 15 pixels, nor noise that does not compress.
    optimize: Huffman tables made for each page (two more launches; the header shrinks with the tables, to ~270 bytes for a
    flat colour page); the decoded pixels are those of the plain file.
    subsampling: "4:2:0", "4:2:2" or "4:4:4", the chroma of the colour files; grey: False, or "auto" - a three-channel page
    whose pixels all have B == G == R (tested on the device, after the preset's resize) becomes a grey file.
    bilevel: False, or "auto" - a two-valued page (every sample 0 or 255, B == G == R; tested on the device on the page as it
    arrived) gets an EncodedBilevel, a Group 4 file (yomitoku_amd/ccitt.py), in place of the EncodedJpeg: full size whatever
    the preset (scale 1.0), lossless, untouched by optimize / subsampling / grey / capacities; every other page goes the way it
    goes without the switch, in the same call.  The test is one more launch and one more wait for its answer - with
    grey="auto" and no page to resize the two tests share that wait.
    bilevel: "otsu" or "adaptive" - every GREY-VALUED page (one channel, or B == G == R everywhere; a grey photograph too: it is
    the caller's decision about the job) is thresholded on the device, by Otsu's threshold of the page or by a locally adaptive
    one (yomitoku_amd/ccitt.py; tests/binarize_ref.py is the definition), and gets an EncodedBilevel with `method` and
    `threshold` set, exactly as above: full size, scale 1.0.  A colour page goes the way it goes without the switch.  The
    launches that threshold stand where the test stands, in front of the same single wait for the pages' flags.
    mrc: False, True or {"bg_cell": 2, "fg_cell": 8} (yomitoku_amd/mrc.py: check_mrc) - of the pages `bilevel` leaves, one channel or
    three, every page with ink and with paper outside it gets an EncodedMrc in place of the EncodedJpeg: its ink mask as a Group 4
    file and two low-resolution layers as JPEG files at the preset's quality - full size whatever the preset (scale 1.0);
    `optimize` and `subsampling` apply to the two layer files as they would to a page, `grey` and `capacities` do not (a layer's
    capacity is its raw bytes plus 2048).  A page without ink or without paper goes the way it goes without the switch.  The
    separation is launched behind `bilevel`'s wait and has one wait of its own, for its flags: with both switches on that is one
    further wait; the layers then join the JPEG launches and the masks the Group 4 launches, and the files come back in the same
    two copies.  The dict may also hold "despeckle" (as `despeckle` below takes it) and "blobs" (False, True or {"side": 128,
    "fill": 64}: yomitoku_amd/despeckle.py, check_blobs): the ink filtered on the device before the separation - specks and
    pinholes removed, and every component at least `side` high and wide that fills `fill` / 256 of its box, the dark part of a
    picture, left to the background; the mask's `despeckled` is then an InkFiltered.  No further wait.
    despeckle: False, True (4 and 4), an int or {"black": n, "white": n} (yomitoku_amd/despeckle.py: check_despeckle) - every
    page that gets a Group 4 file of its own, the "auto" pages included, has its 8-connected black components of fewer than
    `black` pixels cleared and then its 4-connected white components of fewer than `white` pixels filled, on the device,
    between the threshold and the coder; the entry's `despeckled` says how many.  It is the caller's decision about the job:
    bilevel="auto" with the switch is no longer lossless.  It needs `bilevel`; the masks of layered pages are not touched.  Four
    launches a colour behind `bilevel`'s wait, no wait of its own: the counts come back with the files' lengths.
    lossless: False, True or {"budget": bytes per pixel} (yomitoku_amd/flate.py: check_lossless) - of the pages `bilevel` and `mrc`
    leave, one channel or three, every page gets an EncodedLossless in place of the EncodedJpeg: a zlib stream of its PNG-filtered
    rows, full size whatever the preset (scale 1.0); `optimize`, `subsampling` and `capacities` do not apply to it, `grey="auto"`
    does: a three-channel page with B == G == R everywhere is written as one channel.  Five launches behind the sort, no wait of
    their own.  With a budget a page goes lossless only where its file takes at most that many bytes a pixel - the size is exact
    after the first two launches, which one further wait follows - and otherwise gets exactly the JPEG it gets without the switch.
    Anything else is a ValueError before any device work.  A 4:4:4 file is larger: noise may no longer fit the default capacity."""
    return encode_page_files(pages, page_files(image_quality, optimize, subsampling, grey, bilevel, mrc, despeckle=despeckle, lossless=lossless),
                             stream, scratch, capacities)


def encode_jpeg(page, image_quality: str = "high", stream=None, optimize: bool = False, subsampling: str = "4:2:0",
                grey=False, bilevel=False, mrc=False):
    """One page; raises what `encode_jpeg_pages` would have put in its place.  The file's capacity is the page's raw byte
    count, and the header alone takes about 620 bytes (330 for a grey page): a colour page below roughly 15 x 15 pixels, or noise
    that does not compress, raises YmkError here and in `serve(jpeg=...)` - `encode_jpeg_pages(..., capacities=[...])` gives
    such a page the room it needs.  bilevel="auto": an EncodedBilevel where the page is two-valued; "otsu" / "adaptive": where
    it is grey-valued, thresholded.  mrc: an EncodedMrc where the page has ink and paper (yomitoku_amd/mrc.py)."""
    res = encode_jpeg_pages([page], image_quality, stream, optimize=optimize, subsampling=subsampling, grey=grey, bilevel=bilevel, mrc=mrc)[0]
    if isinstance(res, BaseException):
        raise res
    return res
