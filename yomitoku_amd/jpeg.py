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
"""

from __future__ import annotations

import ctypes
import functools
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib, imaging
from .utils.searchable_pdf import IMAGE_QUALITY_PRESETS

PAGE_WORDS, RESIZE_WORDS = 16, 16  # YMK_JPEG_PAGE_WORDS, YMK_PIL_RESIZE_U8_WORDS
MAX_SIDE = 16383
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
    arr = ctypes.c_int * max(1, n)
    sizes = (ctypes.c_int64 * (9 if optimize else 6))()
    name = "ymk_jpeg_scratch_bytes_opt_mode" if optimize else "ymk_jpeg_scratch_bytes_mode"
    _lib.check(getattr(_lib.load(), name)(arr(*[s[0] for s in shapes]), arr(*[s[1] for s in shapes]), arr(*[s[2] for s in shapes]),
                                          None if modes is None else arr(*[int(m) for m in modes]), n, sizes), name)
    return tuple(int(v) for v in sizes)


@functools.lru_cache(maxsize=64)
def _lanczos(in_size: int, out_size: int):
    return imaging.pil_lanczos_coeffs(in_size, out_size)  # ~10 ms of host time per new (in, out) pair: the pages of a job share theirs


def _addr_words(ptr: int):
    return np.array([ptr & 0xFFFFFFFF, ptr >> 32], dtype=np.uint32).view(np.int32)


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
        rec[k, 0:2] = _addr_words(p.data_ptr())
        rec[k, 2:8] = (h, w, ch, mcu, blk, iv)
        rec[k, 8:10] = _addr_words(out_at)
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


def _grown(scratch: dict, key: str, count: int, dtype, device=None, pinned=False) -> torch.Tensor:
    """scratch[key] with room for `count` elements: kept between calls, replaced (never resized) when it is too small."""
    t = scratch.get(key)
    if t is None or t.numel() < count or (not pinned and t.device != device):
        count = max(int(count * 1.25), 1024)
        t = torch.empty(count, dtype=dtype, pin_memory=True) if pinned else torch.empty(count, dtype=dtype, device=device)
        scratch[key] = t
    return t


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
        recs[k, 0:2] = _addr_words(p.data_ptr())
        recs[k, 2:9] = (h, w, ch, oh, ow, ksx, ksy)
        for j, t in enumerate((xb, xk, yb, yk)):
            recs[k, 9 + j] = at
            tables.append(t.reshape(-1))
            at += t.size
        recs[k, 13:15] = _addr_words(out.data_ptr())
        outs.append(out)
    blob = np.concatenate([recs.reshape(-1)] + tables).astype(np.int32, copy=False)
    blob_dev = imaging._stage_blob(blob, dev)
    _lib.check(_lib.load().ymk_pil_resize_u8(blob_dev.data_ptr(), blob.size, len(pages), max(s[0] for s in sizes),
                                             max(s[1] for s in sizes), _lib.current_stream_ptr()), "ymk_pil_resize_u8")
    return outs


def _as_device_page(page, device) -> torch.Tensor:
    if isinstance(page, torch.Tensor):
        t = page
    else:
        arr = np.ascontiguousarray(np.asarray(page))
        if arr.dtype != np.uint8:
            raise ValueError(f"a page is uint8, got {arr.dtype}")
        t = torch.from_numpy(arr)
    if t.dtype != torch.uint8 or not (t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 3)):
        raise ValueError(f"a page is uint8 H x W x 3 (B G R) or H x W, got {t.dtype} {tuple(t.shape)}")
    if min(t.shape[:2]) < 1 or max(t.shape[:2]) > MAX_SIDE:
        raise ValueError(f"a page has 1..{MAX_SIDE} pixels on a side, got {tuple(t.shape[:2])}")
    if t.device.type != "cuda":
        t = t.to(device, non_blocking=False)
    return t.contiguous()


def _grey_launch(pages: Sequence[torch.Tensor], scratch: dict):
    """Launch the grey test of the three-channel pages among `pages` on the current stream and the copy of its answer to
    pinned memory; waits for nothing.  -> (their indices, the pinned answer), or None where there is no such page."""
    cand = [k for k, p in enumerate(pages) if p.dim() == 3]
    if not cand:
        return None
    device = pages[cand[0]].device
    rec = np.zeros((len(cand), PAGE_WORDS), np.int32)
    for j, k in enumerate(cand):
        rec[j, 0:2] = _addr_words(pages[k].data_ptr())
        rec[j, 2:5] = (int(pages[k].shape[0]), int(pages[k].shape[1]), 3)
    blob_dev = imaging._stage_blob(rec.reshape(-1), device)
    diff = _grown(scratch, "grey", len(cand), torch.int32, device)
    _lib.check(_lib.load().ymk_jpeg_pages_grey(blob_dev.data_ptr(), rec.size, len(cand), max(int(pages[k].shape[0]) * int(pages[k].shape[1]) for k in cand),
                                               diff.data_ptr(), _lib.current_stream_ptr()), "ymk_jpeg_pages_grey")
    pin = _grown(scratch, "pin_grey", len(cand), torch.int32, pinned=True)
    pin[: len(cand)].copy_(diff[: len(cand)], non_blocking=True)
    return cand, pin


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


def _gather_files(parts: Sequence, scratch: dict, key: str = "pin_bytes") -> list:
    """parts: (device buffer, byte offset, length or -1) per file -> their bytes (None for -1): packed on the device, then one
    copy through pinned memory and one wait."""
    good = [(buf, at, n) for buf, at, n in parts if n >= 0]
    total = sum(n for _, _, n in good)
    host = None
    if total:
        packed = torch.cat([buf[at : at + n] for buf, at, n in good])
        pin = _grown(scratch, key, total, torch.uint8, pinned=True)
        pin[:total].copy_(packed, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        host = pin[:total].numpy()
    out, at = [], 0
    for _, _, n in parts:
        out.append(None if n < 0 else host[at : at + n].tobytes())
        at += max(n, 0)
    return out


def encode_jpeg_pages(pages: Sequence, image_quality: str = "high", stream=None, scratch: Optional[dict] = None,
                      capacities: Optional[Sequence[int]] = None, optimize: bool = False, subsampling: str = "4:2:0",
                      grey=False, bilevel=False, mrc=False) -> list:
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
    two copies.
    Anything else is a ValueError before any device work.  A 4:4:4 file is larger: noise may no longer fit the default capacity."""
    preset = jpeg_preset(image_quality)
    colour_mode = check_modes(subsampling, grey)
    mrc_params = None
    if mrc is not False:
        from . import ccitt
        from . import mrc as layered  # imports this module

        mrc_params = layered.check_mrc(mrc)
    if bilevel is not False:
        from . import ccitt  # imports this module

        ccitt.check_bilevel(bilevel)
    quality, long_side = int(preset["jpeg_quality"]), preset["max_long_side"]
    out: list = [None] * len(pages)
    if not pages:
        return out
    if not torch.cuda.is_available():
        raise _lib.YmkError("encode_jpeg_pages needs a HIP device (there is no host fallback)")
    device = next((p.device for p in pages if isinstance(p, torch.Tensor) and p.device.type == "cuda"),
                  torch.device("cuda", torch.cuda.current_device()))
    scratch = {} if scratch is None else scratch
    lib = _lib.load()
    with torch.cuda.device(device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(device)):
        live, devs = [], []
        for k, page in enumerate(pages):
            try:
                devs.append(_as_device_page(page, device))
                live.append(k)
            except Exception as exc:  # noqa: BLE001 - only this page fails
                out[k] = exc
        if not live:
            return out
        large = [long_side is not None and max(int(p.shape[0]), int(p.shape[1])) > long_side for p in devs]
        two, test, early_grey, thresholds = [False] * len(devs), None, None, [None] * len(devs)
        if bilevel is not False:
            # on the pages as they arrived: the preset's resample would leave a two-valued page grey-valued.  Where no page can be
            # resized the grey test sees the same pixels before and after that step: it is launched here and shares the wait
            # "otsu" / "adaptive": the launches that threshold every page in place of the test; `two` is then "grey-valued"
            test = ccitt.start_test(devs, scratch) if bilevel == "auto" else ccitt.start_binarize(devs, scratch, bilevel)
            if grey == "auto" and not any(large):
                early_grey = _grey_launch(devs, scratch)
            torch.cuda.current_stream().synchronize()
            two = test.answers()
            thresholds = test.thresholds() if bilevel != "auto" else [None] * len(devs)
        sep, sep_of = None, {}  # the separation of the pages `bilevel` left, and page -> its index there where its flag is 1
        if mrc_params is not None:
            cand = [j for j in range(len(devs)) if not two[j]]
            if cand:
                # with `bilevel` the ink goes where the test packed these pages' rows, which nothing reads any more: one buffer
                # of packed rows for the one set of Group 4 launches
                shared = None if test is None else (test.packed, [test.packed_at[j] for j in cand], test.packed_bytes)
                sep = layered.launch([devs[j] for j in cand], mrc_params, scratch, packed=shared)
                torch.cuda.current_stream().synchronize()
                sep_of = {j: i for i, (j, flag) in enumerate(zip(cand, sep.flags())) if flag == 1}
        scales = [1.0] * len(live)
        todo = []
        for j, p in enumerate(devs):
            h, w = int(p.shape[0]), int(p.shape[1])
            if large[j] and not two[j] and j not in sep_of:
                scales[j] = long_side / max(w, h)
                todo.append((j, (max(int(h * scales[j]), 1), max(int(w * scales[j]), 1))))
        if todo:
            for (j, _), small in zip(todo, resize_pages([devs[j] for j, _ in todo], [s for _, s in todo])):
                devs[j] = small
        rest = [j for j in range(len(devs)) if not two[j] and j not in sep_of]  # the pages that get a JPEG file: all of them without `bilevel`
        jdevs = [devs[j] for j in rest]
        caps = None if capacities is None else [int(capacities[live[j]]) for j in rest]
        n_plain = len(jdevs)
        if early_grey is not None:
            all_grey = _grey_answers(len(devs), early_grey)
            as_grey = [all_grey[j] for j in rest]
        else:
            as_grey = grey_pages(jdevs, scratch) if grey == "auto" and jdevs else [False] * len(jdevs)
        if sep_of:  # behind the plain pages the two layers of every layered page, foreground first: pages like any other
            if caps is None:
                caps = [p.numel() for p in jdevs]
            for j, i in sep_of.items():
                jdevs += [sep.foreground(i), sep.background(i)]
            caps += [p.numel() + layered.LAYER_ROOM for p in jdevs[n_plain:]]
            as_grey = list(as_grey) + [False] * (len(jdevs) - n_plain)
        sizes = []
        if jdevs:
            modes = [0 if p.dim() == 2 else (MODE_GREY if g else colour_mode) for p, g in zip(jdevs, as_grey)]
            if not any(modes):
                modes = None  # the defaults: the table and the sizes of every call before there were modes
            blob, offsets, out_bytes = page_table(jdevs, quality, caps, optimize, modes)
            sized = scratch_sizes([(int(p.shape[0]), int(p.shape[1]), 1 if p.dim() == 2 else 3) for p in jdevs], optimize, modes)
            mcus, blocks, intervals, coef_b, stream_b, iv_b = sized[:6]
            coef = _grown(scratch, "coef", coef_b // 2, torch.int16, device)
            bits = _grown(scratch, "stream", stream_b // 4, torch.int32, device)
            ivals = _grown(scratch, "intervals", iv_b // 4, torch.int32, device)
            files = _grown(scratch, "out", out_bytes, torch.uint8, device)
            lengths = _grown(scratch, "lengths", len(jdevs), torch.int32, device)
            blob_dev = imaging._stage_blob(blob, device)
            if optimize:
                hist = _grown(scratch, "hist", sized[6] // 4, torch.int32, device)
                tables = _grown(scratch, "tables", sized[7] // 4, torch.int32, device)
                dht = _grown(scratch, "dht", sized[8] // 4, torch.int32, device)
                _lib.check(lib.ymk_jpeg_encode_pages_opt(blob_dev.data_ptr(), blob.size, len(jdevs), mcus, blocks, intervals, coef.data_ptr(),
                                                         hist.data_ptr(), tables.data_ptr(), dht.data_ptr(), bits.data_ptr(), stream_b,
                                                         ivals.data_ptr(), files.data_ptr(), out_bytes, lengths.data_ptr(),
                                                         _lib.current_stream_ptr()), "ymk_jpeg_encode_pages_opt")
            else:
                _lib.check(lib.ymk_jpeg_encode_pages(blob_dev.data_ptr(), blob.size, len(jdevs), mcus, blocks, intervals, coef.data_ptr(),
                                                     bits.data_ptr(), stream_b, ivals.data_ptr(), files.data_ptr(), out_bytes,
                                                     lengths.data_ptr(), _lib.current_stream_ptr()), "ymk_jpeg_encode_pages")
            # the lengths first (one small copy), then the files' bytes, packed on the device, in one copy
            pin_len = _grown(scratch, "pin_lengths", len(jdevs), torch.int32, pinned=True)
            pin_len[: len(jdevs)].copy_(lengths[: len(jdevs)], non_blocking=True)
        which = [j for j in range(len(devs)) if two[j]]
        if sep_of:  # the masks behind the two-valued pages; `coded` is what holds the packed rows of both
            if test is None:
                coded, which = sep, list(sep_of.values())
            else:
                coded, which = test, which + list(sep_of)
        else:
            coded = test
        if which:  # the Group 4 files: launched behind the JPEG stages, their lengths and bytes in the same two copies' waits
            g4_files, g4_offsets, g4_lengths = ccitt.launch_encode(coded, which, scratch)
            g4_pin = _grown(scratch, "g4_pin_lengths", len(which), torch.int32, pinned=True)
            g4_pin[: len(which)].copy_(g4_lengths[: len(which)], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        parts = []
        if jdevs:
            sizes = pin_len[: len(jdevs)].tolist()
            parts += [(files, offsets[i], sizes[i]) for i in range(len(jdevs))]
        if which:
            parts += [(g4_files, g4_offsets[i], n) for i, n in enumerate(g4_pin[: len(which)].tolist())]
        datas = _gather_files(parts, scratch)
        def jpeg_entry(i, p, k, scale, what="the JPEG file"):
            if sizes[i] < 0:
                cap = caps[i] if caps is not None else p.numel()
                return _lib.YmkError(f"page {k}: {what} does not fit its capacity of {cap} bytes")
            one = p.dim() == 2 or as_grey[i]
            return EncodedJpeg(datas[i], int(p.shape[1]), int(p.shape[0]), one, float(scale), bool(optimize), None if one else subsampling)

        for i, j in enumerate(rest):
            out[live[j]] = jpeg_entry(i, devs[j], live[j], scales[j])
        n_two = len(which) - len(sep_of)
        for i, j in enumerate(which[:n_two]):
            out[live[j]] = ccitt.bilevel_entry(devs[j], datas[len(jdevs) + i], live[j], bilevel, thresholds[j])
        for i, j in enumerate(sep_of):
            k, at = live[j], n_plain + 2 * i
            parts3 = [ccitt.bilevel_entry(devs[j], datas[len(jdevs) + n_two + i], k, "adaptive"),
                      jpeg_entry(at, jdevs[at], k, 1.0, "the foreground's file"), jpeg_entry(at + 1, jdevs[at + 1], k, 1.0, "the background's file")]
            failed = [e for e in parts3 if isinstance(e, BaseException)]
            out[k] = failed[0] if failed else layered.EncodedMrc(parts3[0], parts3[2], parts3[1], int(devs[j].shape[1]), int(devs[j].shape[0]), 1.0,
                                                                mrc_params["bg_cell"], mrc_params["fg_cell"])
    return out


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
