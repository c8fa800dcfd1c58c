"""Lossless files of pages that are already on the device: a zlib stream (RFC 1950; one dynamic-Huffman Deflate block) of the
page's PNG-filtered rows - a PNG's IDAT as it is, and what a searchable PDF embeds as a `/FlateDecode` image with `/Predictor 15`
(utils/searchable_pdf.py).  For born-digital pages - rasterised PDFs, screenshots, slides, forms - and pages with drawn graphics:
flat colour with hard edges, where a JPEG rings around every stroke and is the larger file.

    encoded = encode_lossless_pages(pages)                      # device tensors or host arrays, uint8 H x W x 3 (B G R) or H x W
    encoded[0].to_png()                                         # IHDR + one IDAT + IEND
    encode_jpeg_pages(pages, "high", lossless=True)             # every page `bilevel` and `mrc` leave, as an EncodedLossless
    encode_jpeg_pages(pages, "high", lossless={"budget": 0.5})  # ... where its file takes at most half a byte a pixel; else the JPEG

The whole file is made on the device (yomitoku_amd/csrc/ymk_flate.hip; DESIGN.md, "Lossless pages"): a wave per row segment filters
the row (the PNG filter of the smallest sum of absolute values), finds matches at six fixed distances, parses greedily and counts
symbols; a wave per page makes the page's own Huffman tables and knows the file's exact size; then the segments are coded into slots,
their bit counts scanned, and every word of every file gathered - as the Group 4 path does.  The definition is tests/flate_ref.py,
which `zlib.decompress` and Pillow read back to the exact pixels.  The host sees the files' sizes and their bytes, through pinned
memory.  There is no host fallback.
"""

from __future__ import annotations

import ctypes
import math
import struct
import zlib
from dataclasses import dataclass
from typing import ClassVar, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib, imaging
from .devpages import addr_words, entered, gather_files, grown, shape_args, to_pinned

PAGE_WORDS, HIST_WORDS, HEAD_WORDS = 16, 320, 160  # YMK_FLATE_PAGE_WORDS, YMK_FLATE_HIST_WORDS, YMK_FLATE_HEAD_WORDS
SEGMENT = 8192  # filtered bytes of a row segment


@dataclass
class EncodedLossless:
    """One page as a zlib stream of its PNG-filtered rows (a row: its filter type, then R G B or grey bytes).  `channels`: 3, or 1 -
    of a one-channel page, and of a three-channel page that `grey="auto"` found grey.  `scale` is 1.0: a lossless page is never
    resized."""

    data: bytes
    width: int
    height: int
    channels: int
    scale: float = 1.0
    lossless: ClassVar[bool] = True  # what utils/searchable_pdf.py recognises the object by

    @property
    def nbytes(self) -> int:
        return len(self.data)

    def to_png(self) -> bytes:
        """The stream as a PNG: IHDR (8 bits; colour type 2, or 0 for one channel), one IDAT, IEND."""
        def chunk(kind: bytes, body: bytes) -> bytes:
            return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))

        head = struct.pack(">IIBBBBB", self.width, self.height, 8, 2 if self.channels == 3 else 0, 0, 0, 0)
        return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", head) + chunk(b"IDAT", bytes(self.data)) + chunk(b"IEND", b"")


def check_lossless(lossless=False) -> Optional[dict]:
    """False -> None; True -> {"budget256": None}: every page; {"budget": b}, b a positive finite number of bytes a pixel ->
    {"budget256": ceil(256 b)}: a page whose file fits.  The test is in integers (`within_budget`): nbytes * 256 <= budget256 * h * w.
    Anything else - another value, an unknown key, a budget that is no positive finite number - is a ValueError."""
    if lossless is False:
        return None
    if lossless is True:
        return {"budget256": None}
    if not isinstance(lossless, dict):
        raise ValueError(f"unknown jpeg lossless {lossless!r}: False, True or {{'budget': bytes per pixel}}")
    unknown = sorted(set(lossless) - {"budget"}, key=str)
    if unknown:
        raise ValueError(f"unknown jpeg lossless key {unknown[0]!r}: 'budget'")
    if "budget" not in lossless:
        return {"budget256": None}
    budget = lossless["budget"]
    if isinstance(budget, bool) or not isinstance(budget, (int, float)) or not math.isfinite(budget) or budget <= 0:
        raise ValueError(f"jpeg lossless budget {budget!r}: a positive finite number of bytes per pixel")
    return {"budget256": max(1, math.ceil(budget * 256))}


def within_budget(nbytes: int, h: int, w: int, budget256: Optional[int]) -> bool:
    return budget256 is None or int(nbytes) * 256 <= int(budget256) * int(h) * int(w)


def file_capacity(h: int, w: int, channels: int = 3) -> int:
    """The bytes no lossless file of an h x w x channels page exceeds: 15 bits a filtered byte, the longest header, end-of-block,
    78 9C, the pad and the checksum (the proof is in ymk_flate.hip; tests/flate_ref.py: file_capacity)."""
    n = int(_lib.load().ymk_flate_file_capacity(int(h), int(w), int(channels)))
    if n < 0:
        raise ValueError(f"a page has 1..16383 pixels on a side and 1 or 3 channels, got {(h, w, channels)}")
    return n


def scratch_sizes(shapes: Sequence) -> tuple:
    """(segments, bytes of the filtered rows, of the tokens, of each per-segment array, of the offsets, of the slots, of each of the
    histograms and tables, of the heads) of pages of `shapes` = (h, w) or (h, w, channels)."""
    sizes = (ctypes.c_int64 * 8)()
    _lib.check(_lib.load().ymk_flate_scratch_bytes(*shape_args(shapes, channels=True), len(shapes), sizes), "ymk_flate_scratch_bytes")
    return tuple(int(v) for v in sizes)


def _shape(p) -> tuple:
    return int(p.shape[0]), int(p.shape[1]), 1 if p.dim() == 2 else 3


def _slot_words(n: int) -> int:
    return (15 * n + 31) // 32 + 1  # no segment of n filtered bytes takes more than 15 n bits


def _row_layout(w: int, ch: int) -> tuple:
    """(segments, slot words) of a row of w pixels of ch channels, as ymk_flate.hip lays them out."""
    n = 1 + w * ch
    segs = -(-n // SEGMENT)
    return segs, (segs - 1) * _slot_words(SEGMENT) + _slot_words(n - (segs - 1) * SEGMENT)


def page_table(pages: Sequence[torch.Tensor], capacities: Optional[Sequence[int]] = None, grey_at: Optional[Sequence[int]] = None):
    """(int32 words of the page table of include/ymk.h, per page the byte offset of its file in the output, the output's bytes).
    capacities: bytes per page's file (default: `file_capacity`, which no file exceeds); grey_at: word 15 per page (default 0)."""
    rec = np.zeros((len(pages), PAGE_WORDS), np.int32)
    filt = seg = slot = out_at = 0
    offsets = []
    for k, p in enumerate(pages):
        h, w, ch = _shape(p)
        row_segs, row_slot = _row_layout(w, ch)
        cap = file_capacity(h, w, ch) if capacities is None else int(capacities[k])
        rec[k, 0:2] = addr_words(p.data_ptr())
        rec[k, 2:6] = (h, w, ch, k)
        rec[k, 6:8], rec[k, 8:10], rec[k, 10:12], rec[k, 12:14] = addr_words(filt), addr_words(seg), addr_words(slot), addr_words(out_at)
        rec[k, 14] = cap
        rec[k, 15] = 0 if grey_at is None else int(grey_at[k])
        offsets.append(out_at)
        filt, seg, slot = filt + h * (1 + w * ch), seg + h * row_segs, slot + h * row_slot
        out_at += -(-cap // 16) * 16
    return rec.reshape(-1), offsets, out_at


class _Coding:
    """The launches of a call's lossless pages: `start` queues the rows and the tables (after them every file's exact size is
    known), `finish` the coding of the pages that go on - all of them, or those within the budget."""

    def __init__(self, pages: Sequence[torch.Tensor], scratch: dict, grey: bool = False, capacities: Optional[Sequence[int]] = None):
        self.pages, self.scratch, self.n = list(pages), scratch, len(pages)
        device = pages[0].device
        self.grey_dev, grey_at = None, None
        if grey:  # the existing device test, in buffers of its own: its answer is read by the kernels, and by the host with the sizes
            from .jpeg import _grey_launch  # noqa: PLC0415 - jpeg.py imports this module

            own = scratch.setdefault("fl_grey", {})
            launched = _grey_launch(self.pages, own)
            if launched is not None:
                self.grey_dev, grey_at = own["grey"], [0] * self.n
                for j, k in enumerate(launched[0]):
                    grey_at[k] = j + 1
        self.blob, self.offsets, self.out_bytes = page_table(self.pages, capacities, grey_at)
        shapes = [_shape(p) for p in self.pages]
        self.segs, filt_b, tok_b, seg_b, off_b, self.slot_b, hist_b, head_b = scratch_sizes(shapes)
        self.filt_b = filt_b
        self.max_rows = max(s[0] for s in shapes)
        self.max_row_segs = max(_row_layout(s[1], s[2])[0] for s in shapes)
        self.largest = int(self.blob.reshape(-1, PAGE_WORDS)[:, 14].max())
        g = lambda key, count, dtype: grown(scratch, key, count, dtype, device)  # noqa: E731
        self.filt, self.tokens = g("fl_filt", filt_b, torch.uint8), g("fl_tokens", tok_b // 2, torch.int16)
        self.segtok, self.segadler, self.segbits = (g(key, seg_b // 4, torch.int32) for key in ("fl_segtok", "fl_segadler", "fl_segbits"))
        self.hist, self.tables = g("fl_hist", hist_b // 4, torch.int32), g("fl_tables", hist_b // 4, torch.int32)
        self.head, self.off, self.slots = g("fl_head", head_b // 4, torch.int32), g("fl_off", off_b // 8, torch.int64), g("fl_slots", self.slot_b // 4, torch.int32)
        self.out, self.sizes = g("fl_out", self.out_bytes, torch.uint8), g("fl_sizes", 2 * self.n, torch.int32)
        self.blob_dev = imaging._stage_blob(self.blob, device)
        self.pin = None

    def _common(self, blob_dev, words, n):
        return (blob_dev.data_ptr(), words, n, self.n, self.filt_b, self.segs, self.slot_b, self.out_bytes)

    def _grey_ptr(self):
        return None if self.grey_dev is None else self.grey_dev.data_ptr()

    def to_host(self):
        """Queue the copy of the sizes (per page: the file's bytes or -1, the channels it is coded with) to pinned memory."""
        self.pin = to_pinned(self.scratch, "fl_pin_sizes", self.sizes, 2 * self.n)

    def answers(self) -> List[tuple]:
        """Per page (bytes or -1, channels) - once the stream has been waited for."""
        return [tuple(v) for v in self.pin[: 2 * self.n].view(-1, 2).tolist()]

    def start(self):
        """Rows and tables: the first phase, all a page over the budget costs."""
        lib, stream = _lib.load(), _lib.current_stream_ptr()
        common = self._common(self.blob_dev, self.blob.size, self.n)
        _lib.check(lib.ymk_flate_rows(*common, self.max_rows, self.max_row_segs, self._grey_ptr(), self.filt.data_ptr(), self.tokens.data_ptr(),
                                      self.segtok.data_ptr(), self.segadler.data_ptr(), self.hist.data_ptr(), stream), "ymk_flate_rows")
        _lib.check(lib.ymk_flate_tables(*common, self._grey_ptr(), self.hist.data_ptr(), self.segadler.data_ptr(), self.tables.data_ptr(),
                                        self.head.data_ptr(), self.sizes.data_ptr(), stream), "ymk_flate_tables")
        self.to_host()

    def finish(self, which: Sequence[int]):
        """Code, scan and gather the pages `which` of a started call."""
        if not which:
            return
        lib, stream = _lib.load(), _lib.current_stream_ptr()
        rec = self.blob.reshape(-1, PAGE_WORDS)[list(which)]
        blob = np.ascontiguousarray(rec).reshape(-1)
        common = self._common(imaging._stage_blob(blob, self.pages[0].device), blob.size, len(which))
        _lib.check(lib.ymk_flate_code(*common, self.max_rows, self.max_row_segs, self.tokens.data_ptr(), self.segtok.data_ptr(),
                                      self.tables.data_ptr(), self.head.data_ptr(), self.slots.data_ptr(), self.segbits.data_ptr(), stream), "ymk_flate_code")
        _lib.check(lib.ymk_flate_scan(*common, self.segbits.data_ptr(), self.head.data_ptr(), self.off.data_ptr(), self.sizes.data_ptr(), stream),
                   "ymk_flate_scan")
        _lib.check(lib.ymk_flate_gather(*common, self.slots.data_ptr(), self.head.data_ptr(), self.off.data_ptr(), self.out.data_ptr(),
                                        int(rec[:, 14].max()), stream), "ymk_flate_gather")
        self.to_host()

    def run(self):
        """All five phases in one call (ymk_flate_encode_pages): every page goes on."""
        _lib.check(_lib.load().ymk_flate_encode_pages(
            *self._common(self.blob_dev, self.blob.size, self.n), self.max_rows, self.max_row_segs, self._grey_ptr(), self.filt.data_ptr(),
            self.tokens.data_ptr(), self.segtok.data_ptr(), self.segadler.data_ptr(), self.segbits.data_ptr(), self.hist.data_ptr(),
            self.tables.data_ptr(), self.head.data_ptr(), self.off.data_ptr(), self.slots.data_ptr(), self.out.data_ptr(), self.largest,
            self.sizes.data_ptr(), _lib.current_stream_ptr()), "ymk_flate_encode_pages")
        self.to_host()


def launch(pages: Sequence[torch.Tensor], scratch: dict, budget256: Optional[int] = None, grey: bool = False,
           capacities: Optional[Sequence[int]] = None):
    """Launch the lossless coding of device pages (uint8 H x W x 3 or H x W, contiguous) on the current stream.  Without a budget:
    everything, and no wait.  With one: the first phase, ONE wait for the files' sizes, then the rest for the pages within it.
    -> (the _Coding, per page whether it goes on)."""
    coding = _Coding(pages, scratch, grey, capacities)
    if budget256 is None:
        coding.run()
        return coding, [True] * len(pages)
    coding.start()
    torch.cuda.current_stream().synchronize()
    keep = [size < 0 or within_budget(size, int(p.shape[0]), int(p.shape[1]), budget256) for p, (size, _) in zip(pages, coding.answers())]
    coding.finish([k for k, go in enumerate(keep) if go])
    return coding, keep


def lossless_entry(page: torch.Tensor, data: Optional[bytes], channels: int, k: int, capacity: Optional[int] = None):
    """A page's entry from its file's bytes; None (a size of -1) is a YmkError, as a JPEG page's."""
    if data is None:
        cap = file_capacity(*_shape(page)) if capacity is None else capacity
        return _lib.YmkError(f"page {k}: the lossless file does not fit its capacity of {cap} bytes")
    return EncodedLossless(data, int(page.shape[1]), int(page.shape[0]), int(channels), 1.0)


def encode_lossless_pages(pages: Sequence, stream=None, scratch: Optional[dict] = None,
                          budget: Optional[float] = None) -> List[Union[EncodedLossless, Exception]]:
    """One entry per page, in order: its EncodedLossless, or the exception that page raised - a ValueError for a page that is not
    uint8 H x W x 3 / H x W, and for a page whose file exceeds `budget` bytes a pixel (None: no budget; otherwise a positive finite
    number, as `check_lossless` takes it).  pages: device tensors and / or host arrays.  stream: the torch stream to launch on
    (default: the current one); scratch: a dict the caller keeps between calls to reuse the device and pinned buffers.  The file's
    capacity is `file_capacity`, which no file exceeds: a page cannot fail for room."""
    budget256 = None if budget is None else check_lossless({"budget": budget})["budget256"]
    scratch = {} if scratch is None else scratch
    with entered(pages, stream, "encode_lossless_pages needs") as (_, live, devs, out):
        if not live:
            return out
        coding, keep = launch(devs, scratch, budget256)
        torch.cuda.current_stream().synchronize()
        answers = coding.answers()
        datas = gather_files([(coding.out, coding.offsets[j], answers[j][0] if keep[j] else -1) for j in range(len(devs))], scratch, "fl_pin_bytes")
        for j, k in enumerate(live):
            if not keep[j]:
                out[k] = ValueError(f"page {k}: the lossless file of {answers[j][0]} bytes exceeds the budget of {budget} bytes a pixel")
            else:
                out[k] = lossless_entry(devs[j], datas[j], answers[j][1], k)
    return out
