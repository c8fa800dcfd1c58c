"""CCITT Group 4 (ITU-T T.6) files of two-valued pages that are already on the device: what a searchable PDF embeds as a
`/CCITTFaxDecode` image (utils/searchable_pdf.py) - lossless, and a fraction of the JPEG's bytes on a 1-bit scan.

    encoded = encode_g4_pages(pages)                      # device tensors or host arrays, uint8 H x W x 3 (B G R) or H x W
    encode_jpeg_pages(pages, "high", bilevel="auto")      # the two-valued pages as EncodedBilevel, the others as EncodedJpeg

A page is two-valued when every sample is 0 or 255 and, of three channels, B == G == R everywhere; a sample of 0 is black.  That
is tested on the device (no thresholding: the path is lossless by construction), in the launch that also packs the page's rows
to bits; then every row of every such page is coded against the row above by a thread of its own, the rows' bit counts are
summed per page, and every 32-bit word of every file is gathered from the rows' codes (yomitoku_amd/csrc/ymk_ccitt.hip;
DESIGN.md, "Two-valued pages").  The definition is tests/ccitt_ref.py, which is held to libtiff's Group 4 strips.  The host sees
the pages' flags, the files' lengths and their bytes, through pinned memory.  There is no host fallback.
"""

from __future__ import annotations

import ctypes
import struct
from dataclasses import dataclass
from typing import ClassVar, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib, imaging
from .jpeg import _addr_words, _as_device_page, _gather_files, _grown

PAGE_WORDS = 16  # YMK_G4_PAGE_WORDS


@dataclass
class EncodedBilevel:
    """One two-valued page as a raw T.6 stream: the codes MSB first in each byte, rows not byte-aligned, EOFB at the end,
    zero-padded to a byte; 0 bits of the decoded image are white (`BlackIs1 false`, TIFF's MinIsWhite).  `scale` is 1.0: a
    two-valued page is never resized."""

    data: bytes
    width: int
    height: int
    scale: float = 1.0
    bilevel: ClassVar[bool] = True  # what utils/searchable_pdf.py recognises the object by

    def to_tiff(self) -> bytes:
        """A minimal little-endian TIFF with the stream as its single Group 4 strip."""
        tags = [(256, 4, self.width), (257, 4, self.height), (258, 3, 1), (259, 3, 4), (262, 3, 0), (273, 4, None), (277, 3, 1),
                (278, 4, self.height), (279, 4, len(self.data)), (293, 4, 0)]
        at = 8 + 2 + 12 * len(tags) + 4  # header, count, entries, next-IFD offset: where the strip starts
        out = [struct.pack("<2sHIH", b"II", 42, 8, len(tags))]
        for tag, kind, value in tags:
            value = at if value is None else value
            out.append(struct.pack("<HHII" if kind == 4 else "<HHIHH", tag, kind, 1, *((value,) if kind == 4 else (value, 0))))
        return b"".join(out) + struct.pack("<I", 0) + bytes(self.data)


def check_bilevel(bilevel=False) -> bool:
    """Whether two-valued pages get Group 4 files; a `bilevel` that is neither False nor "auto" is a ValueError."""
    if bilevel is not False and not (isinstance(bilevel, str) and bilevel == "auto"):
        raise ValueError(f"unknown jpeg bilevel {bilevel!r}: False or 'auto'")
    return bilevel is not False


def file_capacity(h: int, w: int) -> int:
    """The bytes no Group 4 file of an h x w page exceeds (h rows of at most 7 w + 21 bits, EOFB, the pad)."""
    n = int(_lib.load().ymk_g4_file_capacity(int(h), int(w)))
    if n < 0:
        raise ValueError(f"a page has 1..16383 pixels on a side, got {(h, w)}")
    return n


def scratch_sizes(shapes: Sequence) -> tuple:
    """(rows, bytes of the packed rows, of the rows' slots, of their bit counts, of their bit offsets) of pages of `shapes` =
    (h, w, ...)."""
    n = len(shapes)
    arr = ctypes.c_int * max(1, n)
    sizes = (ctypes.c_int64 * 5)()
    _lib.check(_lib.load().ymk_g4_scratch_bytes(arr(*[int(s[0]) for s in shapes]), arr(*[int(s[1]) for s in shapes]), n, sizes),
               "ymk_g4_scratch_bytes")
    return tuple(int(v) for v in sizes)


def page_table(pages: Sequence[torch.Tensor], packed_at: Optional[Sequence[int]] = None, capacities: Optional[Sequence[int]] = None):
    """(int32 words of the page table of include/ymk.h, per page the word offset of its packed rows, per page the byte offset of
    its file in the output, the output's bytes).  packed_at: where the pages' packed rows are (default: one page behind the
    other); capacities: bytes per page's file (default: `file_capacity`, which no file exceeds)."""
    lib = _lib.load()
    rec = np.zeros((len(pages), PAGE_WORDS), np.int32)
    row = pack = slot = out_at = 0
    packs, offsets = [], []
    for k, p in enumerate(pages):
        h, w = int(p.shape[0]), int(p.shape[1])
        at = pack if packed_at is None else int(packed_at[k])
        cap = file_capacity(h, w) if capacities is None else int(capacities[k])
        rec[k, 0:2] = _addr_words(p.data_ptr())
        rec[k, 2:6] = (h, w, 1 if p.dim() == 2 else 3, row)
        rec[k, 6:8] = _addr_words(at)
        rec[k, 8:10] = _addr_words(out_at)
        rec[k, 10] = cap
        rec[k, 11:13] = _addr_words(slot)
        packs.append(at)
        offsets.append(out_at)
        row, pack, slot = row + h, pack + h * (-(-w // 32)), slot + h * int(lib.ymk_g4_slot_words(w))
        out_at += -(-cap // 16) * 16
    return rec.reshape(-1), packs, offsets, out_at


class _Test:
    """The test-and-pack launch of a call: the pages' packed rows on the device, their flags on the way to pinned memory."""

    def __init__(self, pages, packed, packed_at, packed_bytes, pin):
        self.pages, self.packed, self.packed_at, self.packed_bytes, self.pin = pages, packed, packed_at, packed_bytes, pin

    def answers(self) -> List[bool]:
        """Per page whether it is two-valued - once the stream the test was launched on has been waited for."""
        return [v == 0 for v in self.pin[: len(self.pages)].tolist()]


def start_test(pages: Sequence[torch.Tensor], scratch: dict) -> _Test:
    """Launch the test of device pages (uint8 H x W x 3 or H x W, contiguous) on the current stream - one launch over all of
    them, which also packs their rows (ymk_g4_test_pack) - and the copy of its flags to pinned memory.  Waits for nothing."""
    device = pages[0].device
    blob, packed_at, _, _ = page_table(pages, capacities=[0] * len(pages))
    packed_bytes = scratch_sizes([p.shape for p in pages])[1]
    packed = _grown(scratch, "g4_packed", packed_bytes // 4, torch.int32, device)
    flags = _grown(scratch, "g4_flags", len(pages), torch.int32, device)
    blob_dev = imaging._stage_blob(blob, device)
    _lib.check(_lib.load().ymk_g4_test_pack(blob_dev.data_ptr(), blob.size, len(pages), max(int(p.shape[0]) * int(p.shape[1]) for p in pages),
                                            flags.data_ptr(), packed.data_ptr(), packed_bytes, _lib.current_stream_ptr()), "ymk_g4_test_pack")
    pin = _grown(scratch, "g4_pin_flags", len(pages), torch.int32, pinned=True)
    pin[: len(pages)].copy_(flags[: len(pages)], non_blocking=True)
    return _Test(list(pages), packed, packed_at, packed_bytes, pin)


def launch_encode(test: _Test, which: Sequence[int], scratch: dict, capacities: Optional[Sequence[int]] = None):
    """Launch the coding of the pages `which` of a finished test on the current stream (ymk_g4_encode_pages: rows, scan,
    concatenate).  -> (the buffer of the files, per page its byte offset there, the files' lengths on the device)."""
    pages = [test.pages[j] for j in which]
    device = pages[0].device
    blob, _, offsets, out_bytes = page_table(pages, [test.packed_at[j] for j in which], capacities)
    rows, _, slot_b, bits_b, off_b = scratch_sizes([p.shape for p in pages])
    slots = _grown(scratch, "g4_slots", slot_b // 4, torch.int32, device)
    rowbits = _grown(scratch, "g4_rowbits", bits_b // 4, torch.int32, device)
    rowoff = _grown(scratch, "g4_rowoff", off_b // 8, torch.int64, device)
    files = _grown(scratch, "g4_out", out_bytes, torch.uint8, device)
    lengths = _grown(scratch, "g4_lengths", len(pages), torch.int32, device)
    blob_dev = imaging._stage_blob(blob, device)
    tallest, largest = max(int(p.shape[0]) for p in pages), int(blob.reshape(-1, PAGE_WORDS)[:, 10].max())
    _lib.check(_lib.load().ymk_g4_encode_pages(blob_dev.data_ptr(), blob.size, len(pages), rows, tallest, test.packed.data_ptr(), test.packed_bytes,
                                               slots.data_ptr(), slot_b, rowbits.data_ptr(), rowoff.data_ptr(), files.data_ptr(), out_bytes, largest,
                                               lengths.data_ptr(), _lib.current_stream_ptr()), "ymk_g4_encode_pages")
    return files, offsets, lengths


def encode_g4_pages(pages: Sequence, stream=None, scratch: Optional[dict] = None) -> List[Union[EncodedBilevel, Exception]]:
    """One entry per page, in order: its EncodedBilevel, or the exception that page raised - a ValueError for a page that is not
    uint8 H x W x 3 / H x W, or not two-valued.  pages: device tensors and / or host arrays.  stream: the torch stream to launch
    on (default: the current one); scratch: a dict the caller keeps between calls to reuse the device and pinned buffers.  The
    file's capacity is `file_capacity`, which no file exceeds: a two-valued page cannot fail for room."""
    out: list = [None] * len(pages)
    if not pages:
        return out
    if not torch.cuda.is_available():
        raise _lib.YmkError("encode_g4_pages needs a HIP device (there is no host fallback)")
    device = next((p.device for p in pages if isinstance(p, torch.Tensor) and p.device.type == "cuda"),
                  torch.device("cuda", torch.cuda.current_device()))
    scratch = {} if scratch is None else scratch
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
        test = start_test(devs, scratch)
        torch.cuda.current_stream().synchronize()
        two = test.answers()
        for j, k in enumerate(live):
            if not two[j]:
                out[k] = ValueError(f"page {k} is not two-valued: a sample that is neither 0 nor 255, or a pixel with B != G or G != R")
        which = [j for j in range(len(devs)) if two[j]]
        if not which:
            return out
        files, offsets, lengths = launch_encode(test, which, scratch)
        pin_len = _grown(scratch, "g4_pin_lengths", len(which), torch.int32, pinned=True)
        pin_len[: len(which)].copy_(lengths[: len(which)], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        sizes = pin_len[: len(which)].tolist()
        for (j, data) in zip(which, _gather_files([(files, offsets[i], sizes[i]) for i in range(len(which))], scratch, "g4_pin_bytes")):
            out[live[j]] = bilevel_entry(devs[j], data, live[j])
    return out


def bilevel_entry(page: torch.Tensor, data: Optional[bytes], k: int):
    """A page's entry from its file's bytes; None (a length of -1: by the slot bound that cannot be) is a YmkError."""
    if data is None:
        return _lib.YmkError(f"page {k}: the Group 4 file does not fit its capacity")
    return EncodedBilevel(data, int(page.shape[1]), int(page.shape[0]), 1.0)

