"""CCITT Group 4 (ITU-T T.6) files of two-valued pages that are already on the device: what a searchable PDF embeds as a
`/CCITTFaxDecode` image (utils/searchable_pdf.py) - lossless, and a fraction of the JPEG's bytes on a 1-bit scan.

    encoded = encode_g4_pages(pages)                      # device tensors or host arrays, uint8 H x W x 3 (B G R) or H x W
    encode_jpeg_pages(pages, "high", bilevel="auto")      # the two-valued pages as EncodedBilevel, the others as EncodedJpeg
    encode_g4_pages(pages, binarize="otsu")               # grey-valued pages, thresholded on the device ("otsu" | "adaptive")
    encode_jpeg_pages(pages, "high", bilevel="adaptive")  # the grey-valued pages as EncodedBilevel, the others as EncodedJpeg

A page is two-valued when every sample is 0 or 255 and, of three channels, B == G == R everywhere; a sample of 0 is black.  That
is tested on the device (no thresholding: the path is lossless by construction), in the launch that also packs the page's rows
to bits; then every row of every such page is coded against the row above by a thread of its own, the rows' bit counts are
summed per page, and every 32-bit word of every file is gathered from the rows' codes (yomitoku_amd/csrc/ymk_ccitt.hip;
DESIGN.md, "Two-valued pages").  The definition is tests/ccitt_ref.py, which is held to libtiff's Group 4 strips.  The host sees
the pages' flags, the files' lengths and their bytes, through pinned memory.  There is no host fallback.

Thresholded pages (`binarize=` / `bilevel=` "otsu" or "adaptive"; DESIGN.md, "Thresholded pages").  What people scan is grey-valued:
paper noise, soft edges, a gradient of light.  The caller may ask, per job, that every grey-valued page - one channel, or three
with B == G == R everywhere - be turned into bits on the device and coded as Group 4: by one threshold per page (Otsu's, from the
page's histogram) or by a locally adaptive one (Bradley-Roth: black where a pixel is 15 % below the mean of its window, from a
summed-area table).  Both are integer definitions, tests/binarize_ref.py, which the device equals bit for bit
(yomitoku_amd/csrc/ymk_binarize.hip); the row coder, the scan and the gather behind them are those of the two-valued path.  A
grey PHOTOGRAPH is binarised too: the switch is the caller's decision about a job, not a guess about a page.  On a two-valued
page both give exactly the file of "auto".
"""

from __future__ import annotations

import ctypes
import struct
from dataclasses import InitVar, dataclass
from typing import ClassVar, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib, imaging
from .devpages import PACKED_ROWS, SUMMED_AREA, addr_words, entered, gather_files, grown, shape_args, to_pinned

PAGE_WORDS = 16  # YMK_G4_PAGE_WORDS


@dataclass
class EncodedBilevel:
    """One two-valued page as a raw T.6 stream: the codes MSB first in each byte, rows not byte-aligned, EOFB at the end,
    zero-padded to a byte; 0 bits of the decoded image are white (`BlackIs1 false`, TIFF's MinIsWhite).  `scale` is 1.0: a
    two-valued page is never resized.  `method`: "auto" for a page that arrived two-valued, "otsu" / "adaptive" for one that was
    thresholded; `threshold`: Otsu's t* (black iff p <= t*), None for the other two; `despeckled`: what despeckling removed
    before the page was coded (yomitoku_amd/despeckle.py: Despeckled; of a layered page's mask whose ink was filtered, an
    InkFiltered), None where it did not run.  It is the constructor's last
    argument and an attribute, not a dataclass field: `==` and `repr` ignore it, `dataclasses.fields()` does not list it, and
    `dataclasses.replace()` gives a copy whose `despeckled` is None unless it is passed again."""

    data: bytes
    width: int
    height: int
    scale: float = 1.0
    method: str = "auto"
    threshold: Optional[int] = None
    bilevel: ClassVar[bool] = True  # what utils/searchable_pdf.py recognises the object by
    # the last argument, kept as an attribute and not among dataclasses.fields(): an entry's fields, its equality and its recorded
    # form (tools/record_page_files_golden.py) are those of an entry made before there was despeckling
    despeckled: InitVar[Optional["Despeckled"]] = None  # noqa: F821 - yomitoku_amd/despeckle.py

    def __post_init__(self, despeckled=None):
        self.despeckled = despeckled

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


BILEVEL_MODES = ("auto", "otsu", "adaptive")
BINARIZE_MODES = BILEVEL_MODES[1:]  # the two that threshold


def check_bilevel(bilevel=False) -> bool:
    """Whether pages get Group 4 files - the two-valued ones ("auto"), or every grey-valued one, thresholded ("otsu",
    "adaptive"); a `bilevel` that is neither False nor one of the three is a ValueError."""
    if bilevel is not False and not (isinstance(bilevel, str) and bilevel in BILEVEL_MODES):
        raise ValueError(f"unknown jpeg bilevel {bilevel!r}: False, 'auto', 'otsu' or 'adaptive'")
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
    sizes = (ctypes.c_int64 * 5)()
    _lib.check(_lib.load().ymk_g4_scratch_bytes(*shape_args(shapes), len(shapes), sizes), "ymk_g4_scratch_bytes")
    return tuple(int(v) for v in sizes)


def page_table(pages: Sequence[torch.Tensor], packed_at: Optional[Sequence[int]] = None, capacities: Optional[Sequence[int]] = None,
               tables: bool = False):
    """(int32 words of the page table of include/ymk.h, per page the word offset of its packed rows, per page the byte offset of
    its file in the output, the output's bytes).  packed_at: where the pages' packed rows are (default: one page behind the
    other); capacities: bytes per page's file (default: `file_capacity`, which no file exceeds); tables: words 14-15 say where
    the page's summed-area table is (the binariser's, one page behind the other) - zeros without."""
    lib = _lib.load()
    rec = np.zeros((len(pages), PAGE_WORDS), np.int32)
    row = pack = slot = out_at = sat = 0
    packs, offsets = [], []
    for k, p in enumerate(pages):
        h, w = int(p.shape[0]), int(p.shape[1])
        at = pack if packed_at is None else int(packed_at[k])
        cap = file_capacity(h, w) if capacities is None else int(capacities[k])
        rec[k, 0:2] = addr_words(p.data_ptr())
        rec[k, 2:6] = (h, w, 1 if p.dim() == 2 else 3, row)
        rec[k, 6:8] = addr_words(at)
        rec[k, 8:10] = addr_words(out_at)
        rec[k, 10] = cap
        rec[k, 11:13] = addr_words(slot)
        if tables:
            rec[k, 14:16] = addr_words(sat)
            sat += h * w
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
    packed = grown(scratch, PACKED_ROWS, packed_bytes // 4, torch.int32, device)
    flags = grown(scratch, "g4_flags", len(pages), torch.int32, device)
    blob_dev = imaging._stage_blob(blob, device)
    _lib.check(_lib.load().ymk_g4_test_pack(blob_dev.data_ptr(), blob.size, len(pages), max(int(p.shape[0]) * int(p.shape[1]) for p in pages),
                                            flags.data_ptr(), packed.data_ptr(), packed_bytes, _lib.current_stream_ptr()), "ymk_g4_test_pack")
    return _Test(list(pages), packed, packed_at, packed_bytes, to_pinned(scratch, "g4_pin_flags", flags, len(pages)))


class _Binarized(_Test):
    """The launches that threshold a call's pages: as _Test, with `answers` saying which pages are grey-valued, and Otsu's
    thresholds behind the flags in the same pinned buffer."""

    method = "auto"

    def flags(self) -> List[int]:
        return self.pin[: len(self.pages)].tolist()

    def thresholds(self) -> List[Optional[int]]:
        """Per page Otsu's t* (None under "adaptive") - once the stream has been waited for."""
        n = len(self.pages)
        return self.pin[n : 2 * n].tolist() if self.method == "otsu" else [None] * n


def binarize_scratch_sizes(shapes: Sequence) -> tuple:
    """(bytes of the histograms, bytes of the summed-area tables) of pages of `shapes` = (h, w, ...)."""
    sizes = (ctypes.c_int64 * 2)()
    _lib.check(_lib.load().ymk_bin_scratch_bytes(*shape_args(shapes), len(shapes), sizes), "ymk_bin_scratch_bytes")
    return tuple(int(v) for v in sizes)


def start_binarize(pages: Sequence[torch.Tensor], scratch: dict, method: str) -> _Binarized:
    """Launch the thresholding of device pages (uint8 H x W x 3 or H x W, contiguous) on the current stream - the stage-level
    entry, as `start_test` is for "auto": the grey test (with the histograms under "otsu": ymk_bin_test_hist), then
    ymk_bin_otsu + ymk_bin_otsu_pack or ymk_bin_adaptive_pack, then the copy of the flags and thresholds to pinned memory.
    Waits for nothing.  After a wait: `.answers()` / `.flags()` (0 grey-valued, 1 not), `.thresholds()`, and `.packed`, the
    pages' packed rows at the word offsets `.packed_at` - of every page, whatever its flag."""
    if method not in BINARIZE_MODES:
        raise ValueError(f"unknown bilevel method {method!r}: 'otsu' or 'adaptive'")
    lib, device, n = _lib.load(), pages[0].device, len(pages)
    blob, packed_at, _, _ = page_table(pages, capacities=[0] * n, tables=method == "adaptive")
    shapes = [p.shape for p in pages]
    packed_bytes = scratch_sizes(shapes)[1]
    hist_bytes, sat_bytes = binarize_scratch_sizes(shapes)
    packed = grown(scratch, PACKED_ROWS, packed_bytes // 4, torch.int32, device)
    answer = grown(scratch, "bin_answer", 2 * n, torch.int32, device)  # the flags, then the thresholds: one copy
    blob_dev = imaging._stage_blob(blob, device)
    stream = _lib.current_stream_ptr()
    most = max(int(p.shape[0]) * int(p.shape[1]) for p in pages)
    if method == "otsu":
        hist = grown(scratch, "bin_hist", hist_bytes // 4, torch.int32, device)
        _lib.check(lib.ymk_bin_test_hist(blob_dev.data_ptr(), blob.size, n, most, answer.data_ptr(), hist.data_ptr(), stream), "ymk_bin_test_hist")
        thresholds = answer.data_ptr() + 4 * n
        _lib.check(lib.ymk_bin_otsu(n, hist.data_ptr(), thresholds, stream), "ymk_bin_otsu")
        _lib.check(lib.ymk_bin_otsu_pack(blob_dev.data_ptr(), blob.size, n, most, thresholds, packed.data_ptr(), packed_bytes, stream),
                   "ymk_bin_otsu_pack")
    else:
        sat = grown(scratch, SUMMED_AREA, sat_bytes // 4, torch.int32, device)
        _lib.check(lib.ymk_bin_test_hist(blob_dev.data_ptr(), blob.size, n, most, answer.data_ptr(), None, stream), "ymk_bin_test_hist")
        _lib.check(lib.ymk_bin_adaptive_pack(blob_dev.data_ptr(), blob.size, n, max(int(p.shape[0]) for p in pages),
                                             max(int(p.shape[1]) for p in pages), sat.data_ptr(), sat_bytes, packed.data_ptr(), packed_bytes,
                                             stream), "ymk_bin_adaptive_pack")
    pin = to_pinned(scratch, "bin_pin_answer", answer, 2 * n if method == "otsu" else n, room=2 * n)
    res = _Binarized(list(pages), packed, packed_at, packed_bytes, pin)
    res.method = method
    return res


def launch_encode(test: _Test, which: Sequence[int], scratch: dict, capacities: Optional[Sequence[int]] = None):
    """Launch the coding of the pages `which` of a finished test on the current stream (ymk_g4_encode_pages: rows, scan,
    concatenate).  -> (the buffer of the files, per page its byte offset there, the files' lengths on the device)."""
    pages = [test.pages[j] for j in which]
    device = pages[0].device
    blob, _, offsets, out_bytes = page_table(pages, [test.packed_at[j] for j in which], capacities)
    rows, _, slot_b, bits_b, off_b = scratch_sizes([p.shape for p in pages])
    slots = grown(scratch, "g4_slots", slot_b // 4, torch.int32, device)
    rowbits = grown(scratch, "g4_rowbits", bits_b // 4, torch.int32, device)
    rowoff = grown(scratch, "g4_rowoff", off_b // 8, torch.int64, device)
    files = grown(scratch, "g4_out", out_bytes, torch.uint8, device)
    lengths = grown(scratch, "g4_lengths", len(pages), torch.int32, device)
    blob_dev = imaging._stage_blob(blob, device)
    tallest, largest = max(int(p.shape[0]) for p in pages), int(blob.reshape(-1, PAGE_WORDS)[:, 10].max())
    _lib.check(_lib.load().ymk_g4_encode_pages(blob_dev.data_ptr(), blob.size, len(pages), rows, tallest, test.packed.data_ptr(), test.packed_bytes,
                                               slots.data_ptr(), slot_b, rowbits.data_ptr(), rowoff.data_ptr(), files.data_ptr(), out_bytes, largest,
                                               lengths.data_ptr(), _lib.current_stream_ptr()), "ymk_g4_encode_pages")
    return files, offsets, lengths


def encode_g4_pages(pages: Sequence, stream=None, scratch: Optional[dict] = None,
                    binarize: Optional[str] = None, despeckle=False) -> List[Union[EncodedBilevel, Exception]]:
    """One entry per page, in order: its EncodedBilevel, or the exception that page raised - a ValueError for a page that is not
    uint8 H x W x 3 / H x W, or not two-valued.  pages: device tensors and / or host arrays.  stream: the torch stream to launch
    on (default: the current one); scratch: a dict the caller keeps between calls to reuse the device and pinned buffers.  The
    file's capacity is `file_capacity`, which no file exceeds: a two-valued page cannot fail for room.
    binarize: None, or "otsu" / "adaptive" - every grey-valued page (one channel, or B == G == R everywhere) is thresholded on
    the device and coded; a page that is not grey-valued gets a ValueError entry.
    despeckle: False, True, an int or {"black": n, "white": n} (yomitoku_amd/despeckle.py: check_despeckle) - the specks and
    pinholes below that size are removed from every page's bits on the device before they are coded, and the entry's
    `despeckled` says how many; anything else is a ValueError before any device work.  With it a two-valued page's file is no
    longer lossless."""
    from . import despeckle as specks

    clean = specks.check_despeckle(despeckle)
    if binarize is not None and not (isinstance(binarize, str) and binarize in BINARIZE_MODES):
        raise ValueError(f"unknown bilevel method {binarize!r}: None, 'otsu' or 'adaptive'")
    scratch = {} if scratch is None else scratch
    with entered(pages, stream, "encode_g4_pages needs") as (_, live, devs, out):
        if not live:
            return out
        # sort: the test, or the launches that threshold, and one wait for the pages' flags
        test = start_test(devs, scratch) if binarize is None else start_binarize(devs, scratch, binarize)
        torch.cuda.current_stream().synchronize()
        two = test.answers()
        thresholds = test.thresholds() if binarize is not None else [None] * len(devs)
        for j, k in enumerate(live):
            if not two[j] and binarize is None:
                out[k] = ValueError(f"page {k} is not two-valued: a sample that is neither 0 nor 255, or a pixel with B != G or G != R")
            elif not two[j]:
                out[k] = ValueError(f"page {k} is not grey-valued: a pixel with B != G or G != R (bilevel {binarize!r} takes no colour page)")
        which = [j for j in range(len(devs)) if two[j]]
        if not which:
            return out
        # despeckle the pages that qualify in place; launch Group 4; then one wait, one gather, the entries
        if clean is not None:
            pin_cc = to_pinned(scratch, "cc_pin_counts", specks.launch(test, which, clean, scratch), 4 * len(which))
        files, offsets, lengths = launch_encode(test, which, scratch)
        pin_len = to_pinned(scratch, "g4_pin_lengths", lengths, len(which))
        torch.cuda.current_stream().synchronize()
        sizes = pin_len[: len(which)].tolist()
        went = [None] * len(which) if clean is None else [specks.result(clean, four) for four in pin_cc[: 4 * len(which)].view(-1, 4).tolist()]
        for i, (j, data) in enumerate(zip(which, gather_files([(files, offsets[i], sizes[i]) for i in range(len(which))], scratch, "g4_pin_bytes"))):
            out[live[j]] = bilevel_entry(devs[j], data, live[j], binarize or "auto", thresholds[j], went[i])
    return out


def bilevel_entry(page: torch.Tensor, data: Optional[bytes], k: int, method: str = "auto", threshold: Optional[int] = None, despeckled=None):
    """A page's entry from its file's bytes; None (a length of -1: by the slot bound that cannot be) is a YmkError."""
    if data is None:
        return _lib.YmkError(f"page {k}: the Group 4 file does not fit its capacity")
    return EncodedBilevel(data, int(page.shape[1]), int(page.shape[0]), 1.0, method, threshold, despeckled)

