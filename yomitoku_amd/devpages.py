"""What the page-file modules (jpeg.py, ccitt.py, mrc.py, deskew.py, despeckle.py) share: how a call's pages get onto the device, the scratch
buffers a caller keeps between calls, and the way an answer or the files' bytes reach the host - through pinned memory, behind
one wait."""

from __future__ import annotations

import contextlib
import ctypes
from typing import Callable, Optional, Sequence

import numpy as np
import torch

from . import _lib

MAX_SIDE = 16383

# The scratch keys that more than one module uses.  A scratch dict belongs to one stream at a time (serve: one per wave slot,
# used by the render thread; the page-skew step: one, on the copy stream), so the steps that share a buffer are serialised:
#   PACKED_ROWS  the pages' rows as bits.  Written by ccitt.start_test / start_binarize, by mrc.launch (the ink - under `bilevel`
#                into the test's own buffer, behind its wait) and by deskew.launch; rewritten in place by despeckle.launch (whose
#                labels and areas are keys of its own); read by ccitt.launch_encode.
#   SUMMED_AREA  the "adaptive" rule's summed-area tables.  Written and read inside ccitt.start_binarize, mrc.launch and
#                deskew.launch, each done with it before the next launch of the stream starts.
#   LUMA_PLANE   the luminance planes of colour pages.  Written and read inside mrc.launch and deskew.launch, likewise.
PACKED_ROWS, SUMMED_AREA, LUMA_PLANE = "g4_packed", "bin_sat", "dsk_luma"


def grown(scratch: dict, key: str, count: int, dtype, device=None, pinned=False) -> torch.Tensor:
    """scratch[key] with room for `count` elements: kept between calls, replaced (never resized) when it is too small."""
    t = scratch.get(key)
    if t is None or t.numel() < count or (not pinned and t.device != device):
        count = max(int(count * 1.25), 1024)
        t = torch.empty(count, dtype=dtype, pin_memory=True) if pinned else torch.empty(count, dtype=dtype, device=device)
        scratch[key] = t
    return t


def to_pinned(scratch: dict, key: str, dev: torch.Tensor, count: int, room: Optional[int] = None) -> torch.Tensor:
    """Queue the copy of the first `count` elements of `dev` to scratch[key], a pinned buffer with room for `room` (default
    `count`), on the current stream; waits for nothing.  -> the pinned buffer."""
    pin = grown(scratch, key, count if room is None else room, dev.dtype, pinned=True)
    pin[:count].copy_(dev[:count], non_blocking=True)
    return pin


def addr_words(ptr: int):
    return np.array([ptr & 0xFFFFFFFF, ptr >> 32], dtype=np.uint32).view(np.int32)


def shape_args(shapes: Sequence, channels: bool = False) -> list:
    """[heights, widths] - channels: and the channel counts - of `shapes` = (h, w) or (h, w, channels) as the int arrays the
    library's *_scratch_bytes entries take."""
    arr = ctypes.c_int * max(1, len(shapes))
    cols = [arr(*[int(s[0]) for s in shapes]), arr(*[int(s[1]) for s in shapes])]
    if channels:
        cols.append(arr(*[1 if len(s) == 2 else int(s[2]) for s in shapes]))
    return cols


def as_device_page(page, device) -> torch.Tensor:
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


@contextlib.contextmanager
def entered(pages: Sequence, stream, what: str, check: Optional[Callable] = None):
    """The start of every entry that takes a call's pages: -> (device, live, devs, out) with the device of the first device page
    (default: the current one) and `stream` (default: that device's current one) current inside the block.  `devs`: the pages
    that are pages, as contiguous device tensors; `live`: their indices in the call; `out`: one slot per page of the call, the
    exception of a page that is none - or that `check(k, page, dev)` raised for - already in its place.  No pages: (None, [],
    [], []) and no device is asked for.  Pages and no HIP device: a YmkError that starts with `what`."""
    out: list = [None] * len(pages)
    if not pages:
        yield None, [], [], out
        return
    if not torch.cuda.is_available():
        raise _lib.YmkError(f"{what} a HIP device (there is no host fallback)")
    device = next((p.device for p in pages if isinstance(p, torch.Tensor) and p.device.type == "cuda"),
                  torch.device("cuda", torch.cuda.current_device()))
    with torch.cuda.device(device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(device)):
        live, devs = [], []
        for k, page in enumerate(pages):
            try:
                dev = as_device_page(page, device)
                if check is not None:
                    check(k, page, dev)
                devs.append(dev)
                live.append(k)
            except Exception as exc:  # noqa: BLE001 - only this page fails
                out[k] = exc
        yield device, live, devs, out


def gather_files(parts: Sequence, scratch: dict, key: str = "pin_bytes") -> list:
    """parts: (device buffer, byte offset, length or -1) per file -> their bytes (None for -1): packed on the device, then one
    copy through pinned memory and one wait."""
    good = [(buf, at, n) for buf, at, n in parts if n >= 0]
    total = sum(n for _, _, n in good)
    host = None
    if total:
        pin = to_pinned(scratch, key, torch.cat([buf[at : at + n] for buf, at, n in good]), total)
        torch.cuda.current_stream().synchronize()
        host = pin[:total].numpy()
    out, at = [], 0
    for _, _, n in parts:
        out.append(None if n < 0 else host[at : at + n].tobytes())
        at += max(n, 0)
    return out
