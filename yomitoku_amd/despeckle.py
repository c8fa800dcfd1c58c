"""Despeckled pages: the specks and pinholes of a thresholded page removed on the device, between the threshold and the Group 4
coder.

    encode_g4_pages(pages, binarize="otsu", despeckle=True)              # EncodedBilevel.despeckled says what went
    encode_jpeg_pages(pages, "high", bilevel="adaptive", despeckle={"black": 4})
    analyzer.serve(sources, jpeg="high", jpeg_bilevel="otsu", jpeg_despeckle=True)
    clean, counts = despeckle_masks([mask], black=4, white=4)[0]         # the kernel alone: bool H x W in, bool H x W out

Paper grain, dust and sensor noise survive any threshold as isolated black specks and white pinholes, and T.6, which codes a row
against the row above, pays for each of them twice.  The rule (tests/despeckle_ref.py is the definition, which the device equals
bit for bit; yomitoku_amd/csrc/ymk_cc.hip; DESIGN.md, "Despeckled pages"):

  1. every 8-connected component of black pixels with fewer than `black` pixels becomes white;
  2. on the result, every 4-connected component of white pixels with fewer than `white` pixels becomes black.

0 leaves that colour alone.  A component that touches the page's edge is no exception.  The default is 4 for both: dust is 1 to 3
pixels, and the smallest marks of Japanese print are larger - dakuten, handakuten and the ring of the full stop at 10 pt and
300 dpi are around 20 pixels; on the clean golden page 4 moves 35 to 41 pixels, on a noisy one the file shrinks to a fifth.  It is
a default, not a claim about every scan.

On the device the work is connected-component labelling of packed bit rows: per colour a union-find over 64 x 16 tiles in LDS, a
lock-free merge across the tiles' seams, the components' areas, and the flip - four launches, no wait.  There is no host fallback.

Out: the masks of layered pages, the ink of the page-skew step, despeckling by shape rather than area, a choice of n per page.
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

DEFAULT = 4
MOST = 65535
KEYS = ("black", "white")


def check_despeckle(value=False) -> Optional[dict]:
    """`despeckle` of a call: False -> None; True -> {"black": 4, "white": 4}; an int n -> n for both; a dict with either of
    "black" and "white" or both -> those, a missing one 0.  Each value is an int in 0..65535: the size below which a component of
    that colour goes, 0 to leave the colour alone.  Both 0, an unknown key, another type or a value out of range is a ValueError.
    4 is the default because dust is 1 to 3 pixels and the smallest marks of print are several times that (the module's
    docstring): a default, not a claim about every scan."""
    if value is False:
        return None
    if value is True:
        return {"black": DEFAULT, "white": DEFAULT}
    if isinstance(value, int):
        out = {"black": value, "white": value}
    elif isinstance(value, dict) and all(k in KEYS for k in value):
        out = {k: value.get(k, 0) for k in KEYS}
    else:
        raise ValueError(f"unknown jpeg despeckle {value!r}: False, True, an int or a dict with any of {list(KEYS)}")
    for key, n in out.items():
        if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= MOST:
            raise ValueError(f"jpeg despeckle[{key!r}] is an int in 0..{MOST}, got {n!r}")
    if not any(out.values()):
        raise ValueError(f"jpeg despeckle {value!r} removes nothing: black or white is at least 1")
    return {k: int(n) for k, n in out.items()}


@dataclass(frozen=True)
class Despeckled:
    """What despeckling did to one page: the two sizes it ran with, and the components and pixels of each colour that went."""

    black: int
    white: int
    black_components: int
    black_pixels: int
    white_components: int
    white_pixels: int


def tile() -> tuple:
    """(width, height) of the labelling kernel's tile: YMK_CC_TILE_W x YMK_CC_TILE_H."""
    from . import _lib

    lib = _lib.load()
    return int(lib.ymk_cc_tile_w()), int(lib.ymk_cc_tile_h())


def scratch_sizes(shapes: Sequence) -> tuple:
    """(bytes of the labels, bytes of the areas) of pages of `shapes` = (h, w, ...): 4 bytes a pixel each."""
    from . import _lib
    from .devpages import shape_args

    sizes = (ctypes.c_int64 * 2)()
    _lib.check(_lib.load().ymk_cc_scratch_bytes(*shape_args(shapes), len(shapes), sizes), "ymk_cc_scratch_bytes")
    return tuple(int(v) for v in sizes)


def page_table(shapes: Sequence, packed_at: Sequence[int]) -> np.ndarray:
    """int32 [n][16]: the Group 4 page table of include/ymk.h as ymk_cc_despeckle_pages reads it - h, w, the packed rows at
    `packed_at`, the labels and areas one page behind the other."""
    from .ccitt import PAGE_WORDS
    from .devpages import addr_words

    rec = np.zeros((len(shapes), PAGE_WORDS), np.int32)
    at = 0
    for k, (h, w) in enumerate(shapes):
        rec[k, 2:5] = (h, w, 1)
        rec[k, 6:8] = addr_words(int(packed_at[k]))
        rec[k, 14:16] = addr_words(at)
        at += h * w
    return rec


def launch(test, which: Sequence[int], params: dict, scratch: dict, edit_table=None, buffers=None):
    """Queue the despeckling of the pages `which` of a finished ccitt._Test / _Binarized (or anything with its `pages`, `packed`,
    `packed_at`, `packed_bytes`) on the current stream, in place in `test.packed` (ymk_cc_despeckle_pages).  Waits for nothing.
    -> the counts on the device, int32 [len(which)][4]: black components, black pixels, white components, white pixels.
    params: check_despeckle's dict.  scratch: the labels and areas are keys of their own ("cc_labels", "cc_areas").
    edit_table: a function that may change the int32 [n][16] page table before it is staged (the tests' malformed record);
    buffers: (labels, areas), the tests' poisoned ones, in place of scratch's."""
    import torch

    from . import _lib, imaging
    from .devpages import grown

    shapes = [(int(test.pages[j].shape[0]), int(test.pages[j].shape[1])) for j in which]
    device, n = test.packed.device, len(shapes)
    blob = page_table(shapes, [test.packed_at[j] for j in which])
    if edit_table is not None:
        edit_table(blob)
    label_b, area_b = scratch_sizes(shapes)
    if buffers is None:
        buffers = grown(scratch, "cc_labels", label_b // 4, torch.int32, device), grown(scratch, "cc_areas", area_b // 4, torch.int32, device)
    labels, areas = buffers
    counts = grown(scratch, "cc_counts", 4 * n, torch.int32, device)
    blob_dev = imaging._stage_blob(blob.reshape(-1), device)
    _lib.check(_lib.load().ymk_cc_despeckle_pages(blob_dev.data_ptr(), blob.size, n, max(h for h, _ in shapes),
                                                  max(w for _, w in shapes), test.packed.data_ptr(), test.packed_bytes, labels.data_ptr(),
                                                  label_b, areas.data_ptr(), area_b, int(params["black"]), int(params["white"]), counts.data_ptr(),
                                                  _lib.current_stream_ptr()), "ymk_cc_despeckle_pages")
    return counts


def result(params: dict, four: Sequence[int]) -> Despeckled:
    """The Despeckled of one page from its four counts."""
    return Despeckled(int(params["black"]), int(params["white"]), *[int(v) for v in four])


class _Masks:
    """What `launch` reads of a test: the masks as the pages (their shapes), their packed rows one page behind the other."""

    def __init__(self, masks, device):
        import torch

        from .mrc import pack_mask

        rows = [pack_mask(m, device) for m in masks]
        at = np.cumsum([0] + [r.numel() for r in rows]).tolist()
        self.pages, self.packed_at = list(masks), at[:-1]
        self.packed = torch.cat([r.reshape(-1) for r in rows] + [torch.zeros(at[-1] % 2, dtype=torch.int32, device=device)])
        self.packed_bytes = self.packed.numel() * 4

    def rows(self, j: int):
        """The packed rows of mask j, int32 [h][ceil(w / 32)]: a view of `packed`."""
        h, rw = int(self.pages[j].shape[0]), -(-int(self.pages[j].shape[1]) // 32)
        return self.packed[self.packed_at[j] : self.packed_at[j] + h * rw].view(h, rw)


def unpack_rows(rows, w: int):
    """int32 [h][ceil(w / 32)] packed rows (the leftmost pixel of a word in bit 31) -> bool [h][w], on the rows' device."""
    import torch

    shifts = torch.arange(31, -1, -1, dtype=torch.int64, device=rows.device)
    bits = (rows.to(torch.int64).unsqueeze(-1) >> shifts) & 1
    return bits.reshape(rows.shape[0], -1)[:, :w].to(torch.bool)


def despeckle_masks(masks: Sequence, black: int = DEFAULT, white: int = DEFAULT, stream=None, scratch: Optional[dict] = None) -> list:
    """One entry per mask, in order: (the clean mask, a bool H x W device tensor; its Despeckled) - or the ValueError of a mask
    that is not 2-D bool or whose side is not in 1..16383.  masks: bool H x W arrays or tensors, True = black.  black, white: the
    sizes, as check_despeckle's dict has them.  stream: the torch stream to launch on (default: the current one); scratch: a dict
    the caller keeps between calls.  One wait, for the counts."""
    import torch

    from . import _lib
    from .devpages import MAX_SIDE, to_pinned

    params = check_despeckle({"black": black, "white": white})
    out: list = [None] * len(masks)
    live = []
    masks = [m if isinstance(m, torch.Tensor) else np.asarray(m) for m in masks]
    for k, m in enumerate(masks):
        shape, dtype = tuple(m.shape), m.dtype
        if dtype not in (torch.bool, np.dtype(bool)) or len(shape) != 2:
            out[k] = ValueError(f"a mask is bool H x W, got {dtype} {shape}")
        elif min(shape) < 1 or max(shape) > MAX_SIDE:
            out[k] = ValueError(f"a mask has 1..{MAX_SIDE} pixels on a side, got {shape}")
        else:
            live.append(k)
    if not live:
        return out
    if not torch.cuda.is_available():
        raise _lib.YmkError("despeckle_masks needs a HIP device (there is no host fallback)")
    device = next((masks[k].device for k in live if isinstance(masks[k], torch.Tensor) and masks[k].device.type == "cuda"),
                  torch.device("cuda", torch.cuda.current_device()))
    scratch = {} if scratch is None else scratch
    with torch.cuda.device(device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(device)):
        test = _Masks([masks[k] for k in live], device)
        counts = launch(test, list(range(len(live))), params, scratch)
        pin = to_pinned(scratch, "cc_pin_counts", counts, 4 * len(live))
        torch.cuda.current_stream().synchronize()
        four = pin[: 4 * len(live)].view(-1, 4).tolist()
        for j, k in enumerate(live):
            out[k] = (unpack_rows(test.rows(j), int(masks[k].shape[1])), result(params, four[j]))
    return out
