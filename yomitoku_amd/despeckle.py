"""Despeckled pages: the specks and pinholes of a thresholded page removed on the device, between the threshold and the Group 4
coder.

    encode_g4_pages(pages, binarize="otsu", despeckle=True)              # EncodedBilevel.despeckled says what went
    encode_jpeg_pages(pages, "high", bilevel="adaptive", despeckle={"black": 4})
    analyzer.serve(sources, jpeg="high", jpeg_bilevel="otsu", jpeg_despeckle=True)
    clean, counts = despeckle_masks([mask], black=4, white=4)[0]         # the kernel alone: bool H x W in, bool H x W out
    encode_jpeg_pages(pages, "high", mrc={"despeckle": True, "blobs": {"side": 48}})   # the ink masks of layered pages
    clean, filtered = filter_masks([mask], black=4, white=4, side=128, fill=64)[0]     # that filter alone

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

The ink masks of layered pages (yomitoku_amd/mrc.py: `mrc={"despeckle": ..., "blobs": ...}`) go through the same two steps and a
third, by shape (tests/ink_filter_ref.py is the definition; ymk_cc_filter_pages):

  3. on the result, every 8-connected black component whose bounding box is at least `side` pixels high and wide and which fills
     at least `fill` / 256 of that box becomes white.

That is the dark part of a picture, a solid patch, a photograph: as ink it would be a hard-edged mask over a colour averaged per
cell, as paper it is a picture in the background layer.  A frame or a table's grid is as large but fills little of its box; a glyph
is small.  The blob step is not offered for Group 4 pages: there it would delete content, not move it to another layer.  On the
device it is a third pass of four launches: label, merge, every component's exact area and box, the flip.

Out: the ink of the page-skew step, a choice of the parameters per page, picture regions taken from the layout model.
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


BLOB_DEFAULTS = {"side": 128, "fill": 64}
BLOB_SIDES = (2, 16383)
BLOB_FILLS = (1, 256)


def check_blobs(value=False) -> Optional[dict]:
    """`blobs` of a layered page's options: False -> None; True -> {"side": 128, "fill": 64}; a dict with either of "side" and
    "fill" or both -> the defaults with those.  `side`: an int in 2..16383, the pixels a component's bounding box has to reach in
    both directions; `fill`: an int in 1..256, the part of that box, in 256ths, that the component's pixels have to reach.  An
    unknown key, another type or a value out of range is a ValueError.
    128 pixels is a 31 pt glyph at 300 dpi: body text, headings and most display type stay below it whatever they fill.  A quarter
    of the box (64) is above any grid or frame and below any picture seen so far - the golden page's table grid fills 0.07 of its
    box, its clip art 0.39.  Defaults, not a claim about every scan."""
    if value is False:
        return None
    if value is True:
        return dict(BLOB_DEFAULTS)
    if not isinstance(value, dict) or any(k not in BLOB_DEFAULTS for k in value):
        raise ValueError(f"unknown jpeg mrc blobs {value!r}: False, True or a dict with any of {sorted(BLOB_DEFAULTS)}")
    out = dict(BLOB_DEFAULTS)
    for key, v in value.items():
        lo, hi = BLOB_SIDES if key == "side" else BLOB_FILLS
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f"jpeg mrc blobs[{key!r}] is an int in {lo}..{hi}, got {v!r}")
        out[key] = int(v)
    return out


@dataclass(frozen=True)
class Despeckled:
    """What despeckling did to one page: the two sizes it ran with, and the components and pixels of each colour that went."""

    black: int
    white: int
    black_components: int
    black_pixels: int
    white_components: int
    white_pixels: int


@dataclass(frozen=True)
class InkFiltered:
    """What the ink filter did to one mask: the four parameters it ran with (0 where a step was off), and the components and
    pixels that went in each of the three steps."""

    black: int
    white: int
    side: int
    fill: int
    black_components: int
    black_pixels: int
    white_components: int
    white_pixels: int
    blob_components: int
    blob_pixels: int


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


def filter_scratch_sizes(shapes: Sequence) -> tuple:
    """(bytes of the labels, of the areas, of the boxes) of pages of `shapes` = (h, w, ...): 4, 4 and 12 bytes a pixel."""
    from . import _lib
    from .devpages import shape_args

    sizes = (ctypes.c_int64 * 3)()
    _lib.check(_lib.load().ymk_cc_filter_scratch_bytes(*shape_args(shapes), len(shapes), sizes), "ymk_cc_filter_scratch_bytes")
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


def filter_params(speck: Optional[dict], blobs: Optional[dict]) -> dict:
    """check_despeckle's and check_blobs' dicts (None: that part is off) as the four numbers of ymk_cc_filter_pages."""
    speck, blobs = speck or {"black": 0, "white": 0}, blobs or {"side": 0, "fill": 0}
    return {"black": int(speck["black"]), "white": int(speck["white"]), "side": int(blobs["side"]), "fill": int(blobs["fill"])}


def launch_filter(test, which: Sequence[int], params: dict, scratch: dict, edit_table=None, buffers=None, counts=None):
    """`launch` for the ink filter (ymk_cc_filter_pages): the two passes and the blob pass on the pages `which` of `test`, in place
    in `test.packed`, on the current stream.  Waits for nothing.  -> the counts on the device, int32 [len(which)][6]: black
    components, black pixels, white components, white pixels, blob components, blob pixels.  params: filter_params' dict.
    scratch: the boxes are a key of their own ("cc_boxes"), 12 bytes a pixel, and not touched where `side` is 0.  edit_table: as
    `launch`; buffers: (labels, areas, boxes); counts: a caller's int32 device tensor of 6 len(which) words in place of scratch's
    (mrc.launch: behind its flags, so that one copy takes both to the host)."""
    import torch

    from . import _lib, imaging
    from .devpages import grown

    shapes = [(int(test.pages[j].shape[0]), int(test.pages[j].shape[1])) for j in which]
    device, n = test.packed.device, len(shapes)
    blob = page_table(shapes, [test.packed_at[j] for j in which])
    if edit_table is not None:
        edit_table(blob)
    label_b, area_b, box_b = filter_scratch_sizes(shapes)
    side = int(params["side"])
    if buffers is None:
        buffers = (grown(scratch, "cc_labels", label_b // 4, torch.int32, device), grown(scratch, "cc_areas", area_b // 4, torch.int32, device),
                   grown(scratch, "cc_boxes", box_b // 4, torch.int32, device) if side else None)
    labels, areas, boxes = buffers
    if counts is None:
        counts = grown(scratch, "cc_counts6", 6 * n, torch.int32, device)
    assert counts.numel() >= 6 * n and counts.is_contiguous()
    blob_dev = imaging._stage_blob(blob.reshape(-1), device)
    _lib.check(_lib.load().ymk_cc_filter_pages(blob_dev.data_ptr(), blob.size, n, max(h for h, _ in shapes), max(w for _, w in shapes),
                                               test.packed.data_ptr(), test.packed_bytes, labels.data_ptr(), label_b, areas.data_ptr(), area_b,
                                               None if boxes is None else boxes.data_ptr(), box_b if boxes is not None else 0,
                                               int(params["black"]), int(params["white"]), side, int(params["fill"]), counts.data_ptr(),
                                               _lib.current_stream_ptr()), "ymk_cc_filter_pages")
    return counts


def filter_result(params: dict, six: Sequence[int]) -> InkFiltered:
    """The InkFiltered of one page from its six counts."""
    return InkFiltered(int(params["black"]), int(params["white"]), int(params["side"]), int(params["fill"]), *[int(v) for v in six])


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


def filter_masks(masks: Sequence, black: int = DEFAULT, white: int = DEFAULT, side: int = BLOB_DEFAULTS["side"],
                 fill: int = BLOB_DEFAULTS["fill"], stream=None, scratch: Optional[dict] = None) -> list:
    """One entry per mask, in order: (the clean mask, a bool H x W device tensor; its InkFiltered) - or the ValueError of a mask
    that is not 2-D bool or whose side is not in 1..16383.  masks: bool H x W arrays or tensors, True = ink.  black, white: the
    sizes of check_despeckle, both 0 to skip the two steps; side, fill: check_blobs' numbers, side 0 to skip the blob step.  A call
    that skips all three is a ValueError.  stream, scratch: as despeckle_masks.  One wait, for the counts."""
    import torch

    from . import _lib
    from .devpages import MAX_SIDE, to_pinned

    speck = check_despeckle({"black": black, "white": white}) if (black or white) else None
    if isinstance(side, bool) or not isinstance(side, int):
        raise ValueError(f"side is an int, 0 or {BLOB_SIDES[0]}..{BLOB_SIDES[1]}, got {side!r}")
    blobs = check_blobs({"side": side, "fill": fill}) if side != 0 else None
    if speck is None and blobs is None:
        raise ValueError("filter_masks with black, white and side all 0 removes nothing")
    params = filter_params(speck, blobs)
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
        raise _lib.YmkError("filter_masks needs a HIP device (there is no host fallback)")
    device = next((masks[k].device for k in live if isinstance(masks[k], torch.Tensor) and masks[k].device.type == "cuda"),
                  torch.device("cuda", torch.cuda.current_device()))
    scratch = {} if scratch is None else scratch
    with torch.cuda.device(device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(device)):
        test = _Masks([masks[k] for k in live], device)
        counts = launch_filter(test, list(range(len(live))), params, scratch)
        pin = to_pinned(scratch, "cc_pin_counts6", counts, 6 * len(live))
        torch.cuda.current_stream().synchronize()
        six = pin[: 6 * len(live)].view(-1, 6).tolist()
        for j, k in enumerate(live):
            out[k] = (unpack_rows(test.rows(j), int(masks[k].shape[1])), filter_result(params, six[j]))
    return out
