"""Page skew: the pages of a wave estimated and turned upright on the device, before any network sees them.

    corrected, skews = deskew_pages(pages)                    # device tensors or host arrays, uint8 H x W x 3 (B G R) or H x W
    skews = estimate_skew_pages(pages, {"max_angle": 3.0})    # the estimate alone
    analyzer.serve(sources, deskew=True)                      # every entry ends with the page's PageSkew

A scan that lies a few degrees askew on the glass defeats axis-aligned layout, table and cell boxes and the reading order, and the
page image of a searchable PDF stays crooked.  The estimator is a projection-profile search, all integers ("Page
skew"; the definition is tests/deskew_ref.py, which the device equals bit for bit; yomitoku_amd/csrc/ymk_deskew.hip):

  - ink: the luminance plane under the binariser's "adaptive" threshold (yomitoku_amd/ccitt.py), as packed rows;
  - for each angle k step, k = -K .. K, the ink's row and column profiles along axes turned by that angle, and the score
    S_k = the sum of the squared differences of neighbouring bins of both: text lines, rulings and vertical text make the
    profiles jagged exactly when the axes are theirs;
  - the angle of the largest S_k - of equal ones the smallest |k|, then the negative one -, and 0 where that is inside the dead band
    (`min_angle`) or not 12.5 % above the upright score;
  - a bilinear rotation in fixed point about the page's centre, same size, paper white (255) outside.

Positive = the content is turned counter-clockwise on the screen (Pillow's rotate(+a) of an upright page estimates +a); the
correction turns it back.  The host never waits for the decision: the rotation reads it from device words, and the words reach
the host through pinned memory behind the launches.  There is no host fallback.

Out: quarter turns (TextRecognizer's `rec_orientation_fallback` stays the per-line answer), perspective and curl, a border other
than white, `serve_sharded`.
"""

from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

SHIFT = 14  # the fixed point of the angle table: s, c = round(2^14 sin, cos)
MAX_ANGLES = 401
DEFAULTS = {"max_angle": 5.0, "step": 0.1, "min_angle": 0.3}
PAGE_WORDS = 16  # YMK_DSK_PAGE_WORDS
CHOICE_WORDS = 8  # YMK_DSK_CHOICE_WORDS


def half_count(step: float, max_angle: float) -> int:
    """K: the angles are k step, k = -K .. K, the largest not above max_angle."""
    return int(math.floor(max_angle / step + 1e-9))


def angle_table(step: float = DEFAULTS["step"], max_angle: float = DEFAULTS["max_angle"]) -> np.ndarray:
    """int32 [2 K + 1][2]: (s_k, c_k) = (round(sin(k step) 2^14), round(cos(k step) 2^14)), k = -K .. K, in degrees.  THE table:
    the device and the definition (tests/deskew_ref.py) both take their integers from here."""
    K = half_count(step, max_angle)
    rows = []
    for k in range(-K, K + 1):
        theta = math.radians(abs(k) * step)
        s = int(round(math.sin(theta) * (1 << SHIFT)))
        rows.append((s if k >= 0 else -s, int(round(math.cos(theta) * (1 << SHIFT)))))
    return np.array(rows, np.int32).reshape(-1, 2)


def dead_band(step: float, min_angle: float) -> int:
    """The smallest m >= 0 with m step >= min_angle: an estimate with |k| < m is inside the dead band and becomes 0."""
    return max(0, int(math.ceil(min_angle / step - 1e-9)))


def check_deskew(deskew=False) -> Optional[dict]:
    """`deskew` of a call: False -> None; True -> the defaults; a dict with any of max_angle, step, min_angle (degrees) -> the
    defaults with those.  Anything else is a ValueError, and so are a step that is not positive, a negative angle, a max_angle
    above 45 and more than 401 angles."""
    if deskew is False:
        return None
    if deskew is True:
        return dict(DEFAULTS)
    if not isinstance(deskew, dict) or any(k not in DEFAULTS for k in deskew):
        raise ValueError(f"unknown deskew {deskew!r}: False, True or a dict with any of {sorted(DEFAULTS)}")
    out = dict(DEFAULTS)
    for key, value in deskew.items():
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value):
            raise ValueError(f"deskew[{key!r}] is a number of degrees, got {value!r}")
        out[key] = float(value)
    if out["step"] <= 0:
        raise ValueError(f"deskew step must be positive, got {out['step']}")
    if out["max_angle"] < 0 or out["max_angle"] > 45 or out["min_angle"] < 0:
        raise ValueError(f"deskew angles: 0 <= max_angle <= 45 and 0 <= min_angle, got {out['max_angle']}, {out['min_angle']}")
    if 2 * half_count(out["step"], out["max_angle"]) + 1 > MAX_ANGLES:
        raise ValueError(f"deskew: at most {MAX_ANGLES} angles, max_angle {out['max_angle']} at step {out['step']} makes "
                         f"{2 * half_count(out['step'], out['max_angle']) + 1}")
    return out


def rotation_matrix(h: int, w: int, s: int, c: int) -> np.ndarray:
    """2 x 3 float64: corrected-page pixel coordinates (X, Y) -> original-page coordinates, the rotation's own source
    coordinates (SX, SY) / 2^15 exactly."""
    a, b = c / (1 << SHIFT), s / (1 << SHIFT)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    return np.array([[a, b, cx - a * cx - b * cy], [-b, a, cy + b * cx - a * cy]], np.float64)


@dataclass
class PageSkew:
    """What was found and done for one page.  angle: degrees the content was turned counter-clockwise on the screen and has
    been turned back by, 0.0 for a page left as it was; index: k (angle = k step); score, score_upright: S of the best angle
    and S_0; estimated: False for a page too large for the profile (it is left as it was); matrix: 2 x 3 float64, corrected-page
    pixel coordinates -> original-page coordinates (the identity for angle 0)."""

    angle: float = 0.0
    index: int = 0
    score: int = 0
    score_upright: int = 0
    estimated: bool = True
    matrix: np.ndarray = field(default_factory=lambda: np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], np.float64))

    def to_original(self, points) -> np.ndarray:
        """Points (..., 2) as (x, y) of the corrected page -> float64 (..., 2) on the original page."""
        pts = np.asarray(points, np.float64)
        return pts @ self.matrix[:, :2].T + self.matrix[:, 2]


def _checked_table(params: dict):
    """(the angle table, s_max, dead) of a call's parameters, the table checked by the library."""
    from . import _lib

    table = np.ascontiguousarray(angle_table(params["step"], params["max_angle"]))
    s_max = ctypes.c_int()
    _lib.check(_lib.load().ymk_dsk_check_angles(table.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(table), ctypes.byref(s_max)),
               "ymk_dsk_check_angles")
    return table, int(s_max.value), dead_band(params["step"], params["min_angle"])


def scratch_sizes(shapes: Sequence, n_angles: int, s_max: int):
    """((bytes of the planes, the summed-area tables, the packed rows, the scores, the choice words), per page whether it is
    estimated) of pages of `shapes` = (h, w) or (h, w, 3)."""
    from . import _lib
    from .devpages import shape_args

    n = len(shapes)
    sizes, fits = (ctypes.c_int64 * 5)(), (ctypes.c_int * max(1, n))()
    _lib.check(_lib.load().ymk_dsk_scratch_bytes(*shape_args(shapes, channels=True), n, n_angles, s_max, sizes, fits), "ymk_dsk_scratch_bytes")
    return tuple(int(v) for v in sizes), [bool(fits[k]) for k in range(n)]


def page_table(pages: Sequence, dsts: Sequence) -> np.ndarray:
    """int32 [n][16]: the page table of include/ymk.h ("Page skew") - the planes, packed rows and summed-area tables one page
    behind the other; dsts[k]: the destination tensor of page k, or None (estimate only)."""
    from .devpages import addr_words

    rec = np.zeros((len(pages), PAGE_WORDS), np.int32)
    pack = luma = sat = 0
    for k, p in enumerate(pages):
        h, w, ch = int(p.shape[0]), int(p.shape[1]), 1 if p.dim() == 2 else 3
        rec[k, 0:2] = addr_words(p.data_ptr())
        rec[k, 2:5] = (h, w, ch)
        rec[k, 6:8] = addr_words(pack)
        if ch == 3:
            rec[k, 8:10] = addr_words(luma)
            luma += -(-(h * w) // 16) * 16
        if dsts[k] is not None:
            rec[k, 11:13] = addr_words(dsts[k].data_ptr())
        rec[k, 14:16] = addr_words(sat)
        pack, sat = pack + h * (-(-w // 32)), sat + h * w
    return rec


class _Launched:
    """The launches of one call: the pages' shapes, `corrected` (None: estimate only), the device buffers the stages wrote - for
    the tests - and the choice words on their way to pinned memory.  It does not hold the pages that went in."""

    def __init__(self, shapes, corrected, params, table, pin, buffers):
        self.shapes, self.corrected, self.params, self.table, self.pin, self.buffers = shapes, corrected, params, table, pin, buffers

    def skews(self) -> List[PageSkew]:
        """Per page its PageSkew - once the stream the launches went to has been waited for."""
        n, K = len(self.shapes), len(self.table) // 2
        words = self.pin[: n * CHOICE_WORDS].numpy().reshape(n, CHOICE_WORDS).copy()
        big = words[:, 2:6].copy().view(np.uint64)
        out = []
        for j, (h, w) in enumerate(self.shapes):
            k, flag = int(words[j, 0]), int(words[j, 1])
            s, c = self.table[k + K].tolist()
            out.append(PageSkew(k * self.params["step"] if k else 0.0, k, int(big[j, 0]), int(big[j, 1]), flag == 1, rotation_matrix(h, w, s, c)))
        return out


def launch(pages: Sequence, params: dict, scratch: dict, rotate: bool = True, pin_scratch: Optional[dict] = None, edit_table=None) -> _Launched:
    """Queue the whole step for device pages (uint8 H x W x 3 or H x W, contiguous) on the current stream: luminance, ink, scores,
    choice, - `rotate` - the turned pages into fresh tensors, and the copy of the choice words to pinned memory.  Waits for
    nothing.  scratch: the device buffers, kept between calls; pin_scratch: where the pinned words live (default: scratch) - a
    caller with several calls in flight keeps one per call.  edit_table: a function that may change the int32 [n][16] page table
    before it is staged (the tests' malformed record)."""
    import torch

    from . import _lib, imaging
    from .devpages import LUMA_PLANE, PACKED_ROWS, SUMMED_AREA, grown, to_pinned

    lib, device, n = _lib.load(), pages[0].device, len(pages)
    assert lib.ymk_dsk_page_words() == PAGE_WORDS
    table, s_max, dead = _checked_table(params)
    (luma_b, sat_b, packed_b, scores_b, choice_b), _ = scratch_sizes([tuple(p.shape) for p in pages], len(table), s_max)
    corrected = [torch.empty_like(p) for p in pages] if rotate else None
    rec = page_table(pages, corrected if rotate else [None] * n)
    if edit_table is not None:
        edit_table(rec)
    luma = grown(scratch, LUMA_PLANE, max(luma_b, 16), torch.uint8, device)
    sat = grown(scratch, SUMMED_AREA, sat_b // 4, torch.int32, device)
    packed = grown(scratch, PACKED_ROWS, packed_b // 4, torch.int32, device)
    scores = grown(scratch, "dsk_scores", scores_b // 8, torch.int64, device)
    answer = grown(scratch, "dsk_answer", n * (CHOICE_WORDS + PAGE_WORDS), torch.int32, device)  # the choice words, then the planes' table
    blob = np.concatenate([rec.reshape(-1), table.reshape(-1)])
    blob_dev = imaging._stage_blob(blob, device)
    table_ptr = blob_dev.data_ptr() + 4 * rec.size
    planes_ptr = answer.data_ptr() + 4 * n * CHOICE_WORDS
    _lib.check(lib.ymk_dsk_pages(blob_dev.data_ptr(), rec.size, n, max(int(p.shape[0]) for p in pages), max(int(p.shape[1]) for p in pages),
                                 luma.data_ptr(), luma_b, sat.data_ptr(), sat_b, packed.data_ptr(), packed_b, planes_ptr, table_ptr, len(table),
                                 s_max, dead, scores.data_ptr(), answer.data_ptr(), 1 if rotate else 0, _lib.current_stream_ptr()),
               "ymk_dsk_pages")
    pin = to_pinned(scratch if pin_scratch is None else pin_scratch, "dsk_pin_choice", answer, n * CHOICE_WORDS)
    buffers = {"luma": luma, "packed": packed, "scores": scores, "choice": answer, "blob": blob_dev}
    return _Launched([(int(p.shape[0]), int(p.shape[1])) for p in pages], corrected, params, table, pin, buffers)


def _run(pages: Sequence, deskew, stream, scratch, rotate: bool):
    import torch

    from .devpages import entered

    params = check_deskew(deskew)
    if params is None:
        raise ValueError("deskew=False: there is nothing to estimate")
    scratch = {} if scratch is None else scratch
    with entered(pages, stream, "page skew needs") as (_, live, devs, out_skews):
        out_pages = list(out_skews)  # a page's exception stands in both
        if live:
            done = launch(devs, params, scratch, rotate=rotate)
            torch.cuda.current_stream().synchronize()
            for j, (k, skew) in enumerate(zip(live, done.skews())):
                out_skews[k] = skew
                out_pages[k] = done.corrected[j] if rotate else None
    return out_pages, out_skews


def estimate_skew_pages(pages: Sequence, deskew=True, stream=None, scratch: Optional[dict] = None) -> list:
    """One entry per page, in order: its PageSkew - what `deskew_pages` would do to it -, or the exception that page raised (not
    uint8, not H x W x 3 / H x W).  pages: device tensors and / or host arrays; deskew: True or the dict `check_deskew` takes;
    stream: the torch stream to launch on (default: the current one); scratch: a dict the caller keeps between calls."""
    return _run(pages, deskew, stream, scratch, rotate=False)[1]


def deskew_pages(pages: Sequence, deskew=True, stream=None, scratch: Optional[dict] = None):
    """(corrected device pages, [PageSkew]), one entry each per page, in order - a fresh uint8 tensor of the page's shape (a copy
    for angle 0) and its PageSkew -, or in both lists the exception that page raised.  Arguments as `estimate_skew_pages`."""
    return _run(pages, deskew, stream, scratch, rotate=True)
