"""Plain CPU definitions of what the page / text-line pre-processing kernels (yomitoku_amd/csrc/ymk_image.hip) compute, written
from the kernels' header comments and the published cv2 / Pillow algorithms.  NumPy only: no GPU, no yomitoku_amd, no oracle.

Where oracle/cvlike.py states the same operation these use another formulation (box integrals by overlap lengths against the
tap table, exact integer warp weights against the float table, whole-array cell sums against per-cell loops), so that
tests/test_image_ref_host.py can hold the two against each other.

The cases of tests/test_image_ops_gpu.py live here too, so the CPU module checks the references on the very same inputs."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

DET_MEAN = (0.485, 0.456, 0.406)  # det_preprocess: tensor channel c is BGR channel c with mean / std [c]
DET_STD = (0.229, 0.224, 0.225)


def noise_page(seed: int, h: int, w: int) -> np.ndarray:
    """uint8 h x w x 3 noise: every byte independent, so an index error changes bytes."""
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


# ------------------------------------------------------------------ cv2.resize(INTER_AREA)
def _overlap(a: float, b: float, n: int) -> np.ndarray:
    """Length of [a, b) inside each of the pixels [i, i + 1), i < n."""
    i = np.arange(n, dtype=np.float64)
    return np.maximum(0.0, np.minimum(b, i + 1.0) - np.maximum(a, i))


def box_weights(ssize: int, dsize: int) -> np.ndarray:
    """float64 [dsize, ssize]: the share of source pixel i in destination cell d = [d * scale, (d + 1) * scale), divided by the
    length of the cell that lies inside the image, min(scale, ssize - d * scale)."""
    scale = ssize / dsize
    w = np.zeros((dsize, ssize), dtype=np.float64)
    for d in range(dsize):
        a = d * scale
        w[d] = _overlap(a, a + scale, ssize) / min(scale, ssize - a)
    return w


def box_overlaps_are_clean(ssize: int, dsize: int) -> bool:
    """True when every partial overlap of the area rule is 0 or >= 1/64, in exact rational arithmetic.  cv2 drops partial
    taps <= 1e-3 without renormalising; where none is that small its tap table and the box integral are the same numbers."""
    scale = Fraction(ssize, dsize)
    for d in range(dsize):
        a, b = d * scale, (d + 1) * scale
        for i in range(math.floor(a), min(math.ceil(b), ssize)):
            ov = min(b, Fraction(i + 1)) - max(a, Fraction(i))
            if 0 < ov < Fraction(1, 64):
                return False
    return True


def linear_area_axis(ssize: int, dsize: int):
    """cv2's INTER_AREA rule for an axis handled by the linear resizer: (first source index int64 [dsize], second index, fraction
    float64 holding the float32 value cv2 stores).  sx = floor(d * scale); fx = (float)((d + 1) - (sx + 1) / scale), negative
    -> 0, else its fractional part; an index outside [0, ssize - 1) is clamped and its fraction set to 0."""
    scale = ssize / dsize
    inv = 1.0 / scale
    d = np.arange(dsize, dtype=np.float64)
    s0 = np.floor(d * scale)
    fx = ((d + 1.0) - (s0 + 1.0) * inv).astype(np.float32)
    fx = np.where(fx <= 0, np.float32(0.0), fx - np.floor(fx)).astype(np.float32)
    s0 = s0.astype(np.int64)
    low, high = s0 < 0, s0 >= ssize - 1
    fx = np.where(low | high, np.float32(0.0), fx)
    s0 = np.where(low, 0, np.where(high, ssize - 1, s0))
    return s0, np.minimum(s0 + 1, ssize - 1), fx.astype(np.float64)


def det_scales(h: int, w: int, oh: int, ow: int):
    return h / oh, w / ow


def det_resize64(img_u8: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """float64 [oh, ow, 3]: cv2.resize(float image, (ow, oh), INTER_AREA) without any rounding but cv2's own (float) casts."""
    h, w = img_u8.shape[:2]
    src = img_u8.astype(np.float64)
    sy, sx = det_scales(h, w, oh, ow)
    if sx >= 1.0 and sy >= 1.0:
        wy, wx = box_weights(h, oh), box_weights(w, ow)
        return np.einsum("yi,ijc,xj->yxc", wy, src, wx, optimize=True)
    x0, x1, fx = linear_area_axis(w, ow)
    y0, y1, fy = linear_area_axis(h, oh)
    rows = src[:, x0] * (1.0 - fx)[None, :, None] + src[:, x1] * fx[None, :, None]
    return rows[y0] * (1.0 - fy)[:, None, None] + rows[y1] * fy[:, None, None]


def det_normalise64(resized: np.ndarray) -> np.ndarray:
    """[oh, ow, 3] BGR in pixel units -> float64 [3, oh, ow]: / 255, (x - mean[c]) / std[c]."""
    x = resized.astype(np.float64) / 255.0
    x = (x - np.array(DET_MEAN, dtype=np.float64)) / np.array(DET_STD, dtype=np.float64)
    return np.ascontiguousarray(np.transpose(x, (2, 0, 1)))


def det_ref64(img_u8_bgr: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """k_det_preprocess in float64: [3, oh, ow]."""
    return det_normalise64(det_resize64(img_u8_bgr, oh, ow))


def det_normalise32(resized_f32: np.ndarray) -> np.ndarray:
    """The reference's own normalisation of a float32 resize (standardization_image): / 255 in float32, (x - mean) / std in
    float64, back to float32 -> [3, oh, ow].  With oracle.cvlike.resize_area in front this is the fp32 restatement."""
    assert resized_f32.dtype == np.float32
    x = resized_f32 / np.float32(255.0)
    x = ((x.astype(np.float64) - np.array(DET_MEAN)) / np.array(DET_STD)).astype(np.float32)
    return np.ascontiguousarray(np.transpose(x, (2, 0, 1)))


def det_bound(e32: float, ref64: np.ndarray) -> float:
    """What the fp32 kernel has to stay within: 4 x the error of the fp32 restatement, and never less than 2^-22 of the largest
    value (the restatement can be exact up to its final cast)."""
    return max(4.0 * e32, 2.0 ** -22 * float(np.abs(ref64).max()))


# (h, w) -> (oh, ow).  The mixed cases (one axis grows, the other shrinks: the linear rule on both) come at two shrink factors:
# below 2 a cell never covers more than two pixels and the linear rule's two taps ARE the box integral (1.25: weights 0.6 / 0.4
# either way), so only a factor >= 2 - here 3, where the rule takes two pixels of the three a cell covers - can tell the
# branch condition `sx >= 1 && sy >= 1` from `||`.
DET_CASES = [((45, 61), (32, 32)), ((64, 96), (32, 32)), ((32, 32), (32, 32)), ((40, 24), (32, 32)), ((24, 40), (32, 32)),
             ((96, 24), (32, 32)), ((24, 96), (32, 32)), ((32, 24), (32, 352)), ((32, 2), (32, 98)),
             ((20, 28), (32, 64)), ((1, 1), (32, 32)), ((8, 600), (8, 300)), ((669, 33), (32, 32)), ((33, 669), (32, 32))]
DET_REFUSED = ((672, 32), (32, 32))  # the one the entry refuses
# (ssize, dsize, d) of an enlarged axis where d * (ssize / dsize) is an integer n in exact arithmetic but n - 1 ulp in double
# (220 * (24 / 352) = 14.999999999999998, 49 * (2 / 98) = 0.9999999999999999): sx = n - 1, the linear rule's fraction comes out
# as exactly 1.0f, and `fx - floor(fx)` is what makes it 0 - pixel n - 1 with weight 1, as cv2 computes it.  Without that line the
# kernel would take pixel n.  The only inputs on which the line changes a value.
DET_FRACTION_ONE = [(24, 352, 220), (2, 98, 49)]
DET_MIXED = [((40, 24), (32, 32)), ((24, 40), (32, 32)), ((96, 24), (32, 32)), ((24, 96), (32, 32))]


def det_page(h: int, w: int) -> np.ndarray:
    return noise_page(1000 + 7 * h + w, h, w)


# ------------------------------------------------------------------ cv2.warpPerspective(INTER_LINEAR, BORDER_CONSTANT 0), uint8
def warp_coords(minv, ww: int, wh: int):
    """Fixed-point source coordinates (int64 [wh, ww] each, in 1/32 px) of every destination pixel: double coordinates, 32 / W,
    clamped to the int range, rounded half to even."""
    m = np.asarray(minv, dtype=np.float64).reshape(9)
    x = np.arange(ww, dtype=np.float64)[None, :]
    y = np.arange(wh, dtype=np.float64)[:, None]
    x0 = m[0] * x + m[1] * y + m[2]
    y0 = m[3] * x + m[4] * y + m[5]
    wd = m[6] * x + m[7] * y + m[8]
    nz = wd != 0.0
    wd = np.where(nz, 32.0 / np.where(nz, wd, 1.0), 0.0)
    lo, hi = -2147483648.0, 2147483647.0
    xi = np.rint(np.clip(x0 * wd, lo, hi)).astype(np.int64)
    yi = np.rint(np.clip(y0 * wd, lo, hi)).astype(np.int64)
    return xi, yi


def warp_ref(roi_u8: np.ndarray, minv, ww: int, wh: int) -> np.ndarray:
    """k_warp_quads on one crop: roi_u8 [bh, bw, 3] (the bounding box of the quad, in the channel order wanted) -> uint8
    [wh, ww, 3].  The four bilinear weights are the exact integers (32 - ax)(32 - ay) * 32 .. ax * ay * 32 (sum 32768); a tap
    outside the box counts 0; the sum is rounded as (acc + 2^14) >> 15."""
    bh, bw = roi_u8.shape[:2]
    xi, yi = warp_coords(minv, ww, wh)
    sx, sy, ax, ay = xi >> 5, yi >> 5, xi & 31, yi & 31
    pad = np.zeros((bh + 2, bw + 2, 3), dtype=np.int64)  # index 0 and the last: everything outside the box
    pad[1:-1, 1:-1] = roi_u8
    acc = np.zeros((wh, ww, 3), dtype=np.int64)
    for dy, dx, wt in ((0, 0, (32 - ax) * (32 - ay) * 32), (0, 1, ax * (32 - ay) * 32), (1, 0, (32 - ax) * ay * 32),
                       (1, 1, ax * ay * 32)):
        yy = np.clip(sy + dy + 1, 0, bh + 1)
        xx = np.clip(sx + dx + 1, 0, bw + 1)
        acc += pad[yy, xx] * wt[:, :, None]
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------ rotation, INTER_AREA down-scale on uint8, canvas
def area_branch(rw: int, rh: int, nw: int, nh: int) -> str:
    """Which of cv2's routes resize(INTER_AREA) of an rw x rh uint8 image to nw x nh (never larger) takes: "copy" (same size:
    the caller skips the resize), "fast2" (ResizeAreaFast, 2 x 2), "fast" (ResizeAreaFast, another integer factor), "general"
    (the area table).  Fast means both scales are integers within DBL_EPSILON."""
    if (nw, nh) == (rw, rh):
        return "copy"
    fx, fy = rw / nw, rh / nh
    ix, iy = int(round(fx)), int(round(fy))
    eps = 2.220446049250313e-16
    if abs(fx - ix) < eps and abs(fy - iy) < eps:
        return "fast2" if (ix, iy) == (2, 2) else "fast"
    return "general"


def _area_taps32(ssize: int, dsize: int):
    """Per destination index the (source index, float32 weight) taps of the area table, from overlap lengths: a pixel the cell
    covers fully weighs 1 / cell, a partly covered one its overlap / cell unless the overlap is <= 1e-3 (dropped)."""
    scale = ssize / dsize
    taps = []
    for d in range(dsize):
        a = d * scale
        b = a + scale
        cell = min(scale, ssize - a)
        ov = _overlap(a, b, ssize)
        row = []
        for i in np.flatnonzero(ov > 0).tolist():
            if ov[i] < 1.0 and ov[i] <= 1e-3:
                continue
            row.append((i, np.float32(ov[i] / cell)))
        taps.append(row)
    return taps


def area_resize_u8(img_u8: np.ndarray, nw: int, nh: int) -> np.ndarray:
    """cv2.resize(uint8 image, (nw, nh), INTER_AREA), down-scaling only, by the route `area_branch` names."""
    rh, rw = img_u8.shape[:2]
    branch = area_branch(rw, rh, nw, nh)
    if branch == "copy":
        return img_u8.copy()
    if branch in ("fast2", "fast"):
        ix, iy = rw // nw, rh // nh
        s = np.zeros((nh, nw, 3), dtype=np.int64)
        for dy in range(iy):
            for dx in range(ix):
                s += img_u8[dy: dy + iy * nh: iy, dx: dx + ix * nw: ix]
        if branch == "fast2":
            return ((s + 2) >> 2).astype(np.uint8)
        v = np.rint(s.astype(np.float32) * (np.float32(1.0) / np.float32(ix * iy)))
        return np.clip(v, 0, 255).astype(np.uint8)
    src = img_u8.astype(np.float32)
    tx, ty = _area_taps32(rw, nw), _area_taps32(rh, nh)
    rows = np.zeros((rh, nw, 3), dtype=np.float32)  # float32 sums in tap order, as cv2 accumulates them
    for d, taps in enumerate(tx):
        for i, wt in taps:
            rows[:, d] = rows[:, d] + src[:, i] * wt
    out = np.zeros((nh, nw, 3), dtype=np.float32)
    for d, taps in enumerate(ty):
        for k, (i, wt) in enumerate(taps):
            out[d] = wt * rows[i] if k == 0 else out[d] + wt * rows[i]
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)  # saturate_cast<uchar>: round half to even


def crop_resize_ref(warped_u8: np.ndarray, desc, out_h: int, batch_w: int) -> np.ndarray:
    """k_crop_resize_norm on one crop: warped_u8 [wh, ww, 3]; desc: anything with rot, flip, rw, rh, nw, nh (a CropDesc record
    or a dict) -> float32 [3, out_h, batch_w].  The resize route comes from the sizes alone, not from desc's fast_x / fast_y."""
    get = (lambda k: int(desc[k]))
    img = warped_u8
    if get("rot"):
        img = np.rot90(img, k=1)  # cv2.ROTATE_90_COUNTERCLOCKWISE
    if get("flip"):
        img = img[::-1, ::-1]  # a 180 degree turn
    rw, rh, nw, nh = get("rw"), get("rh"), get("nw"), get("nh")
    assert img.shape[:2] == (rh, rw) and nw <= batch_w and nh <= out_h
    small = area_resize_u8(np.ascontiguousarray(img), nw, nh)
    out = np.full((3, out_h, batch_w), -1.0, dtype=np.float32)
    t = np.transpose(small, (2, 0, 1)).astype(np.float32) / np.float32(255.0)
    out[:, :nh, :nw] = (t - np.float32(0.5)) / np.float32(0.5)
    return out


# ------------------------------------------------------------------ cv2.resize(fx=0.5, fy=0.5, INTER_AREA) on uint8
def half_size(n: int) -> int:
    return int(round(n * 0.5))  # saturate_cast<int>: round half to even


def halve_ref(img_u8: np.ndarray) -> np.ndarray:
    """k_halve_u8c3: [h, w, 3] -> [half_size(h), half_size(w), 3].  Cell (y, x) holds source rows 2y, 2y + 1 and columns 2x,
    2x + 1 as far as they exist: four pixels -> (s + 2) >> 2, fewer -> rint(float32(s) / count), none -> 0."""
    h, w = img_u8.shape[:2]
    dh, dw = half_size(h), half_size(w)
    big = np.zeros((2 * dh + 2, 2 * dw + 2, 3), dtype=np.int64)
    have = np.zeros((2 * dh + 2, 2 * dw + 2), dtype=np.int64)
    big[:h, :w] = img_u8
    have[:h, :w] = 1
    big, have = big[: 2 * dh, : 2 * dw], have[: 2 * dh, : 2 * dw]
    s = big.reshape(dh, 2, dw, 2, 3).sum(axis=(1, 3))
    n = have.reshape(dh, 2, dw, 2).sum(axis=(1, 3))[:, :, None]
    cut = np.rint(s.astype(np.float32) / np.maximum(n, 1).astype(np.float32)).astype(np.int64)
    return np.where(n == 4, (s + 2) >> 2, np.where(n == 0, 0, cut)).astype(np.uint8)


HALVE_CASES = [(2, 2), (3, 3), (5, 7), (6, 5), (4, 513), (4, 515)]
HALVE_REFUSED = (1, 9)

# ------------------------------------------------------------------ the text-line cases (page 200 x 136, canvas 32 x 800)
CROP_PAGE_HW = (200, 136)
CROP_CANVAS = (32, 800)


def crop_page() -> np.ndarray:
    return noise_page(77, *CROP_PAGE_HW)


def _rect(x, y, w, h):
    return [[x, y], [x + w, y], [x + w, y + h], [x, y + h]]


# name -> (quad, translation only?, turned by 90 degrees?)
WARP_QUADS = {
    "upright": (_rect(10, 20, 80, 30), True, False),
    "page": (_rect(0, 0, 136, 200), True, False),
    "corners": ([[0, 2], [133, 0], [136, 197], [3, 200]], False, False),
    "slant_a": ([[20, 60], [120, 75], [115, 110], [16, 97]], False, False),
    "slant_b": ([[30, 130], [110, 120], [118, 170], [35, 185]], False, False),
    "vertical": ([[100, 10], [125, 12], [123, 190], [99, 188]], False, True),
}
# short side 64 .. 127 px: source_downscale cuts these from pyramid level 1
WARP_QUADS_LEVEL1 = {
    "wide": ([[4, 6], [130, 10], [128, 90], [2, 84]], False, False),
    "square": ([[10, 100], [100, 104], [98, 190], [8, 186]], False, False),
    "upright": (_rect(6, 20, 120, 70), True, False),
    "vertical": ([[30, 5], [100, 8], [98, 196], [28, 192]], False, True),
}
# name -> (quad, resize route, turned?): every route upright and turned; "fast4" (4 x 4) is there because 3 x 3 sums have no
# rounding ties (s / 9 is never k + 1/2), so only an even factor can tell round-half-even from round-half-up
STAGE2_QUADS = {
    "copy": (_rect(50, 100, 40, 20), "copy", False),
    "fast2": (_rect(8, 30, 120, 64), "fast2", False),
    "fast3": (_rect(5, 50, 126, 96), "fast", False),
    "fast4": (_rect(0, 60, 136, 128), "fast", False),
    "general": (_rect(0, 0, 136, 200), "general", False),
    "copy_rot": (_rect(100, 5, 20, 90), "copy", True),
    "fast2_rot": (_rect(60, 4, 64, 192), "fast2", True),
    "fast3_rot": (_rect(20, 1, 96, 198), "fast", True),
    "general_rot": (_rect(3, 90, 40, 96), "general", True),
}
