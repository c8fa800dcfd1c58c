"""The definition of the device's page-skew estimator and rotation (yomitoku_amd/deskew.py, yomitoku_amd/csrc/ymk_deskew.hip;
DESIGN.md, "Page skew"), in plain NumPy / Python integers.  A helper like tests/binarize_ref.py and tests/ccitt_ref.py: the
device must equal it bit for bit; tests/test_deskew_host.py holds it to a literal per-pixel loop and to exact rational
arithmetic.  The one thing it shares with the product is the function that makes the integer angle table
(yomitoku_amd.deskew.angle_table) and the one that turns `min_angle` into an index (dead_band): the device only ever sees
those integers, and both sides must see the same ones.

Luminance.  A one-channel page is its own; of B G R, Y = (29 B + 150 G + 77 R + 128) >> 8.
Ink.  binarize_ref.black_mask(Y, "adaptive"): Bradley-Roth, unchanged.
Angles.  k = -K .. K, theta_k = k step; s_k = round(sin theta_k 2^14), c_k = round(cos theta_k 2^14).
Profiles.  Every ink pixel (x, y) adds one to row bin (y c_k + x s_k + off_r) >> 14 and to column bin (x c_k - y s_k + off_q)
>> 14; off_r = w << 14 and off_q = h << 14 make both non-negative.
Score.  S_k = sum_b (P_row[b + 1] - P_row[b])^2 + sum_b (P_col[b + 1] - P_col[b])^2 in Python integers, b from the empty bin
below the first to the last bin, whose upper neighbour is empty: an offset that is another multiple of 2^14 moves the bins and
leaves S_k alone.
Choice.  The k of the largest S_k; of equal ones the smallest |k|, then the negative one.  The angle is 0 where |k| is below
the dead band (|theta_k| < min_angle) or 8 S_k < 9 S_0.
Sign.  Positive = the content is turned counter-clockwise on the screen: Pillow's rotate(+a) of an upright page estimates +a.
Rotation by k != 0, same size, channel by channel: u = 2 X - (w - 1), v = 2 Y - (h - 1); SX = c u + s v + ((w - 1) << 14),
SY = -s u + c v + ((h - 1) << 14); x0 = SX >> 15, fx = (SX >> 7) & 255, the same for y; out = ((256 - fx)(256 - fy) p00 +
fx (256 - fy) p10 + (256 - fx) fy p01 + fx fy p11 + 32768) >> 16, a tap outside the page being 255.  All shifts floor.
Nothing overflows 32 bits for sides up to 16383: |c u|, |s v| <= 2^14 * 16382 < 2^28 and (w - 1) << 14 < 2^28, so |SX| < 3 * 2^28;
the blend is at most 2^16 * 255 + 2^15 < 2^24.  k = 0 leaves the bytes as they are.
"""

from __future__ import annotations

import numpy as np

from tests import binarize_ref
from yomitoku_amd.deskew import SHIFT, angle_table, dead_band

ONE = 1 << SHIFT


def luminance(page):
    """H x W uint8 of a uint8 page, H x W or H x W x 3 (B G R)."""
    page = np.asarray(page)
    if page.ndim == 2:
        return page
    p = page.astype(np.int64)
    return ((29 * p[..., 0] + 150 * p[..., 1] + 77 * p[..., 2] + 128) >> 8).astype(np.uint8)


def ink(page):
    """H x W bool, True = ink."""
    return binarize_ref.black_mask(luminance(page), "adaptive")


def profiles(mask, s, c):
    """(row profile, column profile) of an ink mask at one angle, int64, bin 0 = offset w << 14 / h << 14."""
    h, w = mask.shape
    ys, xs = np.nonzero(mask)
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    r = (ys * c + xs * s + (w << SHIFT)) >> SHIFT
    q = (xs * c - ys * s + (h << SHIFT)) >> SHIFT
    return np.bincount(r, minlength=h + 2 * w + 2).astype(np.int64), np.bincount(q, minlength=w + 2 * h + 2).astype(np.int64)


def _sharpness(profile) -> int:
    d = np.diff(np.concatenate([[0], profile, [0]]).astype(np.int64))
    return int((d * d).sum())  # at most (h + 2 w) * (2 * 16383)^2 < 2^47


def scores(mask, table):
    """[S_k] as Python integers, one per row (s, c) of `table`."""
    out = []
    for s, c in np.asarray(table).tolist():
        pr, pq = profiles(mask, s, c)
        out.append(_sharpness(pr) + _sharpness(pq))
    return out


def choose(S, dead=0):
    """(k, S of the best angle, S_0): k the chosen index, 0 inside the dead band |k| < `dead` or without the 9 / 8 margin."""
    K = len(S) // 2
    best = 0
    for k in sorted(range(-K, K + 1), key=lambda k: (abs(k), k)):  # 0, -1, 1, -2, 2 ...: the first of equal ones wins
        if S[k + K] > S[best + K]:
            best = k
    s_best, s_zero = int(S[best + K]), int(S[K])
    if abs(best) < dead or 8 * s_best < 9 * s_zero:
        best = 0
    return best, s_best, s_zero


def estimate(page, step=0.1, max_angle=5.0, min_angle=0.3):
    """(k, angle in degrees, S of the best angle, S_0) of a page."""
    table = angle_table(step, max_angle)
    k, s_best, s_zero = choose(scores(ink(page), table), dead_band(step, min_angle))
    return k, k * step, s_best, s_zero


def source_coordinates(h, w, s, c):
    """(SX, SY), int64 H x W: where the rotation by (s, c) reads output pixel (X, Y), in units of 2^-15 pixels."""
    u = 2 * np.arange(w, dtype=np.int64)[None, :] - (w - 1)
    v = 2 * np.arange(h, dtype=np.int64)[:, None] - (h - 1)
    return c * u + s * v + ((w - 1) << SHIFT), -s * u + c * v + ((h - 1) << SHIFT)


def rotate(page, s, c):
    """The page turned by the angle of (s, c): what undoes a skew of that angle.  (s, c) = (0, 2^14) copies."""
    page = np.asarray(page)
    if s == 0 and c == ONE:
        return page.copy()
    h, w = page.shape[:2]
    sx, sy = source_coordinates(h, w, s, c)
    x0, fx, y0, fy = sx >> 15, (sx >> 7) & 255, sy >> 15, (sy >> 7) & 255
    src = page.reshape(h, w, -1).astype(np.int64)

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        got = src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
        return np.where(inside[..., None], got, 255)

    fx, fy = fx[..., None], fy[..., None]
    out = ((256 - fx) * (256 - fy) * tap(y0, x0) + fx * (256 - fy) * tap(y0, x0 + 1) + (256 - fx) * fy * tap(y0 + 1, x0)
           + fx * fy * tap(y0 + 1, x0 + 1) + 32768) >> 16
    return out.astype(np.uint8).reshape(page.shape)


def deskew(page, step=0.1, max_angle=5.0, min_angle=0.3):
    """(the corrected page, k, S of the best angle, S_0)."""
    k, _, s_best, s_zero = estimate(page, step, max_angle, min_angle)
    s, c = angle_table(step, max_angle)[k + (len(angle_table(step, max_angle)) // 2)].tolist()
    return (rotate(page, s, c) if k else np.asarray(page).copy()), k, s_best, s_zero
