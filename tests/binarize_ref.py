"""The definition of the device's binariser for grey-valued pages (yomitoku_amd/ccitt.py, yomitoku_amd/csrc/ymk_binarize.hip),
in plain NumPy / Python.  A helper like tests/ccitt_ref.py: it shares no code with the product, and the device must equal it bit
for bit; tests/test_binarize_host.py holds it to exact rational arithmetic and to a literal per-pixel loop.

A page is grey-valued when it has one channel, or three with B == G == R at every pixel; p is that one value.  1 = black, as in
ccitt_ref.black_mask.

"otsu": one threshold per page.  hist[0..255] over the pixels, N their number.  For t in 0..254: w0 = sum_{i<=t} hist[i],
w1 = N - w0, m0 = sum_{i<=t} i hist[i], m1 = sum_i i hist[i] - m0, all int64; d = m1 w0 - m0 w1 (both products are at most
255 N^2 / 4 < 2^62 for the largest page, 16383^2 pixels); sigma(t) = float64(d) * float64(d) / float64(w0 w1), the product w0 w1
in int64 first: three IEEE operations in this order.  t* is the smallest t with w0 > 0 and w1 > 0 whose sigma is strictly greater
than every earlier one's; 0 where no t has both classes (a uniform page).  Black iff p <= t*.

"adaptive": Bradley-Roth with a mean window, integers only.  r = max(1, max(h, w) // 16); the window of (y, x) is rows
[y - r, y + r] x columns [x - r, x + r] clipped to the page, n its pixel count, S its sum (at most 255 * 2047^2 < 2^31).  Black
iff p n 20 <= S 17 in 64 bits: 15 % below the local mean.
"""

from __future__ import annotations

import numpy as np

METHODS = ("otsu", "adaptive")


def is_grey_valued(page) -> bool:
    """Whether a uint8 page, H x W or H x W x 3, is grey-valued."""
    page = np.asarray(page)
    if page.dtype != np.uint8 or page.ndim not in (2, 3) or (page.ndim == 3 and page.shape[2] != 3):
        return False
    return page.ndim == 2 or bool((page[..., 0] == page[..., 1]).all() and (page[..., 1] == page[..., 2]).all())


def grey(page):
    """H x W uint8: the one value of every pixel of a grey-valued page."""
    page = np.asarray(page)
    return page if page.ndim == 2 else page[..., 0]


def histogram(page):
    return np.bincount(grey(page).reshape(-1), minlength=256).astype(np.int64)


def otsu_sigmas(hist):
    """[(t, sigma(t))] of the t in 0..254 with both classes non-empty."""
    hist = np.asarray(hist, np.int64)
    total_w, total_m = int(hist.sum()), int((hist * np.arange(256, dtype=np.int64)).sum())
    out, w0, m0 = [], 0, 0
    for t in range(255):
        w0 += int(hist[t])
        m0 += t * int(hist[t])
        w1, m1 = total_w - w0, total_m - m0
        if w0 > 0 and w1 > 0:
            d = np.int64(m1) * np.int64(w0) - np.int64(m0) * np.int64(w1)
            dd = np.float64(d)
            out.append((t, np.float64(dd * dd) / np.float64(np.int64(w0) * np.int64(w1))))
    return out


def otsu_threshold(page) -> int:
    best, at = None, 0
    for t, sigma in otsu_sigmas(histogram(page)):
        if best is None or sigma > best:
            best, at = sigma, t
    return at


def window_sums(p):
    """(n, S) per pixel, int64: the pixel count and the sum of its clipped window."""
    p = np.asarray(p).astype(np.int64)
    h, w = p.shape
    r = max(1, max(h, w) // 16)
    table = np.zeros((h + 1, w + 1), np.int64)
    table[1:, 1:] = p.cumsum(0).cumsum(1)
    ya, yb = np.maximum(np.arange(h) - r, 0), np.minimum(np.arange(h) + r, h - 1) + 1
    xa, xb = np.maximum(np.arange(w) - r, 0), np.minimum(np.arange(w) + r, w - 1) + 1
    n = (yb - ya)[:, None] * (xb - xa)[None, :]
    s = table[yb][:, xb] - table[ya][:, xb] - table[yb][:, xa] + table[ya][:, xa]
    return n.astype(np.int64), s


def black_mask(page, method):
    """H x W bool, True = black, of a grey-valued page under `method`."""
    p = grey(page)
    if method == "otsu":
        return p <= otsu_threshold(page)
    if method == "adaptive":
        n, s = window_sums(p)
        return p.astype(np.int64) * n * 20 <= s * 17
    raise ValueError(method)


def gradient_page():
    """(page, ink): the 96 x 160 page the two methods differ on - background 120 + 0.8 x, ink 70 below it where
    (x // 3 + y // 5) % 7 == 0, seeded noise of +-4 - and its ink mask."""
    h, w = 96, 160
    y, x = np.mgrid[0:h, 0:w]
    ink = (x // 3 + y // 5) % 7 == 0
    noise = np.random.default_rng(20240607).integers(-4, 5, (h, w))
    page = np.floor(120 + 0.8 * x).astype(np.int64) - 70 * ink + noise
    return np.clip(page, 0, 255).astype(np.uint8), ink
