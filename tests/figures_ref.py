"""The definition of a figure crop (yomitoku_amd/figures.py; yomitoku_amd/csrc/ymk_crop.hip), as plain NumPy.

The exporters cut `img[y1:y2, x1:x2]` with `x1, y1, x2, y2 = map(int, figure.box)` (yomitoku_amd/export.py: _save_figures; the
reference's export/*.py do the same).  `int()` truncates toward zero; the rectangle here is that one clamped to the page, and
a box that leaves nothing has no crop.  For a box inside the page - what the layout parser hands out - the two agree."""
import numpy as np


def rect(box, h, w):
    """(x1, y1, x2, y2) in pixels, or None for an empty rectangle."""
    x1, y1, x2, y2 = (int(v) for v in box)
    x1, x2 = min(max(x1, 0), w), min(max(x2, 0), w)
    y1, y2 = min(max(y1, 0), h), min(max(y2, 0), h)
    if x2 <= x1 or y2 <= y1:
        return None
    return x1, y1, x2, y2


def crop(page, box):
    """The crop of `box` from a [h][w][3] or [h][w] page as a contiguous array, or None."""
    page = np.asarray(page)
    r = rect(box, page.shape[0], page.shape[1])
    if r is None:
        return None
    x1, y1, x2, y2 = r
    return np.ascontiguousarray(page[y1:y2, x1:x2])


def crop_rect(page, r):
    """The crop at a rectangle that `rect` made."""
    x1, y1, x2, y2 = r
    return np.ascontiguousarray(np.asarray(page)[y1:y2, x1:x2])
