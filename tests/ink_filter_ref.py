"""The definition of the ink filter of layered pages (yomitoku_amd/despeckle.py: filter_masks; yomitoku_amd/mrc.py: the keys
"despeckle" and "blobs"; yomitoku_amd/csrc/ymk_cc.hip: ymk_cc_filter_pages; DESIGN.md, "Layered pages"): plain NumPy and Python on
top of tests/despeckle_ref.py.  The device equals it bit for bit, in the mask and in the six counts;
tests/test_ink_filter_host.py holds step 3 to scipy.ndimage.label and find_objects.

    clean, (black_components, black_pixels, white_components, white_pixels, blob_components, blob_pixels) = \\
        filter_ink(M, black, white, side, fill)

1. and 2. are despeckle_ref.despeckle(M, black, white): the 8-connected black components with fewer than `black` pixels go, then
   the 4-connected white components with fewer than `white` pixels are filled; a size of 0 skips that colour.
3. on the result, every 8-connected black component with a bounding box of bh rows x bw columns (inclusive extents) and an area
   of a pixels becomes white where

       bh >= side   and   bw >= side   and   256 a >= fill bh bw

   in integers.  side == 0 skips the step.  `fill` is in 256ths of the box: a picture, a solid patch or a dark photograph fills its
   box; a frame, a table's grid or a large glyph does not.  A component that touches the page's edge is no exception."""
import numpy as np

from tests import despeckle_ref


def boxes(mask):
    """The 8-connected components of the True pixels of a bool H x W mask, in the order a row-major scan meets their first pixel:
    a list of (pixels [(y, x), ...], (y_min, y_max, x_min, x_max))."""
    out = []
    for comp in despeckle_ref.components(mask, despeckle_ref.NEIGHBOURS_8):
        ys, xs = [y for y, _ in comp], [x for _, x in comp]
        out.append((comp, (min(ys), max(ys), min(xs), max(xs))))
    return out


def is_blob(area, bh, bw, side, fill):
    """The rule of step 3 for one component, in Python's integers."""
    return bh >= side and bw >= side and 256 * area >= fill * bh * bw


def remove_blobs(mask, side, fill):
    """(the mask without its blobs, how many those were, how many pixels they had, their (y_min, y_max, x_min, x_max, area))."""
    mask = np.array(mask, bool)
    gone = pixels = 0
    found = []
    if side > 0:
        for comp, (y0, y1, x0, x1) in boxes(mask):
            if is_blob(len(comp), y1 - y0 + 1, x1 - x0 + 1, int(side), int(fill)):
                gone, pixels = gone + 1, pixels + len(comp)
                found.append((y0, y1, x0, x1, len(comp)))
                for y, x in comp:
                    mask[y, x] = False
    return mask, gone, pixels, found


def filter_ink(M, black, white, side, fill):
    """M: bool H x W, True = ink.  -> (the clean mask, the six counts)."""
    M = np.asarray(M, bool)
    assert M.ndim == 2
    step2, four = despeckle_ref.despeckle(M, black, white)
    clean, gone, pixels, _ = remove_blobs(step2, side, fill)
    return clean, tuple(four) + (gone, pixels)
