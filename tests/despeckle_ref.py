"""The definition of despeckling (yomitoku_amd/despeckle.py; yomitoku_amd/csrc/ymk_cc.hip; DESIGN.md, "Despeckled pages"): plain
NumPy and Python, a literal flood fill with an explicit stack.  The device equals it bit for bit, in the mask and in the counts;
tests/test_despeckle_host.py holds it to scipy.ndimage.label.

    clean, (black_components, black_pixels, white_components, white_pixels) = despeckle(black, n_black, n_white)

1. the 8-connected components of the True (black) pixels: every one with fewer than n_black pixels becomes False;
2. on the result of 1, the 4-connected components of the False (white) pixels: every one with fewer than n_white pixels becomes
   True.

n == 0 leaves that colour alone.  There is no exception for a component that touches the page's border: a 1 x 1 white page with
n_white = 4 becomes black.  8 for black and 4 for white is the usual dual pairing: a diagonal stroke is one object and the two
sides of it are separate holes.  Two passes, in this order, the second on the result of the first: removing a speck can only
merge white regions, never make a small one."""
import numpy as np

NEIGHBOURS_8 = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
NEIGHBOURS_4 = ((-1, 0), (0, -1), (0, 1), (1, 0))


def components(mask, neighbours):
    """The connected components of the True pixels of a bool H x W mask under `neighbours`: a list of lists of (y, x), in the
    order a row-major scan meets their first pixel."""
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    todo = [bytearray(row) for row in mask.astype(np.uint8)]  # Python's own containers: a pixel is 1 until the fill has taken it
    out = []
    for y0 in range(h):
        for x0 in range(w):
            if not todo[y0][x0]:
                continue
            todo[y0][x0] = 0
            stack, pixels = [(y0, x0)], []
            while stack:
                y, x = stack.pop()
                pixels.append((y, x))
                for dy, dx in neighbours:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w and todo[yy][xx]:
                        todo[yy][xx] = 0
                        stack.append((yy, xx))
            out.append(pixels)
    return out


def remove_small(mask, n, neighbours):
    """(the mask without its components of fewer than n pixels, how many those were, how many pixels they had)."""
    mask = np.array(mask, bool)
    gone = pixels = 0
    if n > 0:
        for comp in components(mask, neighbours):
            if len(comp) < n:
                gone, pixels = gone + 1, pixels + len(comp)
                for y, x in comp:
                    mask[y, x] = False
    return mask, gone, pixels


def despeckle(black, n_black, n_white):
    """black: bool H x W, True = black.  -> (the clean mask, (black components removed, their pixels, white components filled,
    their pixels))."""
    black = np.asarray(black, bool)
    assert black.ndim == 2
    step1, bc, bp = remove_small(black, int(n_black), NEIGHBOURS_8)
    white, wc, wp = remove_small(~step1, int(n_white), NEIGHBOURS_4)
    return ~white, (bc, bp, wc, wp)


def golden_page(path):
    """The golden page taken as grey, uint8 842 x 596 (Pillow's `convert("L")`, as tests/test_deskew_host.py builds it)."""
    from PIL import Image

    return np.asarray(Image.open(path).convert("L"))


def noisy_page(img):
    """A scan's noise on a grey page, seeded: Gaussian grain of sigma 12 on every pixel, then dust - one pixel in 500 replaced by
    a dark value below 90."""
    rng = np.random.default_rng(0)
    noisy = np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)
    dust = rng.random(img.shape) < 0.002
    return np.where(dust, rng.integers(0, 90, img.shape), noisy).astype(np.uint8)
