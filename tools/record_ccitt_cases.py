"""Record tests/golden/ccitt_g4_cases.npz: two-valued pages and the Group 4 strips libtiff (through Pillow) writes for them -
what tests/test_ccitt_host.py holds the definition, tests/ccitt_ref.py, to, and tests/test_ccitt_gpu.py the device to.

    python tools/record_ccitt_cases.py            # needs Pillow with libtiff

Per case `name`: `<name>.shape` (h, w), `<name>.bits` (np.packbits of the rows, 1 = black, each row padded to a byte) and
`<name>.strip` (the strip's bytes).
"""
import io
import os
import sys

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "ccitt_g4_cases.npz")


def libtiff_strip(black) -> bytes:
    """libtiff's Group 4 strip of a page (H x W bool, True = black), all rows in one strip."""
    black = np.ascontiguousarray(black, dtype=bool)
    buf = io.BytesIO()
    Image.fromarray(black).save(buf, "TIFF", compression="group4", tiffinfo={278: black.shape[0]})
    buf.seek(0)
    tags = Image.open(buf).tag_v2
    (at,), (n,) = tags[273], tags[279]
    return buf.getvalue()[at : at + n]


def runs_page(pairs, tail=4):
    """Two rows, the first white: the second is, per (white, black) of `pairs`, that white run and that black run, then `tail`
    white pixels.  Against the white row every pair is coded in horizontal mode."""
    row = []
    for white, black in pairs:
        row += [False] * white + [True] * black
    row += [False] * tail
    page = np.zeros((2, len(row)), bool)
    page[1] = row
    return page


def drift_page(h=38, w=150):
    """Strokes whose edges move by -4 ... +4 columns from row to row (every vertical code, horizontal mode at 4), one stroke
    that ends half way down and one that begins there (pass codes, a run that appears)."""
    page = np.zeros((h, w), bool)
    left, steps = 60, [0, 1, -1, 2, -2, 3, -3, 4, -4]
    for y in range(h):
        left += steps[y % len(steps)]
        page[y, left : left + 7] = True
        page[y, 100 + (y % 5) : 104 + 2 * (y % 3)] = True
        if y < h // 2:
            page[y, 10:14] = True
            page[y, 130:131] = True
        else:
            page[y, 20:29] = True
    return page


def long_runs(h, w, seed):
    """Rows of a few runs each, with lengths round 1792, 2560 and 2624, the multiples of 64 between and the whole row."""
    rng = np.random.default_rng(seed)
    page = np.zeros((h, w), bool)
    marks = [1791, 1792, 1793, 2559, 2560, 2561, 2623, 2624, 2625, 2687, 2688]
    for y in range(h):
        at, black = 0, bool(y & 1)
        while at < w:
            n = int(rng.choice(marks)) if rng.random() < 0.8 else int(rng.integers(1, 40))
            page[y, at : at + n] = black
            at, black = at + n, not black
    return page


def cases():
    rng = np.random.default_rng(20240607)
    out = {}
    for h, w in ((1, 1), (1, 7), (2, 31), (3, 32), (3, 33), (2, 63), (5, 64), (4, 65), (9, 100)):
        out[f"noise_{h}x{w}"] = rng.random((h, w)) < 0.5
    out["black_1x1"] = np.ones((1, 1), bool)
    for density in (0.05, 0.5, 0.95):
        out[f"noise_40x300_{int(density * 100):02d}"] = rng.random((40, 300)) < density
    out["white_70x33"] = np.zeros((70, 33), bool)
    out["black_70x33"] = np.ones((70, 33), bool)
    out["drift"] = drift_page()
    out["long_3x2700"] = long_runs(3, 2700, 1)
    out["long_2x5300"] = long_runs(2, 5300, 2)
    page = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "test_page.jpg")).convert("L"))
    out["golden_crop"] = page[150:450, 100:500] < 128
    # two-row pages that between them use every terminating and every make-up code of both colours
    out["terminating"] = runs_page([(k, k) for k in range(1, 64)])
    out["white_run_0"] = runs_page([(0, 5), (9, 2)])
    black_to_the_end = np.zeros((2, 12), bool)
    black_to_the_end[0, 2:] = True  # b1 = 2, b2 = w, a1 = w: horizontal, a white run of 12 and a black run of 0
    out["black_run_0"] = black_to_the_end
    for k in range(1, 41, 3):  # 64 k ... 64 (k + 2), a terminating code of 0 behind each
        out[f"makeup_{64 * k}"] = runs_page([(64 * j, 64 * j) for j in range(k, min(k + 3, 41))])
    out["makeup_2560_twice"] = runs_page([(2560 + 2560 + 70, 2560 + 2624)])
    return out


def main():
    if not features.check("libtiff"):
        sys.exit("Pillow has no libtiff: nothing to record against")
    arrays = {}
    for name, black in cases().items():
        arrays[name + ".shape"] = np.array(black.shape, np.int32)
        arrays[name + ".bits"] = np.packbits(black, axis=1)
        arrays[name + ".strip"] = np.frombuffer(libtiff_strip(black), np.uint8)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes,", len(arrays) // 3, "cases")


if __name__ == "__main__":
    main()
