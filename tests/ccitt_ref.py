"""The definition of the device's CCITT Group 4 (ITU-T T.6) encoder for two-valued pages (yomitoku_amd/ccitt.py,
yomitoku_amd/csrc/ymk_ccitt.hip), in plain NumPy / Python.  A helper like tests/jpeg_modes_ref.py: it shares no code with the
product, and the device must equal it bit for bit; tests/test_ccitt_host.py holds it to libtiff's Group 4 strips.

A page is two-valued when every sample is 0 or 255 and, with three channels, B == G == R everywhere.  A sample of 0 is black.
The stream: every row coded against the row above (row 0 against an all-white row), the codes MSB first in each byte, rows not
byte-aligned, then EOFB (000000000001 twice) and zero bits up to a whole byte.

A row: a0 starts before column 0 with colour white.  a1 is the next change of the coding row beyond a0, a2 the change after a1;
b1 the first change of the reference row beyond a0 to the colour opposite a0's, b2 the change after b1; a missing change is w.
  b2 < a1          pass       0001                                    a0 = b2, colour kept
  |a1 - b1| <= 3   vertical   V0 1, VR1-3 011 000011 0000011,        a0 = a1, colour flips
                              VL1-3 010 000010 0000010 (VR: a1 right of b1)
  otherwise        horizontal 001 + run a0a1 + run a1a2               a0 = a2   (the first run is counted from column 0)
until a0 >= w.  A run n: while n >= 2624 the code of 2560; then, if n >= 64, the make-up code of 64 (n >> 6); then the
terminating code of what is left.
"""

from __future__ import annotations

import struct

import numpy as np


def _table(text):
    return [(int(b), int(c, 16)) for b, c in (item.split(",") for item in text.strip("()").split(")("))]


# (bits, code), index = run length (terminating) or run length / 64 - 1 (make-up)
WHITE_TERM = _table(
    "(8,35)(6,07)(4,7)(4,8)(4,B)(4,C)(4,E)(4,F)(5,13)(5,14)(5,07)(5,08)(6,08)(6,03)(6,34)(6,35)(6,2A)(6,2B)(7,27)(7,0C)(7,08)(7,17)"
    "(7,03)(7,04)(7,28)(7,2B)(7,13)(7,24)(7,18)(8,02)(8,03)(8,1A)(8,1B)(8,12)(8,13)(8,14)(8,15)(8,16)(8,17)(8,28)(8,29)(8,2A)(8,2B)"
    "(8,2C)(8,2D)(8,04)(8,05)(8,0A)(8,0B)(8,52)(8,53)(8,54)(8,55)(8,24)(8,25)(8,58)(8,59)(8,5A)(8,5B)(8,4A)(8,4B)(8,32)(8,33)(8,34)")
WHITE_MAKEUP = _table(
    "(5,1B)(5,12)(6,17)(7,37)(8,36)(8,37)(8,64)(8,65)(8,68)(8,67)(9,CC)(9,CD)(9,D2)(9,D3)(9,D4)(9,D5)(9,D6)(9,D7)(9,D8)(9,D9)(9,DA)"
    "(9,DB)(9,98)(9,99)(9,9A)(6,18)(9,9B)")
BLACK_TERM = _table(
    "(10,37)(3,2)(2,3)(2,2)(3,3)(4,3)(4,2)(5,03)(6,05)(6,04)(7,04)(7,05)(7,07)(8,04)(8,07)(9,18)(10,17)(10,18)(10,08)(11,67)(11,68)"
    "(11,6C)(11,37)(11,28)(11,17)(11,18)(12,CA)(12,CB)(12,CC)(12,CD)(12,68)(12,69)(12,6A)(12,6B)(12,D2)(12,D3)(12,D4)(12,D5)(12,D6)"
    "(12,D7)(12,6C)(12,6D)(12,DA)(12,DB)(12,54)(12,55)(12,56)(12,57)(12,64)(12,65)(12,52)(12,53)(12,24)(12,37)(12,38)(12,27)(12,28)"
    "(12,58)(12,59)(12,2B)(12,2C)(12,5A)(12,66)(12,67)")
BLACK_MAKEUP = _table(
    "(10,0F)(12,C8)(12,C9)(12,5B)(12,33)(12,34)(12,35)(13,6C)(13,6D)(13,4A)(13,4B)(13,4C)(13,4D)(13,72)(13,73)(13,74)(13,75)(13,76)"
    "(13,77)(13,52)(13,53)(13,54)(13,55)(13,5A)(13,5B)(13,64)(13,65)")
EXTENDED_MAKEUP = _table("(11,08)(11,0C)(11,0D)(12,12)(12,13)(12,14)(12,15)(12,16)(12,17)(12,1C)(12,1D)(12,1E)(12,1F)")  # 1792 - 2560
assert [len(t) for t in (WHITE_TERM, WHITE_MAKEUP, BLACK_TERM, BLACK_MAKEUP, EXTENDED_MAKEUP)] == [64, 27, 64, 27, 13]

PASS = (4, 1)
HORIZONTAL = (3, 1)
VERTICAL = {0: (1, 1), 1: (3, 3), 2: (6, 3), 3: (7, 3), -1: (3, 2), -2: (6, 2), -3: (7, 2)}  # a1 - b1 -> code
EOFB = (24, 0x001001)


def run_codes(n, black):
    """The codes, [(bits, code)], of a run of n pixels of that colour."""
    term, makeup = (BLACK_TERM, BLACK_MAKEUP) if black else (WHITE_TERM, WHITE_MAKEUP)
    out = []
    while n >= 2624:
        out.append(EXTENDED_MAKEUP[-1])
        n -= 2560
    if n >= 64:
        k = n >> 6
        out.append(makeup[k - 1] if k <= 27 else EXTENDED_MAKEUP[k - 28])
        n -= k << 6
    out.append(term[n])
    return out


def _next(row, start, value, w):
    """The first column >= start at which `row` is `value`; w where there is none."""
    hit = np.flatnonzero(row[start:] == value) if start < w else ()
    return start + int(hit[0]) if len(hit) else w


def row_steps(cur, ref):
    """The steps of the row `cur` (bool, True = black) against the row `ref`: ("pass",), ("vertical", a1 - b1) or
    ("horizontal", run a0a1, run a1a2, whether the first run is black)."""
    w = len(cur)
    ref_change = np.empty(w, bool)
    ref_change[0] = ref[0]
    ref_change[1:] = ref[1:] != ref[:-1]
    out, a0, colour = [], -1, False
    while a0 < w:
        a1 = _next(cur, a0 + 1, not colour, w)
        b1 = _next(ref_change & (ref != colour), a0 + 1, True, w)
        b2 = _next(ref, b1 + 1, colour, w)
        if b2 < a1:
            out.append(("pass",))
            a0 = b2
        elif abs(a1 - b1) <= 3:
            out.append(("vertical", a1 - b1))
            a0, colour = a1, not colour
        else:
            a2 = _next(cur, a1 + 1, colour, w)
            out.append(("horizontal", a1 - max(a0, 0), a2 - a1, colour))
            a0 = a2
    return out


def row_codes(cur, ref):
    """The codes, [(bits, code)], of the row `cur` against the row `ref`."""
    out = []
    for step in row_steps(cur, ref):
        if step[0] == "pass":
            out.append(PASS)
        elif step[0] == "vertical":
            out.append(VERTICAL[step[1]])
        else:
            out.append(HORIZONTAL)
            out += run_codes(step[1], step[3])
            out += run_codes(step[2], not step[3])
    return out


def pack_codes(codes) -> tuple:
    """(the codes' bits as bytes - MSB first, zero-padded to a byte -, their number of bits)."""
    bits = []
    for n, code in codes:
        bits.extend((code >> (n - 1 - k)) & 1 for k in range(n))
    return np.packbits(np.array(bits, np.uint8)).tobytes(), len(bits)


def encode_rows(black):
    """Per row of `black` (H x W bool, True = black) its (bytes, bit count), each row's bits on their own."""
    black = np.asarray(black, bool)
    above = np.zeros(black.shape[1], bool)
    out = []
    for row in black:
        out.append(pack_codes(row_codes(row, above)))
        above = row
    return out


def encode_g4(black) -> bytes:
    """The T.6 stream of a page: `black` is H x W, True (non-zero) = black."""
    black = np.asarray(black, bool)
    codes = []
    above = np.zeros(black.shape[1], bool)
    for row in black:
        codes += row_codes(row, above)
        above = row
    codes.append(EOFB)
    return pack_codes(codes)[0]


def is_bilevel(page) -> bool:
    """Whether a uint8 page, H x W or H x W x 3, is two-valued: every sample 0 or 255 and, of three channels, B == G == R."""
    page = np.asarray(page)
    if page.dtype != np.uint8 or page.ndim not in (2, 3) or (page.ndim == 3 and page.shape[2] != 3):
        return False
    if not bool(((page == 0) | (page == 255)).all()):
        return False
    return page.ndim == 2 or bool((page[..., 0] == page[..., 1]).all() and (page[..., 1] == page[..., 2]).all())


def black_mask(page):
    """H x W bool, True = black (a sample of 0), of a two-valued page."""
    page = np.asarray(page)
    return (page if page.ndim == 2 else page[..., 0]) == 0


def pack_rows(black):
    """The device's packed rows: uint32 [H][ceil(W / 32)], 1 = black, the leftmost pixel of a word in its bit 31."""
    black = np.asarray(black, bool)
    h, w = black.shape
    padded = np.zeros((h, -(-w // 32) * 32), np.uint8)
    padded[:, :w] = black
    return np.packbits(padded, axis=1).view(">u4").astype(np.uint32).reshape(h, -1)


def to_tiff(data: bytes, width: int, height: int) -> bytes:
    """A minimal little-endian TIFF with the stream as its single Group 4 strip, MinIsWhite."""
    tags = [(256, 4, width), (257, 4, height), (258, 3, 1), (259, 3, 4), (262, 3, 0), (273, 4, 0), (277, 3, 1), (278, 4, height),
            (279, 4, len(data)), (293, 4, 0)]
    at = 8 + 2 + 12 * len(tags) + 4
    out = struct.pack("<2sHI", b"II", 42, 8) + struct.pack("<H", len(tags))
    for tag, kind, value in tags:
        value = at if tag == 273 else value
        out += struct.pack("<HHI", tag, kind, 1) + (struct.pack("<I", value) if kind == 4 else struct.pack("<HH", value, 0))
    return out + struct.pack("<I", 0) + data
