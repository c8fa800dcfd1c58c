"""The definition of the device JPEG encoder (yomitoku_amd/csrc/ymk_jpeg.hip), in plain NumPy / Python, written for clarity.

A helper like tests/overlay_ref.py: it shares no code with the product, and the device must equal it byte for byte.

File format: baseline sequential DCT, JFIF 1.01.  Colour pages (H x W x 3, B G R): three components, 4:2:0, MCU = 16 x 16
pixels, block order Y0 Y1 Y2 Y3 Cb Cr.  Grey pages (H x W): one component, MCU = 8 x 8.  Quantisation tables: Annex K scaled
by the IJG quality rule.  Huffman tables: Annex K.3 - K.6.  Restart interval = one MCU row, RSTm cycling mod 8.  Marker
order: SOI, APP0, DQT (luminance), DQT (chrominance), SOF0, DHT x 4 (DC 0, AC 0, DC 1, AC 1), DRI, SOS, scan, EOI; a grey file
has one DQT and the two luminance DHTs.

Pixel rules (all integer):
  1. edge replication: the page is extended to whole MCUs by repeating its last column and its last row;
  2. colour: Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
             Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
             Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16        (libjpeg's 16-bit tables, full range)
  3. chroma: the mean of each 2 x 2 square, (a + b + c + d + bias) >> 2 with bias 1 in even output columns and 2 in odd ones
     (libjpeg's alternating bias: no drift towards either side);
  4. samples minus 128, then libjpeg's `islow` forward DCT: 13-bit constants, two passes, rows first, the row pass keeping two
     extra bits; its output is 8 x the orthonormal DCT;
  5. quantisation: c = sign(v) * ((|v| + d / 2) // d) with the divisor d = 8 q; DC clamped to [-1024, 1023], AC to
     [-1023, 1023] (what the Huffman categories 11 / 10 can hold).

Rules 2 - 5 are libjpeg's; rule 1 is libjpeg's as well wherever a component's block count is even in both directions (libjpeg
fills a missing block of an MCU with the DC of its neighbour rather than with replicated pixels).  Where it is, the file
equals Pillow's `save(quality=q, restart_marker_rows=1)` (tests/test_jpeg_host.py reports it).
"""

from __future__ import annotations

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])

LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                   87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120,
                   101, 72, 92, 95, 98, 112, 100, 103, 99])
CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
                     99, 99, 99, 99] + [99] * 32)

# Annex K.3 - K.6: (number of codes of each length 1..16, the symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
            0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16,
            0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45,
            0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
            0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94,
            0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
            0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8,
            0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
            0xF9, 0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
              0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34,
              0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44,
              0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
              0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92,
              0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
              0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
              0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
              0xF9, 0xFA])


# --------------------------------------------------------------------------------------------------------------- tables
def quant_tables(quality: int):
    """(luminance, chrominance) in natural (row-major) order, int64 [64] each: the IJG rule."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (LUMA_Q, CHROMA_Q))


def huffman_codes(spec):
    """symbol -> (code, length), the canonical assignment of Annex C."""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


# --------------------------------------------------------------------------------------------------------------- pixels
def _fdct_pass(d, first: bool):
    """One pass of the islow DCT along the LAST axis of d (int64 [..., 8])."""
    c = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069,
             f2053=16819, f2562=20995, f3072=25172)
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    shift = 11 if first else 15          # CONST_BITS - PASS1_BITS | CONST_BITS + PASS1_BITS

    def descale(x, n):
        return (x + (1 << (n - 1))) >> n

    out = np.empty_like(d)
    if first:
        out[..., 0], out[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[..., 0], out[..., 4] = descale(t10 + t11, 2), descale(t10 - t11, 2)
    z1 = (t12 + t13) * c["f0541"]
    out[..., 2] = descale(z1 + t13 * c["f0765"], shift)
    out[..., 6] = descale(z1 - t12 * c["f1847"], shift)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * c["f1175"]
    t4, t5, t6, t7 = t4 * c["f0298"], t5 * c["f2053"], t6 * c["f3072"], t7 * c["f1501"]
    z1, z2, z3, z4 = -z1 * c["f0899"], -z2 * c["f2562"], -z3 * c["f1961"] + z5, -z4 * c["f0390"] + z5
    out[..., 7] = descale(t4 + z1 + z3, shift)
    out[..., 5] = descale(t5 + z2 + z4, shift)
    out[..., 3] = descale(t6 + z2 + z3, shift)
    out[..., 1] = descale(t7 + z1 + z4, shift)
    return out


def fdct(blocks):
    """int64 [..., 8, 8] samples (already minus 128) -> 8 x the DCT, rows first."""
    rows = _fdct_pass(blocks.astype(np.int64), True)
    return np.swapaxes(_fdct_pass(np.swapaxes(rows, -1, -2), False), -1, -2)


def _blocks_of(plane, q_natural):
    """int64 [h][w] samples (h, w multiples of 8) -> quantised, zig-zag int16 [h / 8][w / 8][64]."""
    h, w = plane.shape
    b = (plane - 128).reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2)
    v = fdct(b).reshape(h // 8, w // 8, 64)
    d = (q_natural * 8)[None, None, :]
    c = np.sign(v) * ((np.abs(v) + d // 2) // d)
    c[..., 1:] = np.clip(c[..., 1:], -1023, 1023)
    c[..., 0] = np.clip(c[..., 0], -1024, 1023)
    return c[..., ZIGZAG].astype(np.int16)


def planes(page):
    """The component planes of a page, extended to whole MCUs: [Y] for a grey page, [Y, Cb, Cr] (chroma at half size) else."""
    page = np.asarray(page)
    grey = page.ndim == 2
    m = 8 if grey else 16
    h, w = page.shape[:2]
    page = np.pad(page, ((0, -h % m), (0, -w % m)) + (() if grey else ((0, 0),)), mode="edge").astype(np.int64)
    if grey:
        return [page]
    b, g, r = page[..., 0], page[..., 1], page[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    out = [y]
    for c in (cb, cr):
        s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
        bias = 1 + (np.arange(s.shape[1]) & 1)
        out.append((s + bias[None, :]) >> 2)
    return out


def coefficients(page, quality: int):
    """Zig-zag int16 [blocks][64] in scan order: MCU rows top to bottom, MCUs left to right, Y0 Y1 Y2 Y3 Cb Cr inside one."""
    ql, qc = quant_tables(quality)
    p = planes(page)
    if len(p) == 1:
        return _blocks_of(p[0], ql).reshape(-1, 64)
    y, cb, cr = _blocks_of(p[0], ql), _blocks_of(p[1], qc), _blocks_of(p[2], qc)
    mh, mw = cb.shape[:2]
    out = np.empty((mh, mw, 6, 64), np.int16)
    out[:, :, 0], out[:, :, 1] = y[0::2, 0::2], y[0::2, 1::2]
    out[:, :, 2], out[:, :, 3] = y[1::2, 0::2], y[1::2, 1::2]
    out[:, :, 4], out[:, :, 5] = cb, cr
    return out.reshape(-1, 64)


# --------------------------------------------------------------------------------------------------------------- entropy
class _Bits:
    """A bit string, most significant bit first, kept as one Python integer (an interval is a few thousand bytes)."""

    def __init__(self):
        self.value, self.length = 0, 0

    def put(self, code, length):
        self.value = self.value << length | code
        self.length += length

    def stuffed_bytes(self) -> bytes:
        """Padded with 1-bits to a byte, every FF followed by 00."""
        pad = -self.length % 8
        self.put((1 << pad) - 1, pad)
        return self.value.to_bytes(self.length // 8, "big").replace(b"\xff", b"\xff\x00")


def _magnitude(v):
    """(category, the category's low bits) of a coefficient or DC difference."""
    cat = int(abs(v)).bit_length()
    return cat, (v if v >= 0 else v - 1) & ((1 << cat) - 1)


def encode_interval(blocks, components, dc_tables, ac_tables) -> bytes:
    """The stuffed bytes of one restart interval: blocks int [n][64] zig-zag, components [n] (0 luminance, 1 Cb, 2 Cr)."""
    out = _Bits()
    pred = [0, 0, 0]
    for blk, comp in zip(np.asarray(blocks), components):
        dc, ac = dc_tables[min(comp, 1)], ac_tables[min(comp, 1)]
        cat, low = _magnitude(int(blk[0]) - pred[comp])
        pred[comp] = int(blk[0])
        out.put(*dc[cat])
        out.put(low, cat)
        last = 0  # zig-zag index of the previous non-zero coefficient
        for k in (np.flatnonzero(blk[1:]) + 1).tolist():
            run = k - last - 1
            while run > 15:  # ZRL: sixteen zeros
                out.put(*ac[0xF0])
                run -= 16
            cat, low = _magnitude(int(blk[k]))
            out.put(*ac[run << 4 | cat])
            out.put(low, cat)
            last = k
        if last < 63:  # EOB: the rest is zero
            out.put(*ac[0x00])
    return out.stuffed_bytes()


def _segment(marker, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(height, width, grey, quality) -> bytes:
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += _segment(0xDB, bytes([0]) + bytes(ql[ZIGZAG].tolist()))
    if not grey:
        out += _segment(0xDB, bytes([1]) + bytes(qc[ZIGZAG].tolist()))
    comps = [(1, 0x11, 0)] if grey else [(1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)]
    out += _segment(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([len(comps)]) +
                    b"".join(bytes(c) for c in comps))
    tables = [(0x00, DC_LUMA), (0x10, AC_LUMA)] + ([] if grey else [(0x01, DC_CHROMA), (0x11, AC_CHROMA)])
    for ident, (bits, vals) in tables:
        out += _segment(0xC4, bytes([ident]) + bytes(bits) + bytes(vals))
    m = 8 if grey else 16
    out += _segment(0xDD, (-(-width // m)).to_bytes(2, "big"))
    scan = [(1, 0x00)] if grey else [(1, 0x00), (2, 0x11), (3, 0x11)]
    out += _segment(0xDA, bytes([len(scan)]) + b"".join(bytes(c) for c in scan) + bytes([0, 63, 0]))
    return out


def assemble(coefs, height, width, grey, quality) -> bytes:
    """The file from its coefficients (int16 [blocks][64], as `coefficients` orders them)."""
    m, per = (8, 1) if grey else (16, 6)
    mw, mh = -(-width // m), -(-height // m)
    coefs = np.asarray(coefs).reshape(mh, mw * per, 64)
    comps = [0] * (mw * per) if grey else [0, 0, 0, 0, 1, 2] * mw
    dc = [huffman_codes(DC_LUMA), huffman_codes(DC_CHROMA)]
    ac = [huffman_codes(AC_LUMA), huffman_codes(AC_CHROMA)]
    out = bytearray(header(height, width, grey, quality))
    for r in range(mh):
        out += encode_interval(coefs[r], comps, dc, ac)
        if r + 1 < mh:
            out += bytes([0xFF, 0xD0 + (r & 7)])
    return bytes(out + b"\xff\xd9")


def encode(page, quality: int) -> bytes:
    page = np.asarray(page)
    h, w = page.shape[:2]
    return assemble(coefficients(page, quality), h, w, page.ndim == 2, quality)
