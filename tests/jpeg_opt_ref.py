"""The definition of the device encoder's optimised Huffman tables (`encode_jpeg_pages(..., optimize=True)`), in plain NumPy /
Python.  A helper like tests/jpeg_ref.py, whose coefficients, interval coder and segments it uses: it shares no code with the
product, and the device must equal it byte for byte.

The file is tests/jpeg_ref.py's with each DHT segment's payload replaced by a table made for THIS page: same pixels, same
coefficients, same markers in the same order, shorter codes.

Histograms.  Up to four per page - DC and AC of the luminance, DC and AC of the chrominance (Cb and Cr share theirs; a grey page
has the luminance pair only).  Every symbol `jpeg_ref.encode_interval` would emit is counted: the DC category of each block
(predictor 0 at the start of every restart interval), `run << 4 | category` per non-zero AC coefficient, 0xF0 per sixteen zeros
before one, 0x00 for an end-of-block.

Table from a histogram: libjpeg's rule (jpeg_gen_optimal_table).
  1. a reserved 257th symbol (index 256) gets frequency 1, so that no real symbol gets the all-ones code;
  2. repeat: c1 = the symbol with the smallest non-zero frequency, among equals the LARGEST index; c2 the same over the rest;
     stop when there is no c2; c1's frequency += c2's, c2's = 0; every symbol of either subtree gets one bit longer and the two
     subtrees become one;
  3. count the codes of each length;
  4. limit to 16 bits (Annex K.3, Figure K.3): for i from the longest length down to 17, while bits[i] > 0: j = the largest
     length below i - 1 in use; bits[i] -= 2, bits[i - 1] += 1, bits[j + 1] += 2, bits[j] -= 1.  (libjpeg stops with an error
     above 32 bits; the loop here starts at whatever the longest length is, the same thing wherever libjpeg has an answer.)
  5. one code less at the longest length in use: the reserved symbol's;
  6. the symbols by (code length before limiting, value), ascending.
A histogram without a symbol gives a table without a code.  Codes: Annex C (`jpeg_ref.huffman_codes`).
"""

from __future__ import annotations

import numpy as np

from tests import jpeg_ref


def _layout(height, width, grey):
    m, per = (8, 1) if grey else (16, 6)
    mw, mh = -(-width // m), -(-height // m)
    comps = [0] * mw if grey else [0, 0, 0, 0, 1, 2] * mw
    return mw, mh, per, comps


def histograms(coefs, height, width, grey):
    """(dc, ac): int64 [2][16] and [2][256], index 0 luminance, 1 chrominance, of the file `jpeg_ref.assemble` would code."""
    mw, mh, per, comps = _layout(height, width, grey)
    coefs = np.asarray(coefs).reshape(mh, mw * per, 64)
    dc, ac = np.zeros((2, 16), np.int64), np.zeros((2, 256), np.int64)
    for row in coefs:
        pred = [0, 0, 0]
        for blk, comp in zip(row, comps):
            t = min(comp, 1)
            dc[t, int(abs(int(blk[0]) - pred[comp])).bit_length()] += 1
            pred[comp] = int(blk[0])
            last = 0
            for k in (np.flatnonzero(blk[1:]) + 1).tolist():
                run = k - last - 1
                while run > 15:
                    ac[t, 0xF0] += 1
                    run -= 16
                ac[t, run << 4 | int(abs(int(blk[k]))).bit_length()] += 1
                last = k
            if last < 63:
                ac[t, 0x00] += 1
    return dc, ac


def code_sizes(freq):
    """Step 2: the code length of each of the 257 symbols (0: absent) before limiting."""
    freq = [int(f) for f in freq] + [0] * (256 - len(freq)) + [1]
    size, tree = [0] * 257, list(range(257))
    while True:
        c1 = c2 = -1
        v = None
        for i in range(257):
            if freq[i] and (v is None or freq[i] <= v):
                v, c1 = freq[i], i
        v = None
        for i in range(257):
            if freq[i] and i != c1 and (v is None or freq[i] <= v):
                v, c2 = freq[i], i
        if c2 < 0:
            return size
        freq[c1] += freq[c2]
        freq[c2] = 0
        t1, t2 = tree[c1], tree[c2]
        for i in range(257):
            if tree[i] in (t1, t2):
                size[i] += 1
                tree[i] = t1


def optimal_table(freq):
    """(bits [16], vals) - the form of jpeg_ref.DC_LUMA - from the frequencies of up to 256 symbols."""
    if not any(int(f) for f in freq):
        return [0] * 16, []
    size = code_sizes(freq)
    longest = max(size)
    bits = [0] * (max(longest, 16) + 1)
    for s in size:
        if s:
            bits[s] += 1
    for i in range(longest, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [s for _, s in sorted((size[s], s) for s in range(256) if size[s])]
    return bits[1:17], vals


def page_tables(coefs, height, width, grey):
    """[(DHT identifier, (bits, vals))] in the file's order: DC 0, AC 0, then DC 1, AC 1 of a colour page."""
    dc, ac = histograms(coefs, height, width, grey)
    out = [(0x00, optimal_table(dc[0])), (0x10, optimal_table(ac[0]))]
    if not grey:
        out += [(0x01, optimal_table(dc[1])), (0x11, optimal_table(ac[1]))]
    return out


def dht_segments(tables) -> bytes:
    return b"".join(jpeg_ref._segment(0xC4, bytes([ident]) + bytes(bits) + bytes(vals)) for ident, (bits, vals) in tables)


def lut_words(tables):
    """The device's table of a page: uint32 [2][256 + 16], symbol -> code | length << 16, AC entries first, 0 where absent."""
    out = np.zeros((2, 272), np.uint32)
    for ident, spec in tables:
        for sym, (code, length) in jpeg_ref.huffman_codes(spec).items():
            out[ident & 1, sym + (0 if ident >> 4 else 256)] = code | length << 16
    return out


def header(height, width, grey, quality, tables) -> bytes:
    plain = jpeg_ref.header(height, width, grey, quality)
    at, first, dri = 2, None, None  # walk the segments behind SOI
    while at < len(plain):
        if plain[at + 1] == 0xC4 and first is None:
            first = at
        if plain[at + 1] == 0xDD:
            dri = at
        at += 2 + int.from_bytes(plain[at + 2 : at + 4], "big")
    return plain[:first] + dht_segments(tables) + plain[dri:]


def assemble(coefs, height, width, grey, quality, tables=None) -> bytes:
    """The file from its coefficients; tables: default the page's own optimal ones."""
    mw, mh, per, comps = _layout(height, width, grey)
    if tables is None:
        tables = page_tables(coefs, height, width, grey)
    codes = {ident: jpeg_ref.huffman_codes(spec) for ident, spec in tables}
    dc, ac = [codes[0x00], codes.get(0x01)], [codes[0x10], codes.get(0x11)]
    coefs = np.asarray(coefs).reshape(mh, mw * per, 64)
    out = bytearray(header(height, width, grey, quality, tables))
    for r in range(mh):
        out += jpeg_ref.encode_interval(coefs[r], comps, dc, ac)
        if r + 1 < mh:
            out += bytes([0xFF, 0xD0 + (r & 7)])
    return bytes(out + b"\xff\xd9")


def encode(page, quality: int) -> bytes:
    page = np.asarray(page)
    h, w = page.shape[:2]
    return assemble(jpeg_ref.coefficients(page, quality), h, w, page.ndim == 2, quality)
