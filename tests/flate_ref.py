"""The definition of the lossless page files (yomitoku_amd/flate.py; yomitoku_amd/csrc/ymk_flate.hip; DESIGN.md, "Lossless pages"):
plain NumPy / Python, the thing the device equals byte for byte.  A file is a zlib stream (RFC 1950) of the page's PNG-filtered
rows in ONE final dynamic-Huffman Deflate block (RFC 1951), so `zlib.decompress` gives the filtered rows back, the stream is a
PNG's IDAT as it is, and a PDF's /FlateDecode with /Predictor 15 reads the same bytes.

1. Samples.  Rows of R G B bytes (a page arrives B G R: the swap is part of the definition) or of one grey byte.
2. Filter.  Every row under PNG filter types 0-4 (left / up / up-left are 0 outside the page); a candidate's cost is the sum of
   abs(int8(byte)); the smallest cost wins, a tie goes to the smallest type.  A filtered row: the type byte, then the bytes.
3. Segments.  A filtered row is cut into consecutive segments of at most SEGMENT bytes; no match reaches outside its segment.
4. Matches.  At position i of a segment, for each distance d of DISTANCES with i >= d, L_d(i) = the number of positions k = i,
   i + 1, ... with b[k] == b[k - d], capped at 258 and at the segment's end.  The longest wins, a tie goes to the smallest d.
   The parse is greedy from the segment's start: a match where the best length is >= 3 (then skip it), else a literal.
   A token is a uint16: the literal's byte, or 0x8000 | index of d << 9 | length - 3.
5. Tables.  Per page the histogram of the literal / length symbols (286; end-of-block counted once) and of the distance symbols
   (30).  `huff_lengths(freq, limit)`: no used symbol: no code; one: length 1; else libjpeg's merge rule - repeatedly the
   smallest non-zero frequency c1 (among equals the LARGEST symbol), the next smallest c2 likewise; c1 takes the sum, c2 goes to
   zero, every symbol below either is one bit longer - then Figure K.3's limiter of ITU-T T.81 with `limit` in place of 16 (no
   reserved code point: the Kraft sum stays 1), then the counts per length handed out to the symbols in the order (length before
   limiting, symbol).  limit 15 for both alphabets, 7 for the code-length alphabet.  A page with no match declares distance
   symbol 0 with length 1.  Codes are canonical (RFC 1951, 3.2.2).
   The header's code lengths - HLIT literal / length ones, then HDIST distance ones, one sequence - are run-length coded by a
   greedy rule, from the front: at a value v with r equal values from here on: v == 0 and r >= 3: symbol 18 (r >= 11) or 17 for
   min(r, 138) of them; else v equal to the value before it and r >= 3: symbol 16 for min(r, 6); else v itself.  HLIT = max(257,
   the last used symbol + 1), HDIST = max(1, ...), HCLEN = max(4, the last used place in RFC 1951's order + 1).
6. Stream.  78 9C, the block (BFINAL 1, BTYPE 2: header, the segments' tokens in order, end-of-block), zero bits to a byte, the
   Adler-32 of all filtered bytes, high byte first.
"""

import struct
import zlib

import numpy as np

SEGMENT = 8192
DISTANCES = (1, 2, 3, 4, 6, 8)
MAX_MATCH, MIN_MATCH = 258, 3
N_LIT, N_DIST, N_CL = 286, 30, 19
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
HEADER_BITS_MAX = 3 + 14 + 3 * N_CL + (N_LIT + N_DIST) * (7 + 7)  # every code length its own symbol of 7 bits with 7 extra bits


def file_capacity(h: int, w: int, c: int) -> int:
    """The bytes no file of an h x w x c page exceeds.  Proof: a literal costs at most 15 bits for its byte; a match costs at most
    15 + 5 bits for its length and 15 + 1 for its distance (the distances up to 8 have at most one extra bit), 36 bits for at
    least 3 bytes; so the tokens cost at most 15 bits a filtered byte, end-of-block 15, the header HEADER_BITS_MAX; the zlib
    header is 2 bytes, the pad below one, the checksum 4."""
    n = h * (1 + w * c)
    return 2 + (HEADER_BITS_MAX + 15 * n + 15 + 7) // 8 + 4


# ------------------------------------------------------------------------------------------------ 1, 2: samples, filter
def samples(page: np.ndarray) -> np.ndarray:
    """h x (w * c) bytes: R G B of a B G R page, or the grey plane."""
    page = np.asarray(page)
    assert page.dtype == np.uint8 and (page.ndim == 2 or (page.ndim == 3 and page.shape[2] == 3))
    if page.ndim == 3:
        page = page[:, :, ::-1]
    return np.ascontiguousarray(page).reshape(page.shape[0], -1)


def _paeth(a, b, c):
    a, b, c = a.astype(np.int32), b.astype(np.int32), c.astype(np.int32)
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c)).astype(np.uint8)


def filter_rows(rows: np.ndarray, bpp: int):
    """(the filtered rows, h x (1 + w c) bytes; the filter types, h)."""
    h, n = rows.shape
    out = np.zeros((h, 1 + n), np.uint8)
    types = np.zeros(h, np.int32)
    zero = np.zeros(n, np.uint8)
    for y in range(h):
        cur = rows[y]
        up = rows[y - 1] if y else zero
        left = np.concatenate([np.zeros(bpp, np.uint8), cur[:-bpp]]) if n > bpp else np.zeros(n, np.uint8)
        upleft = np.concatenate([np.zeros(bpp, np.uint8), up[:-bpp]]) if n > bpp else np.zeros(n, np.uint8)
        cands = [cur, cur - left, cur - up, cur - ((left.astype(np.int32) + up.astype(np.int32)) >> 1).astype(np.uint8),
                 cur - _paeth(left, up, upleft)]
        costs = [int(np.abs(c.view(np.int8).astype(np.int32)).sum()) for c in cands]
        t = int(np.argmin(costs))  # the first of equals
        types[y] = t
        out[y, 0] = t
        out[y, 1:] = cands[t]
    return out, types


# ------------------------------------------------------------------------------------------------ 3, 4: segments, matches
def segments_of(filtered: np.ndarray):
    """The segments of all rows, in order, as byte arrays."""
    segs = []
    for row in filtered:
        for at in range(0, len(row), SEGMENT):
            segs.append(row[at : at + SEGMENT])
    return segs


def best_matches(seg: np.ndarray):
    """(best length, index of its distance) at every position of a segment."""
    n = len(seg)
    best, which = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for j, d in enumerate(DISTANCES):
        if n <= d:
            continue
        eq = np.zeros(n, bool)
        eq[d:] = seg[d:] == seg[:-d]
        at = np.arange(n)
        stop = np.minimum.accumulate(np.where(eq, n, at)[::-1])[::-1]  # the first position from i on that does not repeat
        run = np.minimum(stop - at, MAX_MATCH)
        better = run > best
        best[better], which[better] = run[better], j
    return best, which


def parse(seg: np.ndarray) -> np.ndarray:
    best, which = best_matches(seg)
    out, i, n = [], 0, len(seg)
    while i < n:
        if best[i] >= MIN_MATCH:
            out.append(0x8000 | int(which[i]) << 9 | int(best[i]) - MIN_MATCH)
            i += int(best[i])
        else:
            out.append(int(seg[i]))
            i += 1
    return np.array(out, np.uint16)


def length_symbol(length: int):
    """(symbol, extra bits, their value) of a match length 3 ... 258."""
    v = length - 3
    if v == 255:
        return 285, 0, 0
    if v < 8:
        return 257 + v, 0, 0
    e = v.bit_length() - 3
    return 257 + 4 * (e + 1) + ((v >> e) & 3), e, v & ((1 << e) - 1)


def distance_symbol(j: int):
    """(symbol, extra bits, their value) of DISTANCES[j]: 1 2 3 4 are symbols 0-3, 6 is the second of 5-6, 8 of 7-8."""
    return (j, 0, 0) if j < 4 else (j, 1, 1)


_LENGTH_SYMBOLS = np.array([length_symbol(v + 3)[0] for v in range(256)], np.int64)
_LENGTH_EXTRA = np.array([length_symbol(v + 3)[1] for v in range(256)], np.int64)


def histograms(tokens_of_segments):
    tokens = np.concatenate(tokens_of_segments).astype(np.int64)
    match = (tokens & 0x8000) != 0
    lit = np.bincount(tokens[~match], minlength=N_LIT) + np.bincount(_LENGTH_SYMBOLS[tokens[match] & 0x1FF], minlength=N_LIT)
    dist = np.bincount((tokens[match] >> 9) & 7, minlength=N_DIST)  # the symbol of DISTANCES[j] is j
    lit[256] += 1
    return lit.astype(np.int64), dist.astype(np.int64)


# ------------------------------------------------------------------------------------------------ 5: tables
def huff_lengths(freq, limit: int) -> np.ndarray:
    freq = [int(v) for v in freq]
    n = len(freq)
    out = np.zeros(n, np.int32)
    used = [s for s in range(n) if freq[s] > 0]
    if not used:
        return out
    if len(used) == 1:
        out[used[0]] = 1
        return out
    f, ln, grp = list(freq), [0] * n, list(range(n))
    while True:
        live = [s for s in range(n) if f[s] > 0]
        if len(live) < 2:
            break
        c1 = min(live, key=lambda s: (f[s], -s))
        c2 = min((s for s in live if s != c1), key=lambda s: (f[s], -s))
        f[c1] += f[c2]
        f[c2] = 0
        for s in range(n):
            if grp[s] in (c1, c2):
                ln[s] += 1
                grp[s] = c1
    longest = max(ln)
    bits = [0] * (max(longest, limit) + 2)
    for s in used:
        bits[ln[s]] += 1
    for i in range(longest, limit, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    order = sorted(used, key=lambda s: (ln[s], s))
    at = 0
    for length in range(1, limit + 1):
        for _ in range(bits[length]):
            out[order[at]] = length
            at += 1
    assert at == len(used)
    return out


def canonical_codes(lengths) -> np.ndarray:
    """RFC 1951, 3.2.2: the codes as numbers, most significant bit first."""
    lengths = [int(v) for v in lengths]
    count = [0] * 17
    for v in lengths:
        count[v] += v > 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = np.zeros(len(lengths), np.int64)
    for s, v in enumerate(lengths):
        if v:
            out[s] = nxt[v]
            nxt[v] += 1
    return out


def run_length_code(seq):
    """The greedy rule of the header: [(code-length symbol, extra bits, their value)]."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, r = seq[i], 1
        while i + r < n and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 3:
            r = min(r, 138)
            out.append((18, 7, r - 11) if r >= 11 else (17, 3, r - 3))
        elif i > 0 and seq[i - 1] == v and r >= 3:
            r = min(r, 6)
            out.append((16, 2, r - 3))
        else:
            r = 1
            out.append((int(v), 0, 0))
        i += r
    return out


class BitWriter:
    """Deflate's packing: the first bit is the lowest of byte 0; a Huffman code goes in most significant bit first."""

    def __init__(self):
        self.acc, self.held, self.n, self.out = 0, 0, 0, bytearray()

    def put(self, value: int, bits: int):
        self.acc |= (value & ((1 << bits) - 1)) << self.held
        self.held += bits
        self.n += bits
        while self.held >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.held -= 8

    def put_code(self, code: int, bits: int):
        self.put(int(format(code, f"0{bits}b")[::-1], 2) if bits else 0, bits)

    def tobytes(self) -> bytes:
        return bytes(self.out) + (bytes([self.acc]) if self.held else b"")


class Tables:
    """The three length sets of a page's histograms, the codes, the header's bits."""

    def __init__(self, lit_hist, dist_hist):
        self.lit_len = huff_lengths(lit_hist, 15)
        self.dist_len = huff_lengths(dist_hist, 15)
        if not self.dist_len.any():
            self.dist_len[0] = 1
        self.hlit = max(257, int(np.flatnonzero(self.lit_len)[-1]) + 1)
        self.hdist = max(1, int(np.flatnonzero(self.dist_len)[-1]) + 1)
        self.rle = run_length_code([int(v) for v in self.lit_len[: self.hlit]] + [int(v) for v in self.dist_len[: self.hdist]])
        cl_hist = np.zeros(N_CL, np.int64)
        for s, _, _ in self.rle:
            cl_hist[s] += 1
        self.cl_len = huff_lengths(cl_hist, 7)
        self.hclen = max(4, max(k for k, s in enumerate(CL_ORDER) if self.cl_len[s]) + 1)
        self.lit_code, self.dist_code, self.cl_code = canonical_codes(self.lit_len), canonical_codes(self.dist_len), canonical_codes(self.cl_len)

    def header(self, w: BitWriter):
        w.put(1, 1)
        w.put(2, 2)
        w.put(self.hlit - 257, 5)
        w.put(self.hdist - 1, 5)
        w.put(self.hclen - 4, 4)
        for s in CL_ORDER[: self.hclen]:
            w.put(int(self.cl_len[s]), 3)
        for s, eb, ev in self.rle:
            w.put_code(int(self.cl_code[s]), int(self.cl_len[s]))
            w.put(ev, eb)

    def header_bits(self) -> int:
        return 17 + 3 * self.hclen + sum(int(self.cl_len[s]) + eb for s, eb, _ in self.rle)

    def put_tokens(self, w: BitWriter, tokens):
        for t in tokens.tolist():
            if t & 0x8000:
                s, eb, ev = length_symbol((t & 0x1FF) + 3)
                w.put_code(int(self.lit_code[s]), int(self.lit_len[s]))
                w.put(ev, eb)
                s, eb, ev = distance_symbol((t >> 9) & 7)
                w.put_code(int(self.dist_code[s]), int(self.dist_len[s]))
                w.put(ev, eb)
            else:
                w.put_code(int(self.lit_code[t]), int(self.lit_len[t]))

    def token_bits(self, tokens) -> int:
        t = tokens.astype(np.int64)
        match = (t & 0x8000) != 0
        v, j = t[match] & 0x1FF, (t[match] >> 9) & 7
        return int(self.lit_len[t[~match]].sum() + self.lit_len[_LENGTH_SYMBOLS[v]].sum() + _LENGTH_EXTRA[v].sum() + self.dist_len[j].sum() + (j >= 4).sum())


# ------------------------------------------------------------------------------------------------ 6: the stream
class Encoded:
    """Every intermediate of one page, and its file."""

    def __init__(self, page: np.ndarray):
        page = np.asarray(page)
        self.height, self.width = int(page.shape[0]), int(page.shape[1])
        self.channels = 1 if page.ndim == 2 else 3
        self.filtered, self.types = filter_rows(samples(page), self.channels)
        self.segments = segments_of(self.filtered)
        self.tokens = [parse(seg) for seg in self.segments]
        self.lit_hist, self.dist_hist = histograms(self.tokens)
        self.tables = Tables(self.lit_hist, self.dist_hist)
        self.segment_bits = [self.tables.token_bits(t) for t in self.tokens]
        w = BitWriter()
        self.tables.header(w)
        assert w.n == self.tables.header_bits() <= HEADER_BITS_MAX
        for t in self.tokens:
            self.tables.put_tokens(w, t)
        w.put_code(int(self.tables.lit_code[256]), int(self.tables.lit_len[256]))
        self.adler = zlib.adler32(self.filtered.tobytes())
        self.data = b"\x78\x9c" + w.tobytes() + struct.pack(">I", self.adler)
        assert len(self.data) <= file_capacity(self.height, self.width, self.channels)


def encode(page: np.ndarray) -> bytes:
    return Encoded(page).data


def unfilter(filtered: np.ndarray, bpp: int) -> np.ndarray:
    """The rows of PNG-filtered rows, by a literal loop a byte at a time (PNG, 9.2)."""
    h, n = filtered.shape[0], filtered.shape[1] - 1
    out = np.zeros((h, n), np.int32)
    for y in range(h):
        t = int(filtered[y, 0])
        for x in range(n):
            a = out[y, x - bpp] if x >= bpp else 0
            b = out[y - 1, x] if y else 0
            c = out[y - 1, x - bpp] if y and x >= bpp else 0
            if t == 0:
                pred = 0
            elif t == 1:
                pred = a
            elif t == 2:
                pred = b
            elif t == 3:
                pred = (a + b) >> 1
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            out[y, x] = (int(filtered[y, 1 + x]) + pred) & 255
    return out.astype(np.uint8)


def decode(data: bytes, h: int, w: int, c: int) -> np.ndarray:
    """The page of a file, as it arrived (B G R or grey)."""
    raw = np.frombuffer(zlib.decompress(data), np.uint8).reshape(h, 1 + w * c)
    rows = unfilter(raw, c)
    return rows.reshape(h, w) if c == 1 else np.ascontiguousarray(rows.reshape(h, w, 3)[:, :, ::-1])
