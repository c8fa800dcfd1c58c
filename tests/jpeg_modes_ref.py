"""The definition of the device JPEG encoder's per-page modes (`encode_jpeg_pages(..., subsampling=..., grey="auto")`), in plain
NumPy / Python.  A helper like tests/jpeg_ref.py, whose tables, DCT, quantiser, interval coder and segments it uses: it shares no
code with the product, and the device must equal it byte for byte.

The file is tests/jpeg_ref.py's with three generalisations.  With the luminance sampling factors (hs, vs) = (1, 1) for 4:4:4,
(2, 1) for 4:2:2 and (2, 2) for 4:2:0:
  MCU and padding   an MCU is 8 hs x 8 vs pixels; the page is edge-replicated to whole MCUs;
  block order       an MCU's blocks are its hs vs luminance blocks in row-major order, then Cb, then Cr (3 / 4 / 6 blocks);
                    luminance uses table 0, chrominance table 1;
  chroma            4:4:4: the Cb / Cr planes at full resolution;
                    4:2:2: the mean of each horizontal pair, (a + b + bias) >> 1 with bias 0 in even output columns and 1 in odd
                    ones (libjpeg's h2v1_downsample);
                    4:2:0: rule 3 of tests/jpeg_ref.py;
  header            the SOF0 luminance byte is hs << 4 | vs, chrominance 0x11; DRI = ceil(w / (8 hs)): one restart interval per
                    MCU row, RSTm cycling mod 8; everything else is jpeg_ref.header's.
A page all of whose pixels have B == G == R, asked for as a grey file, is the one-component file of its channel-0 plane:
`jpeg_ref.encode(page[..., 0], q)`.

Against Pillow 12.2 (libjpeg-turbo) `save(quality=q, subsampling=s, restart_marker_rows=1)`: 4:4:4 is byte-equal at every size
(no component ever needs a dummy block); 4:2:2 wherever ceil(w / 8) is even, at any height (elsewhere libjpeg fills the missing
luminance block from its neighbour's DC, as tests/jpeg_ref.py explains for 4:2:0); tests/test_jpeg_modes_host.py holds both.
"""

from __future__ import annotations

import numpy as np

from tests import jpeg_opt_ref, jpeg_ref

SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}


def planes(page, subsampling):
    """[Y, Cb, Cr] of a colour page (H x W x 3, B G R), extended to whole MCUs, the chroma at its subsampled size."""
    hs, vs = SAMPLING[subsampling]
    page = np.asarray(page)
    h, w = page.shape[:2]
    page = np.pad(page, ((0, -h % (8 * vs)), (0, -w % (8 * hs)), (0, 0)), mode="edge").astype(np.int64)
    b, g, r = page[..., 0], page[..., 1], page[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    out = [y]
    for c in (cb, cr):
        if (hs, vs) == (1, 1):
            out.append(c)
        elif (hs, vs) == (2, 1):
            s = c[:, 0::2] + c[:, 1::2]
            out.append((s + (np.arange(s.shape[1]) & 1)[None, :]) >> 1)
        else:
            s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
            out.append((s + (1 + (np.arange(s.shape[1]) & 1))[None, :]) >> 2)
    return out


def coefficients(page, quality: int, subsampling):
    """Zig-zag int16 [blocks][64] in scan order: MCU rows top to bottom, MCUs left to right, Y.. Cb Cr inside one."""
    hs, vs = SAMPLING[subsampling]
    ql, qc = jpeg_ref.quant_tables(quality)
    y, cb, cr = planes(page, subsampling)
    y, cb, cr = jpeg_ref._blocks_of(y, ql), jpeg_ref._blocks_of(cb, qc), jpeg_ref._blocks_of(cr, qc)
    mh, mw = cb.shape[:2]
    out = np.empty((mh, mw, hs * vs + 2, 64), np.int16)
    for j in range(vs):
        for i in range(hs):
            out[:, :, j * hs + i] = y[j::vs, i::hs]
    out[:, :, hs * vs], out[:, :, hs * vs + 1] = cb, cr
    return out.reshape(-1, 64)


def _layout(height, width, subsampling):
    hs, vs = SAMPLING[subsampling]
    mw, mh = -(-width // (8 * hs)), -(-height // (8 * vs))
    return mw, mh, hs * vs + 2, ([0] * (hs * vs) + [1, 2]) * mw


def header(height, width, quality, subsampling) -> bytes:
    """jpeg_ref.header's colour header with this mode's luminance sampling byte and restart interval."""
    hs, vs = SAMPLING[subsampling]
    plain = jpeg_ref.header(height, width, False, quality)
    at, where = 2, {}  # walk the segments behind SOI
    while at < len(plain):
        where.setdefault(plain[at + 1], at)
        at += 2 + int.from_bytes(plain[at + 2 : at + 4], "big")
    sof, dri = where[0xC0], where[0xDD]
    assert plain[sof + 11] == 0x22  # marker, length, precision, height, width, components, id: the luminance sampling byte
    mw = -(-width // (8 * hs))
    return plain[: sof + 11] + bytes([hs << 4 | vs]) + plain[sof + 12 : dri + 4] + mw.to_bytes(2, "big") + plain[dri + 6 :]


def _swap_dht(plain: bytes, tables) -> bytes:
    """`plain` with its DHT segments replaced by those of `tables` (jpeg_opt_ref.header's walk)."""
    at, first, dri = 2, None, None
    while at < len(plain):
        if plain[at + 1] == 0xC4 and first is None:
            first = at
        if plain[at + 1] == 0xDD:
            dri = at
        at += 2 + int.from_bytes(plain[at + 2 : at + 4], "big")
    return plain[:first] + jpeg_opt_ref.dht_segments(tables) + plain[dri:]


def histograms(coefs, height, width, subsampling):
    """jpeg_opt_ref.histograms for this mode's block order."""
    mw, mh, per, comps = _layout(height, width, subsampling)
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


def page_tables(coefs, height, width, subsampling):
    """The page's own tables by jpeg_opt_ref's rule: [(DHT identifier, (bits, vals))], DC 0, AC 0, DC 1, AC 1."""
    dc, ac = histograms(coefs, height, width, subsampling)
    return [(0x00, jpeg_opt_ref.optimal_table(dc[0])), (0x10, jpeg_opt_ref.optimal_table(ac[0])),
            (0x01, jpeg_opt_ref.optimal_table(dc[1])), (0x11, jpeg_opt_ref.optimal_table(ac[1]))]


def assemble(coefs, height, width, quality, subsampling, optimize=False) -> bytes:
    """The file from its coefficients (int16 [blocks][64], as `coefficients` orders them)."""
    mw, mh, per, comps = _layout(height, width, subsampling)
    head = header(height, width, quality, subsampling)
    if optimize:
        tables = page_tables(coefs, height, width, subsampling)
        head = _swap_dht(head, tables)
        codes = {ident: jpeg_ref.huffman_codes(spec) for ident, spec in tables}
        dc, ac = [codes[0x00], codes[0x01]], [codes[0x10], codes[0x11]]
    else:
        dc = [jpeg_ref.huffman_codes(jpeg_ref.DC_LUMA), jpeg_ref.huffman_codes(jpeg_ref.DC_CHROMA)]
        ac = [jpeg_ref.huffman_codes(jpeg_ref.AC_LUMA), jpeg_ref.huffman_codes(jpeg_ref.AC_CHROMA)]
    coefs = np.asarray(coefs).reshape(mh, mw * per, 64)
    out = bytearray(head)
    for r in range(mh):
        out += jpeg_ref.encode_interval(coefs[r], comps, dc, ac)
        if r + 1 < mh:
            out += bytes([0xFF, 0xD0 + (r & 7)])
    return bytes(out + b"\xff\xd9")


def is_grey(page) -> bool:
    page = np.asarray(page)
    return page.ndim == 3 and bool((page[..., 0] == page[..., 1]).all() and (page[..., 0] == page[..., 2]).all())


def encode(page, quality: int, subsampling="4:2:0", grey=False, optimize=False) -> bytes:
    """The file of `encode_jpeg_pages(..., subsampling=subsampling, grey=grey, optimize=optimize)` for one page: an H x W page
    is jpeg_ref's grey file whatever the mode; grey "auto": a colour page with B == G == R everywhere is that of its channel 0."""
    page = np.asarray(page)
    if page.ndim == 3 and grey == "auto" and is_grey(page):
        page = np.ascontiguousarray(page[..., 0])
    if page.ndim == 2:
        return jpeg_opt_ref.encode(page, quality) if optimize else jpeg_ref.encode(page, quality)
    h, w = page.shape[:2]
    return assemble(coefficients(page, quality, subsampling), h, w, quality, subsampling, optimize)
