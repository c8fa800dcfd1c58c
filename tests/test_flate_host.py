"""CPU checks of the lossless page files: the definition (tests/flate_ref.py) decodes through zlib and Pillow to the exact pixels,
stays within 1.15 x zlib level 6 on the golden page and within its capacity on the adversarial cases, its filter and table steps
agree with literal second implementations, the options are checked in one place, and the PDF writer embeds the stream as it is."""

import functools
import inspect
import io
import os
import re
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import flate_ref as R
from yomitoku_amd import flate
from yomitoku_amd.jpeg import check_jpeg_preset, page_files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def golden_page() -> np.ndarray:
    return np.ascontiguousarray(np.array(Image.open(os.path.join(ROOT, "tests", "golden", "test_page.jpg")).convert("RGB"))[:, :, ::-1])


def _striped(w: int) -> np.ndarray:
    page = np.zeros((3, w, 3), np.uint8)
    page[:, ::7] = (200, 90, 10)
    page[1, 5::11, 1] = 77
    return page


def _cases() -> dict:
    rng = np.random.default_rng(11)
    crop = golden_page()[100:196, 100:260]
    return {"1x1": rng.integers(0, 256, (1, 1, 3), dtype=np.uint8), "1x3": rng.integers(0, 256, (1, 3, 3), dtype=np.uint8),
            "3x1": rng.integers(0, 256, (3, 1, 3), dtype=np.uint8), "flat": np.full((33, 67, 3), 77, np.uint8),
            "noise": rng.integers(0, 256, (40, 70, 3), dtype=np.uint8), "crop": np.ascontiguousarray(crop),
            "grey": np.ascontiguousarray(crop[:, :, 1]), "one_segment": _striped(2730), "two_segments": _striped(2731)}


@functools.lru_cache(maxsize=None)
def encoded(name: str) -> R.Encoded:
    return R.Encoded(_cases()[name])


def _entry(e: R.Encoded) -> flate.EncodedLossless:
    return flate.EncodedLossless(e.data, e.width, e.height, e.channels)


@pytest.mark.parametrize("name", list(_cases()))
def test_the_definition_decodes_through_zlib_and_pillow_to_the_exact_pixels(name):
    page, e = _cases()[name], encoded(name)
    assert e.data[:2] == b"\x78\x9c" and zlib.decompress(e.data) == e.filtered.tobytes()
    assert np.array_equal(R.decode(e.data, e.height, e.width, e.channels), page)
    got = np.asarray(Image.open(io.BytesIO(_entry(e).to_png())))
    assert np.array_equal(got, page if page.ndim == 2 else page[:, :, ::-1])
    assert len(e.data) <= R.file_capacity(e.height, e.width, e.channels) == flate.file_capacity(e.height, e.width, e.channels)
    assert _entry(e).nbytes == len(e.data) and _entry(e).scale == 1.0


def test_segments_and_the_special_cases_are_what_the_names_say():
    assert [len(s) for s in encoded("one_segment").segments] == [8191] * 3
    assert [len(s) for s in encoded("two_segments").segments] == [8192, 2] * 3
    noise = encoded("noise")
    assert not noise.dist_hist.any() and noise.tables.dist_len.tolist() == [1] + [0] * 29 and noise.tables.hdist == 1  # one declared code
    assert all((t < 256).all() for t in noise.tokens)
    assert encoded("flat").dist_hist.sum() > 0 and len(encoded("flat").data) < 100


def test_no_match_reaches_outside_its_segment():
    e = encoded("two_segments")
    for seg, tokens in zip(e.segments, e.tokens):
        covered = sum(int(t & 0x1FF) + 3 if t & 0x8000 else 1 for t in tokens.tolist())
        assert covered == len(seg)


@pytest.mark.parametrize("threshold", [False, True])
def test_size_cap_against_zlib_level_6_on_the_golden_page(threshold):
    page = golden_page()
    if threshold:
        page = (np.where(page < 128, 0, 255)).astype(np.uint8)
    e = R.Encoded(page)
    assert zlib.decompress(e.data) == e.filtered.tobytes()
    ratio = len(e.data) / len(zlib.compress(e.filtered.tobytes(), 6))
    print(f"golden page{' thresholded' if threshold else ''}: {len(e.data)} bytes, {ratio:.3f} x zlib level 6")
    assert ratio <= 1.15


def test_the_filter_step_agrees_with_a_literal_per_byte_loop():
    for name in ("crop", "grey", "1x3", "3x1", "noise"):
        page = _cases()[name]
        rows, bpp = R.samples(page), 1 if page.ndim == 2 else 3
        want = []
        for y in range(rows.shape[0]):
            best = None
            for t in range(5):
                out, cost = [t], 0
                for x in range(rows.shape[1]):
                    a = int(rows[y, x - bpp]) if x >= bpp else 0
                    b = int(rows[y - 1, x]) if y else 0
                    c = int(rows[y - 1, x - bpp]) if y and x >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = (0, a, b, (a + b) >> 1, a if pa <= pb and pa <= pc else (b if pb <= pc else c))[t]
                    v = (int(rows[y, x]) - pred) & 255
                    out.append(v)
                    cost += v if v < 128 else 256 - v
                if best is None or cost < best[0]:
                    best = (cost, out)
            want.append(best[1])
        assert encoded(name).filtered.tolist() == want, name
        assert np.array_equal(R.unfilter(encoded(name).filtered, bpp), rows), name


def _lengths_by_chains(freq, limit: int) -> list:
    """A literal second implementation: libjpeg's jpeg_gen_optimal_table with its `others` chains (jchuff.c), without the reserved
    code point and with `limit` in place of 16."""
    n = len(freq)
    f, codesize, others = [int(v) for v in freq], [0] * n, [-1] * n
    used = [s for s in range(n) if f[s]]
    if len(used) == 1:
        return [int(s == used[0]) for s in range(n)]
    while True:
        c1, v = -1, 1 << 62
        for i in range(n):
            if f[i] and f[i] <= v:
                v, c1 = f[i], i
        c2, v = -1, 1 << 62
        for i in range(n):
            if f[i] and f[i] <= v and i != c1:
                v, c2 = f[i], i
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * (max(codesize) + limit + 2)
    for s in used:
        bits[codesize[s]] += 1
    for i in range(max(codesize), limit, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    out, symbols = [0] * n, [s for size in range(1, max(codesize) + 1) for s in range(n) if codesize[s] == size]  # jchuff.c's huffval order
    at = 0
    for length in range(1, limit + 1):
        for _ in range(bits[length]):
            out[symbols[at]] = length
            at += 1
    return out


def _fibonacci(n: int) -> list:
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def _kraft(lengths) -> float:
    return sum(2.0 ** -int(v) for v in lengths if v)


def test_a_fibonacci_histogram_forces_both_limits_and_the_kraft_sum_stays_one():
    for n, limit in ((40, 15), (R.N_CL, 7), (R.N_DIST, 15)):
        freq = _fibonacci(n)
        lengths = R.huff_lengths(freq, limit)
        assert max(_lengths_by_chains(freq, 64)) > limit  # the merges alone go deeper: the limiter binds
        assert lengths.max() == limit and lengths.min() >= 1 and _kraft(lengths) == 1.0
        assert lengths.tolist() == _lengths_by_chains(freq, limit)
    rng = np.random.default_rng(3)
    for _ in range(40):  # and on histograms of every kind the two implementations agree, the sum is one, no length is above the limit
        n = int(rng.integers(2, R.N_LIT + 1))
        freq = (rng.integers(0, 4, n) * rng.integers(0, 1000, n) ** int(rng.integers(1, 4))).tolist()
        if sum(v > 0 for v in freq) < 2:
            continue
        for limit in (15, 7) if sum(v > 0 for v in freq) <= 128 else (15,):
            lengths = R.huff_lengths(freq, limit)
            assert lengths.tolist() == _lengths_by_chains(freq, limit)
            assert _kraft(lengths) == 1.0 and lengths.max() <= limit and ((lengths > 0) == (np.array(freq) > 0)).all()


def test_one_used_symbol_and_two_used_symbols():
    one = [0] * 30
    one[7] = 5
    assert R.huff_lengths(one, 15).tolist() == [int(s == 7) for s in range(30)]
    two = [0] * 30
    two[3], two[20] = 1, 1000
    assert R.huff_lengths(two, 15).tolist() == [int(s in (3, 20)) for s in range(30)] and _kraft(R.huff_lengths(two, 15)) == 1.0
    assert not R.huff_lengths([0] * 30, 15).any()
    fib = np.zeros(R.N_LIT, np.int64)
    fib[100:135], fib[256] = _fibonacci(35), 1
    t = R.Tables(fib, np.zeros(R.N_DIST, np.int64))
    assert t.lit_len.max() == 15 and _kraft(t.lit_len) == 1.0 and t.dist_len.tolist() == [1] + [0] * 29
    assert _kraft(t.cl_len) == 1.0 and t.cl_len.max() <= 7 and t.header_bits() <= R.HEADER_BITS_MAX
    codes = R.canonical_codes(t.lit_len)  # canonical: prefix-free in (length, symbol) order
    seen = sorted((format(int(c), f"0{int(n)}b") for c, n in zip(codes, t.lit_len) if n), key=lambda b: (len(b), b))
    assert all(not b.startswith(a) for i, a in enumerate(seen) for b in seen[i + 1 :])


def test_the_capacity_holds_on_the_adversarial_cases():
    for h, w, c in ((1, 1, 1), (1, 1, 3), (40, 70, 3), (3, 2731, 3), (64, 64, 1)):
        page = np.random.default_rng(h * w).integers(0, 256, (h, w) if c == 1 else (h, w, 3), dtype=np.uint8)
        assert len(R.encode(page)) <= R.file_capacity(h, w, c) == flate.file_capacity(h, w, c)
    assert flate.file_capacity(1, 1, 1) == 2 + (R.HEADER_BITS_MAX + 15 * 2 + 15 + 7) // 8 + 4
    with pytest.raises(ValueError):
        flate.file_capacity(0, 5, 3)
    with pytest.raises(ValueError):
        flate.file_capacity(5, 5, 2)


def test_options_are_checked_in_one_place():
    assert flate.check_lossless(False) is None and flate.check_lossless(True) == {"budget256": None}
    assert flate.check_lossless({"budget": 0.05}) == {"budget256": 13} and flate.check_lossless({"budget": 2}) == {"budget256": 512}
    assert flate.within_budget(13 * 100, 10, 10 * 256 // 256, 13 * 256) and flate.within_budget(10, 1, 1, None)
    assert flate.within_budget(13, 16, 16, 13) and not flate.within_budget(14, 16, 16, 13)  # nbytes * 256 <= budget256 * h * w
    assert check_jpeg_preset("high").lossless is None
    assert check_jpeg_preset("high", jpeg_lossless=True).lossless == {"budget256": None}
    assert page_files("low", lossless={"budget": 0.5}).lossless == {"budget256": 128}
    from yomitoku_amd.jpeg import PageFiles

    assert PageFiles("high", False, "4:2:0", False, False, None).lossless is None  # existing constructions keep working
    for bad in ("auto", 1, 0.5, None, [], {"budget": 0}, {"budget": -1}, {"budget": float("inf")}, {"budget": float("nan")}, {"budget": "1"},
                {"budget": None}, {"budget": True}, {"bytes": 1}, {"budget": 1, "more": 2}):
        with pytest.raises(ValueError, match="lossless"):
            check_jpeg_preset("high", jpeg_lossless=bad)
    with pytest.raises(ValueError, match="jpeg_lossless.*needs jpeg="):
        check_jpeg_preset(None, jpeg_lossless=True)
    check_jpeg_preset(None, jpeg_lossless=False)


def test_serve_signatures_and_refusals_before_a_source_is_read():
    from yomitoku_amd.document_analyzer import OCR, DocumentAnalyzer
    from yomitoku_amd.table_semantic_parser import TableSemanticParser

    def sources():
        raise AssertionError("a source was read")
        yield

    for cls in (DocumentAnalyzer, OCR):
        assert inspect.signature(cls.serve).parameters["jpeg_lossless"].default is False
        an = object.__new__(cls)
        with pytest.raises(ValueError, match="jpeg_lossless"):
            cls.serve(an, sources(), jpeg_lossless=True)
        with pytest.raises(ValueError, match="lossless"):
            cls.serve(an, sources(), jpeg="high", jpeg_lossless={"budgets": 1})
    assert "jpeg_lossless" not in inspect.signature(TableSemanticParser.serve).parameters


def test_serve_sharded_refuses_the_switch():
    from yomitoku_amd import distributed

    server = object.__new__(distributed.ShardedServer)  # the refusal comes before the server's state is touched
    with pytest.raises(NotImplementedError, match="jpeg_lossless"):
        distributed.ShardedServer.serve_local(server, [], jpeg="high", jpeg_lossless=True)
    with pytest.raises(NotImplementedError, match="jpeg_lossless"):
        distributed.ShardedServer.serve_local(server, [], jpeg="high", jpeg_lossless={"budget": 1})


def _stream_of_object(pdf: bytes, marker: bytes) -> tuple:
    at = pdf.index(marker)
    start = pdf.rindex(b" 0 obj\n", 0, at)
    head = pdf[start : pdf.index(b"stream\n", at)]
    length = int(re.search(rb"/Length (\d+)", head).group(1))
    body = pdf.index(b"stream\n", at) + len(b"stream\n")
    return head, pdf[body : body + length]


def test_searchable_pdf_embeds_the_stream_as_it_is():
    from types import SimpleNamespace

    from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

    doc = SimpleNamespace(words=[])
    for name, colours, space in (("crop", 3, b"/DeviceRGB"), ("grey", 1, b"/DeviceGray")):
        e, page = encoded(name), _cases()[name]
        pdf = searchable_pdf_bytes([_entry(e)], [doc])
        head, stream = _stream_of_object(pdf, b"/Predictor 15")
        want = f"/Filter /FlateDecode /DecodeParms << /Predictor 15 /Colors {colours} /BitsPerComponent 8 /Columns {e.width} >>".encode()
        assert want in head and b"/ColorSpace " + space in head and f"/Width {e.width} /Height {e.height}".encode() in head
        assert stream == e.data
        rows = np.frombuffer(zlib.decompress(stream), np.uint8).reshape(e.height, 1 + e.width * colours)
        assert np.array_equal(R.unfilter(rows, colours), R.samples(page))  # inflated and un-predicted by a literal loop: the page


def test_a_document_mixing_all_four_entry_kinds_is_written():
    from types import SimpleNamespace

    from tests import ccitt_ref
    from yomitoku_amd.ccitt import EncodedBilevel
    from yomitoku_amd.jpeg import EncodedJpeg
    from yomitoku_amd.mrc import EncodedMrc
    from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

    def jpeg_of(arr):
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, format="JPEG", quality=85)
        return EncodedJpeg(buf.getvalue(), arr.shape[1], arr.shape[0], arr.ndim == 2)

    page = _cases()["crop"]
    bits = page[:, :, 1] < 128
    mask = EncodedBilevel(ccitt_ref.encode_g4(bits), page.shape[1], page.shape[0])
    layered = EncodedMrc(mask, jpeg_of(page[::2, ::2, ::-1].copy()), jpeg_of(page[::8, ::8, ::-1].copy()), page.shape[1], page.shape[0], 1.0, 2, 8)
    entries = [jpeg_of(page[:, :, ::-1].copy()), mask, layered, _entry(encoded("crop")), _entry(encoded("grey"))]
    doc = SimpleNamespace(words=[])
    pdf = searchable_pdf_bytes(entries, [doc] * len(entries))
    assert pdf.startswith(b"%PDF-") and pdf.count(b"/Type /Page ") == 5
    assert pdf.count(b"/Predictor 15") == 2 and pdf.count(b"/CCITTFaxDecode") == 2 and pdf.count(b"/DCTDecode") == 3
