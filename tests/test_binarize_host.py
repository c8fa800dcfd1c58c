"""The binariser's definition (tests/binarize_ref.py) against exact rational arithmetic and a literal per-pixel loop, the page
the two methods differ on, and the host side of serve(jpeg_bilevel="otsu" | "adaptive"): the values the checks take and refuse,
EncodedBilevel's two new fields, the PDF writer.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from tests import binarize_ref, ccitt_ref
from tests.test_jpeg_host import _doc


def seeded_pages():
    """name -> page: noise, bimodal, two-valued and uniform pages, one and three channels, a few odd sizes."""
    rng = np.random.default_rng(77)
    out = {}
    for k, (h, w) in enumerate([(1, 1), (1, 9), (7, 5), (12, 12), (33, 20), (17, 64)]):
        out[f"noise_{h}x{w}"] = rng.integers(0, 256, (h, w), dtype=np.uint8)
        out[f"narrow_{h}x{w}"] = rng.integers(100 + k, 104 + k, (h, w), dtype=np.uint8)
        two = rng.random((h, w)) < 0.3
        out[f"bimodal_{h}x{w}"] = np.clip(np.where(two, 60, 190) + rng.integers(-25, 26, (h, w)), 0, 255).astype(np.uint8)
        out[f"two_valued_{h}x{w}"] = np.where(two, 0, 255).astype(np.uint8)
        out[f"ends_{h}x{w}"] = rng.choice(np.array([0, 1, 254, 255], np.uint8), (h, w))
    for v in (0, 128, 255):
        out[f"uniform_{v}"] = np.full((6, 11), v, np.uint8)
    for name in ("noise_12x12", "two_valued_7x5", "bimodal_33x20"):
        out[name + "_bgr"] = np.ascontiguousarray(np.stack([out[name]] * 3, -1))
    return out


PAGES = seeded_pages()


def exact_otsu(page) -> int:
    """Otsu's threshold with the between-class variance d^2 / (w0 w1) as a Fraction: no rounding anywhere."""
    p = binarize_ref.grey(page).reshape(-1).astype(np.int64)
    best, at = None, 0
    for t in range(255):
        low, high = p[p <= t], p[p > t]
        if len(low) and len(high):
            d = int(high.sum()) * len(low) - int(low.sum()) * len(high)
            sigma = Fraction(d * d, len(low) * len(high))
            if best is None or sigma > best:
                best, at = sigma, t
    return at


def loop_adaptive(p):
    """The adaptive rule, pixel by pixel, as the words of the definition say it."""
    h, w = p.shape
    r = max(1, max(h, w) // 16)
    out = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            n = s = 0
            for yy in range(y - r, y + r + 1):
                for xx in range(x - r, x + r + 1):
                    if 0 <= yy < h and 0 <= xx < w:
                        n += 1
                        s += int(p[yy, xx])
            out[y, x] = int(p[y, x]) * n * 20 <= s * 17
    return out


@pytest.mark.parametrize("name", sorted(PAGES))
def test_otsu_in_float64_equals_otsu_in_exact_arithmetic(name):
    assert binarize_ref.otsu_threshold(PAGES[name]) == exact_otsu(PAGES[name])


def test_otsu_on_two_hundred_seeded_histograms_equals_exact_arithmetic():
    """Pages of up to 16383^2 pixels stand behind these histograms: the counts are drawn large, so that d passes 2^53 and the
    conversions to float64 round."""
    rng = np.random.default_rng(5)
    for k in range(200):
        hist = np.zeros(256, np.int64)
        bins = rng.choice(256, int(rng.integers(1, 40)), replace=False)
        hist[bins] = rng.integers(1, 1 << int(rng.integers(2, 23)), len(bins))
        assert hist.sum() <= 16383 * 16383
        total_w, total_m = int(hist.sum()), int((hist * np.arange(256)).sum())
        best, at, w0, m0 = None, 0, 0, 0
        for t in range(255):
            w0, m0 = w0 + int(hist[t]), m0 + t * int(hist[t])
            w1, m1 = total_w - w0, total_m - m0
            if w0 and w1:
                d = m1 * w0 - m0 * w1
                assert abs(d) < 1 << 62
                sigma = Fraction(d * d, w0 * w1)
                if best is None or sigma > best:
                    best, at = sigma, t
        got, top = 0, None
        for t, sigma in binarize_ref.otsu_sigmas(hist):
            if top is None or sigma > top:
                got, top = t, sigma
        assert got == at, k


@pytest.mark.parametrize("name", [n for n in sorted(PAGES) if PAGES[n].shape[0] <= 12 and PAGES[n].shape[1] <= 12])
def test_adaptive_equals_the_literal_double_loop(name):
    """pages up to 12 x 12: r = 1 everywhere - the window larger than the page on the 1 x 1 page, clipped on the others"""
    p = binarize_ref.grey(PAGES[name])
    assert np.array_equal(binarize_ref.black_mask(PAGES[name], "adaptive"), loop_adaptive(p))


def test_adaptive_window_larger_than_the_page():
    rng = np.random.default_rng(3)
    for h, w in [(1, 1), (1, 2), (2, 1), (2, 3), (1, 40), (3, 48)]:  # r = 1, 1, 1, 1, 2, 3 against 1 - 3 rows
        p = rng.integers(0, 256, (h, w), dtype=np.uint8)
        assert np.array_equal(binarize_ref.black_mask(p, "adaptive"), loop_adaptive(p)), (h, w)


@pytest.mark.parametrize("name", [n for n in sorted(PAGES) if n.startswith("two_valued")])
@pytest.mark.parametrize("method", binarize_ref.METHODS)
def test_a_two_valued_page_gives_the_mask_of_auto(name, method):
    page = PAGES[name]
    assert ccitt_ref.is_bilevel(page)
    assert np.array_equal(binarize_ref.black_mask(page, method), ccitt_ref.black_mask(page))


def test_the_gradient_page_tells_the_methods_apart():
    page, ink = binarize_ref.gradient_page()
    assert page.shape == (96, 160) and 0.1 < ink.mean() < 0.2
    assert np.array_equal(binarize_ref.black_mask(page, "adaptive"), ink)
    wrong = (binarize_ref.black_mask(page, "otsu") != ink).mean()
    assert 0.3 < wrong < 0.45  # one threshold cannot follow the light: more than a third of the page


@pytest.mark.parametrize("value", [0, 128, 255])
def test_uniform_pages(value):
    """no t has both classes: t* = 0, so only a page of 0 is black under "otsu"; p n 20 <= p n 17 holds for p = 0 alone"""
    page = PAGES[f"uniform_{value}"]
    assert binarize_ref.otsu_threshold(page) == 0
    for method in binarize_ref.METHODS:
        assert np.array_equal(binarize_ref.black_mask(page, method), np.full(page.shape, value == 0))


def test_grey_valued():
    assert binarize_ref.is_grey_valued(PAGES["noise_12x12"]) and binarize_ref.is_grey_valued(PAGES["noise_12x12_bgr"])
    colour = PAGES["noise_12x12_bgr"].copy()
    colour[5, 7, 2] ^= 1
    assert not binarize_ref.is_grey_valued(colour) and not binarize_ref.is_grey_valued(PAGES["noise_12x12"].astype(np.float32))


def test_the_checks_take_the_new_values_and_keep_their_refusals():
    from yomitoku_amd.ccitt import check_bilevel
    from yomitoku_amd.serving import check_jpeg_preset

    assert check_bilevel(False) is False
    for good in ("auto", "otsu", "adaptive"):
        assert check_bilevel(good) is True
        check_jpeg_preset("high", jpeg_bilevel=good)
        with pytest.raises(ValueError, match="jpeg_bilevel"):
            check_jpeg_preset(None, jpeg_bilevel=good)
    for bad in (True, 1, 0, None, "always", "yes", "Otsu", "adaptive ", b"otsu"):
        with pytest.raises(ValueError, match="bilevel"):
            check_bilevel(bad)
        with pytest.raises(ValueError, match="bilevel"):
            check_jpeg_preset("high", jpeg_bilevel=bad)


def test_serve_refuses_the_new_values_without_jpeg_before_a_source_is_read():
    from types import SimpleNamespace

    from tests.test_serving import StubAnalyzer
    from yomitoku_amd.document_analyzer import OCR, DocumentAnalyzer
    from yomitoku_amd.serving import PagePipeline, check_jpeg_preset

    def sources():
        raise AssertionError("a source was read")
        yield

    pipe = PagePipeline(StubAnalyzer(), wave=2, in_flight=1)
    try:
        for mode in ("otsu", "adaptive"):
            for serve in (lambda **kw: DocumentAnalyzer.serve(SimpleNamespace(visualize=False), sources(), **kw),
                          lambda **kw: OCR.serve(SimpleNamespace(visualize=False), sources(), **kw), lambda **kw: pipe.serve(sources(), files=check_jpeg_preset(**{"jpeg": None, **kw}))):
                with pytest.raises(ValueError, match="jpeg_bilevel"):
                    serve(jpeg_bilevel=mode)
                with pytest.raises(ValueError, match="bilevel"):
                    serve(jpeg="high", jpeg_bilevel=mode.upper())
    finally:
        pipe.close()


def test_encoded_bilevel_keeps_its_constructor_and_gains_two_defaults():
    from yomitoku_amd.ccitt import EncodedBilevel

    e = EncodedBilevel(b"\x00\x10\x01", 8, 1)
    assert (e.data, e.width, e.height, e.scale, e.method, e.threshold) == (b"\x00\x10\x01", 8, 1, 1.0, "auto", None)
    assert EncodedBilevel(b"x", 3, 2, 1.0) == EncodedBilevel(b"x", 3, 2, method="auto", threshold=None)
    e = EncodedBilevel(b"x", 3, 2, 1.0, "otsu", 131)
    assert (e.method, e.threshold, e.bilevel) == ("otsu", 131, True)


def test_the_pdf_writer_embeds_a_thresholded_page_as_ccitt():
    from yomitoku_amd.ccitt import EncodedBilevel
    from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

    page, _ = binarize_ref.gradient_page()
    data = ccitt_ref.encode_g4(binarize_ref.black_mask(page, "otsu"))
    entry = EncodedBilevel(data, page.shape[1], page.shape[0], 1.0, "otsu", binarize_ref.otsu_threshold(page))
    pdf = searchable_pdf_bytes([entry], [_doc()], "high")
    assert pdf.count(b"/Filter /CCITTFaxDecode") == 1 and b"/DCTDecode" not in pdf and data in pdf
    assert b"/Width 160 /Height 96" in pdf and b"/BitsPerComponent 1" in pdf
