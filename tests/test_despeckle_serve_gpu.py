"""encode_g4_pages(despeckle=...) and DocumentAnalyzer.serve / OCR.serve(jpeg=..., jpeg_bilevel=..., jpeg_despeckle=...): the
Group 4 file of a page is that of the definitions in a row - tests/binarize_ref.py, tests/despeckle_ref.py, tests/ccitt_ref.py -
byte for byte, its `despeckled` the definition's counts; everything else about the entry, every other page of the job and the
schemas are those of the job without the switch.  The analyzers and their seeded weights are those of tests/test_serving_gpu.py
and tests/test_ocr_serve_gpu.py."""
import functools
import os

import numpy as np
import pytest

from tests import binarize_ref, ccitt_ref
from tests import despeckle_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_page.jpg")
NOISY, COLOUR, TWO_VALUED = 0, 1, 2


@functools.lru_cache(maxsize=None)
def grey_pages():
    """The 96 x 160 gradient page of the binariser's tests with salt and pepper on it, and the noisy golden page."""
    page, _ = binarize_ref.gradient_page()
    rng = np.random.default_rng(31)
    hit = rng.random(page.shape)
    salted = np.where(hit < 0.01, 0, np.where(hit > 0.99, 255, page)).astype(np.uint8)
    return salted, R.noisy_page(R.golden_page(GOLDEN))


@functools.lru_cache(maxsize=None)
def expected(index, method, n_black=4, n_white=4):
    """(the file, the counts) of grey page `index` by the definitions - computed once"""
    clean, counts = R.despeckle(binarize_ref.black_mask(grey_pages()[index], method), n_black, n_white)
    return ccitt_ref.encode_g4(clean), counts


@pytest.mark.parametrize("method", ["otsu", "adaptive"])
def test_encode_g4_pages_codes_the_despeckled_bits(dev, method):
    from yomitoku_amd.ccitt import EncodedBilevel, encode_g4_pages
    from yomitoku_amd.despeckle import Despeckled

    pages = list(grey_pages())
    scratch = {}
    plain = encode_g4_pages(pages, binarize=method, scratch=scratch)
    got = encode_g4_pages(pages, binarize=method, despeckle=True, scratch=scratch)
    for k, (entry, before) in enumerate(zip(got, plain)):
        data, counts = expected(k, method)
        assert isinstance(entry, EncodedBilevel) and entry.data == data
        assert entry.despeckled == Despeckled(4, 4, *counts) and counts[1] > 0
        assert (entry.method, entry.threshold, entry.width, entry.height, entry.scale) == (before.method, before.threshold, before.width, before.height, 1.0)
        # without the switch: the bytes of before, and nothing said
        assert before.despeckled is None and before.data == ccitt_ref.encode_g4(binarize_ref.black_mask(pages[k], method))
    assert 2 * len(got[1].data) < len(plain[1].data)  # what it is for: the noisy golden page
    # one colour only, through the other entry; the next call without the switch is plain again
    from yomitoku_amd.jpeg import encode_jpeg_pages

    one = encode_jpeg_pages(pages, "high", bilevel=method, despeckle={"white": 3}, scratch=scratch)
    for k, entry in enumerate(one):
        data, counts = expected(k, method, 0, 3)
        assert entry.data == data and entry.despeckled == Despeckled(0, 3, *counts) and counts[:2] == (0, 0)
    again = encode_g4_pages(pages, binarize=method, scratch=scratch)
    assert [e.data for e in again] == [e.data for e in plain] and all(e.despeckled is None for e in again)


def test_a_two_valued_page_under_auto_is_despeckled_too(dev):
    from yomitoku_amd.ccitt import encode_g4_pages
    from yomitoku_amd.despeckle import Despeckled

    black = binarize_ref.black_mask(grey_pages()[0], "otsu")
    page = np.where(black, 0, 255).astype(np.uint8)
    got = encode_g4_pages([page, np.full((5, 7, 3), 128, np.uint8)], despeckle=5)
    clean, counts = R.despeckle(black, 5, 5)
    assert got[0].data == ccitt_ref.encode_g4(clean) and got[0].despeckled == Despeckled(5, 5, *counts) and got[0].method == "auto"
    assert isinstance(got[1], ValueError)  # not two-valued: as without the switch


# ---------------------------------------------------------------------------------------------------------------- serve
@pytest.fixture(scope="module")
def ocr(dev):
    from tests.test_ocr_serve_gpu import _ocr

    an = _ocr()
    yield an
    an.close()


@pytest.fixture(scope="module")
def analyzer(dev):
    from tests.test_serving_gpu import _analyzer

    an = _analyzer()
    yield an
    an.close()


@pytest.fixture(scope="module")
def job():
    """Three small pages as load_image hands them over, B G R: a noisy grey scan, a colour page, a 1-bit scan."""
    from yomitoku_amd.utils.synth import synthetic_page_with_truth

    out = [synthetic_page_with_truth(3 + i, h, w)[0] for i, (h, w) in enumerate([(600, 640), (640, 600), (500, 700)])]
    g = R.noisy_page(out[NOISY][..., 1])
    out[NOISY] = np.ascontiguousarray(np.stack([g] * 3, -1))
    v = np.where(out[TWO_VALUED][..., 1] < 128, 0, 255).astype(np.uint8)
    out[TWO_VALUED] = np.ascontiguousarray(np.stack([v] * 3, -1))
    assert [binarize_ref.is_grey_valued(p) for p in out] == [True, False, True]
    return out


def _by_definition(page, method, n_black, n_white):
    clean, counts = R.despeckle(binarize_ref.black_mask(page, method), n_black, n_white)
    return ccitt_ref.encode_g4(clean), counts


def test_ocr_serve_despeckles_the_group4_pages_of_a_mixed_job(ocr, job):
    from yomitoku_amd.ccitt import EncodedBilevel
    from yomitoku_amd.despeckle import Despeckled
    from yomitoku_amd.jpeg import EncodedJpeg
    from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

    base = ocr.serve(job, wave=2, jpeg="high", jpeg_bilevel="otsu")
    got = ocr.serve(job, wave=2, jpeg="high", jpeg_bilevel="otsu", jpeg_despeckle={"black": 4})
    assert len(got) == len(base) == 3
    for k, (entry, plain) in enumerate(zip(got, base)):
        assert isinstance(entry, tuple) and len(entry) == len(plain) == 2
        assert entry[0].model_dump() == plain[0].model_dump()  # OCR sees the page as it arrived
        if k == COLOUR:
            assert isinstance(entry[1], EncodedJpeg) and entry[1] == plain[1] and entry[1].data == plain[1].data
            continue
        data, counts = _by_definition(job[k], "otsu", 4, 0)
        assert isinstance(entry[1], EncodedBilevel) and entry[1].data == data and entry[1].despeckled == Despeckled(4, 0, *counts)
        assert plain[1].despeckled is None
        assert (entry[1].method, entry[1].threshold, entry[1].width, entry[1].height) == ("otsu", plain[1].threshold, plain[1].width, plain[1].height)
    assert got[NOISY][1].despeckled.black_components > 100 and len(got[NOISY][1].data) < len(base[NOISY][1].data)
    pdf = searchable_pdf_bytes([e[1] for e in got], [e[0] for e in got])
    assert pdf.count(b"/Filter /CCITTFaxDecode") == 2 and pdf.count(b"/Filter /DCTDecode") == 1
    # the switch belongs to the job: the next one is as before, byte for byte
    after = ocr.serve(job, wave=2, jpeg="high", jpeg_bilevel="otsu")
    assert [e[1] for e in after] == [e[1] for e in base] and [e[1].data for e in after] == [e[1].data for e in base]


def test_document_analyzer_serve_despeckles_one_page(analyzer, job):
    from yomitoku_amd.despeckle import Despeckled

    base = analyzer.serve(job[:1], wave=2, jpeg="high", jpeg_bilevel="adaptive")
    got = analyzer.serve(job[:1], wave=2, jpeg="high", jpeg_bilevel="adaptive", jpeg_despeckle=True)
    data, counts = _by_definition(job[NOISY], "adaptive", 4, 4)
    assert got[0][0].model_dump() == base[0][0].model_dump()
    assert got[0][1].data == data and got[0][1].despeckled == Despeckled(4, 4, *counts) and got[0][1].method == "adaptive"
    assert base[0][1].despeckled is None and len(data) < len(base[0][1].data)


def test_the_refusals_come_before_a_source_is_read(ocr, analyzer):
    def sources():
        raise AssertionError("a source was read")
        yield

    for an in (ocr, analyzer):
        with pytest.raises(ValueError, match="jpeg_despeckle"):
            an.serve(sources(), wave=2, jpeg_despeckle=True)
        with pytest.raises(ValueError, match="no Group 4 file to clean"):
            an.serve(sources(), wave=2, jpeg="high", jpeg_despeckle=True)
        for bad in (0, {"black": 0}, {"speck": 4}, "yes", 70000):
            with pytest.raises(ValueError, match="despeckle"):
                an.serve(sources(), wave=2, jpeg="high", jpeg_bilevel="otsu", jpeg_despeckle=bad)
