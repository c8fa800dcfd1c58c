"""DocumentAnalyzer.serve / OCR.serve(jpeg=..., jpeg_bilevel="otsu" | "adaptive"): a grey-valued page's entry ends with the
Group 4 file of the thresholded page - full size -, every other page's with the JPEG file it gets without the switch, and the
schemas and overlays are those of the job without it: the networks see the page as it arrived.  The analyzers and their seeded
weights are those of tests/test_serving_gpu.py and tests/test_ocr_serve_gpu.py; the definition is tests/binarize_ref.py."""
import numpy as np
import pytest

from tests import binarize_ref, ccitt_ref
from tests.test_serving_gpu import _analyzer

pytestmark = pytest.mark.gpu

GREY, COLOUR, TWO_VALUED = 0, 1, 2


@pytest.fixture(scope="module")
def analyzer(dev):
    an = _analyzer()
    yield an
    an.close()


@pytest.fixture(scope="module")
def ocr(dev):
    from tests.test_ocr_serve_gpu import _ocr

    an = _ocr()
    yield an
    an.close()


@pytest.fixture(scope="module")
def pages():
    """Three small pages as load_image hands them over, B G R: a grey-valued scan, a colour page, a 1-bit scan."""
    from yomitoku_amd.utils.synth import synthetic_page_with_truth

    out = [synthetic_page_with_truth(3 + i, h, w)[0] for i, (h, w) in enumerate([(640, 600), (600, 640), (500, 700)])]
    g = out[GREY][..., 1]
    out[GREY] = np.ascontiguousarray(np.stack([g] * 3, -1))
    v = np.where(out[TWO_VALUED][..., 1] < 128, 0, 255).astype(np.uint8)
    out[TWO_VALUED] = np.ascontiguousarray(np.stack([v] * 3, -1))
    assert [binarize_ref.is_grey_valued(p) for p in out] == [True, False, True]
    assert [ccitt_ref.is_bilevel(p) for p in out] == [False, False, True]
    return out


@pytest.mark.parametrize("method", binarize_ref.METHODS)
@pytest.mark.parametrize("which", ["analyzer", "ocr"])
def test_serve_gives_thresholded_group4_files_next_to_the_jpegs(which, method, pages, request):
    from yomitoku_amd.ccitt import EncodedBilevel
    from yomitoku_amd.jpeg import EncodedJpeg, encode_jpeg_pages
    from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

    an = request.getfixturevalue(which)
    base = an.serve(pages, wave=2, jpeg="high")
    got = an.serve(pages, wave=2, jpeg="high", jpeg_bilevel=method)
    files = encode_jpeg_pages(pages, "high", bilevel=method)
    assert len(got) == len(base) == 3
    for k, (page, entry, plain) in enumerate(zip(pages, got, base)):
        assert isinstance(entry, tuple) and len(entry) == 2
        assert entry[0].model_dump() == plain[0].model_dump()
        assert entry[1] == files[k]
        if k == COLOUR:
            assert isinstance(entry[1], EncodedJpeg) and entry[1] == plain[1]
        else:
            mask = binarize_ref.black_mask(page, method)
            assert isinstance(entry[1], EncodedBilevel) and entry[1].data == ccitt_ref.encode_g4(mask)
            assert (entry[1].width, entry[1].height, entry[1].scale, entry[1].method) == (page.shape[1], page.shape[0], 1.0, method)
            assert entry[1].threshold == (binarize_ref.otsu_threshold(page) if method == "otsu" else None)
    assert got[TWO_VALUED][1].data == an.serve(pages[TWO_VALUED:], wave=2, jpeg="high", jpeg_bilevel="auto")[0][1].data
    pdf = searchable_pdf_bytes([e[1] for e in got], [e[0] for e in got])
    assert pdf.count(b"/Filter /CCITTFaxDecode") == 2 and pdf.count(b"/Filter /DCTDecode") == 1
    # the switch belongs to the job: the next one is plain again
    after = an.serve(pages[:2], wave=2, jpeg="high")
    assert [e[1] for e in after] == [e[1] for e in base[:2]]


@pytest.mark.parametrize("which", ["analyzer", "ocr"])
def test_overlays_are_those_of_the_job_without_the_switch(which, pages, request):
    an = request.getfixturevalue(which)
    base = an.serve(pages, wave=2, overlays=True, jpeg="high")
    got = an.serve(pages, wave=2, overlays=True, jpeg="high", jpeg_bilevel="adaptive")
    for entry, plain in zip(got, base):
        assert len(entry) == len(plain) >= 3
        assert entry[0].model_dump() == plain[0].model_dump()
        assert all(np.array_equal(a, b) for a, b in zip(entry[1:-1], plain[1:-1]))
    assert [getattr(e[-1], "bilevel", False) for e in got] == [True, False, True]


def test_the_new_values_are_refused_without_jpeg_before_a_source_is_read(analyzer, ocr):
    def sources():
        raise AssertionError("a source was read")
        yield

    for an in (analyzer, ocr):
        for method in binarize_ref.METHODS:
            with pytest.raises(ValueError, match="jpeg_bilevel"):
                an.serve(sources(), wave=2, jpeg_bilevel=method)
        for bad in ("Otsu", "bradley", True):
            with pytest.raises(ValueError, match="bilevel"):
                an.serve(sources(), wave=2, jpeg="high", jpeg_bilevel=bad)
