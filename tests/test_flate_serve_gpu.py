"""DocumentAnalyzer.serve / OCR.serve(jpeg=..., jpeg_lossless=...): every page the other switches leave ends with its
EncodedLossless - byte for byte the definition's file (tests/flate_ref.py), decoding to the page as it arrived - and the schemas are
those of the job without the switch; `jpeg_bilevel` and `jpeg_mrc` decide first and write what they wrote; `jpeg_grey="auto"` makes
a grey three-channel page a one-channel file; a page over the budget gets exactly the JPEG of the job without the switch; with
`deskew` the file is of the corrected page.  The analyzers and their seeded weights are those of tests/test_serving_gpu.py and
tests/test_ocr_serve_gpu.py."""
import io

import numpy as np
import pytest

from tests import ccitt_ref, deskew_ref, mrc_ref
from tests import flate_ref as R
from tests.test_serving_gpu import _analyzer

pytestmark = pytest.mark.gpu


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


def _text_page(seed: int, h: int, w: int) -> np.ndarray:
    """The top-left h x w pixels of a synthetic 600 x 640 page, as load_image hands them over (B G R)."""
    from yomitoku_amd.utils.synth import synthetic_page_with_truth

    return np.ascontiguousarray(synthetic_page_with_truth(seed, 600, 640)[0][:h, :w])


def _flat_page() -> np.ndarray:
    """Flat colour with hard edges and no ink: two tints of about the same lightness."""
    page = np.empty((64, 96, 3), np.uint8)
    page[:, :48], page[:, 48:] = (200, 220, 240), (230, 215, 200)
    page[20:40, 10:30] = (210, 235, 225)
    return page


@pytest.fixture(scope="module")
def pages():
    return [_text_page(3, 96, 160), _flat_page()]


def _check(entry, page, channels=3):
    from PIL import Image

    from yomitoku_amd.flate import EncodedLossless

    want = R.encode(page if channels == 3 or page.ndim == 2 else page[:, :, 0])
    assert isinstance(entry, EncodedLossless) and entry.data == want
    assert (entry.width, entry.height, entry.channels, entry.scale, entry.nbytes) == (page.shape[1], page.shape[0], channels, 1.0, len(want))
    got = np.asarray(Image.open(io.BytesIO(entry.to_png())))
    assert np.array_equal(got, page[:, :, ::-1] if channels == 3 else (page if page.ndim == 2 else page[:, :, 0]))


@pytest.mark.parametrize("which", ["analyzer", "ocr"])
def test_every_entry_ends_with_the_definitions_file_and_the_schemas_are_unchanged(which, pages, request):
    from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

    an = request.getfixturevalue(which)
    base = an.serve(pages, wave=2, jpeg="high")
    got = an.serve(pages, wave=2, jpeg="high", jpeg_lossless=True)
    assert len(got) == len(base) == len(pages)
    for entry, plain, page in zip(got, base, pages):
        assert isinstance(entry, tuple) and len(entry) == 2
        assert entry[0].model_dump() == plain[0].model_dump()
        _check(entry[1], page)
        assert np.array_equal(R.decode(entry[1].data, entry[1].height, entry[1].width, 3), page)  # the page as it arrived
    pdf = searchable_pdf_bytes([e[1] for e in got], [e[0] for e in got])
    assert pdf.count(b"/Filter /FlateDecode /DecodeParms << /Predictor 15 /Colors 3") == 2 and b"/DCTDecode" not in pdf
    # the switch belongs to the job: the next one is plain again, byte for byte
    after = an.serve(pages, wave=2, jpeg="high")
    assert [e[1] for e in after] == [e[1] for e in base] and [e[1].data for e in after] == [e[1].data for e in base]


def test_bilevel_and_mrc_decide_first_and_write_what_they_wrote(ocr):
    from yomitoku_amd.ccitt import EncodedBilevel
    from yomitoku_amd.mrc import EncodedMrc

    text = _text_page(4, 96, 160)
    v = np.where(text[..., 1] < 128, 0, 255).astype(np.uint8)
    job = [np.ascontiguousarray(np.stack([v] * 3, -1)), text, np.full((64, 96, 3), 250, np.uint8), _flat_page()]
    assert [ccitt_ref.is_bilevel(p) for p in job] == [True, False, False, False]
    assert [mrc_ref.separate(p)[0] for p in job[1:]] == [1, 0, 0]
    base = ocr.serve(job, wave=4, jpeg="high", jpeg_bilevel="auto", jpeg_mrc=True)
    got = ocr.serve(job, wave=4, jpeg="high", jpeg_bilevel="auto", jpeg_mrc=True, jpeg_lossless=True)
    assert isinstance(got[0][1], EncodedBilevel) and got[0][1] == base[0][1] and got[0][1].data == base[0][1].data
    assert isinstance(got[1][1], EncodedMrc) and got[1][1] == base[1][1]
    assert (got[1][1].mask.data, got[1][1].foreground.data, got[1][1].background.data) == (
        base[1][1].mask.data, base[1][1].foreground.data, base[1][1].background.data)
    for k in (2, 3):
        _check(got[k][1], job[k])
    assert [e[0].model_dump() for e in got] == [e[0].model_dump() for e in base]


def test_grey_auto_writes_a_grey_three_channel_page_as_one_channel(dev, pages):
    from yomitoku_amd.jpeg import encode_jpeg_pages

    g = pages[0][..., 1]
    job = [np.ascontiguousarray(np.stack([g] * 3, -1)), pages[1], np.ascontiguousarray(g)]
    got = encode_jpeg_pages(job, "high", grey="auto", lossless=True)
    _check(got[0], job[0], channels=1)
    _check(got[1], job[1])
    _check(got[2], job[2], channels=1)
    plain = encode_jpeg_pages(job, "high", lossless=True)  # without the test the grey page keeps its three channels
    _check(plain[0], job[0])


def test_a_page_over_the_budget_gets_the_jpeg_of_the_job_without_the_switch(ocr, pages):
    from yomitoku_amd.jpeg import EncodedJpeg, encode_jpeg_pages

    noise = np.random.default_rng(2).integers(0, 256, (64, 96, 3), dtype=np.uint8)
    job = [pages[1], noise]
    assert len(R.encode(job[0])) * 256 <= 13 * 64 * 96 < len(R.encode(noise)) * 256  # ceil(256 x 0.05) = 13
    caps = [4 * p.size for p in job]  # noise does not fit a JPEG's default capacity
    base = encode_jpeg_pages(job, "high", capacities=caps)
    got = encode_jpeg_pages(job, "high", capacities=caps, lossless={"budget": 0.05})
    _check(got[0], job[0])
    assert isinstance(got[1], EncodedJpeg) and got[1] == base[1] and got[1].data == base[1].data
    served = ocr.serve([job[0], pages[0]], wave=2, jpeg="high", jpeg_lossless={"budget": 0.05})
    plain = ocr.serve([job[0], pages[0]], wave=2, jpeg="high")
    _check(served[0][1], job[0])
    assert len(R.encode(pages[0])) * 256 > 13 * pages[0].shape[0] * pages[0].shape[1]  # the textured page: over the budget
    assert isinstance(served[1][1], EncodedJpeg) and served[1][1] == plain[1][1] and served[1][1].data == plain[1][1].data
    assert [e[0].model_dump() for e in served] == [e[0].model_dump() for e in plain]


def test_with_deskew_the_file_is_of_the_corrected_page(ocr):
    from PIL import Image

    from yomitoku_amd.deskew import PageSkew

    page = _text_page(3, 600, 640)
    turned = np.ascontiguousarray(np.asarray(Image.fromarray(page).rotate(-2, Image.BICUBIC, fillcolor=(255, 255, 255))))
    fixed, k = deskew_ref.deskew(turned)[:2]
    assert k != 0
    got = ocr.serve([turned], wave=2, jpeg="high", jpeg_lossless=True, deskew=True)
    assert len(got[0]) == 3 and isinstance(got[0][2], PageSkew) and got[0][2].index == k
    entry = got[0][1]
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(entry.to_png())))[:, :, ::-1], fixed)  # Pillow reads the corrected page back
    assert entry.data == R.encode(fixed)


def test_the_switch_is_refused_before_a_source_is_read(analyzer, ocr):
    def sources():
        raise AssertionError("a source was read")
        yield

    for an in (analyzer, ocr):
        with pytest.raises(ValueError, match="jpeg_lossless"):
            an.serve(sources(), wave=2, jpeg_lossless=True)
        for bad in ("auto", 1, {"budget": 0}, {"bytes": 2}):
            with pytest.raises(ValueError, match="lossless"):
                an.serve(sources(), wave=2, jpeg="high", jpeg_lossless=bad)
