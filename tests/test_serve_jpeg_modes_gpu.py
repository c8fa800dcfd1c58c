"""DocumentAnalyzer.serve / OCR.serve(jpeg=..., jpeg_subsampling="4:4:4", jpeg_grey="auto"): every page's JPEG file in the mode the
job asks for, a grey-valued page as a grey file, made in the render stage.  The analyzers and their seeded weights are those of
tests/test_serving_gpu.py and tests/test_ocr_serve_gpu.py; the files' definition is tests/jpeg_modes_ref.py."""
import io

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_modes_ref
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


@pytest.fixture(scope="module")
def pages():
    """Three small pages; the middle one grey-valued (B == G == R): a black-and-white scan as load_image hands it over."""
    from yomitoku_amd.utils.synth import synthetic_page_with_truth

    out = [synthetic_page_with_truth(3 + i, h, w)[0] for i, (h, w) in enumerate([(640, 600), (600, 640), (500, 700)])]
    out[1] = np.ascontiguousarray(np.stack([out[1][..., 1]] * 3, -1))
    return out


@pytest.fixture(scope="module")
def files(pages):
    """The definition's file of every page at the "high" preset's quality, computed once."""
    return [jpeg_modes_ref.encode(p, 85, "4:4:4", grey="auto") for p in pages]


def _pixels(data):
    image = Image.open(io.BytesIO(data))
    image.load()
    return image.mode, np.asarray(image)


@pytest.mark.parametrize("which", ["analyzer", "ocr"])
def test_serve_444_auto_grey_gives_the_definitions_files_and_the_same_schemas(which, pages, files, request):
    from yomitoku_amd.jpeg import EncodedJpeg, encode_jpeg_pages

    an = request.getfixturevalue(which)
    plain = an.serve(pages, wave=2, jpeg="high")
    got = an.serve(pages, wave=2, jpeg="high", jpeg_subsampling="4:4:4", jpeg_grey="auto")
    opt = an.serve(pages, wave=2, jpeg="high", jpeg_subsampling="4:4:4", jpeg_grey="auto", jpeg_optimize=True)
    direct = encode_jpeg_pages(pages, "high", subsampling="4:4:4", grey="auto")
    for k, (page, want, base, entry, small, alone) in enumerate(zip(pages, files, plain, got, opt, direct)):
        assert isinstance(entry, tuple) and len(entry) == 2 and isinstance(entry[1], EncodedJpeg)
        assert entry[0].model_dump() == base[0].model_dump() == small[0].model_dump()
        assert entry[1].data == want and entry[1] == alone
        assert (entry[1].grey, entry[1].subsampling) == ((True, None) if k == 1 else (False, "4:4:4"))
        assert (entry[1].width, entry[1].height, entry[1].scale, entry[1].optimized) == (page.shape[1], page.shape[0], 1.0, False)
        assert (base[1].grey, base[1].subsampling) == (False, "4:2:0")
        mode, pixels = _pixels(entry[1].data)
        assert mode == ("L" if k == 1 else "RGB") and pixels.shape[:2] == page.shape[:2]
        # with the page's own Huffman tables: the same pixels, fewer bytes
        assert small[1].optimized and (small[1].grey, small[1].subsampling) == (entry[1].grey, entry[1].subsampling)
        assert len(small[1].data) < len(entry[1].data)
        assert _pixels(small[1].data)[0] == mode and np.array_equal(_pixels(small[1].data)[1], pixels)
    # the options belong to the job: the next one is plain again
    after = an.serve(pages[:2], wave=2, jpeg="high")
    assert [e[1] for e in after] == [e[1] for e in plain[:2]]


def test_searchable_pdf_from_the_jobs_output(analyzer, pages, files):
    from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

    out = analyzer.serve(pages, wave=2, jpeg="high", jpeg_subsampling="4:4:4", jpeg_grey="auto")
    pdf = searchable_pdf_bytes([e[1] for e in out], [e[0] for e in out])
    assert [f in pdf for f in files] == [True] * 3
    assert pdf.count(b"/ColorSpace /DeviceRGB") == 2 and pdf.count(b"/ColorSpace /DeviceGray") == 1


def test_bad_values_are_refused_before_a_source_is_read(analyzer, ocr):
    def sources():
        raise AssertionError("a source was read")
        yield

    for an in (analyzer, ocr):
        with pytest.raises(ValueError, match="jpeg_subsampling"):
            an.serve(sources(), wave=2, jpeg_subsampling="4:4:4")
        with pytest.raises(ValueError, match="jpeg_grey"):
            an.serve(sources(), wave=2, jpeg_grey="auto")
        with pytest.raises(ValueError, match="4:1:1"):
            an.serve(sources(), wave=2, jpeg="high", jpeg_subsampling="4:1:1")
