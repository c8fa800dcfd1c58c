"""DocumentAnalyzer.serve / OCR.serve(jpeg=..., jpeg_bilevel="auto"): a two-valued page's entry ends with its Group 4 file -
full size, lossless - and every other page's with the JPEG file it gets without the switch, in the same job.  The analyzers and
their seeded weights are those of tests/test_serving_gpu.py and tests/test_ocr_serve_gpu.py; the files' definition is
tests/ccitt_ref.py."""
import io

import numpy as np
import pytest
from PIL import Image

from tests import ccitt_ref
from tests.test_serving_gpu import _analyzer

pytestmark = pytest.mark.gpu

TWO_VALUED = [1, 4, 5]  # of the good pages
BAD_AT = 2  # of the sources


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
    """Six small pages, two of them wider than the "middle" preset's 2000 pixels; three thresholded at 128 in every channel: a
    1-bit scan as load_image hands it over, B G R with every sample 0 or 255."""
    from yomitoku_amd.utils.synth import synthetic_page_with_truth

    out = [synthetic_page_with_truth(3 + i, h, w)[0] for i, (h, w) in enumerate([(640, 600), (600, 640), (500, 700), (500, 700), (500, 700), (640, 600)])]
    out[3], out[4] = (np.ascontiguousarray(np.hstack([out[k]] * 3)) for k in (3, 4))  # 500 x 2100
    for k in TWO_VALUED:
        v = np.where(out[k][..., 1] < 128, 0, 255).astype(np.uint8)
        out[k] = np.ascontiguousarray(np.stack([v] * 3, -1))
    assert [ccitt_ref.is_bilevel(p) for p in out] == [k in TWO_VALUED for k in range(6)]
    assert all(0.001 < (out[k] == 0).mean() < 0.5 for k in TWO_VALUED)
    return out


@pytest.fixture(scope="module")
def streams(pages):
    """The definition's stream of every two-valued page, computed once."""
    return {k: ccitt_ref.encode_g4(ccitt_ref.black_mask(pages[k])) for k in TWO_VALUED}


def _sources(pages):
    return pages[:BAD_AT] + [np.zeros((50, 60), dtype=np.uint8)] + pages[BAD_AT:]  # a 2-D array: a source the pipeline refuses


@pytest.mark.parametrize("which", ["analyzer", "ocr"])
def test_serve_bilevel_auto_gives_group4_files_next_to_the_jpegs(which, pages, streams, request):
    from yomitoku_amd.ccitt import EncodedBilevel
    from yomitoku_amd.jpeg import EncodedJpeg, encode_jpeg_pages
    from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

    an = request.getfixturevalue(which)
    base = an.serve(_sources(pages), wave=2, jpeg="middle")
    got = an.serve(_sources(pages), wave=2, jpeg="middle", jpeg_bilevel="auto")
    assert len(got) == len(base) == 7 and isinstance(got[BAD_AT], Exception) and isinstance(base[BAD_AT], Exception)
    got, base = got[:BAD_AT] + got[BAD_AT + 1 :], base[:BAD_AT] + base[BAD_AT + 1 :]
    # with the switch off the job's files are encode_jpeg_pages', as they always were
    files = encode_jpeg_pages(pages, "middle")
    assert [e[1] for e in base] == files and all(isinstance(f, EncodedJpeg) for f in files)
    assert [(f.width, f.height) for f in files[3:5]] == [(2000, 476)] * 2 and files[3].scale == 2000 / 2100
    for k, (page, entry, plain) in enumerate(zip(pages, got, base)):
        assert isinstance(entry, tuple) and len(entry) == 2
        assert entry[0].model_dump() == plain[0].model_dump()
        if k in TWO_VALUED:
            assert isinstance(entry[1], EncodedBilevel) and entry[1].data == streams[k]
            assert (entry[1].width, entry[1].height, entry[1].scale) == (page.shape[1], page.shape[0], 1.0)
            image = Image.open(io.BytesIO(entry[1].to_tiff()))
            image.load()
            assert np.array_equal(np.where(np.asarray(image.convert("L")) == 0, 0, 255), page[..., 0])
            assert len(entry[1].data) < len(plain[1].data)
        else:
            assert entry[1] == plain[1]
    pdf = searchable_pdf_bytes([e[1] for e in got], [e[0] for e in got])
    assert pdf.count(b"/Filter /CCITTFaxDecode") == 3 and pdf.count(b"/Filter /DCTDecode") == 3
    assert all(streams[k] in pdf for k in TWO_VALUED) and all(got[k][1].data in pdf for k in (0, 2, 3))
    assert pdf.count(b"/MediaBox [0 0 2100 500]") == 1 and pdf.count(b"/MediaBox [0 0 2000 476]") == 1
    # the other options of the job do not reach a two-valued page; the switch belongs to the job: the next one is plain again
    more = an.serve(pages[:2], wave=2, jpeg="middle", jpeg_bilevel="auto", jpeg_optimize=True, jpeg_subsampling="4:4:4", jpeg_grey="auto")
    assert more[1][1] == got[1][1] and isinstance(more[0][1], EncodedJpeg) and more[0][1].optimized and more[0][1].subsampling == "4:4:4"
    after = an.serve(pages[:2], wave=2, jpeg="middle")
    assert [e[1] for e in after] == files[:2]


def test_bad_values_are_refused_before_a_source_is_read(analyzer, ocr):
    def sources():
        raise AssertionError("a source was read")
        yield

    for an in (analyzer, ocr):
        with pytest.raises(ValueError, match="jpeg_bilevel"):
            an.serve(sources(), wave=2, jpeg_bilevel="auto")
        for bad in (True, "always", 1):
            with pytest.raises(ValueError, match="bilevel"):
                an.serve(sources(), wave=2, jpeg="high", jpeg_bilevel=bad)
