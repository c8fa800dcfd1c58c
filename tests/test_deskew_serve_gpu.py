"""serve(deskew=True): the pages of a job turned upright on the device behind their upload, so that every chain, the overlays and
the page files see the corrected page (yomitoku_amd/serving.py, yomitoku_amd/deskew.py).  What a page gets must be what the
same job gives the page corrected by the definition (tests/deskew_ref.py), and its entry ends with its PageSkew.  The analyzers
and their seeded weights are those of tests/test_ocr_serve_gpu.py and tests/test_serving_gpu.py."""
import os

import numpy as np
import pytest

from tests import deskew_ref as R
from tests.test_ocr_serve_gpu import _ocr
from tests.test_pipeline_gpu import _assert_same_schema
from tests.test_serving_gpu import _analyzer

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_page.jpg")


def _bgr(grey):
    return np.ascontiguousarray(np.stack([np.asarray(grey)] * 3, -1))


@pytest.fixture(scope="module")
def job():
    """(pages, what the definition makes of them as (corrected page, k)): a golden crop turned by 3 degrees, the upright crop,
    a synthetic page with words turned by -2 degrees."""
    from PIL import Image

    from yomitoku_amd.utils.synth import synthetic_page_with_truth

    golden = Image.open(GOLDEN).convert("L")
    synth = synthetic_page_with_truth(3, 640, 600)[0]
    pages = [_bgr(golden.rotate(3, Image.BICUBIC, fillcolor=255))[40:680], _bgr(golden)[40:680],
             np.ascontiguousarray(np.asarray(Image.fromarray(synth).rotate(-2, Image.BICUBIC, fillcolor=(255, 255, 255))))]
    pages = [np.array(p, order="C") for p in pages]
    fixed = [R.deskew(p)[:2] for p in pages]
    assert abs(fixed[0][1] * 0.1 - 3.0) <= 0.1 + 1e-9 and fixed[1][1] == 0 and fixed[1][0].tobytes() == pages[1].tobytes()
    return pages, fixed


@pytest.fixture(scope="module")
def ocr(dev):
    an = _ocr()
    yield an
    an.close()


def _sources(pages, tmp_path):
    return [pages[0], pages[1], str(tmp_path / "nope.png"), pages[2]], [0, 1, 3]


def _check_skews(entries, keep, fixed, pages):
    from yomitoku_amd.deskew import PageSkew

    for k, (_, want_k), page in zip(keep, fixed, pages):
        skew = entries[k][-1]
        assert isinstance(skew, PageSkew) and skew.index == want_k and skew.estimated
        assert skew.angle == pytest.approx(want_k * 0.1) and (skew.angle == 0.0) == (want_k == 0)
        h, w = page.shape[:2]
        assert np.allclose(skew.to_original([(w - 1) / 2, (h - 1) / 2]), [(w - 1) / 2, (h - 1) / 2])


def test_ocr_serve_deskew_equals_serving_the_corrected_pages(ocr, job, tmp_path):
    from yomitoku_amd.schemas import OCRSchema

    pages, fixed = job
    sources, keep = _sources(pages, tmp_path)
    plain_before = ocr.serve(sources, wave=4)
    want = ocr.serve([f[0] for f in fixed], wave=4)
    got = ocr.serve(sources, wave=4, deskew=True)
    assert len(got) == 4 and isinstance(got[2], Exception) and not isinstance(got[2], tuple)  # the source that fails to load
    assert sum(len(w.words) for w in want) > 0
    for k, w in zip(keep, want):
        assert isinstance(got[k], tuple) and len(got[k]) == 2 and isinstance(got[k][0], OCRSchema)
        _assert_same_schema(w.model_dump(), got[k][0].model_dump())
    _check_skews(got, keep, fixed, pages)
    # the upright page: the plain job's entry, plus a PageSkew of angle 0
    _assert_same_schema(plain_before[1].model_dump(), got[1][0].model_dump())
    assert got[1][1].angle == 0.0 and got[1][1].index == 0 and np.array_equal(got[1][1].matrix, [[1, 0, 0], [0, 1, 0]])
    # a job without the switch on the same pipeline, after one with it: today's entries
    after = ocr.serve(sources, wave=4)
    assert isinstance(after[2], Exception)
    for k in keep:
        assert isinstance(after[k], OCRSchema)
        _assert_same_schema(plain_before[k].model_dump(), after[k].model_dump())
    # other angles: a dict of parameters, held to the definition's choice for them
    coarse = ocr.serve(pages[:1], wave=4, deskew={"step": 0.5, "max_angle": 4.0})
    assert coarse[0][1].index == R.estimate(pages[0], 0.5, 4.0)[0] != 0 and coarse[0][1].angle == pytest.approx(0.5 * coarse[0][1].index)
    with pytest.raises(ValueError, match="deskew"):
        ocr.serve(pages[:1], deskew="yes")


def test_ocr_serve_deskew_with_page_files(ocr, job, tmp_path):
    from yomitoku_amd.jpeg import EncodedJpeg, encode_jpeg_pages

    pages, fixed = job
    sources, keep = _sources(pages, tmp_path)
    got = ocr.serve(sources, wave=4, deskew=True, jpeg="high")
    files = encode_jpeg_pages([f[0] for f in fixed], "high")
    assert isinstance(got[2], Exception)
    for k, want in zip(keep, files):
        assert isinstance(got[k], tuple) and len(got[k]) == 3 and isinstance(got[k][1], EncodedJpeg)
        assert got[k][1] == want and got[k][1].data == want.data  # byte for byte the file of the corrected page
    _check_skews(got, keep, fixed, pages)


def test_ocr_serve_deskew_with_overlays_draws_on_the_corrected_page(ocr, job, tmp_path):
    pages, fixed = job
    sources, keep = _sources(pages, tmp_path)
    want = ocr.serve([f[0] for f in fixed], wave=4, overlays=True)
    got = ocr.serve(sources, wave=4, deskew=True, overlays=True)
    assert isinstance(got[2], Exception)
    for k, (schema, picture), page in zip(keep, want, pages):
        assert isinstance(got[k], tuple) and len(got[k]) == 3
        _assert_same_schema(schema.model_dump(), got[k][0].model_dump())
        assert np.array_equal(got[k][1], picture) and got[k][1].shape == page.shape
    assert not np.array_equal(got[0][1], pages[0])  # not the page as it arrived
    _check_skews(got, keep, fixed, pages)


def test_a_page_re_run_alone_is_estimated_again(ocr, job):
    """a wave that fails is re-run page by page from the host originals: every page is corrected again, the culprit fails alone"""
    pages, fixed = job
    det = ocr.detector
    inner = det.forward_pages
    bad = pages[1].copy()
    bad[0, 0, 0] = 7  # upright: the copy keeps the mark

    def touchy(wave_pages, **kw):
        for page in wave_pages:
            if tuple(page.shape) == bad.shape and int(page[0, 0, 0]) == 7:
                raise RuntimeError("detector choked on this page")
        return inner(wave_pages, **kw)

    want = ocr.serve([fixed[0][0], fixed[2][0]], wave=4)
    det.forward_pages = touchy
    try:
        got = ocr.serve([pages[0], bad, pages[2]], wave=4, deskew=True)
    finally:
        del det.forward_pages
    assert isinstance(got[1], RuntimeError) and "choked" in str(got[1])
    assert ocr._pipeline.last_job["retried_pages"] == 3
    for k, w, f in ((0, want[0], fixed[0]), (2, want[1], fixed[2])):
        _assert_same_schema(w.model_dump(), got[k][0].model_dump())
        assert got[k][1].index == f[1]


def test_document_analyzer_serve_deskew_equals_serving_the_corrected_pages(dev, job, tmp_path):
    from yomitoku_amd.schemas import DocumentAnalyzerSchema

    pages, fixed = job
    sources, keep = _sources(pages, tmp_path)
    an = _analyzer()
    try:
        want = an.serve([f[0] for f in fixed], wave=4)
        got = an.serve(sources, wave=4, deskew=True)  # one wave
        assert an._pipeline.last_job["waves"] == 1 and isinstance(got[2], Exception)
        for k, w in zip(keep, want):
            assert isinstance(got[k], tuple) and len(got[k]) == 2 and isinstance(got[k][0], DocumentAnalyzerSchema)
            _assert_same_schema(w.model_dump(), got[k][0].model_dump())
        _check_skews(got, keep, fixed, pages)
        after = an.serve(pages, wave=4)
        assert all(isinstance(e, DocumentAnalyzerSchema) for e in after)
    finally:
        an.close()


def test_serve_sharded_refuses_deskew(job):
    from yomitoku_amd.distributed import ShardedServer

    server = ShardedServer.__new__(ShardedServer)  # no process group: the refusal comes before anything is served
    with pytest.raises(NotImplementedError, match="deskew"):
        server.serve_local(job[0][:1], deskew=True)
