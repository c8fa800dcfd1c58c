"""DocumentAnalyzer.serve(jpeg=..., jpeg_optimize=True): every page's JPEG file coded with Huffman tables of its own, made in the
render stage.  The analyzer and its seeded weights are those of tests/test_serving_gpu.py; the files' definition is
tests/jpeg_opt_ref.py."""
import numpy as np
import pytest

from tests import jpeg_opt_ref
from tests.test_serving_gpu import _analyzer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def analyzer(dev):
    an = _analyzer()
    yield an
    an.close()


@pytest.fixture(scope="module")
def pages():
    from yomitoku_amd.utils.synth import synthetic_page_with_truth

    return [synthetic_page_with_truth(3 + i, h, w)[0] for i, (h, w) in enumerate([(640, 600), (600, 640), (500, 700)])]


@pytest.fixture(scope="module")
def files(pages):
    """The definition's file of every page at the "high" preset's quality, computed once."""
    return [jpeg_opt_ref.encode(p, 85) for p in pages]


def test_serve_jpeg_optimize_gives_the_definitions_files_and_the_same_schemas(analyzer, pages, files):
    from yomitoku_amd.jpeg import EncodedJpeg

    plain = analyzer.serve(pages, wave=2, jpeg="high")
    got = analyzer.serve(pages, wave=2, jpeg="high", jpeg_optimize=True)
    # a second job on the wave slots' used scratch, other pages in each slot (other waves too: its schemas are not compared)
    again = analyzer.serve(pages[::-1], wave=2, jpeg="high", jpeg_optimize=True)[::-1]
    for page, want, base, entry, second in zip(pages, files, plain, got, again):
        assert isinstance(entry, tuple) and len(entry) == 2 and isinstance(entry[1], EncodedJpeg)
        assert entry[0].model_dump() == base[0].model_dump()
        assert entry[1].data == want == second[1].data and entry[1].optimized and not base[1].optimized
        assert len(entry[1].data) < len(base[1].data)
        assert (entry[1].width, entry[1].height, entry[1].grey, entry[1].scale) == (page.shape[1], page.shape[0], False, 1.0)
    # the switch belongs to the job: the next one is plain again
    after = analyzer.serve(pages[:2], wave=2, jpeg="high")
    assert [e[1] for e in after] == [e[1] for e in plain[:2]]


def test_serve_jpeg_optimize_with_overlays_has_four_members(analyzer, pages, files):
    three = analyzer.serve(pages[:2], wave=2, overlays=True)
    four = analyzer.serve(pages[:2], wave=2, overlays=True, jpeg="high", jpeg_optimize=True)
    assert all(isinstance(e, tuple) and len(e) == 4 for e in four)
    for (schema, ocr, lay), entry, want in zip(three, four, files):
        assert entry[0].model_dump() == schema.model_dump()
        assert np.array_equal(entry[1], ocr) and np.array_equal(entry[2], lay)
        assert entry[3].data == want and entry[3].optimized


def test_jpeg_optimize_without_jpeg_is_a_value_error_before_a_source_is_read(analyzer):
    def sources():
        raise AssertionError("a source was read")
        yield

    with pytest.raises(ValueError, match="jpeg_optimize"):
        analyzer.serve(sources(), wave=2, jpeg_optimize=True)


def test_searchable_pdf_embeds_the_optimised_files(analyzer, pages, files):
    from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

    out = analyzer.serve(pages[:2], wave=2, jpeg="high", jpeg_optimize=True)
    pdf = searchable_pdf_bytes([e[1] for e in out], [e[0] for e in out])
    assert [f in pdf for f in files[:2]] == [True, True]
