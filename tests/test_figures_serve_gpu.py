"""serve(figures=...): the crops of every page's `schema.figures`, cut and JPEG-coded in the render stage from the page on the
device (yomitoku_amd/serving.py, yomitoku_amd/figures.py).  Seeded weights detect noise, so a Handover's `layouts` hook puts two
figures on every page; the analyzer and its weights are those of tests/test_serving_gpu.py."""
import numpy as np
import pytest

from tests.test_pipeline_gpu import _assert_same_schema
from tests.test_serving_gpu import _analyzer

pytestmark = pytest.mark.gpu


def _figure_boxes(h, w):
    return [[w // 10, h // 5, w // 2 - 3, h // 2 + 1], [w // 2, (3 * h) // 5, w, h]]  # the second touches the right and bottom edges


@pytest.fixture(scope="module")
def an(dev):
    from yomitoku_amd.schemas import Element, LayoutAnalyzerSchema
    from yomitoku_amd.testing import Handover

    class TwoFigures(Handover):
        def layouts(self, wave, lays):
            out = []
            for (h, w), lay in zip(wave.sizes, lays):
                figures = [Element(id=None, box=b, score=1.0, role=None, contents=None) for b in _figure_boxes(h, w)]
                out.append(LayoutAnalyzerSchema(paragraphs=lay.paragraphs, tables=lay.tables, figures=figures))
            return out

    analyzer = _analyzer()
    analyzer.handover = TwoFigures()
    yield analyzer
    analyzer.close()


@pytest.fixture(scope="module")
def pages():
    from PIL import Image

    from yomitoku_amd.utils.synth import synthetic_page_with_truth

    flat = [synthetic_page_with_truth(3 + i, h, w)[0] for i, (h, w) in enumerate([(1000, 1400), (1400, 1000), (1000, 1400)])]
    flat[2] = np.array(Image.fromarray(flat[2]).rotate(-2, Image.BICUBIC, fillcolor=(255, 255, 255)), order="C")  # a skewed page
    return flat


def _sources(pages, tmp_path):
    return [pages[0], str(tmp_path / "nope.png"), pages[1], pages[2]], [0, 2, 3]


def test_entries_are_schema_and_page_figures_and_the_files_are_the_host_pages_crops(an, pages, tmp_path):
    from PIL import Image

    from yomitoku_amd.export import export_markdown
    from yomitoku_amd.figures import PageFigures, crop_figure_files
    from yomitoku_amd.jpeg import EncodedJpeg
    from yomitoku_amd.schemas import DocumentAnalyzerSchema

    sources, keep = _sources(pages, tmp_path)
    plain = an.serve(sources, wave=4)
    got = an.serve(sources, wave=4, figures=True)
    assert len(got) == 4 and isinstance(got[1], Exception) and not isinstance(got[1], tuple)  # the source that fails to load
    for k, page in zip(keep, pages):
        assert isinstance(plain[k], DocumentAnalyzerSchema)  # without the switch: the entry of before
        assert isinstance(got[k], tuple) and len(got[k]) == 2
        schema, made = got[k]
        assert isinstance(schema, DocumentAnalyzerSchema) and isinstance(made, PageFigures)
        _assert_same_schema(plain[k].model_dump(), schema.model_dump())
        boxes = [f.box for f in schema.figures]
        assert len(boxes) == 2 and sorted(boxes) == sorted(_figure_boxes(*page.shape[:2]))
        want = crop_figure_files([page], [boxes])[0]
        assert len(made) == 2 and all(isinstance(f, EncodedJpeg) for f in made)
        assert made.rects == want.rects == tuple(tuple(b) for b in boxes) and made == want  # byte for byte
    # what the files are for
    schema, made = got[0]
    path = tmp_path / "out" / "page.md"
    (tmp_path / "out").mkdir()
    md = export_markdown(schema, str(path), figures=made)
    for i, (x1, y1, x2, y2) in enumerate(made.rects):
        name = f"figures/page_figure_{i}.png"
        assert name in md
        with Image.open(tmp_path / "out" / name) as im:
            assert im.format == "JPEG" and im.size == (x2 - x1, y2 - y1)
    # an int and a dict of options; a job without the switch afterwards
    q70 = an.serve(pages[:1], wave=4, figures={"quality": 70, "max_side": 256})
    want = crop_figure_files(pages[:1], [[f.box for f in q70[0][0].figures]], figures={"quality": 70, "max_side": 256})[0]
    assert q70[0][1] == want and max(q70[0][1].files[0].width, q70[0][1].files[0].height) <= 256 and q70[0][1].files[0].scale < 1.0
    after = an.serve(pages[:1], wave=4)
    assert isinstance(after[0], DocumentAnalyzerSchema)
    _assert_same_schema(plain[0].model_dump(), after[0].model_dump())


def test_every_product_together_and_the_crops_are_the_corrected_pages(an, pages, tmp_path):
    from yomitoku_amd.deskew import PageSkew, deskew_pages
    from yomitoku_amd.figures import PageFigures, crop_figure_files
    from yomitoku_amd.jpeg import EncodedJpeg

    sources, keep = _sources(pages, tmp_path)
    got = an.serve(sources, wave=4, overlays=True, jpeg="high", deskew=True, figures=True)
    assert isinstance(got[1], Exception) and not isinstance(got[1], tuple)
    corrected, skews = deskew_pages(pages)
    assert skews[2].index != 0  # the third page was turned
    for k, page, fixed, skew in zip(keep, pages, corrected, skews):
        assert isinstance(got[k], tuple) and len(got[k]) == 6
        schema, ocr, layout, file, made, found = got[k]
        assert ocr.shape == layout.shape == page.shape and isinstance(file, EncodedJpeg) and isinstance(made, PageFigures)
        assert isinstance(found, PageSkew) and found.index == skew.index
        want = crop_figure_files([fixed], [[f.box for f in schema.figures]])[0]
        assert len(made) == 2 and made == want
    turned = crop_figure_files([pages[2]], [[f.box for f in got[3][0].figures]])[0]
    assert got[3][4] != turned  # not the page as it arrived


def test_the_switch_is_checked_before_a_source_is_read(an):
    def sources():
        raise AssertionError("a source was read")
        yield

    for bad in ("x", 0, {"quality": 0}, {"size": 3}):
        with pytest.raises(ValueError, match="figures"):
            an.serve(sources(), figures=bad)


def test_serve_sharded_refuses_figures(pages):
    from yomitoku_amd.distributed import ShardedServer

    server = ShardedServer.__new__(ShardedServer)  # no process group: the refusal comes before anything is served
    with pytest.raises(NotImplementedError, match="figures"):
        server.serve_local(pages[:1], figures=True)
