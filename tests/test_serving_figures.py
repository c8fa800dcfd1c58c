"""The page pipeline's third render product (yomitoku_amd/serving.py: serve(figures=...)) with stub stages on the host, in the
manner of tests/test_serving_ocr.py: the entry shapes of a figures job alone and next to overlays, page files and a page skew,
page order, a page that fails in `finish` or in the figures product, the wave slots, and that a job without a render product
never starts the render thread."""
import threading
from types import SimpleNamespace

import numpy as np
import pytest

from tests.test_serving_ocr import RenderStub, page
from yomitoku_amd.figures import check_figures
from yomitoku_amd.serving import PagePipeline, check_jpeg_preset


class FiguresStub(RenderStub):
    """RenderStub with a recording figures product; a page whose pixel [0, 2, 0] is 88 has no figures product, a job whose
    `options` say so fails the whole launch, and `skew` True gives every wave a stub skew step."""

    def __init__(self, skew=False):
        super().__init__()
        self.skew = skew
        self.figure_calls = []

    def _stage_detect(self, wave):
        super()._stage_detect(wave)
        if self.skew:
            wave.skew = SimpleNamespace(skews=lambda ids=tuple(wave.ids): [f"skew:{i}" for i in ids])

    def _stage_figures(self, wave, results):
        assert threading.current_thread().name == "ymk-render" and wave.pages is not None
        self.figure_calls.append((tuple(wave.ids), wave.job.figures))
        if wave.job.options == "figures launch fails":
            raise RuntimeError("the crop launch failed")
        out = []
        for k, img in enumerate(wave.imgs):
            if isinstance(results[k], BaseException):
                out.append(None)
            elif img[0, 2, 0] == 88:
                out.append(ValueError("this page is no page"))
            else:
                out.append((f"figures:{wave.ids[k]}",))
        return out


def _pages():
    pages = [page(i) for i in range(8)]
    pages[3][0, 2, 0] = 88  # fails in the figures product
    pages[6] = page(6, poison_stage=6)  # fails in finish: the bare exception, never cut
    return pages, [i for i in range(8) if i not in (3, 6)]


def test_entry_shapes_of_a_figures_job():
    in_flight = 2
    an = FiguresStub()
    pipe = PagePipeline(an, wave=3, in_flight=in_flight)
    pages, good = _pages()
    opts = check_figures(True)

    out = pipe.serve(pages, figures=opts)
    assert len(out) == 8
    assert isinstance(out[3], ValueError) and "no page" in str(out[3]) and isinstance(out[6], ValueError) and "poisoned" in str(out[6])
    for i in good:
        schema, made = out[i]
        assert schema[0] == i and made == f"figures:{i}"  # in page order
    # one call per wave, whole waves (two recogniser lanes: the waves may reach the render stage in either order)
    assert sorted(ids for ids, _ in an.figure_calls) == [(0, 1, 2), (3, 4, 5), (6, 7)] and all(o is opts for _, o in an.figure_calls)

    out = pipe.serve(pages, files=check_jpeg_preset("high"), figures=opts)
    for i in good:
        schema, file, made = out[i]
        assert (schema[0], file, made) == (i, f"file:{i}", f"figures:{i}")
    assert isinstance(out[3], ValueError) and isinstance(out[6], ValueError)

    out = pipe.serve(pages, overlays=True, files=check_jpeg_preset("high"), figures=opts)
    for i in good:
        schema, picture, file, made = out[i]
        assert schema[0] == i and int(picture[0, 0, 0]) == i and (file, made) == (f"file:{i}", f"figures:{i}")

    out = pipe.serve(pages, overlays=True, figures=opts)
    for i in good:
        schema, picture, made = out[i]
        assert schema[0] == i and int(picture[0, 0, 0]) == i and made == f"figures:{i}"

    # a launch failure of the product fails the wave's pages, as it does for the other two products
    out = pipe.serve(pages[:4], figures=opts, options="figures launch fails")
    assert all(isinstance(e, RuntimeError) and "crop launch" in str(e) for e in out)

    # without the switch: the entries of before, and the product is not asked
    calls = len(an.figure_calls)
    out = pipe.serve(pages, files=check_jpeg_preset("high"))
    assert [out[i] for i in good + [3]] == [((i, (i + 1000) * 2, 3 if i < 6 else 2), f"file:{i}") for i in good + [3]]
    assert len(an.figure_calls) == calls

    assert pipe._rings.qsize() == in_flight  # every wave slot was given back
    done = []
    t = threading.Thread(target=lambda: done.extend(pipe.serve([page(i) for i in range(3 * (in_flight + 1))], figures=opts)), daemon=True)
    t.start()
    t.join(20)
    assert not t.is_alive(), "a job of in_flight + 1 waves is still waiting for a wave slot"
    assert [e[1] for e in done] == [f"figures:{i}" for i in range(3 * (in_flight + 1))]
    assert pipe._rings.qsize() == in_flight
    pipe.close()


def test_the_figures_stand_behind_the_page_file_and_in_front_of_the_skew():
    pipe = PagePipeline(FiguresStub(skew=True), wave=3, in_flight=2)
    pages, good = _pages()
    opts = check_figures({"quality": 80})
    out = pipe.serve(pages, overlays=True, files=check_jpeg_preset("high"), figures=opts)
    for i in good:
        schema, picture, file, made, skew = out[i]
        assert schema[0] == i and int(picture[0, 0, 0]) == i and (file, made, skew) == (f"file:{i}", f"figures:{i}", f"skew:{i}")
    assert isinstance(out[3], ValueError) and isinstance(out[6], ValueError)  # a failed page stays its bare exception
    out = pipe.serve(pages, figures=opts)
    assert [out[i][1:] for i in good] == [(f"figures:{i}", f"skew:{i}") for i in good]
    out = pipe.serve(pages)  # the skew alone: the pair of before
    assert [out[i][1] for i in good + [3]] == [f"skew:{i}" for i in good + [3]]
    pipe.close()


def test_a_job_without_a_render_product_never_starts_the_render_thread():
    an = FiguresStub()
    pipe = PagePipeline(an, wave=3, in_flight=2)
    out = pipe.serve([page(i) for i in range(5)])
    assert [o[0] for o in out] == list(range(5)) and pipe._render_thread is None and an.figure_calls == []
    out = pipe.serve([page(i) for i in range(5)], figures=None)
    assert [o[0] for o in out] == list(range(5)) and pipe._render_thread is None
    pipe.serve([page(0)], figures=check_figures(True))
    assert pipe._render_thread is not None and pipe._render_thread.is_alive()
    pipe.close()
    assert pipe._render_thread is None


def test_the_public_entries_check_the_switch_before_anything_else():
    """DocumentAnalyzer.serve runs check_figures before the pipeline is built or a source is read; the sharded server refuses."""
    import inspect

    from yomitoku_amd import OCR, DocumentAnalyzer, TableSemanticParser
    from yomitoku_amd.distributed import ShardedServer

    assert inspect.signature(DocumentAnalyzer.serve).parameters["figures"].default is None
    assert "figures" not in inspect.signature(OCR.serve).parameters and "figures" not in inspect.signature(TableSemanticParser.serve).parameters

    def sources():
        raise AssertionError("a source was read")
        yield

    an = DocumentAnalyzer.__new__(DocumentAnalyzer)  # no models: the refusal comes before anything is built
    for bad in ("x", 0, {"quality": 0}, {"size": 3}):
        with pytest.raises(ValueError, match="figures"):
            an.serve(sources(), figures=bad)
    server = ShardedServer.__new__(ShardedServer)  # no process group: the refusal comes before anything is served
    for value in (True, 90, {"quality": 90}):
        with pytest.raises(NotImplementedError, match="figures"):
            server.serve_local([np.zeros((4, 4, 3), np.uint8)], figures=value)
