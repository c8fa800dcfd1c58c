"""serve(overlays=True) with stub stages on the host (the manner of tests/test_serving.py): the render stage's place in the
pipeline - entries become triples in page order, only the waves of an overlays job visit it, a page failing there fails
alone, and its thread exists from the first such job until close()."""
import threading

import numpy as np

from tests.test_serving import StubAnalyzer, page
from yomitoku_amd.serving import PagePipeline


class RenderStub(StubAnalyzer):
    """A page whose third pixel is 77 fails in its drawing; 99 fails the whole render call."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.rendered = []

    def _stage_render(self, wave, results):
        assert wave.pages is not None and wave.dets is not None and wave.recs is not None and wave.lays is not None
        assert threading.current_thread().name == "ymk-render"
        self.rendered.append(tuple(wave.ids))
        out = []
        for k, img in enumerate(wave.imgs):
            if isinstance(results[k], BaseException):
                out.append(None)
            elif img[0, 1, 0] == 99:
                raise RuntimeError("render call failed")
            elif img[0, 1, 0] == 77:
                out.append(ValueError("cannot draw this page"))
            else:
                out.append((np.full((2, 2, 3), wave.ids[k], np.uint8), np.full((2, 2, 3), 100 + wave.ids[k], np.uint8)))
        return out


def _render_threads():
    return [t for t in threading.enumerate() if t.name == "ymk-render"]


def test_triples_in_page_order_then_plain_entries():
    an = RenderStub(delay=0.001)
    pipe = PagePipeline(an, wave=4, in_flight=3)
    assert pipe._render_thread is None and not _render_threads()
    plain = pipe.serve([page(i) for i in range(6)])
    assert [o[0] for o in plain] == list(range(6)) and not an.rendered
    assert pipe._render_thread is None and not _render_threads()  # no overlays job yet: no render thread
    pipe.trace = []
    out = pipe.serve([page(i) for i in range(10)], overlays=True)
    assert len(out) == 10 and all(isinstance(o, tuple) and len(o) == 3 for o in out)
    assert [o[0][0] for o in out] == list(range(10))  # the schema slot holds what finish made
    assert [int(o[1][0, 0, 0]) for o in out] == list(range(10)) and [int(o[2][0, 0, 0]) for o in out] == [100 + i for i in range(10)]
    assert sorted(an.rendered) == [(0, 1, 2, 3), (4, 5, 6, 7), (8, 9)]
    assert len(_render_threads()) == 1
    assert sorted(t[1:3] for t in pipe.trace if t[0] == "render") == sorted((s, n) for s, n in ((t[1], t[2]) for t in pipe.trace if t[0] == "finish"))
    # a plain job after an overlays job: plain entries, no render visit, today's stage names in the trace
    pipe.trace, an.rendered = [], []
    plain = pipe.serve([page(i) for i in range(6)])
    assert [o[0] for o in plain] == list(range(6)) and all(not isinstance(o[1], np.ndarray) for o in plain)
    assert not an.rendered and "render" not in {t[0] for t in pipe.trace}
    tagged = pipe.serve([page(0), page(1)], with_source=True, overlays=True)
    assert [(s, f) for s, f, _ in tagged] == [(0, 0), (1, 0)] and all(len(e) == 3 and isinstance(e[1], np.ndarray) for _, _, e in tagged)
    pipe.close()
    assert pipe._render_thread is None and not _render_threads()


def test_a_page_failing_in_the_render_fails_alone():
    an = RenderStub()
    pipe = PagePipeline(an, wave=4, in_flight=2)
    pages = [page(i) for i in range(10)]
    pages[5][0, 1, 0] = 77
    pages[2] = page(2, poison_stage=5)  # fails in aggregation: the bare exception, never drawn
    out = pipe.serve(pages, overlays=True)
    assert isinstance(out[5], ValueError) and isinstance(out[2], ValueError) and "poisoned" in str(out[2])
    good = [i for i in range(10) if i not in (2, 5)]
    assert [out[i][0][0] for i in good] == good and [int(out[i][1][0, 0, 0]) for i in good] == good
    assert pipe.last_job["retried_pages"] == 0  # a drawing that fails is not re-run
    # the render call itself failing: every page of that wave gets the exception, the other waves and the pipeline go on
    pages = [page(i) for i in range(8)]
    pages[6][0, 1, 0] = 99
    out = pipe.serve(pages, overlays=True)
    assert all(isinstance(out[i], tuple) for i in range(4)) and all(isinstance(out[i], RuntimeError) for i in range(4, 8))
    # a page failing in a network stage is retried alone and its wave mates still get their triples
    pages = [page(i) for i in range(4)]
    pages[1] = page(1, poison_stage=1)
    out = pipe.serve(pages, overlays=True)
    assert isinstance(out[1], RuntimeError) and [out[i][0][0] for i in (0, 2, 3)] == [0, 2, 3]
    assert [o[0] for o in pipe.serve([page(i) for i in range(3)])] == [0, 1, 2]
    pipe.close()
    assert not _render_threads()


def test_sharded_serving_refuses_overlays():
    import pytest

    from yomitoku_amd.distributed import ShardedServer

    server = ShardedServer.__new__(ShardedServer)  # no process group: the refusal comes before anything is served
    with pytest.raises(NotImplementedError, match="overlays"):
        server.serve_local([page(0)], overlays=True)
