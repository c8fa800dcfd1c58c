"""The page pipeline with ONE chain (yomitoku_amd/serving.py: `chains = ("ocr",)`, what OCR.serve declares), with stub stages
on the host in the manner of tests/test_serving.py: page order and waves, per-page failure isolation, the entry shapes of
overlays / jpeg jobs when a page has one picture, and the chain declarations the pipeline refuses.  The stub has no layout,
tables or cells stage at all: a pipeline that looks one up cannot be built for it."""
import threading
import time
from types import SimpleNamespace

import numpy as np
import pytest

from yomitoku_amd.serving import PagePipeline, check_jpeg_preset


class OcrStub:
    """The six stages of the OCR chain and `finish`, moving page ids along; a page whose first pixel is 255 poisons the stage
    named in its second."""

    chains = ("ocr",)
    STAGES = {1: "detect", 2: "boxes", 3: "crops", 4: "recognize", 5: "decode", 6: "finish"}

    def __init__(self, delay=0.0):
        self.text_detector = SimpleNamespace(device="cpu")
        self.delay = delay
        self.lanes_seen = set()
        self.threads_seen = set()

    def _poison(self, wave, stage):
        self.threads_seen.add(threading.current_thread().name)
        for img in wave.imgs:
            if img[0, 0, 0] == 255 and self.STAGES[int(img[0, 0, 1])] == stage:
                raise RuntimeError(f"poisoned page in {stage}")

    def _stage_detect(self, wave):
        time.sleep(self.delay)
        self._poison(wave, "detect")
        wave.maps = [int(img[0, 0, 2]) for img in wave.imgs]

    def _stage_boxes(self, wave):
        self._poison(wave, "boxes")
        wave.dets = [m + 1000 for m in wave.maps]

    def _stage_crops(self, wave):
        self._poison(wave, "crops")
        wave.rec_plan = list(wave.dets)

    def _stage_recognize(self, wave, lane=0):
        self.lanes_seen.add(lane)
        time.sleep(self.delay)
        self._poison(wave, "recognize")
        wave.rec_plan = [d * 2 for d in wave.rec_plan]

    def _stage_decode(self, wave):
        self._poison(wave, "decode")
        wave.recs = wave.rec_plan

    def _stage_finish(self, wave, k):
        if wave.imgs[k][0, 0, 0] == 255 and self.STAGES[int(wave.imgs[k][0, 0, 1])] == "finish":
            raise ValueError("poisoned page in finish")
        return (wave.ids[k], wave.recs[k], len(wave))


def page(tag, poison_stage=0):
    img = np.zeros((4, 4, 3), dtype=np.uint8)
    img[0, 0] = (255 if poison_stage else 0, poison_stage, tag)
    return img


def test_results_in_page_order_and_no_layout_chain_threads():
    an = OcrStub(delay=0.002)
    pipe = PagePipeline(an, wave=4, in_flight=3)
    names = [t.name for t in pipe._threads]
    assert not {"ymk-layout", "ymk-tables", "ymk-cells"} & set(names)
    assert names == ["ymk-detect", "ymk-boxes", "ymk-crops", "ymk-recognize-0", "ymk-recognize-1", "ymk-decode", "ymk-finish"]
    assert sorted(pipe._q) == sorted(["detect", "boxes", "crops", "recognize", "decode", "finish"])
    out = pipe.serve([page(i) for i in range(18)])
    assert [o[0] for o in out] == list(range(18))
    assert [o[1] for o in out] == [(i + 1000) * 2 for i in range(18)]
    assert [o[2] for o in out] == [4] * 16 + [2] * 2  # 4 full waves and a last wave of 2
    assert pipe.last_job == {"pages": 18, "waves": 5, "retried_pages": 0}
    assert an.lanes_seen == {0, 1}
    assert an.threads_seen <= set(names)  # every stage ran on a thread of this pipeline
    assert pipe.serve([]) == []
    pipe.close()
    assert not any(t.is_alive() for t in pipe._threads)


@pytest.mark.parametrize("stage", [1, 2, 3, 4, 5, 6], ids=["detect", "boxes", "crops", "recognize", "decode", "finish"])
def test_a_poisoned_page_fails_alone(stage):
    an = OcrStub()
    pipe = PagePipeline(an, wave=4, in_flight=2)
    pages = [page(i) for i in range(10)]
    pages[5] = page(5, poison_stage=stage)
    out = pipe.serve(pages)
    assert isinstance(out[5], (RuntimeError, ValueError)) and "poisoned" in str(out[5])
    good = [i for i in range(10) if i != 5]
    assert [out[i][0] for i in good] == good and [out[i][1] for i in good] == [(i + 1000) * 2 for i in good]
    if OcrStub.STAGES[stage] != "finish":  # the wave {4..7} was re-run page by page
        assert pipe.last_job["retried_pages"] == 4 and pipe.last_job["waves"] == 3 + 4
        assert [out[i][2] for i in (4, 6, 7)] == [1, 1, 1]
    else:  # aggregation fails per page: no re-run
        assert pipe.last_job["retried_pages"] == 0 and pipe.last_job["waves"] == 3
        assert [out[i][2] for i in (4, 6, 7)] == [4, 4, 4]
    assert [o[0] for o in pipe.serve([page(i) for i in range(3)])] == [0, 1, 2]  # the pipeline is still usable
    pipe.close()


class RenderStub(OcrStub):
    """One picture and one file per page, as 1-tuples; a page whose pixel [0, 1, 0] is 77 cannot be drawn."""

    def _stage_render(self, wave, results):
        assert threading.current_thread().name == "ymk-render" and wave.pages is not None and wave.recs is not None
        out = []
        for k, img in enumerate(wave.imgs):
            if isinstance(results[k], BaseException):
                out.append(None)
            elif img[0, 1, 0] == 77:
                out.append(ValueError("cannot draw this page"))
            else:
                out.append((np.full((2, 2, 3), wave.ids[k], np.uint8),))
        return out

    def _stage_jpeg(self, wave, results):
        return [None if isinstance(results[k], BaseException) else (f"file:{wave.ids[k]}",) for k in range(len(wave))]


def test_entry_shapes_of_overlays_and_jpeg_jobs_and_every_slot_comes_back():
    in_flight = 2
    pipe = PagePipeline(RenderStub(), wave=3, in_flight=in_flight)
    pages = [page(i) for i in range(8)]
    pages[4][0, 1, 0] = 77
    pages[6] = page(6, poison_stage=6)  # fails in finish: the bare exception, never drawn or encoded
    good = [i for i in range(8) if i not in (4, 6)]

    out = pipe.serve(pages, overlays=True)
    assert isinstance(out[4], ValueError) and "cannot draw" in str(out[4]) and isinstance(out[6], ValueError) and "poisoned" in str(out[6])
    for i in good:
        schema, picture = out[i]
        assert schema[0] == i and isinstance(picture, np.ndarray) and int(picture[0, 0, 0]) == i

    out = pipe.serve(pages, files=check_jpeg_preset("high"))
    assert isinstance(out[6], ValueError)
    for i in good + [4]:  # nothing is drawn in a jpeg job: page 4 is fine
        schema, made = out[i]
        assert schema[0] == i and made == f"file:{i}"

    out = pipe.serve(pages, overlays=True, files=check_jpeg_preset("high"))
    assert isinstance(out[4], ValueError) and isinstance(out[6], ValueError)
    for i in good:
        schema, picture, made = out[i]
        assert schema[0] == i and int(picture[0, 0, 0]) == i and made == f"file:{i}"

    assert pipe._rings.qsize() == in_flight  # every wave slot was given back, by the render stage too
    done = []
    t = threading.Thread(target=lambda: done.extend(pipe.serve([page(i) for i in range(3 * (in_flight + 1))], overlays=True)), daemon=True)
    t.start()
    t.join(20)
    assert not t.is_alive(), "a job of in_flight + 1 waves is still waiting for a wave slot"
    assert [e[0][0] for e in done] == list(range(3 * (in_flight + 1)))
    assert pipe._rings.qsize() == in_flight
    pipe.close()


def test_bad_chain_declarations_are_refused_at_construction():
    before = sorted(t.name for t in threading.enumerate() if t.name.startswith("ymk-"))
    split = OcrStub()
    split.split_text_across_cells = True
    with pytest.raises(ValueError, match="split_text_across_cells"):
        PagePipeline(split, wave=2, in_flight=1)
    for chains in ((), ("ocr", "tables")):
        an = OcrStub()
        an.chains = chains
        with pytest.raises(ValueError, match="chains"):
            PagePipeline(an, wave=2, in_flight=1)
    assert sorted(t.name for t in threading.enumerate() if t.name.startswith("ymk-")) == before  # a refused pipeline started nothing
