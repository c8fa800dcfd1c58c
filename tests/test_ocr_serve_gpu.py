"""OCR.serve on the device: the text-only job through the page pipeline with the OCR chain alone (yomitoku_amd/serving.py,
`chains = ("ocr",)`).  Every page must get what `OCR.__call__` gives it alone, a failure stays with its page, the one overlay
is DocumentAnalyzer's OCR picture byte for byte, the JPEG files are `encode_jpeg`'s, and nothing allocates in a forward.  The
config (its OCR half), the seeds and the seven pages are those of tests/test_serving_gpu.py, whose own tests hold that these
weights find words on these pages."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_distributed_gpu import _free_port
from tests.test_pipeline_gpu import _assert_same_schema
from tests.test_serving_gpu import COUNTERS, LITE, _analyzer

pytestmark = pytest.mark.gpu

SHAPES = [(1000, 1400), (1400, 1000), (1000, 1400), (1200, 1600), (1000, 1400), (1400, 1000), (1000, 1400)]


def _ocr(**kw):
    from yomitoku_amd import OCR
    from yomitoku_amd.utils.synth import dbnet_state_dict, parseq_state_dict

    an = OCR(configs=LITE["ocr"], device="cuda:0", **kw)
    an.detector.model.load_state_dict(dbnet_state_dict(1234, out_bias=-2.0))
    an.recognizer.model.load_state_dict(parseq_state_dict(1235, eos_bias=6.0))
    return an


@pytest.fixture(scope="module")
def truth():
    from yomitoku_amd.utils.synth import synthetic_page_with_truth

    return [synthetic_page_with_truth(3 + i, h, w) for i, (h, w) in enumerate(SHAPES)]


@pytest.fixture(scope="module")
def imgs(truth):
    return [t[0] for t in truth]


@pytest.fixture(scope="module")
def ocr(dev):
    an = _ocr()
    yield an
    an.close()


@pytest.fixture(scope="module")
def singles(ocr, imgs):
    """What `__call__` gives every page alone, computed once."""
    out = [ocr(img)[0].model_dump() for img in imgs]
    assert sum(len(s["words"]) for s in out) > 0
    return out


def test_the_analyzer_is_a_stage_analyzer_with_the_reference_names(ocr):
    from yomitoku_amd.serving import StageAnalyzer

    assert isinstance(ocr, StageAnalyzer) and ocr.chains == ("ocr",)
    assert ocr.text_detector is ocr.detector and ocr.text_recognizer is ocr.recognizer and ocr._nets() == (ocr.detector, ocr.recognizer)
    with pytest.raises(AttributeError):
        ocr.text_detector = None  # read-only: the same two objects, not second instances


def test_serve_equals_per_page_calls_and_isolates_bad_sources(ocr, imgs, singles, tmp_path):
    from PIL import Image

    from yomitoku_amd.schemas import OCRSchema

    path = str(tmp_path / "page.png")
    Image.fromarray(imgs[1][:, :, ::-1]).save(path)  # load_image returns BGR
    sources = [imgs[0], path, imgs[2], np.zeros((50, 60), dtype=np.uint8), imgs[3], str(tmp_path / "nope.png"), imgs[4], imgs[5], imgs[6]]
    expect = [singles[0], singles[1], singles[2], None, singles[3], None, singles[4], singles[5], singles[6]]
    for kwargs in ({"wave": 4, "in_flight": 2}, {"wave": 3, "in_flight": 3}, {"wave": 3, "in_flight": 3, "rec_lanes": 1}):
        out = ocr.serve(sources, **kwargs)
        assert len(out) == len(sources)
        for want, got in zip(expect, out):
            if want is None:
                assert isinstance(got, Exception), got
            else:
                assert isinstance(got, OCRSchema)
                _assert_same_schema(want, got.model_dump())
        names = {t.name for t in ocr._pipeline._threads}
        assert not names & {"ymk-layout", "ymk-tables", "ymk-cells"} and ("ymk-recognize" in names) == (kwargs.get("rec_lanes") == 1)
    assert sum(len(s["words"]) for s in singles) > 0
    assert ocr.serve([]) == []
    assert ocr._pipeline._render_thread is None  # no job of this pipeline asked for overlays or files
    # two recogniser forwards in flight by default: a second PARSeq handle on the first one's state dict
    rep = ocr.recognizer._replicas.get(1)
    assert rep is not None and rep._source_sd is ocr.recognizer.model._sd and rep.weight_bytes == ocr.recognizer.model.weight_bytes


def test_a_stage_failure_inside_a_wave_costs_only_its_page(ocr, imgs, singles):
    rec = ocr.recognizer
    inner = rec.forward_plan
    culprit = imgs[2].shape

    def touchy(plan, model=None):
        for _, _, ds, _ in plan["preps"]:
            page0 = ds.page if isinstance(ds.page, torch.Tensor) else ds.page[0]  # a pyramid when some lines use a down-scaled level
            if tuple(page0.shape) == culprit and int(page0[0, 0, 0]) == 7:
                raise RuntimeError("recogniser choked on this page")
        return inner(plan, model)

    bad = imgs[2].copy()
    bad[0, 0, 0] = 7
    rec.forward_plan = touchy
    try:
        out = ocr.serve([imgs[0], imgs[1], bad, imgs[3], imgs[4]], wave=4, in_flight=2)
    finally:
        del rec.forward_plan
    assert isinstance(out[2], RuntimeError) and "choked" in str(out[2])
    for i in (0, 1, 3, 4):
        _assert_same_schema(singles[i], out[i].model_dump())
    assert ocr._pipeline.last_job["retried_pages"] == 4


def test_the_overlay_is_the_document_analyzers_ocr_picture(ocr, imgs, singles):
    from yomitoku_amd.schemas import OCRSchema

    pages = imgs[:2]  # two shapes
    before = [p.copy() for p in pages]
    got = ocr.serve(pages, wave=2, overlays=True)
    an = _analyzer()  # the same detector and recogniser state dicts (tests/test_serving_gpu.py)
    try:
        want = an.serve(pages, wave=2, overlays=True)
    finally:
        an.close()
    assert len(got) == 2
    for page, entry, full, single in zip(pages, got, want, singles):
        assert isinstance(entry, tuple) and len(entry) == 2 and isinstance(entry[0], OCRSchema)
        _assert_same_schema(single, entry[0].model_dump())
        vis = entry[1]
        assert isinstance(vis, np.ndarray) and vis.dtype == np.uint8 and vis.shape == page.shape and vis.flags.owndata
        assert not np.array_equal(vis, page)
        print(f"words {len(entry[0].words)}, drawn pixels {int((vis != page).any(-1).sum())}, differing from DocumentAnalyzer's {int((vis != full[1]).any(-1).sum())}")
        assert np.array_equal(vis, full[1])
    assert all(np.array_equal(a, b) for a, b in zip(pages, before))
    assert all(not isinstance(e, tuple) for e in ocr.serve(pages, wave=2))  # overlays belong to the job


def test_jpeg_files_are_encode_jpegs_and_make_the_searchable_pdf(ocr, imgs, singles):
    import re

    from yomitoku_amd.jpeg import EncodedJpeg, encode_jpeg
    from yomitoku_amd.utils.searchable_pdf import searchable_pdf_bytes

    pages = imgs[:2]
    out = ocr.serve(pages, wave=2, jpeg="high")
    opt = ocr.serve(pages, wave=2, jpeg="high", jpeg_optimize=True)
    both = ocr.serve(pages, wave=2, jpeg="high", overlays=True)
    for page, single, entry, entry_opt, entry_both in zip(pages, singles, out, opt, both):
        assert isinstance(entry, tuple) and len(entry) == 2 and isinstance(entry[1], EncodedJpeg)
        _assert_same_schema(single, entry[0].model_dump())
        plain_file = encode_jpeg(page, "high")
        assert entry[1].data == plain_file.data and not entry[1].optimized
        assert len(entry_opt) == 2 and entry_opt[1].data == encode_jpeg(page, "high", optimize=True).data and entry_opt[1].optimized
        assert len(entry_both) == 3 and isinstance(entry_both[1], np.ndarray) and not np.array_equal(entry_both[1], page)
        assert entry_both[2].data == plain_file.data  # from the clean page, not from the canvas
    pdf = searchable_pdf_bytes([e[1] for e in out], [e[0] for e in out])
    assert pdf.startswith(b"%PDF") and len(re.findall(rb"/Type /Page\b(?!s)", pdf)) == len(pages)
    assert [e[1].data in pdf for e in out] == [True] * len(pages)
    assert searchable_pdf_bytes([e[-1] for e in both], [e[0] for e in both]).startswith(b"%PDF")  # the one-liner, whatever the job drew


def test_a_handover_reaches_the_recogniser(ocr, truth, imgs):
    from yomitoku_amd.schemas import TextDetectorSchema
    from yomitoku_amd.testing import Handover

    class TrueBoxes(Handover):
        def boxes(self, wave, dets):
            return [TextDetectorSchema(points=q, scores=[1.0] * len(q)) for q in self._truth(wave)]

    quads = [t[1] for t in truth[:5]]
    assert all(len(q) > 0 for q in quads)
    ocr.handover = TrueBoxes(truth=quads)
    try:
        out = ocr.serve(imgs[:5], wave=3, in_flight=2)
    finally:
        ocr.handover = None
    for q, page in zip(quads, out):
        assert len(page.words) == len(q)
        assert np.array_equal(np.asarray([w.points for w in page.words]), np.asarray(q))


def test_nothing_allocates_builds_or_waits_and_the_buffers_stay_put(dev, imgs):
    from yomitoku_amd import _lib

    before = {k: _lib.stat(k) for k in COUNTERS}
    an = _ocr()
    try:
        an(imgs[0])
        an(imgs[3])  # another page size
        out = an.serve(imgs + imgs[::-1], wave=4, in_flight=2)
        assert len(out) == 14 and not any(isinstance(o, Exception) for o in out)
        after = {k: _lib.stat(k) for k in COUNTERS}
        assert after == before, {k: after[k] - before[k] for k in COUNTERS}
        nets = (an.detector.model, an.recognizer.model)
        ws = [n.workspace_bytes for n in nets]
        pinned = sum(t.numel() for t in an.detector.post_processor._pinned.values())
        for _ in range(3):
            out = an.serve(imgs[::-1] + imgs, wave=4, in_flight=2)
            assert not any(isinstance(o, Exception) for o in out)
        assert [n.workspace_bytes for n in nets] == ws
        assert sum(t.numel() for t in an.detector.post_processor._pinned.values()) == pinned
    finally:
        an.close()


def test_refusals_come_before_any_source_is_read(ocr):
    def sources():
        raise AssertionError("a source was read")
        yield

    with pytest.raises(ValueError, match="best"):
        ocr.serve(sources(), jpeg="best")
    with pytest.raises(ValueError, match="jpeg_optimize"):
        ocr.serve(sources(), jpeg_optimize=True)
    vis = _ocr(visualize=True)
    try:
        with pytest.raises(NotImplementedError, match="overlays=True"):
            vis.serve(sources())
        assert vis._pipeline is None
    finally:
        vis.close()


SHARDED = r"""
import json, sys
import torch
import torch.distributed as dist

from tests.test_serving_gpu import LITE
from yomitoku_amd import OCR
from yomitoku_amd import distributed as yd
from yomitoku_amd.utils.synth import dbnet_state_dict, parseq_state_dict, synthetic_page_with_truth

torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1)
built = []


def make(device, checkpoints, budget):
    an = OCR(configs=LITE["ocr"], device=str(device))
    an.detector.model.load_state_dict(checkpoints["det"])
    an.recognizer.model.load_state_dict(checkpoints["rec"])
    built.append(an)
    return an


sds = {"det": dbnet_state_dict(1234, out_bias=-2.0), "rec": parseq_state_dict(1235, eos_bias=6.0)}
sources = [synthetic_page_with_truth(3, 1000, 1400)[0], sys.argv[1], synthetic_page_with_truth(4, 1400, 1000)[0], synthetic_page_with_truth(5, 1000, 1400)[0]]
out = yd.serve_sharded(sources, make, sds, wave=2)
server = yd.ShardedServer(make, sds, pin_cores=False)
refused = []
for kwargs in ({"overlays": True}, {"jpeg": "high"}):
    try:
        server.serve_local(sources, **kwargs)
        refused.append(None)
    except NotImplementedError as exc:
        refused.append(str(exc))
direct = server.analyzer.serve(sources, wave=2)
want = [yd._entry_json(e) for e in direct]
words = sum(len(e.words) for e in direct if not isinstance(e, BaseException))
server.close()
dist.barrier()
torch.cuda.synchronize()
dist.destroy_process_group()
print("RESULT " + json.dumps({"out": out, "want": want, "refused": refused, "words": words, "analyzers": len(built),
                              "kinds": [type(a).__name__ for a in built]}))
"""


def test_an_ocr_rides_through_serve_sharded(dev, tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1",
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    proc = subprocess.run([sys.executable, "-c", SHARDED, str(tmp_path / "nope.png")], cwd=root, env=env, capture_output=True, text=True,
                          timeout=240)
    assert proc.returncode == 0, proc.stderr[-3000:]
    line = next(ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT "))
    r = json.loads(line[len("RESULT "):])
    assert r["kinds"] == ["OCR", "OCR"] and r["words"] > 0
    assert len(r["out"]) == 4 and all(isinstance(e, str) for e in r["out"])
    assert "error" in json.loads(r["out"][1]) and r["out"][1] == r["want"][1]  # the file that does not exist, in its place
    for got, want in zip(r["out"], r["want"]):
        _assert_same_schema(json.loads(want), json.loads(got))
    assert sorted(json.loads(r["out"][0])) == ["words"]  # an OCRSchema's JSON: words alone
    assert r["refused"][0] is not None and "overlays" in r["refused"][0] and r["refused"][1] is not None and "jpeg" in r["refused"][1]
