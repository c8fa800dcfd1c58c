"""TableSemanticParser.serve on the MI355X with seeded weights: the parser as the analyzer of the page pipeline
(yomitoku_amd/serving.py) must give each page what `__call__` gives it alone, keep going past a page that fails, carry
`template` / `grid_only` / `kv_only` / `overlays` per job, hold its buffers steady and run under `ShardedServer`.  The set-up
(configs, seeds, fixed table boxes at the hand-over) is that of tests/test_table_semantic_gpu.py; the comparison is
tests/test_pipeline_gpu.py's `_assert_same_schema`: structure, strings and integers exactly, scores to 1e-4 (a forward that sees
another batch may pick another tile shape)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests.test_pipeline_gpu import _assert_same_schema
from tests.test_table_semantic_gpu import FIXED_TABLES, _FixedTables

pytestmark = pytest.mark.gpu

CONFIGS = {"table_detector": {"from_pretrained": False}, "table_cell_parser": {"from_pretrained": False},
           "text_detector": {"from_pretrained": False},
           "text_recognizer": {"model_name": "parseq-tiny-dynw-v4", "from_pretrained": False, "dynamic_width": True, "batch_bucketing": True}}
# five distinct boxes inside 596 x 596 (every page here is at least that large): two pages bring ten crops
FIVE_TABLES = ([30, 40, 330, 240], [350, 250, 550, 550], [20, 300, 300, 560], [340, 30, 580, 230], [100, 120, 500, 480])


class _FiveTables:
    def tables(self, k, tables):
        from yomitoku_amd.schemas import Element

        return [Element(id=None, box=list(b), score=1.0, role=None, contents=None) for b in FIVE_TABLES]


@pytest.fixture(scope="module")
def pages():
    """The golden page (596 wide x 842 high), its mirror, its transpose (842 x 596: a second DBNet input size, so a wave mixes
    size groups) and its upper 700 rows (a third size).  The seeded detector finds no text on the transpose (neither does
    the CPU oracle with the same weights: 89 boxes on the page and on its mirror, 0 on the transpose, 8 on the upper part), so
    the transposed page goes through every job with tables and cells but without words; the upper part is here so that a
    page of another size than the first two carries words as well."""
    from yomitoku_amd.data.functions import load_image

    (img,) = load_image(os.path.join(os.path.dirname(__file__), "golden", "test_page.jpg"))
    assert img.shape[:2] == (842, 596)
    assert all(b[2] <= 596 and b[3] <= 596 for b in FIXED_TABLES + FIVE_TABLES)
    return [img, np.ascontiguousarray(img[:, ::-1]), np.ascontiguousarray(img.transpose(1, 0, 2)), np.ascontiguousarray(img[:700])]


WITH_TEXT = (0, 1, 3)  # the pages the seeded detector finds text on


@pytest.fixture(scope="module")
def parser(dev):
    from yomitoku_amd import TableSemanticParser
    from yomitoku_amd.utils.synth import dbnet_state_dict, parseq_state_dict
    from yomitoku_amd.utils.synth_rtdetr import rtdetr_state_dict

    p = TableSemanticParser(configs=CONFIGS, device="cuda:0")
    p.text_detector.model.load_state_dict(dbnet_state_dict(8, out_bias=-1.5))
    p.text_recognizer.model.load_state_dict(parseq_state_dict(1235, eos_bias=6.0))
    p.layout_parser.model.load_state_dict(rtdetr_state_dict(1240, num_classes=6, score_bias=-2.0))
    p.cell_detector.model.load_state_dict(rtdetr_state_dict(1243, num_classes=6, eval_size=(960, 960), enc_score_gain=12.0, score_bias=-3.0,
                                                            score_gain=2.0))
    p.handover = _FixedTables()  # seeded weights detect noise: the fixed boxes go in on both sides of every comparison
    yield p
    p.close()


@pytest.fixture(scope="module")
def singles(parser, pages):
    """`__call__` on every page, once for the whole module; never changed."""
    out = []
    for k, img in enumerate(pages):
        got = parser(img)[0]
        print("page", k, img.shape[:2], "words", len(got.words), "tables", len(got.tables), "cells", sum(len(t.cells) for t in got.tables))
        assert len(got.tables) > 0 and sum(len(t.cells) for t in got.tables) > 0  # nothing compared is empty
        assert len(got.words) > 0 or k not in WITH_TEXT
        out.append(got.model_dump())
    return out


def test_serve_equals_per_page_calls_and_isolates_failures(parser, pages, singles, tmp_path):
    from PIL import Image

    path = str(tmp_path / "mirror.png")
    Image.fromarray(pages[1][:, :, ::-1]).save(path)  # load_image returns BGR
    missing = str(tmp_path / "nope.png")
    sources = [pages[0], path, np.zeros((50, 60), dtype=np.uint8), pages[2], missing, pages[3]]
    expect = [singles[0], singles[1], None, singles[2], None, singles[3]]
    for wave, in_flight in ((2, 2), (3, 1), (8, 1)):
        out = parser.serve(sources, wave=wave, in_flight=in_flight)
        assert len(out) == len(sources)
        for want, got in zip(expect, out):
            if want is None:
                assert isinstance(got, Exception), got
            else:
                _assert_same_schema(want, got.model_dump())
    assert parser.serve([]) == []
    triples = parser.serve(sources, wave=8, in_flight=1, with_source=True)
    assert [(si, fi) for si, fi, _ in triples] == [(i, 0) for i in range(len(sources))]
    for want, (_, _, got) in zip(expect, triples):
        assert isinstance(got, Exception) if want is None else got.model_dump().keys() == want.keys()


class _ModelSpy:
    """The cell detector's network with the batch size of every forward written down."""

    def __init__(self, model):
        self._model, self.batches = model, []

    def __call__(self, x):
        self.batches.append(int(x.shape[0]))
        return self._model(x)

    def __getattr__(self, name):
        return getattr(self._model, name)


def test_more_crops_than_one_forward(parser, pages, singles):
    """Ten crops against MAX_TABLES_PER_FORWARD == 8: forwards of 5 + 5, every table on its own page."""
    cd = parser.cell_detector
    assert cd.MAX_TABLES_PER_FORWARD == 8
    two = [pages[0], pages[2]]
    model, handover = cd.model, parser.handover
    parser.handover = _FiveTables()
    try:
        want = [parser(img)[0] for img in two]
        spy = cd.model = _ModelSpy(model)
        out = parser.serve(two, wave=2, in_flight=1)
    finally:
        cd.model, parser.handover = model, handover
    assert spy.batches == [5, 5]
    for one, got in zip(want, out):
        assert len(one.tables) > 2  # more tables than the other tests see
        _assert_same_schema(one.model_dump(), got.model_dump())
    # the pages differ in shape and content: a table attributed to the wrong page cannot pass the comparison above; the boxes
    # of every page's tables are the handed ones
    for got in out:
        assert {tuple(t.box) for t in got.tables} <= {tuple(b) for b in FIVE_TABLES}


def test_a_stage_failure_costs_one_page(parser, pages, singles):
    cd = parser.cell_detector
    inner = cd.forward_tables
    assert all(int(p[0, 0, 0]) != 7 for p in pages)

    def touchy(imgs, tables_per_page):
        if any(int(img[0, 0, 0]) == 7 for img in imgs):
            raise RuntimeError("cell detector choked on this page")
        return inner(imgs, tables_per_page)

    bad = pages[1].copy()
    bad[0, 0, 0] = 7
    cd.forward_tables = touchy
    try:
        out = parser.serve([pages[0], pages[3], bad, pages[2]], wave=4, in_flight=2)
    finally:
        del cd.forward_tables
    assert isinstance(out[2], RuntimeError) and "choked" in str(out[2])
    for i, k in ((0, 0), (1, 3), (3, 2)):
        _assert_same_schema(singles[k], out[i].model_dump())
    assert parser._pipeline.last_job["retried_pages"] == 4


def test_job_options(parser, pages, singles, tmp_path):
    two = pages[:2]
    want_grid = [parser(img, grid_only=True)[0].model_dump() for img in two]
    got_grid = parser.serve(two, grid_only=True)
    for want, got in zip(want_grid, got_grid):
        _assert_same_schema(want, got.model_dump())
    for want, got in zip(singles, parser.serve(two)):  # the option did not stay behind
        _assert_same_schema(want, got.model_dump())
    # a template written from page 0's own result, every cell's contents replaced: the job must carry it to `finish`
    template = str(tmp_path / "template.json")
    parser(pages[0])[0].save_template_json(template)
    with open(template, encoding="utf-8") as f:
        doc = json.load(f)
    for table in doc["tables"]:
        for cell in table["cells"].values():
            cell["contents"] = "from the template"
    with open(template, "w", encoding="utf-8") as f:
        json.dump(doc, f)
    want_tmpl = [parser(img, template=template)[0].model_dump() for img in two]
    got_tmpl = parser.serve(two, template=template)
    for want, got in zip(want_tmpl, got_tmpl):
        _assert_same_schema(want, got.model_dump())
    assert any(c.contents == "from the template" for t in got_tmpl[0].tables for c in t.cells.values())
    want_kv = [parser(img, kv_only=True)[0].model_dump() for img in two]
    for want, got in zip(want_kv, parser.serve(two, kv_only=True)):
        _assert_same_schema(want, got.model_dump())


def test_overlays(parser, pages, singles):
    out = parser.serve(pages, overlays=True)
    assert len(out) == len(pages) and all(isinstance(o, tuple) and len(o) == 3 for o in out)
    plain = parser.serve(pages)
    ref = parser.parse_pages(pages, overlays=True)
    for k, (img, one, bare, (schema, vis_layout, vis_ocr), (_, ref_layout, ref_ocr)) in enumerate(zip(pages, singles, plain, out, ref)):
        _assert_same_schema(bare.model_dump(), schema.model_dump(), score_rtol=0.0)  # the same job, with and without pictures
        _assert_same_schema(one, schema.model_dump())
        for vis in (vis_layout, vis_ocr):
            assert isinstance(vis, np.ndarray) and vis.dtype == np.uint8 and vis.shape == img.shape and vis.flags.owndata
        assert not np.array_equal(vis_layout, img) and (k not in WITH_TEXT or not np.array_equal(vis_ocr, img))  # something was drawn
        # a canvas's pixels do not depend on which wave drew it
        assert np.array_equal(vis_layout, ref_layout) and np.array_equal(vis_ocr, ref_ocr)
        assert not np.array_equal(vis_layout, vis_ocr)
    from yomitoku_amd.schemas import TableSemanticParserSchema

    assert all(isinstance(o, TableSemanticParserSchema) for o in plain)  # a job without overlays: bare schemas again


def test_buffers_stay_put_across_jobs(parser, pages):
    """tests/test_serving_gpu.py::test_buffers_stay_put_across_jobs for the parser: ragged waves (two page sizes, waves of two
    and one) must not grow pinned host memory or reallocate a model's workspace once the largest shapes have been seen."""
    job = [pages[0], pages[2], pages[3], pages[2], pages[0]]
    parser.serve(job, wave=2, in_flight=2)
    nets = (parser.text_detector.model, parser.text_recognizer.model, parser.layout_parser.model, parser.cell_detector.model)
    ws = [n.workspace_bytes for n in nets]
    assert all(w > 0 for w in ws)
    pinned = sum(t.numel() for t in parser.text_detector.post_processor._pinned.values())
    for _ in range(3):
        out = parser.serve(job[::-1], wave=2, in_flight=2)
        assert not any(isinstance(o, Exception) for o in out)
    assert [n.workspace_bytes for n in nets] == ws
    assert sum(t.numel() for t in parser.text_detector.post_processor._pinned.values()) == pinned


SHARDED = r"""
import json, os, sys
import numpy as np
import torch
import torch.distributed as dist

from tests.test_table_semantic_gpu import _FixedTables
from tests.test_table_semantic_serve_gpu import CONFIGS
from yomitoku_amd import TableSemanticParser
from yomitoku_amd import distributed as yd
from yomitoku_amd.data.functions import load_image
from yomitoku_amd.utils.synth import dbnet_state_dict, parseq_state_dict
from yomitoku_amd.utils.synth_rtdetr import rtdetr_state_dict

torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1)


def checkpoints():
    return {"det": dbnet_state_dict(8, out_bias=-1.5), "rec": parseq_state_dict(1235, eos_bias=6.0),
            "lay": rtdetr_state_dict(1240, num_classes=6, score_bias=-2.0),
            "cell": rtdetr_state_dict(1243, num_classes=6, eval_size=(960, 960), enc_score_gain=12.0, score_bias=-3.0, score_gain=2.0)}


def make_analyzer(device, sds, budget):
    p = TableSemanticParser(configs=CONFIGS, device=str(device))
    for module, key in ((p.text_detector, "det"), (p.text_recognizer, "rec"), (p.layout_parser, "lay"), (p.cell_detector, "cell")):
        module.model.load_state_dict(sds[key])
    p.handover = _FixedTables()
    return p


(img,) = load_image(os.path.join("tests", "golden", "test_page.jpg"))
two = [img, np.ascontiguousarray(img[:, ::-1])]
server = yd.ShardedServer(make_analyzer, checkpoints, pin_cores=False)
texts = server.run(two, wave=2, in_flight=1, gather="json")
objects = server.run(two, wave=2, in_flight=1, gather="objects")
refused = None
try:
    server.serve_local(two, overlays=True)
except NotImplementedError as exc:
    refused = str(exc)
singles = [server.analyzer(page)[0].model_dump_json() for page in two]
report = server.replicas
dist.barrier()
server.close()
print("RESULT " + json.dumps({"texts": texts, "objects": [o.model_dump_json() for o in objects], "singles": singles, "refused": refused,
                              "replicas": report, "analyzer": type(server.analyzer).__name__}))
"""


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_sharded_one_rank(dev):
    """In the manner of tests/test_distributed_gpu.py: a one-rank "nccl" group in a subprocess; `make_analyzer` returns a
    TableSemanticParser built from the broadcast checkpoints; the gathered JSON text parses to the single-call dumps."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1",
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    proc = subprocess.run([sys.executable, "-c", SHARDED], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-3000:]
    line = next(ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT "))
    r = json.loads(line[len("RESULT "):])
    assert r["analyzer"] == "TableSemanticParser" and r["replicas"]["ranks"] == 1 and r["replicas"]["weights_crc_equal"] is True
    assert len(r["texts"]) == 2 and len(r["objects"]) == 2
    for text, obj, single in zip(r["texts"], r["objects"], r["singles"]):
        want = json.loads(single)
        assert len(want["words"]) > 0 and len(want["tables"]) > 0
        _assert_same_schema(want, json.loads(text))
        _assert_same_schema(want, json.loads(obj))
    assert r["refused"] and "overlays" in r["refused"]
