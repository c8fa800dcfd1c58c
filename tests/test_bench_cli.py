"""bench.py without a GPU: the module imports, its workloads / presets line up with the module catalogs and
constructor signatures, and running it on a box with no HIP device fails loudly (no CPU fallback)."""
import inspect
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_presets_match_catalogs_and_signatures():
    sys.path.insert(0, ROOT)
    import bench
    from yomitoku_amd.layout_parser import LayoutParser
    from yomitoku_amd.table_structure_recognizer import TableStructureRecognizer
    from yomitoku_amd.text_detector import TextDetector
    from yomitoku_amd.text_recognizer import TextRecognizer

    for name in bench.REC_PRESETS:
        assert name in TextRecognizer.model_catalog.list_model()
    lite = bench.LITE_CONFIGS
    for cls, kwargs in ((TextDetector, lite["ocr"]["text_detector"]), (TextRecognizer, lite["ocr"]["text_recognizer"]),
                        (LayoutParser, lite["layout_analyzer"]["layout_parser"]),
                        (TableStructureRecognizer, lite["layout_analyzer"]["table_structure_recognizer"])):
        params = inspect.signature(cls.__init__).parameters
        assert set(kwargs) <= set(params), (cls.__name__, set(kwargs) - set(params))
    # the --lite recogniser switches of the reference CLI (cli/main.py:505-520)
    rec = lite["ocr"]["text_recognizer"]
    assert rec["model_name"] == "parseq-tiny-dynw-v4" and rec["dynamic_width"] and rec["batch_bucketing"] and rec["source_downscale"]
    assert set(bench.CKPT) == {"det", "rec", "lay", "tab"}
    for name, cfgs in bench.MODEL_SETS.items():
        assert name in bench.REC_CKPT_OF_SET
        assert set(cfgs["ocr"]["text_recognizer"]) <= set(inspect.signature(TextRecognizer.__init__).parameters)


def test_bench_refuses_to_run_without_a_hip_device():
    import torch

    if torch.cuda.is_available():
        return  # the GPU tiers run the real thing
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0", "--no-cpu-baseline"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0
    assert "HIP device" in (out.stderr + out.stdout)


def test_dumped_outputs_line_up_field_by_field(tmp_path):
    """bench.py --dump-outputs: a page result flattened to one array per field path (list lengths, strings as code points
    closed by -1, None as -2), written as float64 - and a large float array as a fixed seeded sample in float32."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    from yomitoku_amd.schemas import DocumentAnalyzerSchema

    word = {"points": [[1, 2], [9, 2], [9, 6], [1, 6]], "content": "ab", "direction": "horizontal", "rec_score": 0.5, "det_score": 0.25}
    page = DocumentAnalyzerSchema(paragraphs=[{"box": [1, 2, 9, 6], "contents": "ab", "direction": "horizontal", "order": None, "role": None}],
                                  tables=[], words=[word, dict(word, content="c")], figures=[])
    res = {}
    bench.flatten_result(page, "page", res)
    bench.flatten_result(page.model_copy(update={"words": []}), "page", res)
    assert res["page.words.len"] == [2, 0] and res["page.tables.len"] == [0, 0] and res["page.paragraphs.len"] == [1, 1]
    assert res["page.words.content"] == [97, 98, -1, 99, -1]
    assert res["page.words.points.len"] == [4, 4] and res["page.words.points"][:4] == [1.0, 2.0, 9.0, 2.0]
    assert res["page.words.rec_score"] == [0.5, 0.5] and res["page.paragraphs.order"] == [-2.0, -2.0]
    big = torch.arange(bench.DUMP_SAMPLE + 5, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path / "a"), dict(res, binary=big))
    words = np.load(tmp_path / "a" / "page.words.content.npy")
    assert words.dtype == np.float64 and words.tolist() == res["page.words.content"]
    assert all(np.isfinite(np.load(tmp_path / "a" / f"{k}.npy")).all() for k in res)  # None fields included
    sample = np.load(tmp_path / "a" / "binary.npy")
    assert sample.dtype == np.float32 and sample.size == bench.DUMP_SAMPLE and (np.diff(sample) > 0).all()
    bench.dump_outputs(str(tmp_path / "b"), {"binary": big})
    assert np.array_equal(np.load(tmp_path / "b" / "binary.npy"), sample)
