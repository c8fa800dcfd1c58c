"""TableSemanticParser against the reference's recorded results (tools/record_table_semantic_golden.py): the reference's 11
cell-detector outputs x four modes (default, grid_only, kv_only, merge_same_column_values) x two OCR inputs (none, and a
synthetic word list that exercises the word -> cell assignment, the direction vote and the reading order), through
`__call__` with `run_models` replaced.  `model_dump()`, `to_dict()`, `to_simple()` and `to_structured()` must be equal to what
the reference produced, key for key; so must the template round trip of the case with model-predicted regions."""
import copy
import glob
import gzip
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "table_semantic")
MODES = {"default": {}, "grid_only": {"grid_only": True}, "kv_only": {"kv_only": True}, "merge": {}}
CASES = sorted(os.path.basename(p)[:-8] for p in glob.glob(os.path.join(GOLDEN, "inputs", "case_*.json.gz")))


def _load(*parts):
    with gzip.open(os.path.join(GOLDEN, *parts) + ".gz", "rt", encoding="utf-8") as f:
        return json.load(f)


def _expected(case, ocr, mode):
    """The recorded views of one case.  The fixture stores repeated content once: a mode whose views equal the default mode's
    points at it, and the dump's `words` - the OCR input handed through - are those of the input file."""
    stored = _load("expected", f"{case}_{ocr}.json")
    want = copy.deepcopy(stored["default"] if stored[mode] == {"same_as": "default"} else stored[mode])
    want["dump"]["words"] = _load("inputs", f"{case}.json")["words"] if ocr == "words" else []
    return want


def _run(case_input, with_words, mode, template=None):
    from yomitoku_amd.schemas import OCRSchema, TableDetectorSchema
    from yomitoku_amd.table_semantic_parser import TableSemanticParser

    parser = TableSemanticParser.__new__(TableSemanticParser)  # no networks: the model stage is replaced below
    parser.merge_same_column_values = mode == "merge"
    tables = [TableDetectorSchema.model_validate(t) for t in copy.deepcopy(case_input["tables"])]
    ocr = OCRSchema(words=copy.deepcopy(case_input["words"]) if with_words else [])
    parser.run_models = lambda img: (ocr, tables, [])
    out, vis_layout, vis_ocr = parser(np.zeros((32, 32, 3), dtype=np.uint8), template=template, **MODES[mode])
    assert vis_layout is None and vis_ocr is None
    return out


def _views(out):
    return {"dump": out.model_dump(), "to_dict": out.to_dict(), "to_simple": out.to_simple().model_dump(),
            "to_structured": out.to_structured().model_dump()}


def test_all_recorded_cases_are_present():
    assert CASES == [f"case_{n:02d}" for n in range(11)]
    for case in CASES:
        for ocr in ("empty", "words"):
            assert sorted(_load("expected", f"{case}_{ocr}.json")) == sorted(MODES)
    # 0-9 come from a detector without region classes (the fallback path), 10 has model-predicted regions
    regions = [sum(len(t.get("kv_regions", [])) + len(t.get("grid_regions", [])) for t in _load("inputs", f"{c}.json")["tables"]) for c in CASES]
    assert regions[:10] == [0] * 10 and regions[10] > 0


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("ocr", ["empty", "words"])
@pytest.mark.parametrize("case", CASES)
def test_recorded_case(case, ocr, mode):
    want = _expected(case, ocr, mode)
    got = json.loads(json.dumps(_views(_run(_load("inputs", f"{case}.json"), ocr == "words", mode))))  # tuples as lists, like the fixture
    for view in ("dump", "to_dict", "to_simple", "to_structured"):
        assert got[view] == want[view], view


def test_template_round_trip(tmp_path):
    """save_template_json of the parsed case 10 is the recorded template, and __call__(template=...) gives the recorded result."""
    recorded = _load("template_case_10.json")
    case = _load("inputs", "case_10.json")
    path = str(tmp_path / "template.json")
    _run(case, True, "default").save_template_json(path)
    with open(path, encoding="utf-8") as f:
        assert json.load(f) == recorded["template"]
    got = json.loads(json.dumps(_views(_run(case, True, "default", template=path))))
    assert got == recorded["result"]
