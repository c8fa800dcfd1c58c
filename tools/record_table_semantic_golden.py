#!/usr/bin/env python3
"""ORACLE tooling, for the development container only: it needs the reference checkout that oracle/_refstubs.py points at
(with networkx and pydantic installed) and is the only file of the table-semantic work that touches it.  No test, smoke() or
bench reads that tree; they read what this tool wrote.

    python tools/record_table_semantic_golden.py            # fixtures + the reference's host cost

Writes DATA only, under tests/golden/table_semantic/:

  inputs/case_NN.json.gz    the reference's 11 recorded cell-detector outputs (tests/data/table_semantic_inputs, compact JSON)
                            plus the synthetic word list this tool derives from the cells (see `synthetic_words`)
  expected/case_NN_<ocr>.json.gz  for ocr in (empty, words) and the four modes default / grid_only / kv_only / merge: the reference's
                            TableSemanticParser.__call__ with run_models replaced -> model_dump(), to_dict(), to_simple(), to_structured()
                            (see `expected_of` for how repeated content is stored once)
  template_case_10.json.gz  save_template_json of case 10 and the dump of __call__(template=that file)
  table_semantic_unit_cases.json.gz  the calls that the reference's own tests (test_kv_parser.py, test_table_semantic_parser.py,
                            test_table_semantic_parser_utils.py) make into the reference's functions and schema methods:
                            arguments before the call and results
and profiles/table_semantic_host_ms.json["reference"]: the semantic stage of the largest case, median of 20 after 3 warm-ups.

The reference iterates Python sets of cell ids in a few places, so its output can depend on the interpreter's string hash seed;
run the tool under several PYTHONHASHSEED values (--out DIR) and compare the directories before committing fixtures.
"""
import argparse
import copy
import glob
import json
import os
import statistics
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True  # the reference tree is read-only

from oracle._refstubs import REF_SRC, install_stubs, ref_import  # noqa: E402

MODES = {"default": {}, "grid_only": {"grid_only": True}, "kv_only": {"kv_only": True}, "merge": {"merge": True}}


def load_reference():
    """The reference's parser module with the four model classes and the visualiser replaced by empty stand-ins: only the
    host logic runs."""
    install_stubs()
    for name, attrs in (
        ("yomitoku.text_detector", {"TextDetector": object}),
        ("yomitoku.text_recognizer", {"TextRecognizer": object}),
        ("yomitoku.layout_parser", {"LayoutParser": object}),
        ("yomitoku.layout_analyzer", {"LayoutAnalyzer": object}),
        ("yomitoku.table_cell_detector", {"CellDetector": object}),
        ("yomitoku.utils.visualizer", {"cell_detector_visualizer": None, "det_visualizer": None, "reading_order_visualizer": None}),
        ("yomitoku.export", {"export_csv": None, "export_html": None, "export_markdown": None, "export_json": None}),
    ):
        if name not in sys.modules:
            m = types.ModuleType(name)
            for k, v in attrs.items():
                setattr(m, k, v)
            sys.modules[name] = m
    if not hasattr(sys.modules["omegaconf"], "OmegaConf"):
        sys.modules["omegaconf"].OmegaConf = object
    if "yomitoku.schemas" in sys.modules and not hasattr(sys.modules["yomitoku.schemas"], "__file__"):
        del sys.modules["yomitoku.schemas"]
    return ref_import("yomitoku.table_semantic_parser")


def synthetic_words(tables):
    """A deterministic word list from the cells of `tables` (plain dicts): one word inside every non-group cell whose text is
    the cell's incoming id; every seventh cell gets a second and a third word below the first; every fifth word is vertical;
    per table one word straddles two horizontal neighbours 60 / 40; one word lies outside all cells."""
    words = []

    def add(x1, y1, x2, y2, text):
        x1, y1 = max(0, int(x1)), max(0, int(y1))
        x2, y2 = max(x1 + 1, int(x2)), max(y1 + 1, int(y2))
        direction = "vertical" if len(words) % 5 == 4 else "horizontal"
        words.append({"points": [[x1, y1], [x2, y1], [x2, y2], [x1, y2]], "content": text, "direction": direction,
                      "rec_score": 0.9, "det_score": 0.8})

    far = 0
    for table in tables:
        cells = [c for c in table["cells"] if c["role"] != "group"]
        for k, cell in enumerate(cells):
            x1, y1, x2, y2 = cell["box"]
            far = max(far, x2, y2)
            w, h = x2 - x1, y2 - y1
            if k % 7 == 0:
                for line in range(3):
                    add(x1 + w // 8, y1 + h * line // 3 + 1, x2 - w // 8, y1 + h * (line + 1) // 3 - 1, f"{cell['id']}" + ("" if line == 0 else f".{line}"))
            else:
                add(x1 + w // 8, y1 + h // 6, x2 - w // 8, y2 - h // 6, cell["id"])
        pair = next(((a, b) for a in cells for b in cells
                     if a is not b and 0 <= b["box"][0] - a["box"][2] <= 6 and min(a["box"][3], b["box"][3]) - max(a["box"][1], b["box"][1]) >= 8), None)
        if pair is not None:
            a, b = pair
            top, bottom = max(a["box"][1], b["box"][1]), min(a["box"][3], b["box"][3])
            span = 10 * max(1, min(a["box"][2] - a["box"][0], b["box"][2] - b["box"][0], 60) // 10)
            edge = a["box"][2]
            add(edge - span * 6 // 10, top + 1, b["box"][0] + span * 4 // 10, bottom - 1, "straddle")
    add(far + 40, far + 40, far + 120, far + 70, "outside")
    return words


def run_reference(tsp, tables_json, words, mode, template=None):
    sch = sys.modules["yomitoku.schemas.table_semantic_parser"]
    ocr_mod = sys.modules["yomitoku.schemas"]
    parser = tsp.TableSemanticParser.__new__(tsp.TableSemanticParser)
    parser.visualize = False
    parser.merge_same_column_values = bool(MODES[mode].get("merge"))
    tables = [sch.TableDetectorSchema.model_validate(copy.deepcopy(t)) for t in tables_json]
    ocr = ocr_mod.OCRSchema(words=copy.deepcopy(words))

    async def fake_run_models(_img):
        return ocr, tables, []

    parser.run_models = fake_run_models
    import numpy as np

    kwargs = {k: v for k, v in MODES[mode].items() if k != "merge"}
    out, _, _ = parser(np.zeros((32, 32, 3), dtype=np.uint8), template=template, **kwargs)
    return out


def views(out):
    return {"dump": out.model_dump(), "to_dict": out.to_dict(), "to_simple": out.to_simple().model_dump(),
            "to_structured": out.to_structured().model_dump()}


def write(path, obj):
    """Compact JSON, gzipped (no file name or time stamp in the header: the same data gives the same bytes)."""
    import gzip

    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path + ".gz", "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(json.dumps(obj, ensure_ascii=False, separators=(",", ":")).encode("utf-8"))


def expected_of(tsp, tables, words):
    """{mode: views} as stored: the dump's `words` - the OCR input handed through, which is asserted here - are left to the
    input file, and a mode whose four views equal those of "default" is stored as {"same_as": "default"}."""
    out = {}
    for mode in MODES:
        v = json.loads(json.dumps(views(run_reference(tsp, tables, words, mode))))
        assert v["dump"].pop("words") == words
        out[mode] = {"same_as": "default"} if mode != "default" and v == out["default"] else v
    return out


# ------------------------------------------------------------------------------------------------ unit-level calls
def _plain(v):
    import networkx as nx

    if hasattr(v, "model_dump"):
        return {"__model__": type(v).__name__, "fields": _plain(v.model_dump())}
    if isinstance(v, types.SimpleNamespace):
        return {"__ns__": _plain(vars(v))}
    if isinstance(v, (nx.Graph, nx.DiGraph)):
        return {"__graph__": v.number_of_nodes()}
    if isinstance(v, tuple):
        return {"__tuple__": [_plain(x) for x in v]}
    if isinstance(v, (set, frozenset)):
        return {"__set__": sorted(_plain(x) for x in v)}
    if isinstance(v, dict):
        if not all(isinstance(k, str) for k in v):
            return {"__items__": [[_plain(k), _plain(x)] for k, x in v.items()]}
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, list) or type(v).__name__ == "dict_values":
        return [_plain(x) for x in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    raise TypeError(f"not recordable: {type(v)}")


UNIT_FUNCTIONS = {
    "table_semantic_parser": ["_split_nodes_with_role", "get_cell_by_id", "sort_cells", "_sort_elements", "_assign_ids", "_region_cell_ids",
                              "_resolve_overlapping_regions", "_gap_valley_tol", "_cluster_centers"],
    "kv_parser": ["parse_kv_items"],
    "table_semantic_schemas": ["make_unique_all", "normalize"],
}
UNIT_METHODS = {
    "TableSemanticContentsSchema": ["safe_contents", "find_cell_by_id", "search_cells_by_query"],
    "TableSemanticContentsView": ["kv_items_to_dict", "kv_items_to_nested", "kv_items_to_structured", "grids_to_dict", "grids_to_structured"],
    "TableSemanticParserSchema": ["to_dict", "to_structured", "to_simple"],
}
UNIT_TEST_FILES = ["test_kv_parser.py", "test_table_semantic_parser.py", "test_table_semantic_parser_utils.py"]


def record_unit_cases(tsp, out_dir):
    """Run the reference's own test files with pytest, in this process, against the reference's functions wrapped by a
    recorder.  Only calls made by the tests themselves are kept (not the calls those make in turn); a call whose arguments
    cannot be written as data (a test double, a graph) is skipped and counted.  The three visualiser tests of those files need
    OpenCV and fail here (pytest exit code 1); they call nothing that is recorded."""
    import pytest

    records, skipped, depth = [], {}, [0]

    def recorder(module, name, fn, method_of=None):
        def wrapped(*args, **kwargs):
            if depth[0]:
                return fn(*args, **kwargs)
            try:
                subject = {"TableSemanticContentsView": lambda: args[0].table, "TableSemanticParser": lambda: None}.get(method_of, lambda: args[0] if method_of else None)()
                rest = args[1:] if method_of else args
                before = {"self": _plain(copy.deepcopy(subject)) if method_of else None, "args": _plain(copy.deepcopy(rest))["__tuple__"],
                          "kwargs": _plain(copy.deepcopy(kwargs))}
            except TypeError:
                skipped[name] = skipped.get(name, 0) + 1
                return fn(*args, **kwargs)
            depth[0] += 1
            try:
                out = fn(*args, **kwargs)
            finally:
                depth[0] -= 1
            try:
                records.append({"module": module, "class": method_of, "fn": name, **before, "result": _plain(copy.deepcopy(out)),
                                "args_after": _plain(copy.deepcopy(rest))["__tuple__"]})
            except TypeError:
                skipped[name] = skipped.get(name, 0) + 1
            return out
        return wrapped

    sch = sys.modules["yomitoku.schemas.table_semantic_parser"]
    kvp = sys.modules["yomitoku.kv_parser"]
    for module, mod, names in (("table_semantic_parser", tsp, UNIT_FUNCTIONS["table_semantic_parser"]), ("kv_parser", kvp, UNIT_FUNCTIONS["kv_parser"]),
                               ("table_semantic_schemas", sch, UNIT_FUNCTIONS["table_semantic_schemas"])):
        for name in names:
            setattr(mod, name, recorder(module, name, getattr(mod, name)))
    tsp.parse_kv_items = kvp.parse_kv_items
    for cls, names in UNIT_METHODS.items():
        for name in names:
            setattr(getattr(sch, cls), name, recorder("table_semantic_schemas", name, getattr(getattr(sch, cls), name), method_of=cls))
    for name in ("aggregate", "replace_table_to_paragraphs"):  # the tests call them unbound, with a bare object() as self
        setattr(tsp.TableSemanticParser, name, recorder("table_semantic_parser", name, getattr(tsp.TableSemanticParser, name), method_of="TableSemanticParser"))
    tests = os.path.join(os.path.dirname(REF_SRC), "tests")
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "pytest.ini"), "w").write("[pytest]\n")
        code = pytest.main([*(os.path.join(tests, f) for f in UNIT_TEST_FILES), "-q", "-p", "no:cacheprovider", "--rootdir", tmp,
                            "-c", os.path.join(tmp, "pytest.ini"), "--basetemp", os.path.join(tmp, "bt"), "--import-mode=importlib"])
    per_fn = {}
    for r in records:
        per_fn[r["fn"]] = per_fn.get(r["fn"], 0) + 1
    write(os.path.join(out_dir, "table_semantic_unit_cases.json"),
          {"source": "tests/" + ", tests/".join(UNIT_TEST_FILES) + " of the reference, run against the reference's own functions",
           "pytest_exit_code": int(code), "calls_per_function": per_fn, "skipped_unrecordable": skipped, "calls": records})
    print(f"[unit cases] pytest exit {int(code)}, {len(records)} calls: {per_fn}; skipped {skipped}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "table_semantic"))
    ap.add_argument("--profile", default=os.path.join(ROOT, "profiles", "table_semantic_host_ms.json"))
    ap.add_argument("--no-units", action="store_true")
    args = ap.parse_args()
    tsp = load_reference()
    files = sorted(glob.glob(os.path.join(os.path.dirname(REF_SRC), "tests", "data", "table_semantic_inputs", "*.json")),
                   key=lambda p: int(os.path.basename(p).split("_")[-1].split(".")[0]))
    assert len(files) == 11, files
    largest = None
    for n, path in enumerate(files):
        assert os.path.basename(path) == f"debug_table_raw_{n}.json"
        tables = json.load(open(path, encoding="utf-8"))
        words = synthetic_words(tables)
        write(os.path.join(args.out, "inputs", f"case_{n:02d}.json"), {"tables": tables, "words": words})
        for ocr_name, ocr_words in (("empty", []), ("words", words)):
            write(os.path.join(args.out, "expected", f"case_{n:02d}_{ocr_name}.json"), expected_of(tsp, tables, ocr_words))
        n_cells = sum(len(t["cells"]) for t in tables)
        if largest is None or n_cells > largest[0]:
            largest = (n_cells, n, tables, words)
        print(f"case {n}: {len(tables)} tables, {n_cells} cells, {len(words)} words")
    # template round trip on the case with model-predicted regions
    tables, words = json.load(open(files[10], encoding="utf-8")), None
    words = synthetic_words(tables)
    with tempfile.TemporaryDirectory() as tmp:
        tpath = os.path.join(tmp, "template.json")
        run_reference(tsp, tables, words, "default").save_template_json(tpath)
        template = json.load(open(tpath, encoding="utf-8"))
        write(os.path.join(args.out, "template_case_10.json"), {"template": template, "result": views(run_reference(tsp, tables, words, "default", template=tpath))})
    # host cost of the semantic stage (everything after the networks) on the largest case
    n_cells, n, tables, words = largest
    times = []
    for k in range(23):
        t0 = time.perf_counter()
        run_reference(tsp, tables, words, "default")
        times.append((time.perf_counter() - t0) * 1e3)
    prof = json.load(open(args.profile)) if os.path.exists(args.profile) else {}
    prof["reference"] = {"case": n, "cells": n_cells, "words": len(words), "median_ms": round(statistics.median(times[3:]), 2), "runs": 20, "warmup": 3,
                         "what": "the reference's TableSemanticParser.__call__ with run_models replaced (schema validation of the inputs included), CPU of the development container"}
    os.makedirs(os.path.dirname(args.profile), exist_ok=True)
    json.dump(prof, open(args.profile, "w"), indent=1)
    print("reference host ms", prof["reference"])
    if not args.no_units:
        record_unit_cases(tsp, args.out)


if __name__ == "__main__":
    main()
