"""The calls that the reference's own tests of the table-semantic parser make into its functions and schema methods
(tests/test_kv_parser.py, test_table_semantic_parser.py, test_table_semantic_parser_utils.py of the reference), recorded by
tools/record_table_semantic_golden.py against the reference and replayed here on yomitoku_amd: same arguments in, same results
out, arguments left in the same state.  Plus a few spelled-out cases of the row clustering behind the cell ids."""
import copy
import gzip
import json
import os
from types import SimpleNamespace

import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "table_semantic", "table_semantic_unit_cases.json.gz")


def _load():
    with gzip.open(GOLDEN, "rt", encoding="utf-8") as f:
        return json.load(f)


def _build(v):
    """Recorded JSON -> live arguments: models of THIS package's schemas, namespaces, tuples, sets."""
    from yomitoku_amd import schemas

    if isinstance(v, dict):
        if "__model__" in v:
            return getattr(schemas, v["__model__"])(**v["fields"])
        if "__ns__" in v:
            return SimpleNamespace(**{k: _build(x) for k, x in v["__ns__"].items()})
        if "__tuple__" in v:
            return tuple(_build(x) for x in v["__tuple__"])
        if "__set__" in v:
            return set(_build(x) for x in v["__set__"])
        if "__items__" in v:
            return {_build(k): _build(x) for k, x in v["__items__"]}
        return {k: _build(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_build(x) for x in v]
    return v


def _plain(v):
    """Results in the recorder's form; a graph is recorded by its node count only."""
    from yomitoku_amd.utils.graph import OrderedDiGraph

    if hasattr(v, "model_dump"):
        return {"__model__": type(v).__name__, "fields": _plain(v.model_dump())}
    if isinstance(v, SimpleNamespace):
        return {"__ns__": _plain(vars(v))}
    if isinstance(v, OrderedDiGraph):
        return {"__graph__": len(v)}
    if isinstance(v, tuple):
        return {"__tuple__": [_plain(x) for x in v]}
    if isinstance(v, (set, frozenset)):
        return {"__set__": sorted(_plain(x) for x in v)}
    if isinstance(v, dict):
        if not all(isinstance(k, str) for k in v):
            return {"__items__": [[_plain(k), _plain(x)] for k, x in v.items()]}
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_plain(x) for x in v]
    return v


def _json(v):
    return json.loads(json.dumps(v, ensure_ascii=False))


_CALLS = _load()["calls"]


def _target(call):
    import yomitoku_amd.kv_parser
    import yomitoku_amd.table_semantic_parser
    import yomitoku_amd.table_semantic_schemas

    module = getattr(yomitoku_amd, call["module"])
    if call["class"] is None:
        return getattr(module, call["fn"]), []
    subject = _build(copy.deepcopy(call["self"]))
    if call["class"] == "TableSemanticContentsView":
        return getattr(subject.view, call["fn"]), []
    if call["class"] == "TableSemanticParser":  # the reference's tests call these unbound, with a bare object as self
        parser = module.TableSemanticParser.__new__(module.TableSemanticParser)
        return getattr(parser, call["fn"]), []
    assert type(subject).__name__ == call["class"]
    return getattr(subject, call["fn"]), []


@pytest.mark.parametrize("k", range(len(_CALLS)), ids=[f"{i:03d}_{c['fn']}" for i, c in enumerate(_CALLS)])
def test_recorded_reference_call(k):
    call = _CALLS[k]
    fn, _ = _target(call)
    args = _build(copy.deepcopy(call["args"]))
    out = fn(*args, **_build(copy.deepcopy(call["kwargs"])))
    assert _json(_plain(out)) == call["result"]
    assert _json(_plain(list(args))) == call["args_after"]


def test_fixture_covers_the_reference_tests():
    g = _load()
    assert g["skipped_unrecordable"] == {}
    assert set(g["calls_per_function"]) == {
        "parse_kv_items", "normalize", "make_unique_all", "safe_contents", "find_cell_by_id", "search_cells_by_query", "kv_items_to_dict",
        "grids_to_dict", "kv_items_to_nested", "kv_items_to_structured", "grids_to_structured", "to_structured", "to_simple",
        "_resolve_overlapping_regions", "_split_nodes_with_role", "get_cell_by_id", "sort_cells", "_sort_elements", "_assign_ids",
        "_region_cell_ids", "aggregate", "replace_table_to_paragraphs"}
    assert len(g["calls"]) == sum(g["calls_per_function"].values()) >= 100


# ------------------------------------------------------------------------------------------------ row clustering, spelled out
def _cell(cid, box, role="cell"):
    from yomitoku_amd.schemas import CellSchema

    return CellSchema(id=cid, box=list(box), role=role, contents="", row=None, col=None, row_span=None, col_span=None)


def test_gap_valley_tol_cases():
    from yomitoku_amd.table_semantic_parser import _gap_valley_tol

    assert _gap_valley_tol([]) == 8.0 and _gap_valley_tol([5]) == 8.0
    assert _gap_valley_tol([10, 11, 12]) == 8.0              # a single row: no gap above min_tol
    assert _gap_valley_tol([0, 9], min_tol=8) == 8.5           # one gap of 9 against the reference gap 8: the middle
    # jitter of up to 3 px inside two rows 57 px apart: gaps 1, 1, 2, 2, 57 - the valley is between 2 and 57
    assert _gap_valley_tol([100, 103, 101, 160, 162, 163]) == 29.5


def test_sort_cells_single_row():
    from yomitoku_amd.table_semantic_parser import sort_cells

    cells = [_cell("c0", (200, 10, 300, 40)), _cell("c1", (0, 11, 100, 41)), _cell("c2", (100, 12, 200, 42))]
    out, remap = sort_cells(cells)
    assert remap == {"c1": "r0c0", "c2": "r0c1", "c0": "r0c2"}
    assert [c.id for c in out] == ["r0c0", "r0c1", "r0c2"] and [c.box[0] for c in out] == [0, 100, 200]


def test_sort_cells_two_rows_nine_px_apart():
    """9 px between the top edges against min_tol = 8: two rows (the threshold falls at 8.5)."""
    from yomitoku_amd.table_semantic_parser import sort_cells

    cells = [_cell("a", (0, 0, 50, 9)), _cell("b", (0, 9, 50, 18)), _cell("c", (50, 0, 100, 9)), _cell("g", (0, 0, 100, 18), role="group")]
    out, remap = sort_cells(cells)
    assert remap == {"a": "r0c0", "c": "r0c1", "b": "r1c0", "g": "grp0"}
    assert [c.id for c in out] == ["r0c0", "r0c1", "r1c0", "grp0"]  # values in reading order, groups last


def test_sort_cells_jitter_inside_a_row():
    from yomitoku_amd.table_semantic_parser import sort_cells

    tops = {"a": 100, "b": 103, "c": 101, "d": 160, "e": 162, "f": 163}
    xs = {"a": 0, "b": 100, "c": 200, "d": 0, "e": 100, "f": 200}
    _, remap = sort_cells([_cell(k, (xs[k], tops[k], xs[k] + 100, tops[k] + 50)) for k in tops])
    assert remap == {"a": "r0c0", "b": "r0c1", "c": "r0c2", "d": "r1c0", "e": "r1c1", "f": "r1c2"}
    assert sort_cells([]) == ([], {})
