"""The page-file entries - encode_jpeg_pages, encode_g4_pages, encode_mrc_pages, deskew_pages - launch the same device work, in
the same order, behind the same waits, and write the same bytes as when tests/golden/page_files_calls.json was recorded
(tools/record_page_files_golden.py, whose cases and recorder these are).  The per-feature tests hold the bytes to their
definitions; this one holds the sequence, which decides the speed and which no definition sees."""

import functools
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("defaults", "optimize", "grey_auto", "grey_auto_no_strips", "bilevel_auto_grey_auto_no_strips", "bilevel_otsu",
         "bilevel_adaptive_mrc_optimize_444", "mrc_cells_1_4", "one_scratch_two_cases", "g4_plain", "g4_otsu", "encode_mrc_pages",
         "deskew_two_pages")


@functools.lru_cache(maxsize=None)
def _tool():
    spec = importlib.util.spec_from_file_location("record_page_files_golden", os.path.join(ROOT, "tools", "record_page_files_golden.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@functools.lru_cache(maxsize=None)
def _golden():
    with open(_tool().GOLDEN) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _recorded():
    return json.loads(json.dumps(_tool().record_all()))  # as the file holds it: tuples are lists


def test_the_fixture_holds_these_cases():
    assert sorted(_golden()) == sorted(CASES)
    assert [name for name, _ in _tool().cases(_tool().batch())] == list(CASES)


@pytest.mark.parametrize("case", CASES)
def test_same_launches_same_waits_same_bytes(case):
    want, got = _golden()[case], _recorded()[case]
    assert got["calls"] == want["calls"]
    assert len(got["entries"]) == len(want["entries"])
    for k, (g, w) in enumerate(zip(got["entries"], want["entries"])):
        assert g == w, f"entry {k}"
