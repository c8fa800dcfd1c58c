"""Host check over the Python sources: what the page pipeline (yomitoku_amd/serving.py) asks of an analyzer has ONE
implementation.  DocumentAnalyzer and TableSemanticParser derive from serving.StageAnalyzer and share its chain plumbing, OCR
stages and render stage as the same function objects - neither restates one, and the parser borrows nothing from the
analyzer class; the pipeline stays below both (it imports neither) and owns its own `rec_lanes_asked`."""
import ast
import glob
import os
import re

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yomitoku_amd")
SHARED = ("_submit", "_on_stream", "_stage_detect", "_stage_boxes", "_stage_crops", "_stage_recognize", "_stage_decode", "_stage_render")


def _source(name):
    with open(os.path.join(PKG, name)) as f:
        return f.read()


def test_both_analyzers_share_the_base_class_stages():
    from yomitoku_amd.document_analyzer import DocumentAnalyzer
    from yomitoku_amd.serving import StageAnalyzer
    from yomitoku_amd.table_semantic_parser import TableSemanticParser

    assert issubclass(DocumentAnalyzer, StageAnalyzer) and issubclass(TableSemanticParser, StageAnalyzer)
    for name in SHARED:
        assert getattr(DocumentAnalyzer, name) is getattr(TableSemanticParser, name) is getattr(StageAnalyzer, name), name
        assert name not in vars(DocumentAnalyzer) and name not in vars(TableSemanticParser), name


def test_the_parser_borrows_nothing_and_the_pipeline_imports_no_analyzer():
    assert not re.search(r"=\s*DocumentAnalyzer\.", _source("table_semantic_parser.py"))
    imported = set()
    for node in ast.walk(ast.parse(_source("serving.py"))):
        if isinstance(node, ast.ImportFrom):
            imported.update({node.module or ""} | {a.name for a in node.names})
        elif isinstance(node, ast.Import):
            imported.update(a.name for a in node.names)
    assert imported and not [m for m in imported if re.search(r"document_analyzer|table_semantic_parser", m)]


def test_only_the_pipeline_sets_rec_lanes_asked():
    """Assignments to `<something>.rec_lanes_asked`: one, on `self`, in the constructor of PagePipeline."""
    found = []
    for path in sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True)):
        with open(path) as f:
            found += [(os.path.relpath(path, PKG), m.group(1)) for m in re.finditer(r"([\w.\[\]()]+)\.rec_lanes_asked\s*=(?!=)", f.read())]
    assert found == [("serving.py", "self")]
    tree = ast.parse(_source("serving.py"))
    (pipeline,) = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "PagePipeline"]
    (init,) = [n for n in pipeline.body if isinstance(n, ast.FunctionDef) and n.name == "__init__"]
    assert "rec_lanes_asked" in ast.get_source_segment(_source("serving.py"), init)


def test_a_hook_the_handover_object_lacks_passes_the_value_through():
    """The parser's hand-over objects have `tables` only - and may keep data under any other name (tools/table_semantic_serve_timing.py
    holds its table boxes in `.boxes`, the name of the analyzer's hook after box extraction)."""
    from types import SimpleNamespace

    from yomitoku_amd.serving import StageAnalyzer

    an = StageAnalyzer.__new__(StageAnalyzer)
    value = object()
    for an.handover in (None, SimpleNamespace(tables=lambda k, t: t, boxes=[[1, 2, 3, 4]])):
        assert an._handed("boxes", "wave", value) is value and an._handed("maps", "wave", value) is value
    an.handover = SimpleNamespace(boxes=lambda wave, v: (wave, v))
    assert an._handed("boxes", "wave", value) == ("wave", value)
