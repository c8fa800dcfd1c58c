"""The public surface of TableSemanticParser that needs no GPU: the export, the constructor's argument checks, and the
matrix form of `aggregate` against the plain double loop it replaces."""
import copy

import numpy as np
import pytest


def test_exported_from_the_package():
    import yomitoku_amd
    from yomitoku_amd import TableSemanticParser
    from yomitoku_amd.table_semantic_parser import TableSemanticParser as direct

    assert TableSemanticParser is direct and "TableSemanticParser" in yomitoku_amd.__all__


def test_schemas_are_reachable_from_yomitoku_amd_schemas():
    from yomitoku_amd import schemas, table_semantic_schemas

    for name in ("KvItemSchema", "TableGridSchema", "TableSemanticContentsSchema", "TableSemanticParserSchema", "StructuredDocumentSchema",
                 "SimpleDocumentSchema", "TableSemanticParserTemplateSchema", "CellTemplateSchema", "TemplateMetaSchema"):
        assert getattr(schemas, name) is getattr(table_semantic_schemas, name)
    from yomitoku_amd.schemas import KvItemSchema  # noqa: F401
    assert schemas.CellSchema.__module__ == "yomitoku_amd.schemas"  # the detector's records stay where they were
    with pytest.raises(AttributeError):
        schemas.NoSuchSchema


def test_configs_must_be_a_dict():
    from yomitoku_amd import TableSemanticParser

    with pytest.raises(ValueError, match="configs must be a dict"):
        TableSemanticParser(configs="table.yaml")


def test_visualize_is_not_supported():
    from yomitoku_amd import TableSemanticParser

    with pytest.raises(NotImplementedError, match="visualize=False only"):
        TableSemanticParser(visualize=True)
    parser = TableSemanticParser.__new__(TableSemanticParser)
    assert parser.visualize is False and parser.merge_same_column_values is False
    parser.visualize = True
    with pytest.raises(NotImplementedError):
        parser(np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(NotImplementedError):
        parser.parse_pages([])


def _aggregate_by_double_loop(words, cells, overlap_th=0.2):
    """The assignment as the reference states it: per word the non-group cell with the strictly largest overlap ratio."""
    from yomitoku_amd.geometry import calc_overlap_ratio, quad_to_xyxy
    from yomitoku_amd.reading_order import prediction_reading_order
    from yomitoku_amd.schemas import ParagraphSchema

    per_cell = [[] for _ in cells]
    for word in words:
        box = quad_to_xyxy(word.points)
        best, best_ratio = None, 0
        for k, cell in enumerate(cells):
            if cell.role == "group":
                continue
            ratio, _ = calc_overlap_ratio(cell.box, box)
            if ratio > best_ratio:
                best, best_ratio = k, ratio
        if best is None or best_ratio < overlap_th:
            continue
        per_cell[best].append(ParagraphSchema(box=box, contents=word.content, direction=word.direction, order=0, role=None))
    texts = []
    for inside in per_cell:
        if not inside:
            texts.append("")
            continue
        dirs = [w.direction for w in inside]
        horizontal = dirs.count("horizontal") >= dirs.count("vertical")
        prediction_reading_order(inside, "left2right" if horizontal else "right2left")
        texts.append("".join(w.contents for w in sorted(inside, key=lambda w: w.order)).strip())
    return texts, [len(x) for x in per_cell]


def test_aggregate_matrix_form_equals_the_double_loop():
    """300 random words x 80 cells: an 8 x 8 grid of cells plus 16 `group` cells that cover 2 x 2 blocks of it (a word inside a
    group must still go to the plain cell), words of random size - many straddle borders, some lie on a border exactly half and
    half (ties: the first cell wins), some cover less than the threshold of any cell, some lie outside."""
    from yomitoku_amd.schemas import CellSchema, OCRSchema, WordPrediction
    from yomitoku_amd.table_semantic_parser import TableSemanticParser

    rng = np.random.default_rng(31)
    cells = []
    for r in range(8):
        for c in range(8):
            cells.append(CellSchema(id=f"c{len(cells)}", box=[100 * c, 60 * r, 100 * c + 100, 60 * r + 60], role=["cell", "header", "empty"][(r + c) % 3],
                                    contents=None, row=None, col=None, row_span=None, col_span=None))
    for r in range(0, 8, 2):
        for c in range(0, 8, 2):
            cells.insert(int(rng.integers(0, len(cells))), CellSchema(id=f"g{r}{c}", box=[100 * c, 60 * r, 100 * c + 200, 60 * r + 120], role="group",
                                                                      contents="stale", row=None, col=None, row_span=None, col_span=None))
    assert len(cells) == 80
    words = []
    for k in range(300):
        kind = k % 6
        if kind == 0:    # exactly half in each of two horizontal neighbours
            c, r = int(rng.integers(1, 8)), int(rng.integers(0, 8))
            x1, x2, y1 = 100 * c - 20, 100 * c + 20, 60 * r + 10
            y2 = y1 + 30
        elif kind == 1:  # exactly half in each of two vertical neighbours
            c, r = int(rng.integers(0, 8)), int(rng.integers(1, 8))
            x1, y1, y2 = 100 * c + 10, 60 * r - 15, 60 * r + 15
            x2 = x1 + 50
        elif kind == 2:  # huge: below the threshold for every cell, or just above it for some
            x1, y1 = int(rng.integers(0, 300)), int(rng.integers(0, 200))
            x2, y2 = x1 + int(rng.integers(200, 500)), y1 + int(rng.integers(100, 300))
        else:
            x1, y1 = int(rng.integers(-50, 850)), int(rng.integers(-30, 500))
            x2, y2 = x1 + int(rng.integers(5, 160)), y1 + int(rng.integers(5, 90))
        x1, y1 = max(0, x1), max(0, y1)
        words.append(WordPrediction(points=[[x1, y1], [x2, y1], [x2, y2], [x1, y2]], content=f"w{k} ", direction="vertical" if k % 4 == 0 else "horizontal",
                                    rec_score=0.9, det_score=0.9))
    want, counts = _aggregate_by_double_loop(words, cells)
    assert sum(counts) < len(words) and max(counts) >= 3 and sum(n > 0 for n in counts) >= 40  # dropped words, and crowded cells
    got = copy.deepcopy(cells)
    TableSemanticParser.__new__(TableSemanticParser).aggregate(OCRSchema(words=words), got)
    assert [c.contents for c in got] == want
    assert all(c.contents == "" for c in got if c.role == "group")
    # no words, no cells
    TableSemanticParser.__new__(TableSemanticParser).aggregate(OCRSchema(words=[]), got)
    assert all(c.contents == "" for c in got)
    TableSemanticParser.__new__(TableSemanticParser).aggregate(OCRSchema(words=words), [])
