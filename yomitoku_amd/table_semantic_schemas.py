"""Result types of TableSemanticParser (reference schemas/table_semantic_parser.py:23-1145): the same class names, field
names, defaults and methods, so that `model_dump()` matches key for key.  `CellSchema`, `RegionSchema` and
`TableDetectorSchema` - the records the cell detector hands over - stay in schemas.py; everything here is reachable as
`yomitoku_amd.schemas.<name>` too.

A table is stored normalised: `cells` by id, `kv_items` and `grids` referring to cells by id.  The views
(`table.view`, `doc.to_dict / to_structured / to_simple`) resolve the ids to text (and boxes); the exporters
(`table.export`) write them out.  A template (`save_template_json` / `load_template_json`) overrides roles, contents, kv
items and grids of the tables it matches by position.
"""

from __future__ import annotations

import json
import os
import re
from typing import Any, Dict, List, Literal, Optional, Union

from pydantic import Field, PrivateAttr

from .base import BaseSchema
from .geometry import calc_overlap_ratio, is_bottom_adjacent, is_contained, is_right_adjacent, quad_to_xyxy
from .reading_order import prediction_reading_order
from .schemas import Box, CellSchema, Element, ParagraphSchema, WordPrediction

MatchPolicy = Literal["cell_id", "bbox"]

# reserved keys of the nested kv view (an underscore in front keeps them apart from real key texts):
UNKEYED_KEY = "_unkeyed"       # under it: the values of cells that have no key
NESTED_VALUE_KEY = "_value"    # a parent key that has a value of its own AND child keys keeps the value here


def make_unique_all(seq):
    """Key lists that occur more than once get their occurrence index appended ([k] -> [k, 0], [k, 1]); unique ones stay."""
    total = {}
    for x in seq:
        total[tuple(x)] = total.get(tuple(x), 0) + 1
    seen = {}
    out = []
    for x in seq:
        k = tuple(x)
        out.append(x + [seen.get(k, 0)] if total[k] > 1 else list(x))
        seen[k] = seen.get(k, 0) + 1
    return out


def normalize(text: str) -> str:
    """Drop half- and full-width spaces."""
    return re.sub("[ 　]", "", text)


def _ensure_dir_of(path):
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)


def _write_json(obj, path):
    with open(path, "w", encoding="utf-8") as f:
        json.dump(obj, f, ensure_ascii=False, indent=4)


class TemplateMetaSchema(BaseSchema):
    template_version: str = "beta"
    template_id: Optional[str] = None
    notes: Optional[str] = None
    match_policy: MatchPolicy = "cell_id"


class KvItemSchema(BaseSchema):
    id: Optional[str]
    key: Union[str, List[str]]
    value: str
    box: Optional[Box] = None


class TableGridSchema(BaseSchema):
    id: Optional[str]
    box: Box
    n_row: int
    n_col: int
    col_headers: List[List[str]]
    data: List[List[Optional[str]]]


# ---- the structured view: ids resolved to text, with the cells the text came from
class StructuredCellRefSchema(BaseSchema):
    id: Optional[str]
    box: Box


class StructuredEntrySchema(BaseSchema):
    """key: texts from the outermost header inwards (empty for a keyless cell), matching key_cells one to one.  In kv items
    several values under one key chain are joined in spatial order and value_cells lists them in that order; in a grid
    row value_cells has one entry."""

    key: List[str]
    value: str
    key_cells: List[StructuredCellRefSchema]
    value_cells: List[StructuredCellRefSchema]


class StructuredGridRowSchema(BaseSchema):
    cells: List[StructuredEntrySchema]


class StructuredGridSchema(BaseSchema):
    id: Optional[str]
    box: Box
    n_row: int
    n_col: int
    rows: List[StructuredGridRowSchema]


class StructuredTableSchema(BaseSchema):
    id: Optional[str] = None
    box: Box
    style: str
    kv_items: List[StructuredEntrySchema]
    grids: List[StructuredGridSchema]


class StructuredDocumentSchema(BaseSchema):
    tables: List[StructuredTableSchema]
    paragraphs: List[Element]


# ---- the simple view: text only
class SimpleGridSchema(BaseSchema):
    id: Optional[str]
    rows: List[Dict[str, str]]


class SimpleTableSchema(BaseSchema):
    id: Optional[str] = None
    kv_items: Dict[str, Any]
    grids: List[SimpleGridSchema]


class SimpleDocumentSchema(BaseSchema):
    tables: List[SimpleTableSchema]
    paragraphs: List[Optional[str]]


class TableSemanticContentsSchema(BaseSchema):
    id: Optional[str] = None
    style: str
    box: Box
    cells: Dict[str, CellSchema]
    kv_items: List[KvItemSchema]
    grids: List[TableGridSchema]

    _export: "TableSemanticContentsExport" = PrivateAttr()
    _view: "TableSemanticContentsView" = PrivateAttr()

    def __init__(self, **data):
        super().__init__(**data)
        self._view = TableSemanticContentsView(self)
        self._export = TableSemanticContentsExport(self)

    @property
    def view(self) -> "TableSemanticContentsView":
        return self._view

    @property
    def export(self) -> "TableSemanticContentsExport":
        return self._export

    def safe_contents(self, cell_id, ignore_space=True) -> str:
        cell = self.cells.get(cell_id)
        text = (cell.contents or "") if cell is not None else ""
        return text.replace(" ", "") if ignore_space else text

    def find_cell_by_id(self, cell_id) -> Optional[CellSchema]:
        return self.cells.get(str(cell_id))

    def _value_cells(self):
        return [c for c in self.cells.values() if c.role != "group"]

    def search_cells_by_bbox(self, box) -> List[CellSchema]:
        return [c for c in self._value_cells() if is_contained(box, c.box, threshold=0.5)]

    def search_cells_by_query(self, query: str) -> List[CellSchema]:
        q = normalize(query)
        return [c for c in self.cells.values() if c.contents and c.role != "group" and q in normalize(c.contents)]

    def _search_neighbours(self, key, touches):
        """Every (cell, query cell) contact yields the cell once, so a cell touching two query cells is listed twice."""
        query_cells = self.search_cells_by_query(key)
        return [c for c in self._value_cells() for q in query_cells if touches(q, c)]

    def search_cells_below_key_text(self, key: str) -> List[CellSchema]:
        return self._search_neighbours(key, lambda q, c: is_bottom_adjacent(q.box, c.box))

    def search_cells_right_of_key_text(self, key: str) -> List[CellSchema]:
        return self._search_neighbours(key, lambda q, c: is_right_adjacent(q.box, c.box))

    def search_cells_left_of_key_text(self, key: str) -> List[CellSchema]:
        return self._search_neighbours(key, lambda q, c: is_right_adjacent(c.box, q.box))

    def search_cells_upper_key_text(self, key: str) -> List[CellSchema]:
        return self._search_neighbours(key, lambda q, c: is_bottom_adjacent(c.box, q.box))

    def search_kv_items_by_key(self, key: str) -> List[dict]:
        """{"key": key cells, "value": value cell} for every kv item whose joined key text holds `key`.  For a grid column
        whose header text holds it the reference appends one {"key": header cells, "value": []} per data row - the value
        list is never filled there (schemas/table_semantic_parser.py:445-457), and its header text is looked up by the
        header's TEXT as if it were a cell id, so it is empty and only an empty query matches; both are mirrored."""
        q = normalize(key)
        results: List[dict] = []
        for kv in self.kv_items:
            key_cells = [self.cells.get(k) for k in kv.key]
            text = "".join((c.contents or "") for c in key_cells if c)
            if q in normalize(text):
                results.append({"key": key_cells, "value": self.cells.get(kv.value)})
        for grid in self.grids:
            for header in grid.col_headers:
                col_cells = [self.cells.get(h) for h in header]
                text = "".join(self.safe_contents(c.contents) for c in col_cells if c)
                if q in normalize(text):
                    for _ in grid.data:
                        results.append({"key": col_cells, "value": []})
        return results

    def find_table_by_column_name(self, queries) -> "TableSemanticContentsSchema":
        grids = [g for g in (self.filter_columns_ignore_space(grid, queries) for grid in self.grids) if g is not None]
        return TableSemanticContentsSchema(id=self.id, box=self.box, style=self.style, cells=self.cells, grids=grids,
                                           kv_items=self.kv_items)

    def filter_columns_ignore_space(self, grid, queries) -> Optional[TableGridSchema]:
        """The columns of `grid` whose joined header text holds one of `queries` (spaces ignored); None when none does."""
        wanted = [normalize(q) for q in queries]
        width = max((len(row) for row in grid.data), default=0)
        keep = []
        for i, header in enumerate(grid.col_headers[:width]):
            text = normalize("".join(self.cells.get(h).contents or "" for h in header))
            if any(q in text for q in wanted):
                keep.append(i)
        # a row contributes the kept columns it has; header lists that repeat collapse to their first occurrence
        data = [[row[i] for i in keep if i < len(row)] for row in grid.data]
        data = [r for r in data if r]
        if not data:
            return None
        headers = list(dict.fromkeys(tuple(grid.col_headers[i]) for i in keep))
        return TableGridSchema(id=grid.id, data=data, n_col=len(data[-1]), n_row=len(data), col_headers=headers, box=grid.box)


class TableSemanticContentsExport:
    def __init__(self, table: TableSemanticContentsSchema):
        self.table = table

    def to_json(self, out_path, separator="\n"):
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        _write_json({"kv_items": self.table.view.kv_items_to_nested(separator=separator),
                     "grids": self.table.view.grids_to_dict()}, out_path)

    def grids_to_csv(self, out_path, columns=None, ignore_space=True) -> List[List[List[str]]]:
        """One file per grid, `<out_path without extension>_<grid id>.csv`; returns the rows of every grid."""
        table = self.table if columns is None else self.table.find_table_by_column_name(queries=columns)
        _ensure_dir_of(out_path)
        base = out_path.rsplit(".", 1)[0]
        csvs = []
        for grid in table.grids:
            rows = [[table.safe_contents(cell_id, ignore_space) for cell_id in row] for row in grid.data]
            with open(f"{base}_{grid.id}.csv", "w", encoding="utf-8") as f:
                for row in rows:
                    f.write(",".join(row) + "\n")
            csvs.append(rows)
        return csvs

    def grids_to_json(self, out_path):
        grids = self.table.view.grids_to_dict()
        _ensure_dir_of(out_path)
        _write_json(grids, out_path)
        return grids

    def kv_items_to_json(self, out_path, separator="\n"):
        kv_items = self.table.view.kv_items_to_nested(separator=separator)
        _ensure_dir_of(out_path)
        _write_json(kv_items, out_path)
        return kv_items


class TableSemanticContentsView:
    def __init__(self, table: TableSemanticContentsSchema):
        self.table = table

    def kv_items_to_dict(self, separator="\n") -> dict:
        return self.kv_items_to_nested(separator=separator)

    def _grid_rows(self, grid, guard):
        """Per data row the (column, cell id) pairs that count: not a header cell of its column, first occurrence in the row.
        `guard`: also skip holes (None) and columns beyond col_headers (the structured view; grids_to_dict takes them)."""
        for row in grid.data:
            seen = set()
            picked = []
            for i, cell_id in enumerate(row):
                if guard and i >= len(grid.col_headers):
                    break
                if guard and cell_id is None:
                    continue
                if cell_id in grid.col_headers[i] or cell_id in seen:
                    continue
                seen.add(cell_id)
                picked.append((i, cell_id))
            yield picked

    def grids_to_dict(self, ignore_space=True) -> List[dict]:
        t = self.table
        results = []
        for grid in t.grids:
            records = []
            for picked in self._grid_rows(grid, guard=False):
                keys = make_unique_all([[t.safe_contents(h, ignore_space) for h in grid.col_headers[i]] for i, _ in picked])
                record = {"_".join(map(str, k)): t.safe_contents(cell_id, ignore_space) for k, (_, cell_id) in zip(keys, picked)}
                if record:
                    records.append(record)
            results.append({"id": grid.id, "rows": records})
        return results

    def _cell_refs(self, cell_ids) -> List[StructuredCellRefSchema]:
        """Ids that are not in `cells` are left out without a word (safe_contents answers "" for them)."""
        cells = (self.table.find_cell_by_id(i) for i in cell_ids)
        return [StructuredCellRefSchema(id=c.id, box=c.box) for c in cells if c is not None]

    def _kv_groups(self) -> List[dict]:
        """kv items grouped by their key CELLS (ids, not texts: two fields that happen to carry the same label stay apart;
        keyless cells are never merged), each group's values in spatial order: by y when they spread at least as far
        vertically as horizontally, else by x; values whose cell is missing go last."""
        t = self.table
        groups, by_key = [], {}
        for kv in t.kv_items:
            key_ids = [kv.key] if isinstance(kv.key, str) else list(kv.key)
            group = by_key.get(tuple(key_ids)) if key_ids else None
            if group is None:
                group = {"key_ids": key_ids, "values": []}
                groups.append(group)
                if key_ids:
                    by_key[tuple(key_ids)] = group
            group["values"].append((t.safe_contents(kv.value), t.find_cell_by_id(kv.value), kv.value))
        for group in groups:
            values = group["values"]
            if len(values) < 2:
                continue
            found = [v for v in values if v[1] is not None]
            if found:
                xs = [v[1].box[0] for v in found]
                ys = [v[1].box[1] for v in found]
                axis = 1 if max(ys) - min(ys) >= max(xs) - min(xs) else 0
                found.sort(key=lambda v: v[1].box[axis])
            group["values"] = found + [v for v in values if v[1] is None]
        return groups

    def kv_items_to_structured(self, separator="\n") -> List[StructuredEntrySchema]:
        t = self.table
        return [StructuredEntrySchema(key=[t.safe_contents(i) for i in g["key_ids"]],
                                      value=separator.join(str(v[0]) for v in g["values"]),
                                      key_cells=self._cell_refs(g["key_ids"]),
                                      value_cells=self._cell_refs([v[2] for v in g["values"]]))
                for g in self._kv_groups()]

    def kv_items_to_nested(self, separator="\n") -> dict:
        """The key chains (parent header -> child header) as a tree of dicts.  Nodes are told apart by cell id; children of
        one node that carry the same text (repeated blocks) become a list under that text.  A key with a value and child
        keys keeps the value under "_value"; keyless cells are listed under "_unkeyed"."""
        t = self.table

        def new_node(text):
            return {"text": text, "children": {}, "values": []}

        root = new_node(None)
        for i, group in enumerate(self._kv_groups()):
            chain = [(cid, t.safe_contents(cid)) for cid in group["key_ids"]] or [(f"__keyless_{i}", UNKEYED_KEY)]
            node = root
            for cell_id, text in chain:
                node = node["children"].setdefault(cell_id, new_node(text))
            node["values"].append(separator.join(str(v[0]) for v in group["values"]))
        return self._render_nested_node(root)

    def _render_nested_node(self, node) -> dict:
        by_text = {}
        for child in node["children"].values():
            sub = self._render_nested_node(child)
            if child["values"]:  # one value at most: the groups are unique per key chain
                sub = {NESTED_VALUE_KEY: child["values"][0], **sub} if sub else child["values"][0]
            by_text.setdefault(child["text"], []).append(sub)
        return {text: items[0] if len(items) == 1 else items for text, items in by_text.items()}

    def grids_to_structured(self, ignore_space=True) -> List[StructuredGridSchema]:
        t = self.table
        results = []
        for grid in t.grids:
            rows = []
            for picked in self._grid_rows(grid, guard=True):
                entries = [StructuredEntrySchema(key=[t.safe_contents(h, ignore_space) for h in grid.col_headers[i]],
                                                 value=t.safe_contents(cell_id, ignore_space),
                                                 key_cells=self._cell_refs(grid.col_headers[i]),
                                                 value_cells=self._cell_refs([cell_id]))
                           for i, cell_id in picked]
                if entries:
                    rows.append(StructuredGridRowSchema(cells=entries))
            results.append(StructuredGridSchema(id=grid.id, box=grid.box, n_row=grid.n_row, n_col=grid.n_col, rows=rows))
        return results


# ---- templates
class CellTemplateSchema(BaseSchema):
    id: Optional[str] = None
    box: Optional[Box] = None
    role: Optional[str] = None
    contents: Optional[str] = None


class TableSemanticContentsTemplateSchema(BaseSchema):
    id: Optional[str] = None
    style: Optional[str] = None
    box: Box
    cells: Dict[str, CellTemplateSchema] = Field(default_factory=dict)
    kv_items: Optional[List[KvItemSchema]] = None
    grids: Optional[List[TableGridSchema]] = None


class TableSemanticParserTemplateSchema(BaseSchema):
    meta: TemplateMetaSchema
    tables: List[TableSemanticContentsTemplateSchema]

    def find_table_by_id(self, table_id):
        return next((t for t in self.tables if t.id == str(table_id)), None)


class TableSemanticParserSchema(BaseSchema):
    tables: List[TableSemanticContentsSchema]
    paragraphs: List[Element]
    words: List[WordPrediction]

    def search_words_by_position(self, bbox) -> str:
        """The text of the words at least half inside `bbox`, in reading order."""
        inside = []
        for word in self.words:
            box = quad_to_xyxy(word.points)
            if is_contained(bbox, box, threshold=0.5):
                inside.append(ParagraphSchema(box=box, contents=word.content, direction=word.direction, role=None, order=None))
        dirs = [w.direction for w in inside]
        horizontal = dirs.count("horizontal") > dirs.count("vertical")
        inside = prediction_reading_order(inside, "left2right" if horizontal else "right2left")
        return "".join(w.contents for w in sorted(inside, key=lambda w: w.order))

    @classmethod
    def load_json(cls, json_path: str) -> "TableSemanticParserSchema":
        with open(json_path, "r", encoding="utf-8") as f:
            return TableSemanticParserSchema.model_validate(json.load(f))

    def to_csv(self, outdir):
        for table in self.tables:
            table.export.grids_to_csv(out_path=f"{outdir}/table_{table.id}.csv")

    def to_dict(self, separator="\n"):
        """{table id: {"kv_items": nested dict, "grids": [{"id", "rows"}]}}."""
        return {table.id: {"kv_items": table.view.kv_items_to_nested(separator=separator), "grids": table.view.grids_to_dict()}
                for table in self.tables}

    def to_structured(self, separator="\n") -> StructuredDocumentSchema:
        tables = [StructuredTableSchema(id=t.id, box=t.box, style=t.style,
                                        kv_items=t.view.kv_items_to_structured(separator=separator),
                                        grids=t.view.grids_to_structured())
                  for t in self.tables]
        return StructuredDocumentSchema(tables=tables, paragraphs=self.paragraphs)

    def to_simple(self, separator="\n") -> SimpleDocumentSchema:
        """to_structured without boxes, cell references and scores; header texts that repeat inside a grid row get _0, _1
        ... appended so that no value is lost."""
        doc = self.to_structured(separator=separator)
        tables = []
        for src, table in zip(self.tables, doc.tables):
            grids = []
            for grid in table.grids:
                rows = []
                for row in grid.rows:
                    keys = make_unique_all([list(e.key) for e in row.cells])
                    rows.append({"_".join(map(str, k)): e.value for k, e in zip(keys, row.cells)})
                grids.append(SimpleGridSchema(id=grid.id, rows=rows))
            tables.append(SimpleTableSchema(id=table.id, kv_items=src.view.kv_items_to_nested(separator=separator), grids=grids))
        return SimpleDocumentSchema(tables=tables, paragraphs=[p.contents for p in doc.paragraphs])

    def find_table_by_id(self, table_id):
        return next((t for t in self.tables if t.id == str(table_id)), None)

    def find_table_by_position(self, box) -> Optional[TableSemanticContentsSchema]:
        """The table that `box` covers most of (first among equals), if it covers more than half of it."""
        ratios = [calc_overlap_ratio(box, table.box)[0] for table in self.tables]
        if not ratios:
            return None
        best = ratios.index(max(ratios))
        return self.tables[best] if ratios[best] > 0.5 else None

    def search_kv_items_by_key(self, key: str) -> List[dict]:
        return [hit for table in self.tables for hit in table.search_kv_items_by_key(key)]

    def load_template_json(self, template_path: str) -> "TableSemanticParserSchema":
        with open(template_path, "r", encoding="utf-8") as f:
            template = TableSemanticParserTemplateSchema.model_validate(json.load(f))
        return apply_table_template(self, template)

    def save_template_json(self, out_path: str, include_kv: bool = True, include_grids: bool = True):
        tables = []
        for t in self.tables:
            cells = {str(cid): CellTemplateSchema(id=str(c.id) if c.id is not None else str(cid),
                                                  box=list(c.box) if c.box is not None else None, role=c.role, contents=c.contents)
                     for cid, c in t.cells.items() if c.role != "group"}
            tables.append(TableSemanticContentsTemplateSchema(id=t.id, style=t.style, box=list(t.box), cells=cells,
                                                              kv_items=t.kv_items if include_kv else None,
                                                              grids=t.grids if include_grids else None))
        template = TableSemanticParserTemplateSchema(meta=TemplateMetaSchema(), tables=tables)
        _write_json(template.model_dump(exclude_none=True), out_path)


def _match_cell(table, tcell, policy="cell_id"):
    if policy == "cell_id":
        return table.cells.get(str(tcell.id)) if tcell.id else None
    if policy == "bbox":
        found = table.search_cells_by_bbox(list(tcell.box)) if tcell.box else []
        return found[0] if found else None
    return None


def apply_table_template(tables: TableSemanticParserSchema, tmpl: TableSemanticParserTemplateSchema) -> TableSemanticParserSchema:
    """Per template table, on the parsed table at its position: role and contents of the matched cells are overridden, kv
    items and grids are replaced where the template has them."""
    policy = getattr(tmpl.meta, "match_policy", "cell_id")
    for tmp_table in tmpl.tables:
        table = tables.find_table_by_position(tmp_table.box)
        if table is None:
            continue
        for tcell in tmp_table.cells.values():
            cell = _match_cell(table, tcell, policy=policy)
            if cell is None:
                continue
            if tcell.role is not None:
                cell.role = tcell.role
            if tcell.contents is not None:
                cell.contents = tcell.contents
        if tmp_table.kv_items is not None:
            table.kv_items = tmp_table.kv_items
        if tmp_table.grids is not None:
            table.grids = tmp_table.grids
    return tables


__all__ = ["MatchPolicy", "UNKEYED_KEY", "NESTED_VALUE_KEY", "make_unique_all", "normalize", "TemplateMetaSchema", "KvItemSchema",
           "TableGridSchema", "StructuredCellRefSchema", "StructuredEntrySchema", "StructuredGridRowSchema", "StructuredGridSchema",
           "StructuredTableSchema", "StructuredDocumentSchema", "SimpleGridSchema", "SimpleTableSchema", "SimpleDocumentSchema",
           "TableSemanticContentsSchema", "TableSemanticContentsExport", "TableSemanticContentsView", "CellTemplateSchema",
           "TableSemanticContentsTemplateSchema", "TableSemanticParserTemplateSchema", "TableSemanticParserSchema",
           "apply_table_template"]
