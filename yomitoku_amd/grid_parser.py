"""Grid reconstruction from detected cells, bottom up (reference grid_parser.py:16-923): which cells of a region form rows
and columns, where a cell spans several of them, and which rows are column headers.

The cells become nodes of an adjacency graph ("R"/"L" between horizontal neighbours, "D"/"U" between vertical ones).  A cell
with several neighbours on one side spans several rows (columns): it is cut into unit cells, one per neighbour slot, named
`<id>__dup<k>`, until every node has at most one neighbour per side.  Rows are then the "R" chains, columns the "D" chains,
and the grid entry (r, c) is the node both chains share; the `__dup` suffixes are dropped again, which leaves a spanning cell's
id in every entry it covers.

Every decision - thresholds, slot assignment, the order in which nodes are visited and duplicates numbered - follows the
reference; the graph is yomitoku_amd.utils.graph.OrderedDiGraph, whose iteration order is the contract the results rest on.
Where the reference iterates a Python set of ids (an order that changes from run to run) the order here is the graph's node
order or the geometric one; tests/golden/table_semantic holds the recorded results.
"""

from __future__ import annotations

from .geometry import get_line_with_head, is_bottom_adjacent, is_right_adjacent
from .table_semantic_schemas import TableGridSchema
from .utils.graph import OrderedDiGraph, UnionFind, connected_components

# Adjacency thresholds relative to the cells' own size.  Fixed pixel values break with the resolution and the row pitch (with
# 20 px rows a 20 px threshold makes the cell one row further down a "lower neighbour" and the unit-cell expansion produces
# zero-width slivers), so the lower quartile of the cell heights / widths of the cluster sets the scale.
GRID_DIST_SCALE = 0.5     # distance threshold = scale x this: only gaps well below one row (column) count as adjacency
GRID_IGNORE_SCALE = 0.25  # corner contacts (diagonal neighbours) closer than scale x this are rejected
GRID_DIST_FLOOR = 3.0     # px: ruling thickness and detection noise

# neighbours on one side whose intervals along the split axis have at least this IoU are one slot detected twice; a band header
# over its column headers (IoU ~ 0.3) is a real span and stays apart
OUT_GROUP_IOU_TH = 0.7


def _lower_quantile(values, q=0.25):
    ordered = sorted(values)
    return ordered[min(int(len(ordered) * q), len(ordered) - 1)]


def _calc_adjacency_thresholds(boxes):
    """{"dist", "ignore"} from the smaller of the lower-quartile cell height and width (a robust smallest cell size: merged
    cells do not move it)."""
    if not boxes:
        return {"dist": GRID_DIST_FLOOR, "ignore": GRID_DIST_FLOOR / 2}
    scale = min(_lower_quantile([b[3] - b[1] for b in boxes]), _lower_quantile([b[2] - b[0] for b in boxes]))
    return {"dist": max(GRID_DIST_FLOOR, GRID_DIST_SCALE * scale), "ignore": max(GRID_DIST_FLOOR / 2, GRID_IGNORE_SCALE * scale)}


def _adjacent(predicate, box_a, box_b, thresholds):
    return predicate(box_a, box_b, rule="soft", dist_threshold=thresholds["dist"], ignore_dist_threshold=thresholds["ignore"],
                     overlap_ratio_th=0.25)


def _get_grid_dag(nodes, thresholds=None):
    dag = OrderedDiGraph()
    cells = nodes["cell"] + nodes["empty"] + nodes["header"]
    if thresholds is None:
        thresholds = _calc_adjacency_thresholds([c.box for c in cells])
    for cell in cells:
        dag.add_node(cell.id, bbox=cell.box, role=cell.role, contents=cell.contents)
    for a in cells:
        for b in cells:
            if a.id == b.id:
                continue
            if _adjacent(is_bottom_adjacent, a.box, b.box, thresholds):
                dag.add_edge(a.id, b.id, dir="D")
                dag.add_edge(b.id, a.id, dir="U")
            if _adjacent(is_right_adjacent, a.box, b.box, thresholds):
                dag.add_edge(a.id, b.id, dir="R")
                dag.add_edge(b.id, a.id, dir="L")
    return dag


def _group_outs_by_axis_interval(G, outs, axis, iou_th=OUT_GROUP_IOU_TH):
    """Neighbours `outs` grouped by the IoU of their intervals along `axis` (0: x, 1: y), groups ordered by interval centre.
    Returns (groups of node ids, the union interval of each group)."""
    ivs = [(G.nodes[n]["bbox"][axis], G.nodes[n]["bbox"][axis + 2]) for n in outs]
    parent = list(range(len(outs)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i in range(len(outs)):
        for j in range(i + 1, len(outs)):
            (a1, a2), (b1, b2) = ivs[i], ivs[j]
            inter = max(0.0, min(a2, b2) - max(a1, b1))
            union = max(a2, b2) - min(a1, b1)
            if union > 0 and inter / union >= iou_th:
                parent[find(i)] = find(j)
    members = {}
    for i in range(len(outs)):
        members.setdefault(find(i), []).append(i)
    groups = [[outs[i] for i in idxs] for idxs in members.values()]
    intervals = [(min(ivs[i][0] for i in idxs), max(ivs[i][1] for i in idxs)) for idxs in members.values()]
    order = sorted(range(len(groups)), key=lambda k: (intervals[k][0] + intervals[k][1]) / 2.0)
    return [groups[k] for k in order], [intervals[k] for k in order]


def _assign_slots_by_intervals(lo, hi, groups, intervals, min_len=None):
    """[lo, hi] cut into consecutive slots along the groups' intervals (clipped to [lo, hi], each starting where the previous
    ended).  A group left with `min_len` or less - swallowed by its predecessor: a fused false detection covering a real cell,
    a value cell detected across a column border - gets no slot of its own and joins the previous slot (or, before the first
    slot, the next one); the last slot is stretched to `hi`.  Returns (slots, groups per slot), same length and order."""
    if min_len is None:
        min_len = GRID_DIST_FLOOR
    segs, merged, pending = [], [], []
    cur = lo
    for group, (a, b) in zip(groups, intervals):
        a = max(max(lo, min(a, hi)), cur)
        b = max(max(lo, min(b, hi)), a)
        if b - a <= min_len:
            (merged[-1] if merged else pending).extend(group)
            continue
        merged.append(pending + list(group))
        pending = []
        segs.append([a, b])
        cur = b
    if pending and merged:
        merged[-1].extend(pending)
    if segs:
        segs[-1][1] = hi
    return segs, merged


# what differs between cutting a cell along y (it has several right / left neighbours: rows) and along x (columns)
_SPLIT = {
    "R": dict(axis=1, predicate=is_right_adjacent, cross=("D", "U"), reverse=False, back=("pred", "R")),
    "L": dict(axis=1, predicate=is_right_adjacent, cross=("D", "U"), reverse=True, back=("pred", "L")),
    "D": dict(axis=0, predicate=is_bottom_adjacent, cross=("R", "L"), reverse=False, back=("pred", "D")),
    "U": dict(axis=0, predicate=is_bottom_adjacent, cross=("R", "L"), reverse=True, back=("succ", "D")),
}


def _normalize_with_out_edges(dag, head, dir_key, out_edge_type, in_edge_type, thresholds):
    """Walk from `head` along `out_edge_type` edges; a node with several slots of neighbours on that side is replaced by one
    duplicate per slot (a copy of the node with the slot's share of its box), wired to the slot's neighbours, to each other, to
    the original's neighbours across the split axis (first duplicate: those before it, last: those after it) and to the
    neighbours on the opposite side that still touch it - which are visited again.  Returns the new graph."""
    if thresholds is None:
        thresholds = _calc_adjacency_thresholds([dag.nodes[n]["bbox"] for n in dag.nodes])
    spec = _SPLIT[out_edge_type]
    G = dag.copy()
    queue = [head]
    n_dups = 0

    def typed(u, which, value):
        if which == "pred":
            return [p for p in G.predecessors(u) if G.edge(p, u).get(dir_key) == value]
        return [v for v in G.successors(u) if G.edge(u, v).get(dir_key) == value]

    while queue:
        u = queue.pop(0)
        if u not in G:
            continue
        outs_fwd = typed(u, "succ", out_edge_type)
        if len(outs_fwd) <= 1:
            queue.extend(outs_fwd)
            continue
        axis, (cross_fwd, cross_bwd) = spec["axis"], spec["cross"]
        outs_bwd = typed(u, *spec["back"])
        before = typed(u, "pred", cross_fwd)
        after = typed(u, "succ", cross_fwd)
        box = G.nodes[u]["bbox"]
        groups, intervals = _group_outs_by_axis_interval(G, outs_fwd, axis=axis)
        # a slot much thinner than the smallest cell is no row (column) of its own
        spans, out_groups = _assign_slots_by_intervals(box[axis], box[axis + 2], groups, intervals, min_len=thresholds["ignore"])
        if len(out_groups) <= 1:
            queue.extend(outs_fwd)
            continue
        # slots and groups were built in the same (centre) order, so pairing them cannot twist
        attrs = dict(G.nodes[u])
        dups = []
        for a, b in spans:
            n_dups += 1
            name = f"{u}__dup{n_dups}"
            G.add_node(name, **{**attrs, "bbox": (box[0], a, box[2], b) if axis == 1 else (a, box[1], b, box[3])})
            dups.append(name)
        for group, dup in zip(out_groups, dups):
            for out in group:  # twice-detected cells of one slot all meet the same duplicate
                G.add_edge(dup, out, **{dir_key: out_edge_type})
                G.add_edge(out, dup, **{dir_key: in_edge_type})
        for p in before:
            G.add_edge(dups[0], p, **{dir_key: cross_bwd})
            G.add_edge(p, dups[0], **{dir_key: cross_fwd})
        for p in after:
            G.add_edge(dups[-1], p, **{dir_key: cross_fwd})
            G.add_edge(p, dups[-1], **{dir_key: cross_bwd})
        for a, b in zip(dups, dups[1:]):
            G.add_edge(a, b, **{dir_key: cross_fwd})
            G.add_edge(b, a, **{dir_key: cross_bwd})
        for bwd in outs_bwd:
            for dup in dups:
                pair = (G.nodes[dup]["bbox"], G.nodes[bwd]["bbox"]) if spec["reverse"] else (G.nodes[bwd]["bbox"], G.nodes[dup]["bbox"])
                if _adjacent(spec["predicate"], pair[0], pair[1], thresholds):
                    G.add_edge(bwd, dup, **{dir_key: out_edge_type})
                    G.add_edge(dup, bwd, **{dir_key: in_edge_type})
                    queue.append(bwd)
        G.remove_node(u)
        queue.extend(dups)
    return G


def normalize_row_with_out_edges(dag, head, dir_key="dir", out_edge_type="R", in_edge_type="L", thresholds=None):
    """Cells with several right ("R") or left ("L") neighbours are cut along y."""
    if out_edge_type not in ("R", "L"):
        raise ValueError(f"a row is followed along 'R' or 'L' edges, got {out_edge_type!r}")
    return _normalize_with_out_edges(dag, head, dir_key, out_edge_type, in_edge_type, thresholds)


def normalize_col_with_out_edges(dag, head, dir_key="dir", out_edge_type="D", in_edge_type="U", thresholds=None):
    """Cells with several lower ("D") or upper ("U") neighbours are cut along x."""
    if out_edge_type not in ("D", "U"):
        raise ValueError(f"a column is followed along 'D' or 'U' edges, got {out_edge_type!r}")
    return _normalize_with_out_edges(dag, head, dir_key, out_edge_type, in_edge_type, thresholds)


def _components_with_isolates(dag, dir_value):
    """Components of the undirected graph of the `dir_value` edges, single nodes included."""
    return connected_components(dag.nodes, ((u, v) for u, v, d in dag.edges() if d.get("dir") == dir_value))


def _cluster_heads_by_in_degree(dag, dir_value):
    """(heads, components) of the `dir_value` chains: per component its nodes without an incoming `dir_value` edge, sorted by
    id - or, when every node has one, the smallest id."""
    comps = _components_with_isolates(dag, dir_value)
    has_incoming = {v for _, v, d in dag.edges() if d.get("dir") == dir_value}
    heads = []
    for comp in comps:
        roots = sorted(n for n in comp if n not in has_incoming)
        heads.extend(roots if roots else [min(comp)])
    return heads, comps


def _expand(dag, normalize, forward, backward, dir_key, thresholds):
    G = dag.copy()
    for out_type, in_type in ((forward, backward), (backward, forward)):
        for head in _cluster_heads_by_in_degree(G, dir_value=out_type)[0]:
            G = normalize(G, head, dir_key=dir_key, in_edge_type=in_type, out_edge_type=out_type, thresholds=thresholds)
    return G


def expand_dir_to_uit_row(dag, dir_key="dir", thresholds=None):
    """1:1 right / left neighbours: from the head of every "R" chain, then of every "L" chain."""
    return _expand(dag, normalize_row_with_out_edges, "R", "L", dir_key, thresholds)


def expand_dir_to_uit_col(dag, dir_key="dir", thresholds=None):
    """1:1 lower / upper neighbours: from the head of every "D" chain, then of every "U" chain."""
    return _expand(dag, normalize_col_with_out_edges, "D", "U", dir_key, thresholds)


def _expand_grid_to_unit(dag, thresholds=None):
    return expand_dir_to_uit_col(expand_dir_to_uit_row(dag, thresholds=thresholds), thresholds=thresholds)


def _get_grid_from_dag(dag):
    """rows x columns of node ids (None where a row and a column share no node): rows are the "R" chains from their heads, top
    to bottom; columns the "D" chains, left to right."""
    row_heads = sorted(_cluster_heads_by_in_degree(dag, dir_value="R")[0], key=lambda n: dag.nodes[n]["bbox"][1])
    col_heads = sorted(_cluster_heads_by_in_degree(dag, dir_value="D")[0], key=lambda n: dag.nodes[n]["bbox"][0])
    columns = [set(get_line_with_head(dag, head, dir_value="D")) for head in col_heads]
    grid = []
    for head in row_heads:
        row_nodes = sorted(get_line_with_head(dag, head, dir_value="R"), key=lambda n: dag.nodes[n]["bbox"][0])
        grid.append([next((n for n in row_nodes if n in column), None) for column in columns])
    return grid


def _calc_spans_and_indices_from_raw_grid(raw_data):
    """{cell id: {"row", "col" (0-based, top left), "row_span", "col_span"}} from the extent of the id in the grid."""
    extent = {}
    for r, row in enumerate(raw_data):
        for c, cell_id in enumerate(row):
            if cell_id is None:
                continue
            e = extent.setdefault(cell_id, [r, r, c, c])
            e[0], e[1], e[2], e[3] = min(e[0], r), max(e[1], r), min(e[2], c), max(e[3], c)
    return {cell_id: {"row": r0, "col": c0, "row_span": r1 - r0 + 1, "col_span": c1 - c0 + 1}
            for cell_id, (r0, r1, c0, c1) in extent.items()}


def _assign_cell_positions(cells, data):
    for cell_id, info in _calc_spans_and_indices_from_raw_grid(data).items():
        cell = cells[cell_id]
        cell.row, cell.col, cell.row_span, cell.col_span = info["row"], info["col"], info["row_span"], info["col_span"]


def _remove_dup_suffix_from_data(grid):
    return [[cell_id.split("__dup")[0] if cell_id is not None else None for cell_id in row] for row in grid]


def _by_top(ids, cells):
    """Distinct ids, top to bottom (ids at the same height keep the order given)."""
    return sorted(dict.fromkeys(ids), key=lambda h: cells[h].box[1])


def _get_col_headers_from_grid(grid, is_header_row, cells, clustered_nodes):
    """Per column the ids in its header rows, top to bottom.  Header cells of the cluster that ended up in no header row are
    ordinary cells from here on (their role is rewritten)."""
    header_rows = [row for row, flag in zip(grid, is_header_row) if flag]
    col_headers = [_by_top([row[c] for row in header_rows if row[c] is not None], cells) for c in range(len(grid[0]))]
    header_ids = {h for col in col_headers for h in col}
    in_cluster = {cell.id for cluster in clustered_nodes.values() for cell in cluster}
    for cell in cells.values():
        if cell.role == "header" and cell.id in in_cluster and cell.id not in header_ids:
            cell.role = "cell"
    return col_headers


def _get_grid_bbox(grid, cells):
    boxes = [cells[cell_id].box for row in grid for cell_id in row if cell_id is not None]
    if not boxes:
        return (0.0, 0.0, 0.0, 0.0)
    return (min(b[0] for b in boxes), min(b[1] for b in boxes), max(b[2] for b in boxes), max(b[3] for b in boxes))


def merge_cells(cell1, cell2):
    """(cell, merged?): the union of two cells (id "<id1>_<id2>", contents concatenated) - or, when the ids one of them is made
    of are all part of the other, that other cell unchanged."""
    ids1, ids2 = set(cell1.id.split("_")), set(cell2.id.split("_"))
    if ids1 <= ids2:
        return cell2, False
    if ids2 <= ids1:
        return cell1, False
    b1, b2 = cell1.box, cell2.box
    merged = type(cell1)(id=f"{cell1.id}_{cell2.id}", box=(min(b1[0], b2[0]), min(b1[1], b2[1]), max(b1[2], b2[2]), max(b1[3], b2[3])),
                         role=cell1.role, contents=(cell1.contents + cell2.contents).strip(), row=min(cell1.row, cell2.row),
                         col=min(cell1.col, cell2.col), row_span=cell1.row_span + cell2.row_span,
                         col_span=cell1.col_span + cell2.col_span)
    return merged, True


def _merge_same_column_values(grid, col_headers, cells):
    """Columns whose innermost header is the same cell become one column: per row their cells are merged.  Returns (grid,
    col_headers, the cells the new grid refers to)."""
    columns = UnionFind(len(col_headers))
    for c1 in range(len(col_headers)):
        for c2 in range(c1 + 1, len(col_headers)):
            if col_headers[c1] and col_headers[c2] and col_headers[c1][-1] == col_headers[c2][-1]:
                columns.union(c1, c2)
    groups = columns.groups()
    new_headers = [_by_top([h for c in group for h in col_headers[c]], cells) for group in groups]
    new_grid = []
    for row in grid:
        new_row = []
        for group in groups:
            ids = [row[c] for c in group if row[c] is not None]
            if not ids:
                new_row.append(None)
                continue
            merged = cells[ids[0]]
            for cid in ids[1:]:
                merged, _ = merge_cells(merged, cells[cid])
            new_row.append(merged.id)
            cells[merged.id] = merged
        new_grid.append(new_row)
    used = {cell_id for row in new_grid for cell_id in row if cell_id is not None}
    return new_grid, new_headers, {cid: cell for cid, cell in cells.items() if cid in used}


def parse_grid_from_bottom_up(cells, clustered_nodes, merge_same_column_values=False):
    """`cells`: every cell of the table by id; `clustered_nodes`: {"cell" / "empty" / "header": the cells of one grid region}.
    Returns (TableGridSchema, cells, the unit-cell graph) - `cells` with row / col / spans set, and with
    `merge_same_column_values` cut down to the (merged) cells the grid refers to - or None when no grid comes out."""
    grid_nodes = clustered_nodes["cell"] + clustered_nodes["empty"] + clustered_nodes["header"]
    thresholds = _calc_adjacency_thresholds([c.box for c in grid_nodes])  # one set for the graph and for the expansion
    dag = _expand_grid_to_unit(_get_grid_dag(clustered_nodes, thresholds=thresholds), thresholds=thresholds)
    grid = _get_grid_from_dag(dag)
    if len(grid) == 0 or len(grid[0]) == 0:
        return None
    roles = [[dag.nodes[n]["role"] if n is not None else "empty" for n in row] for row in grid]
    is_header_row = [all(role in ("header", "empty") for role in row) for row in roles]
    grid = _remove_dup_suffix_from_data(grid)
    grid_box = [int(v) for v in _get_grid_bbox(grid, cells)]
    _assign_cell_positions(cells, grid)
    col_headers = _get_col_headers_from_grid(grid, is_header_row, cells, clustered_nodes)
    if merge_same_column_values:
        grid, col_headers, cells = _merge_same_column_values(grid, col_headers, cells)
    schema = TableGridSchema(id=None, n_row=len(grid), n_col=len(grid[0]) if grid else 0, box=grid_box, data=grid, col_headers=col_headers)
    return schema, cells, dag
