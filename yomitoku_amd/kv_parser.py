"""Key-value items from the cells a grid did not claim (reference kv_parser.py:13-626).

Headers (keys) and cells (values) are assigned to the kv regions the cell detector predicted; inside a region neighbouring
nodes are linked ("R"/"L", "D"/"U"), and per connected cluster the key chains are read off by a depth-first walk from the
root headers - along "R" or along "D", whichever reaches more values.  Three rescues then pick up what the regions missed:
a header outside every region that encloses key headers is put in front of their keys; an orphan header followed by orphan
cells becomes a key chain of its own; an unkeyed cell that continues a keyed value to the right or below inherits its key.
What is still unkeyed becomes an item with an empty key.

Where the reference walks a Python set of node ids (the members of a cluster) the order here is the graph's node order:
headers, cells, empties, each in the order given.
"""

from __future__ import annotations

from .geometry import calc_overlap_ratio, is_bottom_adjacent, is_contained, is_right_adjacent, overlap_interval
from .table_semantic_schemas import KvItemSchema
from .utils.graph import OrderedDiGraph

NESTED_CONTAINMENT_TH = 0.8  # share of a key header's interval inside an orphan header's from which it counts as nested


def _assign_cells_to_regions(nodes, regions):
    """({cell id: region id}, {header id: set of region ids}).  A value cell (cell / empty) belongs to the ONE region that covers
    most of it (first among equals); a header may be a row header over several rows and belongs to EVERY region that holds more
    than 20 % of it.  Nodes in no region are left out: they get no edges."""
    cell_to_region, header_to_regions = {}, {}
    if len(regions) == 0:
        return cell_to_region, header_to_regions
    for cell in nodes["cell"] + nodes["empty"]:
        best_id, best_ratio = None, 0.0
        for region in regions:
            if is_contained(region.box, cell.box, threshold=0.2):
                ratio = calc_overlap_ratio(cell.box, region.box)[0]
                if ratio > best_ratio:
                    best_id, best_ratio = region.id, ratio
        if best_id is not None:
            cell_to_region[cell.id] = best_id
    for header in nodes["header"]:
        inside = {region.id for region in regions if is_contained(region.box, header.box, threshold=0.2)}
        if inside:
            header_to_regions[header.id] = inside
    return cell_to_region, header_to_regions


def _attach_left_adjacent_orphan_headers(nodes, header_to_regions):
    """A header in no region takes over the regions of ALL region headers that are its right-hand neighbours: the leading key
    a region box cut off, or a row header spanning several rows (regions), which has to reach the children of each.  Repeated
    until nothing changes, so orphan -> orphan -> region header chains resolve, and recomputed from scratch every pass, so that
    regions a neighbour gains later are picked up.  Headers that were assigned directly keep exactly their regions."""
    headers = nodes["header"]
    orphans = {h.id for h in headers if not header_to_regions.get(h.id)}
    changed = True
    while changed:
        changed = False
        for orphan in headers:
            if orphan.id not in orphans:
                continue
            gathered = set(header_to_regions.get(orphan.id, set()))
            for other in headers:
                if other.id == orphan.id or not header_to_regions.get(other.id):
                    continue
                if is_right_adjacent(orphan.box, other.box):
                    gathered |= header_to_regions[other.id]
            if gathered and gathered != header_to_regions.get(orphan.id):
                header_to_regions[orphan.id] = gathered
                changed = True
    return header_to_regions


def _link(dag, parent, child):
    """Edges for `child` being the right and / or lower neighbour of `parent`."""
    if is_right_adjacent(parent.box, child.box):
        dag.add_edge(parent.id, child.id, dir="R")
        dag.add_edge(child.id, parent.id, dir="L")
    if is_bottom_adjacent(parent.box, child.box):
        dag.add_edge(parent.id, child.id, dir="D")
        dag.add_edge(child.id, parent.id, dir="U")


def _calc_adjacent_header_to_cell(dag, cell_to_region, header_to_regions, headers, cells):
    for header in headers:
        regions = header_to_regions.get(header.id)
        if not regions:
            continue
        for cell in cells:
            region = cell_to_region.get(cell.id)
            if region is not None and region in regions:
                _link(dag, header, cell)


def _calc_adjacent_header_to_header(dag, header_to_regions, nodes):
    """Headers that share at least one region."""
    for node in nodes:
        for parent in nodes:
            if node.id == parent.id:
                continue
            a, b = header_to_regions.get(parent.id), header_to_regions.get(node.id)
            if a and b and a & b:
                _link(dag, parent, node)


def _calc_adjacent_cell_to_cell(dag, cell_to_region, nodes):
    for node in nodes:
        region = cell_to_region.get(node.id)
        if region is None:
            continue
        for parent in nodes:
            if node.id != parent.id and cell_to_region.get(parent.id) == region:
                _link(dag, parent, node)


def get_kv_items_dag(nodes, regions):
    """(graph, cell_to_region, header_to_regions); the assignments are handed on for the orphan rescues."""
    cell_to_region, header_to_regions = _assign_cells_to_regions(nodes, regions)
    header_to_regions = _attach_left_adjacent_orphan_headers(nodes, header_to_regions)
    dag = OrderedDiGraph()
    for node in nodes["header"] + nodes["cell"] + nodes["empty"]:
        dag.add_node(node.id, id=node.id, bbox=node.box, role=node.role, contents=node.contents)
    _calc_adjacent_header_to_cell(dag, cell_to_region, header_to_regions, nodes["header"], nodes["cell"])
    _calc_adjacent_header_to_cell(dag, cell_to_region, header_to_regions, nodes["header"], nodes["empty"])
    _calc_adjacent_header_to_header(dag, header_to_regions, nodes["header"])
    _calc_adjacent_cell_to_cell(dag, cell_to_region, nodes["cell"])
    return dag, cell_to_region, header_to_regions


def _merge_bbox(box1, box2):
    return [min(box1[0], box2[0]), min(box1[1], box2[1]), max(box1[2], box2[2]), max(box1[3], box2[3])]


def _find_root_headers(dag, direction, node_set=None):
    """The headers (of `node_set`, in the graph's node order) that no other header of the set points at along `direction`."""
    members = list(dag.nodes) if node_set is None else [n for n in dag.nodes if n in node_set]
    inside = set(members)
    roots = []
    for h in members:
        if dag.nodes[h]["role"] != "header":
            continue
        if not any(u in inside and dag.nodes[u]["role"] == "header" and dag.edge(u, h).get("dir") == direction
                   for u in dag.predecessors(h)):
            roots.append(h)
    return roots


def _dfs_collect_kv(dag, node_id, key_path, kv_items, cells, kv_cells, allowed_dir):
    """Depth first along `allowed_dir` from a root header; reaching a cell / empty node emits KvItem(key path, node)."""
    if dag.nodes[node_id]["role"] in ("cell", "empty"):
        keys = list(key_path)
        box = _merge_bbox(cells[node_id].box, cells[keys[0]].box) if keys else cells[node_id].box
        kv_items.append(KvItemSchema(id=None, key=keys, value=node_id, box=box))
        kv_cells[node_id] = cells[node_id]
        for k in keys:
            kv_cells[k] = cells[k]
        return
    path = key_path + [node_id]
    for v in dag.successors(node_id):
        if v not in path and dag.edge(node_id, v).get("dir") == allowed_dir:
            _dfs_collect_kv(dag, v, path, kv_items, cells, kv_cells, allowed_dir)


def _nested_ratio(parent_lo, parent_hi, child_lo, child_hi):
    """Share (0 .. 1) of the child interval that lies inside the parent interval."""
    length = child_hi - child_lo
    if length <= 0:
        return 0.0
    return overlap_interval(parent_lo, parent_hi, child_lo, child_hi) / length


def _rescue_nested_orphan_headers(orphan_headers, kv_items, cells, kv_cells):
    """An orphan header that encloses headers already used as the FIRST key of items is put in front of those items' keys.
    "Encloses": the key header's interval lies (80 %) inside the orphan's and is clearly smaller - a header of the same size
    next to it is a sibling heading, not a child.
      sideways: every key header to the right whose y interval is enclosed (a row header over several rows);
      downwards: of the key headers whose x interval is enclosed, the ones directly below the orphan and everything that
      continues them downwards (a heading over several columns and rows)."""
    for orphan in orphan_headers:
        ox1, oy1, ox2, oy2 = orphan.box
        width, height = ox2 - ox1, oy2 - oy1
        heads = {}
        for kv in kv_items:
            head = cells.get(kv.key[0]) if kv.key else None
            if head is not None and head.id != orphan.id:
                heads[head.id] = head
        targets = set()
        for head in heads.values():
            hx1, hy1, hx2, hy2 = head.box
            if hx1 >= ox2 - width * 0.1 and (hy2 - hy1) < height * 0.9 and _nested_ratio(oy1, oy2, hy1, hy2) >= NESTED_CONTAINMENT_TH:
                targets.add(head.id)
        below = [head for head in heads.values()
                 if (head.box[2] - head.box[0]) < width * 0.9 and _nested_ratio(ox1, ox2, head.box[0], head.box[2]) >= NESTED_CONTAINMENT_TH]
        frontier = [head for head in below if is_bottom_adjacent(orphan.box, head.box)]
        linked = {head.id for head in frontier}
        while frontier:
            current = frontier.pop()
            for head in below:
                if head.id not in linked and is_bottom_adjacent(current.box, head.box):
                    linked.add(head.id)
                    frontier.append(head)
        targets |= linked
        if not targets:
            continue
        for kv in kv_items:
            if kv.key and kv.key[0] in targets:
                kv.key = [orphan.id] + list(kv.key)
                kv.box = _merge_bbox(kv.box, orphan.box) if kv.box else list(orphan.box)
        kv_cells[orphan.id] = cells[orphan.id]


def _rescue_orphan_header_cell_pairs(orphan_headers, orphan_cells, kv_items, cells, kv_cells):
    """From every orphan header, to the right and then downwards: follow neighbouring orphan cells depth first; the cell a chain
    ends in is the value, the cells on the way are part of the key (status -> kind of pension -> amount field gives
    key [status, kind of pension], value amount field).  Returns (cells used as values, cells used as keys)."""
    paired_values, used_as_keys = set(), set()
    for orphan in orphan_headers:
        for is_adjacent in (is_right_adjacent, is_bottom_adjacent):
            seen = set()

            def chain(node, key_path):
                children = [c for c in orphan_cells
                            if c.id not in seen and c.id not in paired_values and c.id not in used_as_keys and is_adjacent(node.box, c.box)]
                if not children:
                    if node.id == orphan.id:
                        return
                    kv_items.append(KvItemSchema(id=None, key=list(key_path), value=node.id, box=_merge_bbox(cells[key_path[0]].box, node.box)))
                    for key_id in key_path:
                        kv_cells[key_id] = cells[key_id]
                    kv_cells[node.id] = cells[node.id]
                    paired_values.add(node.id)
                    used_as_keys.update(key_path[1:])
                    return
                seen.update(c.id for c in children)
                for child in children:
                    chain(child, key_path + [node.id])

            chain(orphan, [])
    return paired_values, used_as_keys


def _rescue_orphan_cells_extending_values(kv_items, orphan_cells, cells, kv_cells):
    """An unkeyed cell whose left (preferred) or upper neighbour is a keyed value cell of the same row height (column width:
    the intervals across the contact enclose each other to 80 %) is a continuation of that value - a second line of an entry
    field - and gets an item with the same key; such cells chain.  Full-width note cells and thin gap cells do not match in
    size and are left alone.  Returns the ids that inherited a key."""
    inherited = set()
    value_to_key = {kv.value: list(kv.key) for kv in kv_items if kv.key}  # grows as cells inherit
    directions = ((is_right_adjacent, 1, 3), (is_bottom_adjacent, 0, 2))
    remaining = {c.id: c for c in orphan_cells}

    def same_extent(a, b, lo, hi):
        return (_nested_ratio(a[lo], a[hi], b[lo], b[hi]) >= NESTED_CONTAINMENT_TH
                and _nested_ratio(b[lo], b[hi], a[lo], a[hi]) >= NESTED_CONTAINMENT_TH)

    def key_for(cell):
        for is_adjacent, lo, hi in directions:
            for value_id, value_key in value_to_key.items():
                value_cell = cells.get(value_id)
                if value_cell is not None and is_adjacent(value_cell.box, cell.box) and same_extent(value_cell.box, cell.box, lo, hi):
                    return value_key
        return None

    changed = True
    while changed:
        changed = False
        for cell in list(remaining.values()):
            key = key_for(cell)
            if key is None:
                continue
            kv_items.append(KvItemSchema(id=None, key=list(key), value=cell.id, box=_merge_bbox(cells[key[0]].box, cell.box)))
            kv_cells[cell.id] = cells[cell.id]
            for key_id in key:
                kv_cells[key_id] = cells[key_id]
            value_to_key[cell.id] = list(key)
            inherited.add(cell.id)
            del remaining[cell.id]
            changed = True
    return inherited


def parse_kv_items(nodes, cells, regions):
    """`nodes`: {"header" / "cell" / "empty": cells not claimed by a grid}; `cells`: every cell of the table by id; `regions`:
    the kv regions (with ids).  Returns (kv items, the adjacency graph with the losing direction's edges removed per cluster,
    {id: cell} of every cell an item refers to)."""
    dag, cell_to_region, header_to_regions = get_kv_items_dag(nodes, regions)
    kv_items, kv_cells = [], {}
    for component in dag.weakly_connected_components():
        members = set(component)
        found = {}
        for direction in ("R", "D"):
            items, used = [], {}
            for root in _find_root_headers(dag, direction, members):
                _dfs_collect_kv(dag, root, [], items, cells, used, direction)
            found[direction] = (items, used, len({kv.value for kv in items}))
        # the direction that reaches more values wins, horizontal among equals; the other one's edges leave the cluster
        winner, dropped = ("D", ("R", "L")) if found["D"][2] > found["R"][2] else ("R", ("D", "U"))
        kv_items.extend(found[winner][0])
        kv_cells.update(found[winner][1])
        dag.remove_edges([(u, v) for u, v, d in dag.edges() if u in members and v in members and d.get("dir") in dropped])

    # ---- fallbacks for what the regions did not reach
    orphan_headers = sorted((h for h in nodes["header"] if not header_to_regions.get(h.id)), key=lambda h: (h.box[1], h.box[0]))
    _rescue_nested_orphan_headers(orphan_headers, kv_items, cells, kv_cells)

    visited = {kv.value for kv in kv_items}
    orphan_cells = [c for c in nodes["cell"] + nodes["empty"] if c.id not in cell_to_region and c.id not in visited]
    paired, used_as_keys = _rescue_orphan_header_cell_pairs(orphan_headers, orphan_cells, kv_items, cells, kv_cells)
    visited |= paired | used_as_keys  # a cell that became part of a key is no keyless value either

    # not only cells outside the regions: also cells inside one that the walk did not reach
    unkeyed = [c for c in nodes["cell"] + nodes["empty"] if c.id not in visited]
    visited |= _rescue_orphan_cells_extending_values(kv_items, unkeyed, cells, kv_cells)

    for cell in nodes["cell"] + nodes["empty"]:
        if cell.id not in visited:
            kv_items.append(KvItemSchema(id=None, key=[], value=cell.id, box=cell.box))
            kv_cells[cell.id] = cells[cell.id]
    return kv_items, dag, kv_cells
