"""The host half of the cell detector as the page pipeline uses it (CellDetector.tables_from_raw), without a device: raw
arrays built here, page attribution and order against `postprocess` applied crop by crop the way `__call__` applies it."""
import numpy as np

Q, C = 8, 6  # queries, classes: table, cell, header, empty, kv_item, grid
CATEGORY = ["table", "cell", "header", "empty", "kv_item", "grid"]


def _detector():
    """A CellDetector made without a device: what `postprocess` reads."""
    from yomitoku_amd.layout_parser import RTDETRPostProcessor
    from yomitoku_amd.table_cell_detector import CellDetector

    cd = CellDetector.__new__(CellDetector)
    cd.postprocessor = RTDETRPostProcessor(num_classes=C, num_top_queries=Q)
    cd.thresh_score = 0.5
    cd.label_mapper = dict(enumerate(CATEGORY))
    cd.visualize = False
    return cd


def _raw(detections):
    """logits 1 x Q x C (every score ~ 0 but the given ones) and boxes 1 x Q x 4 (cx, cy, w, h, relative to the crop)."""
    logits = np.full((1, Q, C), -10.0, dtype=np.float32)
    boxes = np.tile(np.array([0.5, 0.5, 0.01, 0.01], dtype=np.float32), (1, Q, 1))
    for q, (category, box) in enumerate(detections):
        logits[0, q, CATEGORY.index(category)] = 5.0 - 0.25 * q
        boxes[0, q] = box
    return logits, boxes


def _element(box):
    from yomitoku_amd.schemas import Element

    return Element(id=None, box=list(box), score=1.0, role=None, contents=None)


def _cases():
    """(page, table box, detections): pages 0 and 2 have tables, page 1 has none."""
    grid = [("cell", [0.25, 0.25, 0.4, 0.4]), ("cell", [0.75, 0.25, 0.4, 0.4]), ("header", [0.25, 0.75, 0.4, 0.4]),
            ("empty", [0.75, 0.75, 0.4, 0.4]), ("grid", [0.5, 0.5, 0.95, 0.95]), ("kv_item", [0.5, 0.25, 0.9, 0.45])]
    return [
        (0, [30, 40, 330, 240], grid),
        # its only cell coincides with the crop and is filtered: the table falls back to one cell, its own box
        (0, [350, 250, 550, 550], [("cell", [0.5, 0.5, 1.0, 1.0])]),
        # nothing detected and the fall-back cell (8 x 8) is noise: the table keeps no cell and is dropped
        (2, [5, 5, 13, 13], []),
        (2, [100, 300, 500, 420], [("cell", [0.3, 0.5, 0.5, 0.8]), ("cell", [0.3, 0.5, 0.3, 0.5]), ("header", [0.8, 0.5, 0.3, 0.8])]),
        (0, [20, 600, 220, 800], grid[:2]),  # raw entries need not come page by page: order within a page is entry order
    ]


def test_tables_from_raw_equals_per_crop_postprocess():
    from yomitoku_amd.schemas import TableDetectorSchema

    cd = _detector()
    raw, want = [], [[], [], []]
    for page, box, detections in _cases():
        logits, boxes = _raw(detections)
        x1, y1, x2, y2 = box
        data = {"size": (y2 - y1, x2 - x1), "offset": (x1, y1)}
        raw.append((page, _element(box), logits, boxes, data))
        table = _element(box)
        cells, kv_regions, grid_regions = cd.postprocess({"pred_logits": logits.copy(), "pred_boxes": boxes.copy()}, dict(data), table.box)
        if len(cells) == 0:
            continue
        want[page].append(TableDetectorSchema(id=None, box=table.box, role=table.role, cells=cells, kv_regions=kv_regions, grid_regions=grid_regions))
    got = cd.tables_from_raw(raw, 3)
    assert [len(p) for p in got] == [3, 0, 1] and [len(p) for p in want] == [3, 0, 1]
    assert [[t.model_dump() for t in p] for p in got] == [[t.model_dump() for t in p] for p in want]
    # the cases are what their comments say
    first, fallback, last = got[0]
    assert len(first.cells) >= 4 and len(first.grid_regions) == 1 and len(first.kv_regions) == 1
    assert [c.box for c in fallback.cells] == [[350, 250, 550, 550]] and fallback.cells[0].role == "cell"
    assert first.box == [30, 40, 330, 240] and last.box == [20, 600, 220, 800]
    assert got[2][0].box == [100, 300, 500, 420] and len(got[2][0].cells) == 2  # the cell inside another is kept, the outer one goes
    assert cd.tables_from_raw([], 2) == [[], []]


# ---------------------------------------------------------------------------------------------------------------------
# filter_contained_rectangles_with_category on one containment matrix per category: the keep flags of the pair loop it
# replaced do not depend on the visiting order, so the matrix form must return the same flags - nested boxes, boxes that
# contain each other (with different and with equal areas) and degenerate boxes included.
def _pair_loop(category_elements, ignore_categories=()):
    """The pair loop the filter was before it was vectorised, kept here as the reference."""
    from yomitoku_amd.geometry import filter_by_flag, is_contained

    for category, elements in category_elements.items():
        if category in ignore_categories:
            continue
        boxes = [e["box"] for e in elements]
        keep = [True] * len(boxes)
        for i, box_i in enumerate(boxes):
            for j in range(i + 1, len(boxes)):
                box_j = boxes[j]
                ij = is_contained(box_i, box_j)
                ji = is_contained(box_j, box_i)
                if ij and ji:
                    area_i = (box_i[2] - box_i[0]) * (box_i[3] - box_i[1])
                    area_j = (box_j[2] - box_j[0]) * (box_j[3] - box_j[1])
                    if area_i > area_j:
                        keep[j] = False
                    else:
                        keep[i] = False
                elif ij:
                    keep[i] = False
                elif ji:
                    keep[j] = False
        category_elements[category] = filter_by_flag(elements, keep)
    return category_elements


def _outcome(fn, elements):
    try:
        return fn({k: [dict(e) for e in v] for k, v in elements.items()}, ignore_categories=["grid"])
    except ZeroDivisionError:
        return "ZeroDivisionError"


def _box_sets(n_sets=300, seed=0):
    """Seeded random integer box sets, each with planted relatives of one of its boxes: one nested in it, one that contains it
    and is contained by it with a smaller area, and a copy (mutual containment, equal areas), put in at random positions."""
    rng = np.random.default_rng(seed)
    for _ in range(n_sets):
        n = int(rng.integers(1, 40))
        xy, wh = rng.integers(0, 300, size=(n, 2)), rng.integers(10, 120, size=(n, 2))
        boxes = np.concatenate([xy, xy + wh], axis=1).tolist()
        x1, y1, x2, y2 = boxes[int(rng.integers(n))]
        for planted in ([x1, y1, x1 + (x2 - x1) // 3, y1 + (y2 - y1) // 3], [x1 + 1, y1, x2, y2], [x1, y1, x2, y2]):
            boxes.insert(int(rng.integers(len(boxes) + 1)), planted)
        yield boxes


def test_vectorised_within_category_filter_equals_the_pair_loop():
    from yomitoku_amd.geometry import is_contained
    from yomitoku_amd.table_cell_detector import filter_contained_rectangles_with_category as vectorised

    seen = {"nested": 0, "mutual": 0, "equal areas": 0, "dropped": 0}
    for boxes in _box_sets():
        for i, a in enumerate(boxes):  # each planted kind occurs in what is compared
            for b in boxes[i + 1:]:
                ab, ba = is_contained(a, b), is_contained(b, a)
                seen["nested"] += ab != ba
                seen["mutual"] += ab and ba
                seen["equal areas"] += ab and ba and (a[2] - a[0]) * (a[3] - a[1]) == (b[2] - b[0]) * (b[3] - b[1])
        half = len(boxes) // 2
        elements = {"cell": [{"box": b, "score": 0.9, "role": "cell"} for b in boxes[:half]],
                    "header": [{"box": b, "score": 0.8, "role": "header"} for b in boxes[half:]],
                    "grid": [{"box": b, "score": 0.7, "role": "grid"} for b in boxes], "empty": []}
        want, got = _outcome(_pair_loop, elements), _outcome(vectorised, elements)
        assert got == want
        assert got["grid"] == elements["grid"]  # an ignored category is left alone
        seen["dropped"] += len(boxes) - len(got["cell"]) - len(got["header"])
    assert all(seen.values()), seen
    # whole sets at once: every kind in ONE category, and float boxes (the quotient is float64 on both sides)
    for boxes in _box_sets(40, seed=1):
        for scale in (1, 0.37):
            elements = {"cell": [{"box": [v * scale for v in b], "role": "cell"} for b in boxes]}
            assert _outcome(vectorised, elements) == _outcome(_pair_loop, elements)


def test_vectorised_filter_and_pair_loop_agree_on_degenerate_boxes():
    """Zero-width, zero-height, zero-area and inverted boxes among ordinary ones.  `is_contained` divides by the raw area of
    the inner box, but only after it has found an intersection of positive integer extent, and such an intersection lies inside
    a box whose truncated - hence raw - width and height are positive: a degenerate box cannot make either form divide by zero.
    So the two forms must agree on the OUTCOME, whichever it is: the same flags, or the same ZeroDivisionError."""
    from yomitoku_amd.table_cell_detector import filter_contained_rectangles_with_category as vectorised

    ordinary = [[0, 0, 100, 100], [10, 10, 60, 60], [10, 10, 60, 61], [200, 50, 260, 90]]
    degenerate = [[20, 20, 20, 50], [20, 20, 50, 20], [30, 30, 30, 30], [50, 50, 40, 40], [0, 0, 100, 0], [0.2, 0.2, 0.8, 0.8],
                  [5.5, 5, 5.5, 40]]
    for k in range(len(degenerate) + 1):
        for boxes in (ordinary[:2] + degenerate[:k] + ordinary[2:], degenerate[:k][::-1] + ordinary, degenerate[:k]):
            elements = {"cell": [{"box": list(b), "role": "cell"} for b in boxes]}
            assert _outcome(vectorised, elements) == _outcome(_pair_loop, elements)
