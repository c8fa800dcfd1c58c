"""Workspace footprint of the four nets at the shapes `DocumentAnalyzer.serve` reserves, bump arena vs planned workspace
("workspace_reuse", include/ymk.h): bump bytes, planned bytes, the live bound no plan can beat, and the two ratios.

    python tools/workspace_report.py [out.json]

Only reservations are made (ymk_model_reserve plans the bound shape on the host and sizes the slab): no forward runs."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yomitoku_amd import _lib  # noqa: E402


def measure(name, net, bound):
    net.set_workspace_reuse(True)
    net.reserve(*bound)
    plan, bump, live = (_lib.stat(k) for k in ("ws_plan_bytes_last", "ws_bump_bytes_last", "ws_live_bound_last"))
    rec = {
        "net": name, "reserve_n_h_w": list(bound), "bump_bytes": bump, "planned_bytes": plan, "live_bound_bytes": live,
        "slab_held_bytes": net.workspace_bytes, "planned_over_live_bound": round(plan / live, 4), "planned_over_bump": round(plan / bump, 4),
    }
    print(json.dumps(rec), flush=True)
    net.close()
    return rec


def main():
    from yomitoku_amd.layout_parser import LayoutParser
    from yomitoku_amd.table_cell_detector import CellDetector
    from yomitoku_amd.table_structure_recognizer import TableStructureRecognizer
    from yomitoku_amd.text_detector import TextDetector
    from yomitoku_amd.text_recognizer import TextRecognizer

    dev = "cuda:0"
    out = []
    det = TextDetector(from_pretrained=False, device=dev)
    cfg = det._cfg.data
    long_side = max(32, int(cfg.limit_size) // 32 * 32)
    short_side = max(32, min(int(cfg.shortest_size), int(cfg.limit_size)) // 32 * 32)
    out.append(measure("dbnet (text detector)", det.model, (det.MAX_PAGES_PER_FORWARD, long_side, short_side)))
    lay = LayoutParser(from_pretrained=False, device=dev)
    out.append(measure("rtdetr (layout parser)", lay.model, (lay.MAX_PAGES_PER_FORWARD, 640, 640)))
    tab = TableStructureRecognizer(from_pretrained=False, device=dev)
    out.append(measure("rtdetr (table structure, 64 crops)", tab.model, (tab.MAX_TABLES_PER_FORWARD, 640, 640)))
    cell = CellDetector(from_pretrained=False, device=dev)
    out.append(measure("rtdetr (table cells, 960 x 960)", cell.model, (cell.MAX_TABLES_PER_FORWARD, 960, 960)))
    rec = TextRecognizer(model_name="parseq-tiny-dynw-v4", from_pretrained=False, device=dev, dynamic_width=True, batch_bucketing=True)
    out.append(measure("parseq-tiny-dynw (a wave's lines)", rec.model, rec._reserve_bounds()))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump({"per_net": out}, f, indent=1)


if __name__ == "__main__":
    main()
