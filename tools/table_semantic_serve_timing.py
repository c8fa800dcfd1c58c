#!/usr/bin/env python3
"""Pages per second of the table-semantic parser over a job of form-like pages, for profiles/table_semantic_serve.json.

    python tools/table_semantic_serve_timing.py --parse-pages [--repeats 3] [--out FILE --key NAME]
    python tools/table_semantic_serve_timing.py --serve [--repeats 3] [--out FILE --key NAME]

64 synthetic 1600 x 1200 pages (`synthetic_page_with_truth`, seeds 0..63), seeded weights.  Seeded weights detect noise, so every
page's TRUE tables are put in at `handover.tables`: the cell detector sees real table crops, 1-2 per page.  Either leg runs one
warm-up job over all pages (every shape, workspace and pinned buffer of the timed jobs exists afterwards), then `--repeats` timed
jobs, each a host clock around a job that ends in a device synchronise.

  --parse-pages   `parse_pages(imgs, wave=8)`: the lock-step loop.  Uses nothing but `TableSemanticParser`, `parse_pages` and the
                  hand-over, so the same file measures an older commit's baseline.
  --serve         `serve(imgs)`: the page pipeline; the last timed job is traced (`pipe.trace`) and reported as busy time per
                  stage and wave - the stage with the largest busy share bounds the job.

`--out FILE --key NAME` stores the leg's JSON object under NAME in FILE (other keys are kept); it is always printed."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAGES, HEIGHT, WIDTH = 64, 1600, 1200


class TrueTables:
    """The hand-over of both legs.  `serve` and `parse_pages` show a page under its position in the job (`parse_pages` of older
    commits: in the wave), one call per page in page order - for `parse_pages` the calls are counted, which holds for both."""

    def __init__(self, boxes_per_page, by_call_order):
        self.boxes, self.by_call_order, self.calls = boxes_per_page, by_call_order, 0

    def tables(self, k, tables):
        from yomitoku_amd.schemas import Element

        if self.by_call_order:
            k, self.calls = self.calls % len(self.boxes), self.calls + 1
        return [Element(id=None, box=[int(v) for v in b], score=1.0, role=None, contents=None) for b in self.boxes[k]]


def build(by_call_order):
    from yomitoku_amd import TableSemanticParser
    from yomitoku_amd.utils.synth import dbnet_state_dict, parseq_state_dict, synthetic_page_with_truth
    from yomitoku_amd.utils.synth_rtdetr import rtdetr_state_dict

    configs = {"table_detector": {"from_pretrained": False}, "table_cell_parser": {"from_pretrained": False},
               "text_detector": {"from_pretrained": False},
               "text_recognizer": {"model_name": "parseq-tiny-dynw-v4", "from_pretrained": False, "dynamic_width": True, "batch_bucketing": True}}
    p = TableSemanticParser(configs=configs, device="cuda:0")
    p.text_detector.model.load_state_dict(dbnet_state_dict(8, out_bias=-1.5))
    p.text_recognizer.model.load_state_dict(parseq_state_dict(1235, eos_bias=6.0))
    p.layout_parser.model.load_state_dict(rtdetr_state_dict(1240, num_classes=6, score_bias=-2.0))
    p.cell_detector.model.load_state_dict(rtdetr_state_dict(1243, num_classes=6, eval_size=(960, 960), enc_score_gain=12.0, score_bias=-3.0,
                                                            score_gain=2.0))
    truth = [synthetic_page_with_truth(seed, HEIGHT, WIDTH) for seed in range(PAGES)]
    p.handover = TrueTables([t[2] for t in truth], by_call_order)
    return p, [t[0] for t in truth]


def timed_jobs(job, repeats):
    import torch

    job()  # warm-up
    torch.cuda.synchronize()
    rates, last = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        last = job()
        torch.cuda.synchronize()
        rates.append(round(PAGES / (time.perf_counter() - t0), 3))
    return rates, last


def units(results):
    ok = [r for r in results if not isinstance(r, BaseException)]
    n = max(1, len(ok))
    return {"failed_pages": len(results) - len(ok), "words_per_page": round(sum(len(r.words) for r in ok) / n, 1),
            "tables_per_page": round(sum(len(r.tables) for r in ok) / n, 2),
            "cells_per_page": round(sum(len(t.cells) for r in ok for t in r.tables) / n, 1)}


def stage_table(trace):
    """Per stage: busy seconds over the job, mean busy milliseconds per wave, and the share of the job's wall time."""
    t0 = min(a for _, _, _, a, _ in trace)
    wall = max(b for _, _, _, _, b in trace) - t0
    stages = {}
    for name, _, _, a, b in trace:
        stages.setdefault(name, []).append(b - a)
    return {"traced_wall_s": round(wall, 3),
            "stages": {name: {"waves": len(d), "busy_s": round(sum(d), 3), "mean_ms_per_wave": round(1e3 * sum(d) / len(d), 2),
                              "max_ms": round(1e3 * max(d), 2), "busy_frac": round(sum(d) / wall, 3)} for name, d in stages.items()}}


def main():
    ap = argparse.ArgumentParser()
    leg = ap.add_mutually_exclusive_group(required=True)
    leg.add_argument("--parse-pages", action="store_true")
    leg.add_argument("--serve", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--key")
    args = ap.parse_args()
    import torch

    parser, imgs = build(by_call_order=args.parse_pages)
    result = {"pages": PAGES, "page": [HEIGHT, WIDTH], "weights": "seeded (synthetic); the pages' true tables handed over", "repeats": args.repeats,
              "device": torch.cuda.get_device_name(0)}
    if args.parse_pages:
        rates, last = timed_jobs(lambda: parser.parse_pages(imgs, wave=8), args.repeats)
        result.update(leg="parse_pages(imgs, wave=8)", pages_per_s=rates, **units(last))
    else:
        state = {"jobs": 0}

        def job():
            state["jobs"] += 1
            if state["jobs"] == args.repeats + 1:  # the last timed job leaves its trace
                parser._pipeline.trace = []
            return parser.serve(imgs)

        rates, last = timed_jobs(job, args.repeats)
        pipe = parser._pipeline
        trace, pipe.trace = pipe.trace, None
        result.update(leg="serve(imgs)", wave=pipe.wave, in_flight=pipe.in_flight, pages_per_s=rates, **units(last), **stage_table(trace))
    parser.close()
    print(json.dumps(result, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        merged = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                merged = json.load(f)
        merged[args.key or result["leg"]] = result
        with open(args.out, "w") as f:
            f.write(json.dumps(merged, indent=1) + "\n")


if __name__ == "__main__":
    main()
