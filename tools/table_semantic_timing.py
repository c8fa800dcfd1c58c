#!/usr/bin/env python3
"""What a TableSemanticParser page costs, for profiles/table_semantic_host_ms.json.

    python tools/table_semantic_timing.py host [--out FILE]    the semantic stage alone (everything after the four networks) on the
                                                               largest recorded case, no GPU: median of 20 runs after 3 warm-ups
    python tools/table_semantic_timing.py gpu [--out FILE]     wall time of one __call__ and of parse_pages over 16 copies of
                                                               tests/golden/test_page.jpg, seeded weights, on the GPU

Each writes one JSON object (to --out, or standard output); the profile file holds them under "product" and "gpu", next to the
"reference" entry that tools/record_table_semantic_golden.py measured."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host():
    from yomitoku_amd.schemas import OCRSchema, TableDetectorSchema
    from yomitoku_amd.table_semantic_parser import TableSemanticParser

    import gzip

    with gzip.open(os.path.join(ROOT, "tests", "golden", "table_semantic", "inputs", "case_05.json.gz"), "rt", encoding="utf-8") as f:
        case = json.load(f)
    parser = TableSemanticParser.__new__(TableSemanticParser)
    times = []
    for _ in range(23):
        t0 = time.perf_counter()  # input validation included, as in the reference's figure
        tables = [TableDetectorSchema.model_validate(t) for t in copy.deepcopy(case["tables"])]
        parser.semantic_stage(OCRSchema(words=copy.deepcopy(case["words"])), tables, [])
        times.append((time.perf_counter() - t0) * 1e3)
    return {"case": 5, "cells": sum(len(t["cells"]) for t in case["tables"]), "words": len(case["words"]),
            "median_ms": round(statistics.median(times[3:]), 2), "runs": 20, "warmup": 3,
            "what": "TableSemanticParser.semantic_stage (schema validation of the inputs included), one CPU core"}


def gpu():
    import torch

    from yomitoku_amd import TableSemanticParser
    from yomitoku_amd.data.functions import load_image
    from yomitoku_amd.schemas import Element
    from yomitoku_amd.utils.synth import dbnet_state_dict, parseq_state_dict
    from yomitoku_amd.utils.synth_rtdetr import rtdetr_state_dict

    (img,) = load_image(os.path.join(ROOT, "tests", "golden", "test_page.jpg"))
    configs = {"table_detector": {"from_pretrained": False}, "table_cell_parser": {"from_pretrained": False},
               "text_detector": {"from_pretrained": False},
               "text_recognizer": {"model_name": "parseq-tiny-dynw-v4", "from_pretrained": False, "dynamic_width": True, "batch_bucketing": True}}
    p = TableSemanticParser(configs=configs, device="cuda:0")
    p.text_detector.model.load_state_dict(dbnet_state_dict(8, out_bias=-1.5))
    p.text_recognizer.model.load_state_dict(parseq_state_dict(1235, eos_bias=6.0))
    p.layout_parser.model.load_state_dict(rtdetr_state_dict(1240, num_classes=6, score_bias=-2.0))
    p.cell_detector.model.load_state_dict(rtdetr_state_dict(1243, num_classes=6, eval_size=(960, 960), enc_score_gain=12.0, score_bias=-3.0,
                                                            score_gain=2.0))

    class TwoTables:  # seeded weights find no tables: two fixed crops keep the cell detector at work
        def tables(self, k, tables):
            return [Element(id=None, box=b, score=1.0, role=None, contents=None) for b in ([30, 40, 330, 240], [350, 250, 550, 550])]

    p.handover = TwoTables()

    def timed(fn, runs, warmup):
        out = []
        for k in range(runs + warmup):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return res, out[warmup:]

    one, t_call = timed(lambda: p(img)[0], 10, 3)
    many, t_pages = timed(lambda: p.parse_pages([img] * 16, wave=8), 5, 2)
    result = {"page": list(img.shape[:2]), "weights": "seeded (synthetic); two fixed 300 x 200 / 200 x 300 table crops per page",
              "words_per_page": len(one.words), "cells_per_page": sum(len(t.cells) for t in one.tables),
              "call_ms_median": round(statistics.median(t_call), 2), "call_ms_min": round(min(t_call), 2), "call_runs": 10,
              "parse_pages_16_ms_median": round(statistics.median(t_pages), 2), "parse_pages_16_ms_min": round(min(t_pages), 2),
              "parse_pages_runs": 5, "parse_pages_ms_per_page": round(statistics.median(t_pages) / 16, 2),
              "device": torch.cuda.get_device_name(0)}
    p.close()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["host", "gpu"])
    ap.add_argument("--out")
    args = ap.parse_args()
    result = host() if args.what == "host" else gpu()
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
