#!/usr/bin/env python3
"""What a text-only job saves by not going through DocumentAnalyzer: bench.py's 64 synthetic 1600 x 1200 host pages, its seeded
and calibrated weights, the pages' truth handed over at `maps` and `boxes` (yomitoku_amd/testing.py: TruthHandover) - through
DocumentAnalyzer.serve and through OCR.serve, in one process (run by hand on the GPU, not by the suite).

    python tools/ocr_serve_timing.py [--reps 3] [--wave 16] [--in-flight 4] [--steps 2] [--out profiles/ocr_serve.json]

Legs, each one job over all pages (`--steps` passes over them, as bench.py's secondary legs: a single pass of four waves mostly
measures the pipeline filling and draining), pages/s = pages / wall time, median and spread (max - min) over `--reps` jobs after
one warm-up job each:
  document     DocumentAnalyzer.serve(pages)                    the headline path: both chains
  ocr          OCR.serve(pages)                                 the OCR chain alone
  ocr_jpeg     OCR.serve(pages, jpeg="high")                    what a searchable PDF embeds, next to the words
These three alternate within a repetition.  Then, each as a block of its own (a change of `rec_lanes` rebuilds the pipeline, which
must not happen inside a timed job):
  ocr_lanes_1 / _2 / _3    OCR.serve(pages, rec_lanes=n)
Also: for one further OCR.serve job and one DocumentAnalyzer.serve job, every stage's busy fraction (the sum of its visits' wall
time over the job's wall time, from `pipe.trace`; `recognize` has `rec_lanes` threads, so its fraction may exceed 1), and the
condition the feature has to meet: the ocr median is not below the document median of the same run."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # as `import yomitoku_amd` does and bench.py too: torch is imported first here
import torch  # noqa: E402

import bench  # noqa: E402


def build_ocr(device, sds, pages):
    """The product's OCR on bench.py's OCR configs and weights, the pages' truth at the two hand-overs of its one chain."""
    from yomitoku_amd import OCR
    from yomitoku_amd.testing import TruthHandover

    an = OCR(configs=bench.MODEL_SETS["lite"]["ocr"], device=str(device))
    an.detector.model.load_state_dict(sds["det"])
    an.recognizer.model.load_state_dict(sds["rec"])
    an.handover = TruthHandover(truth=pages)
    return an


def timed_job(an, host, **kwargs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = an.serve(host, **kwargs)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return len(out) / dt, sum(isinstance(e, BaseException) for e in out), out


def summary(rates):
    return {"pages_per_s": [round(v, 2) for v in rates], "median": round(statistics.median(rates), 2),
            "spread": round(max(rates) - min(rates), 2)}


def stage_busy(an, host, **kwargs):
    """One traced job: per stage the sum of its visits' wall time over the job's wall time, visits, and mean milliseconds."""
    an.serve(host[:1], **kwargs)  # the pipeline exists in the job's shape
    an._pipeline.trace = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    an.serve(host, **kwargs)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    trace, an._pipeline.trace = an._pipeline.trace, None
    spans = {}
    for name, _, _, a, b in trace:
        spans.setdefault(name, []).append(b - a)
    return {"pages_per_s": round(len(host) / dt, 2),
            "stages": {name: {"busy_frac": round(sum(d) / dt, 3), "visits": len(d), "mean_ms": round(1e3 * sum(d) / len(d), 2)}
                       for name, d in spans.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--wave", type=int, default=16)
    ap.add_argument("--in-flight", type=int, default=4)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2, help="passes over the pages per job")
    ap.add_argument("--out")
    args = ap.parse_args()
    device = bench.rank_device(0)
    sds = bench.make_checkpoints("lite")
    sds = bench.calibrate_heads(sds, device, bench.Page(0, device))
    pages = bench.make_pages(list(range(args.pages)), device)
    host = [p.img for p in pages] * args.steps  # page id i -> truth[i % len(truth)]
    doc = bench.build_analyzer(device, sds, "lite")
    doc.truth = pages
    ocr = build_ocr(device, sds, pages)
    shape = {"wave": args.wave, "in_flight": args.in_flight}
    legs = {"document": (doc, {}), "ocr": (ocr, {}), "ocr_jpeg": (ocr, {"jpeg": "high"})}
    result = {"pages_per_job": len(host), "distinct_pages": args.pages, "reps": args.reps, **shape, "device": torch.cuda.get_device_name(0), "legs": {}}
    rates = {name: [] for name in legs}
    failed = 0
    for name, (an, kwargs) in legs.items():  # warm-up: shapes, workspaces, pinned rings, the render thread and its scratch
        an.serve(host, **shape, **kwargs)
    for _ in range(args.reps):
        for name, (an, kwargs) in legs.items():
            rate, bad, out = timed_job(an, host, **shape, **kwargs)
            rates[name].append(rate)
            failed += bad
            if name == "ocr":
                words = sum(len(e.words) for e in out if not isinstance(e, BaseException)) / max(1, len(out))
    for name in legs:
        result["legs"][name] = summary(rates[name])
    result["words_per_page"] = round(words, 1)
    lanes = {}
    for n in (1, 3, 2):  # 2 last: the pipeline is left in its default shape for the traced job
        ocr.serve(host, **shape, rec_lanes=n)
        got = []
        for _ in range(args.reps):
            rate, bad, _ = timed_job(ocr, host, **shape, rec_lanes=n)
            got.append(rate)
            failed += bad
        lanes[n] = summary(got)
    for n in (1, 2, 3):
        result["legs"][f"ocr_lanes_{n}"] = lanes[n]
    result["trace"] = {"ocr": stage_busy(ocr, host, **shape), "document": stage_busy(doc, host, **shape)}
    d, o = result["legs"]["document"], result["legs"]["ocr"]
    result["ocr_over_document"] = round(o["median"] / d["median"], 3)
    result["ocr_not_below_document"] = bool(o["median"] >= d["median"])
    best = max(lanes, key=lambda n: lanes[n]["median"])
    result["rec_lanes"] = {"best": best, "beats_2_by_more_than_the_spread":
                           bool(best != 2 and lanes[best]["median"] - lanes[2]["median"] > max(lanes[best]["spread"], lanes[2]["spread"]))}
    result["failed_entries"] = failed
    ocr.close()
    bench.close_analyzer(doc)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
