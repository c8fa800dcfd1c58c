#!/usr/bin/env python3
"""What turning pages upright on the device costs a job: the device time of the step's four stages, and OCR.serve /
DocumentAnalyzer.serve on bench.py's synthetic 1600 x 1200 pages with the switch off and on (run by hand on the GPU, not by the
suite).

    python tools/deskew_serve_timing.py [--reps 3] [--wave 16] [--out profiles/deskew_serve.json] [--parent parent.json]

Device time: one wave of 16 pages, HIP events around each C-ABI call (median of 10 after a warm-up): the luminance planes, the
ink (the binariser's three launches, unchanged), the scores, the choice, the rotation - once on the pages as they are (upright:
the rotation is a copy) and once on the same pages turned by 2 degrees (every page is rotated).
Jobs: pages/s of OCR.serve and DocumentAnalyzer.serve with the switch off, on, and on with the turned pages: one warm-up job per
leg, then `reps` jobs per leg, the legs alternating within a repetition and each repetition starting with another leg; median
and spread per leg.  The yardstick is the switch-off leg of the same run.
--parent: results of tools/ocr_serve_timing.py made on the parent commit in the same session, before and after this run (its legs
"ocr" and "document" are the jobs of this tool's "off" legs: --steps 1 there): the off legs against them, to confirm the default
path is unaffected.  The gate for that is bench.py, run on both commits in turn."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # as `import yomitoku_amd` does and bench.py too: torch is imported first here
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import bench  # noqa: E402
import ocr_serve_timing  # noqa: E402


def turned(img, angle):
    """A B G R page turned counter-clockwise by `angle` degrees, paper white outside: a scan that lay askew."""
    return np.ascontiguousarray(np.asarray(Image.fromarray(img).rotate(angle, Image.BICUBIC, fillcolor=(255, 255, 255))))


def stage_times(pages_dev, reps=10):
    """One wave of device pages: median device milliseconds of each of the step's calls (HIP events around each), the indices
    chosen, and the scratch the step holds."""
    from yomitoku_amd import _lib
    from yomitoku_amd.deskew import DEFAULTS, _checked_table, page_table, scratch_sizes

    lib, dev, n = _lib.load(), pages_dev[0].device, len(pages_dev)
    stream = torch.cuda.current_stream().cuda_stream
    table, s_max, dead = _checked_table(dict(DEFAULTS))
    sizes, fits = scratch_sizes([tuple(t.shape) for t in pages_dev], len(table), s_max)
    luma_b, sat_b, packed_b, scores_b, choice_b = sizes
    dsts = [torch.empty_like(t) for t in pages_dev]
    rec = page_table(pages_dev, dsts)
    blob = torch.from_numpy(rec.reshape(-1).copy()).to(dev)
    table_dev = torch.from_numpy(table.reshape(-1).copy()).to(dev)
    luma, sat, packed, scores, choice, planes = (torch.empty(max(b, 8), dtype=torch.uint8, device=dev)
                                                 for b in (luma_b, sat_b, packed_b, scores_b, choice_b, n * 64))
    b, bw = blob.data_ptr(), blob.numel()
    most = max(int(t.shape[0]) * int(t.shape[1]) for t in pages_dev)
    tall, wide = max(int(t.shape[0]) for t in pages_dev), max(int(t.shape[1]) for t in pages_dev)
    calls = [
        ("luma", lambda: lib.ymk_dsk_luma(b, bw, n, most, luma.data_ptr(), luma_b, packed_b, sat_b, planes.data_ptr(), stream)),
        ("ink_adaptive_pack_3_launches", lambda: lib.ymk_bin_adaptive_pack(planes.data_ptr(), n * 16, n, tall, wide, sat.data_ptr(), sat_b,
                                                                           packed.data_ptr(), packed_b, stream)),
        ("scores", lambda: lib.ymk_dsk_scores(b, bw, n, packed.data_ptr(), packed_b, sat_b, luma_b, table_dev.data_ptr(), len(table), s_max,
                                              scores.data_ptr(), stream)),
        ("choose", lambda: lib.ymk_dsk_choose(b, bw, n, packed_b, sat_b, luma_b, scores.data_ptr(), len(table), s_max, dead, choice.data_ptr(), stream)),
        ("rotate", lambda: lib.ymk_dsk_rotate(b, bw, n, 3 * most, table_dev.data_ptr(), len(table), choice.data_ptr(), stream)),
    ]
    times = {name: [] for name, _ in calls}
    for rep in range(reps + 1):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
        torch.cuda.synchronize()
        marks[0].record()
        for k, (_, call) in enumerate(calls):
            _lib.check(call())
            marks[k + 1].record()
        torch.cuda.synchronize()
        if rep:  # the first pass warms up
            for k, (name, _) in enumerate(calls):
                times[name].append(marks[k].elapsed_time(marks[k + 1]))
    out = {k: round(statistics.median(v), 3) for k, v in times.items()}
    out["total"] = round(sum(out.values()), 3)
    words = choice.view(torch.int32)[: n * 8].cpu().numpy().reshape(n, 8)
    ink = packed.view(torch.int32)[: packed_b // 4].cpu().numpy().view(np.uint32)
    out["indices"] = [int(v) for v in words[:, 0]]
    out["estimated"] = [bool(v == 1) for v in words[:, 1]]
    out["ink_fraction"] = round(float(np.unpackbits(ink.view(np.uint8)).sum()) / sum(int(t.shape[0]) * int(t.shape[1]) for t in pages_dev), 4)
    out["scratch_mib"] = {"planes": round(luma_b / 2**20, 1), "tables": round(sat_b / 2**20, 1), "packed": round(packed_b / 2**20, 1),
                          "scores": round(scores_b / 2**20, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--wave", type=int, default=16)
    ap.add_argument("--in-flight", type=int, default=4)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--angle", type=float, default=2.0)
    ap.add_argument("--parent", nargs="+", help="results of tools/ocr_serve_timing.py --steps 1 on the parent commit, made before and after this run")
    ap.add_argument("--out")
    args = ap.parse_args()
    device = bench.rank_device(0)
    sds = bench.make_checkpoints("lite")
    sds = bench.calibrate_heads(sds, device, bench.Page(0, device))
    pages = bench.make_pages(list(range(args.pages)), device)
    host = [p.img for p in pages]
    askew = [turned(img, args.angle) for img in host]
    doc = bench.build_analyzer(device, sds, "lite")
    doc.truth = pages
    ocr = ocr_serve_timing.build_ocr(device, sds, pages)
    shape = {"wave": args.wave, "in_flight": args.in_flight}
    result = {"pages_per_job": len(host), "reps": args.reps, **shape, "turned_by_degrees": args.angle, "device": torch.cuda.get_device_name(0)}
    result["device_ms_per_wave"] = {"upright": stage_times([torch.from_numpy(img).to(device) for img in host[: args.wave]]),
                                    "turned": stage_times([torch.from_numpy(img).to(device) for img in askew[: args.wave]])}
    legs = {"off": (host, {}), "on": (host, {"deskew": True}), "on_turned": (askew, {"deskew": True})}
    result["legs"], failed = {}, 0
    for label, an in (("ocr", ocr), ("document", doc)):
        rates, angles = {name: [] for name in legs}, {}
        for srcs, kwargs in legs.values():  # warm-up: shapes, workspaces, pinned rings, the step's scratch
            an.serve(srcs, **shape, **kwargs)
        for rep in range(args.reps):
            order = list(legs)[rep % len(legs) :] + list(legs)[: rep % len(legs)]
            for name in order:
                rate, bad, out = ocr_serve_timing.timed_job(an, legs[name][0], **shape, **legs[name][1])
                rates[name].append(rate)
                failed += bad
                if name != "off":
                    got = [e[-1].angle for e in out if isinstance(e, tuple)]
                    angles[name] = {"pages_turned_back": sum(a != 0.0 for a in got), "median_angle": round(statistics.median(got), 2)}
        result["legs"][label] = {name: {**ocr_serve_timing.summary(rates[name]), **angles.get(name, {})} for name in legs}
        off = result["legs"][label]["off"]
        for name in ("on", "on_turned"):
            leg = result["legs"][label][name]
            leg["median_minus_off_median"] = round(leg["median"] - off["median"], 2)
            leg["within_the_switch_off_spread"] = bool(off["median"] - leg["median"] <= off["spread"])
            leg["ms_per_page_more_than_off"] = round(1e3 / leg["median"] - 1e3 / off["median"], 3)
    if args.parent:
        parents = []
        for path in args.parent:
            with open(path) as f:
                parents.append(json.load(f))
        result["off_against_parent"] = {}
        for label in ("ocr", "document"):
            mine, theirs = result["legs"][label]["off"], [p["legs"][label] for p in parents]
            medians = [t["median"] for t in theirs]
            # a job of 64 pages lasts half a second: two processes of the SAME code differ by more than three jobs of one
            # process do, so the parent is run more than once, around this run, and its runs' range is the yardstick
            result["off_against_parent"][label] = {"parent_runs": theirs, "parent_medians": medians, "off_median": mine["median"],
                                                   "off_median_inside_the_parent_runs_range_widened_by_the_spreads":
                                                       bool(min(medians) - max(t["spread"] for t in theirs) - mine["spread"] <= mine["median"])}
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
