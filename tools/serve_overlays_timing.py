#!/usr/bin/env python3
"""What serve(overlays=True) costs next to serve(): bench.py's 64 synthetic 1600 x 1200 pages and its analyzer, served in turn
without and with overlays (run by hand on the GPU, not by the suite).

    python tools/serve_overlays_timing.py [--reps 3] [--wave 16] [--out FILE]

Reported: pages/s of both forms (median over the repetitions, each repetition one job over all pages), and from the pipeline's
own trace of the overlays jobs every stage's mean time per wave - the render stage next to the longest of the others."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import torch  # noqa: E402

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--wave", type=int, default=16)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--out")
    args = ap.parse_args()
    device = bench.rank_device(0)
    sds = bench.make_checkpoints("lite")
    sds = bench.calibrate_heads(sds, device, bench.Page(0, device))
    pages = bench.make_pages(list(range(args.pages)), device)
    an = bench.build_analyzer(device, sds, "lite")
    an.truth = pages
    host = [p.img for p in pages]
    an.serve(host, wave=args.wave)  # warm-up: shapes, workspaces, pinned rings
    warm = an.serve(host[: args.wave], wave=args.wave, overlays=True)  # the render thread, its pinned buffers, the glyphs
    failed = sum(1 for e in warm if not isinstance(e, tuple))
    torch.cuda.synchronize()
    rates = {"plain": [], "overlays": []}
    stages = {}
    for _ in range(args.reps):
        for form in ("plain", "overlays"):
            an._pipeline.trace = [] if form == "overlays" else None
            t0 = time.perf_counter()
            out = an.serve(host, wave=args.wave, overlays=form == "overlays")
            torch.cuda.synchronize()
            rates[form].append(len(out) / (time.perf_counter() - t0))
            failed += sum(1 for e in out if isinstance(e, BaseException))
            for name, _, n, t_start, t_end in an._pipeline.trace or ():
                if n == args.wave:
                    stages.setdefault(name, []).append((t_end - t_start) * 1e3)
    an._pipeline.trace = None
    per_wave = {name: round(statistics.mean(v), 2) for name, v in stages.items()}
    others = {k: v for k, v in per_wave.items() if k not in ("render", "wait_slot")}
    longest = max(others, key=others.get)
    result = {
        "pages": args.pages, "wave": args.wave, "reps": args.reps, "failed_entries": failed,
        "pages_per_s_plain": [round(v, 2) for v in rates["plain"]], "pages_per_s_overlays": [round(v, 2) for v in rates["overlays"]],
        "pages_per_s_plain_median": round(statistics.median(rates["plain"]), 2),
        "pages_per_s_overlays_median": round(statistics.median(rates["overlays"]), 2),
        "stage_ms_per_wave_overlays_jobs": per_wave, "render_ms_per_wave": per_wave.get("render"),
        "longest_other_stage": longest, "longest_other_stage_ms_per_wave": others[longest],
        "device": torch.cuda.get_device_name(0),
    }
    an.close()
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
