#!/usr/bin/env python3
"""What layered pages cost a job and what they save in bytes: the device time of the separation's stages and of the two encoders
behind them, OCR.serve(jpeg="high") on bench.py's synthetic 1600 x 1200 pages with the switch off and on, and the sizes of the
files (run by hand on the GPU, not by the suite).

    python tools/mrc_serve_timing.py [--reps 3] [--wave 16] [--out profiles/mrc_serve.json] [--parent parent.json ...]
    python tools/mrc_serve_timing.py --merge result.json --parent before.json after.json --out profiles/mrc_serve.json

Device time: one wave of 16 pages, HIP events around each C-ABI call (median of 10 after a warm-up): the luminance planes and the
ink (the page-skew step's calls, unchanged), cells, pull, flags + push; then the JPEG launches on the wave's 32 layers and the
Group 4 launches on its 16 masks - and, for scale, the JPEG launches on the 16 pages themselves, which the layered job no longer
makes.
Jobs: pages/s of OCR.serve(jpeg="high") with the switch off and on: one warm-up job per leg, then `reps` jobs per leg, the legs
alternating within a repetition and each repetition starting with another leg; median and spread per leg.
--parent: results of tools/ocr_serve_timing.py --steps 1 made on the parent commit in the same session, before and after this run
(its leg "ocr_jpeg" is the job of this tool's "off" leg): the off leg against them, to confirm the default path is unaffected.
The gate for that is bench.py, run on both commits in turn.
Sizes: tests/golden/test_page.jpg and the first bench page as a plain and an optimised JPEG and as layered pages at bg_cell 1, 2
and 4 (fg_cell 8), plain and optimised tables, from the project's own encoders."""
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "test_page.jpg")


def _timed(calls, reps):
    """median device milliseconds of each of `calls` = [(name, function)], HIP events around each, after one warm-up pass"""
    from yomitoku_amd import _lib

    times = {name: [] for name, _ in calls}
    for rep in range(reps + 1):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
        torch.cuda.synchronize()
        marks[0].record()
        for k, (_, call) in enumerate(calls):
            _lib.check(call())
            marks[k + 1].record()
        torch.cuda.synchronize()
        if rep:
            for k, (name, _) in enumerate(calls):
                times[name].append(marks[k].elapsed_time(marks[k + 1]))
    return {k: round(statistics.median(v), 3) for k, v in times.items()}


def _jpeg_call(pages_dev, capacities=None):
    """the plain JPEG launches on device pages as one C-ABI call, with buffers of its own"""
    from yomitoku_amd import _lib
    from yomitoku_amd.jpeg import page_table, scratch_sizes

    lib, dev = _lib.load(), pages_dev[0].device
    blob, _, out_bytes = page_table(pages_dev, 85, capacities)
    mcus, blocks, intervals, coef_b, stream_b, iv_b = scratch_sizes([(int(p.shape[0]), int(p.shape[1]), 1 if p.dim() == 2 else 3) for p in pages_dev])[:6]
    coef, bits, ivals, files, lengths = (torch.empty(max(b, 16), dtype=torch.uint8, device=dev) for b in (coef_b, stream_b, iv_b, out_bytes, 4 * len(pages_dev)))
    blob_dev = torch.from_numpy(blob.copy()).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    keep = (coef, bits, ivals, files, lengths, blob_dev)
    return lambda: lib.ymk_jpeg_encode_pages(blob_dev.data_ptr(), blob.size, len(pages_dev), mcus, blocks, intervals, coef.data_ptr(), bits.data_ptr(),
                                             stream_b, ivals.data_ptr(), files.data_ptr(), out_bytes, lengths.data_ptr(), stream) + 0 * len(keep)


def stage_times(pages_dev, params, reps=10):
    """One wave of device pages: median device milliseconds of each stage, the flags, and the scratch the separation holds."""
    from yomitoku_amd import _lib, ccitt
    from yomitoku_amd.mrc import launch, page_table, scratch_sizes

    lib, dev, n = _lib.load(), pages_dev[0].device, len(pages_dev)
    stream = torch.cuda.current_stream().cuda_stream
    bg, fg = params["bg_cell"], params["fg_cell"]
    (luma_b, sat_b, packed_b, pyr_b, layers_b, flags_b), places = scratch_sizes([tuple(t.shape) for t in pages_dev], bg, fg)
    packed_at, at = [], 0
    for t in pages_dev:
        packed_at.append(at)
        at += int(t.shape[0]) * (-(-int(t.shape[1]) // 32))
    rec = page_table(pages_dev, packed_at, places)
    blob = torch.from_numpy(rec.reshape(-1).copy()).to(dev)
    luma, sat, packed, pyr, layers, flags, planes = (torch.empty(max(b, 16), dtype=torch.uint8, device=dev)
                                                     for b in (luma_b, sat_b, packed_b, pyr_b, layers_b, flags_b, n * 64))
    b, bw = blob.data_ptr(), blob.numel()
    tall, wide = max(int(t.shape[0]) for t in pages_dev), max(int(t.shape[1]) for t in pages_dev)
    done = launch(pages_dev, params, {})  # the layers and masks the two encoders are timed on
    torch.cuda.synchronize()
    layered = [j for j, f in enumerate(done.flags()) if f == 1]
    layer_pages = [t for j in layered for t in (done.foreground(j), done.background(j))]
    g4_scratch = {}
    calls = [
        ("luma", lambda: lib.ymk_dsk_luma(b, bw, n, tall * wide, luma.data_ptr(), luma_b, packed_b, sat_b, planes.data_ptr(), stream)),
        ("ink_adaptive_pack_3_launches", lambda: lib.ymk_bin_adaptive_pack(planes.data_ptr(), n * 16, n, tall, wide, sat.data_ptr(), sat_b,
                                                                           packed.data_ptr(), packed_b, stream)),
        ("cells", lambda: lib.ymk_mrc_cells(b, bw, n, tall, wide, bg, fg, packed.data_ptr(), packed_b, pyr.data_ptr(), pyr_b, layers_b, stream)),
        ("pull", lambda: lib.ymk_mrc_pull(b, bw, n, tall, wide, bg, fg, packed_b, pyr.data_ptr(), pyr_b, layers_b, stream)),
        ("flags_push", lambda: lib.ymk_mrc_push(b, bw, n, tall, wide, bg, fg, packed_b, pyr.data_ptr(), pyr_b, layers.data_ptr(), layers_b,
                                                flags.data_ptr(), stream)),
    ]
    if layered:
        calls += [("jpeg_of_the_layers", _jpeg_call(layer_pages, [t.numel() + 2048 for t in layer_pages])),
                  ("group4_of_the_masks", lambda: ccitt.launch_encode(done, layered, g4_scratch) and 0)]
    calls.append(("jpeg_of_the_pages_for_scale", _jpeg_call(pages_dev)))
    out = _timed(calls, reps)
    out["separation_total"] = round(sum(out[k] for k in ("luma", "ink_adaptive_pack_3_launches", "cells", "pull", "flags_push")), 3)
    out["pages_layered"] = len(layered)
    ink = packed.view(torch.int32)[: packed_b // 4].cpu().numpy().view(np.uint32)
    out["ink_fraction"] = round(float(np.unpackbits(ink.view(np.uint8)).sum()) / sum(int(t.shape[0]) * int(t.shape[1]) for t in pages_dev), 4)
    out["scratch_mib"] = {"planes": round(luma_b / 2**20, 1), "tables": round(sat_b / 2**20, 1), "packed": round(packed_b / 2**20, 1),
                          "pyramids": round(pyr_b / 2**20, 1), "layers": round(layers_b / 2**20, 1)}
    return out


def file_sizes(page):
    """bytes of a page as a plain and an optimised JPEG and as layered pages at bg_cell 1, 2, 4"""
    from yomitoku_amd.jpeg import encode_jpeg_pages

    out = {"shape": list(page.shape)}
    for label, optimize in (("plain", False), ("optimized", True)):
        out[f"jpeg_{label}"] = len(encode_jpeg_pages([page], "high", optimize=optimize)[0].data)
        for cell in (1, 2, 4):
            got = encode_jpeg_pages([page], "high", optimize=optimize, mrc={"bg_cell": cell, "fg_cell": 8})[0]
            out[f"layered_{label}_bg_cell_{cell}"] = {"mask": len(got.mask.data), "background": len(got.background.data),
                                                      "foreground": len(got.foreground.data), "total": got.nbytes}
    return out


def against_parent(result, paths):
    """the off leg against the parent commit's runs of the same job (tools/ocr_serve_timing.py --steps 1: its leg "ocr_jpeg")"""
    if not paths:
        return
    parents = []
    for path in paths:
        with open(path) as f:
            parents.append(json.load(f))
    off = result["legs"]["ocr_jpeg_high"]["off"]
    theirs = [p["legs"]["ocr_jpeg"] for p in parents]
    medians = [t["median"] for t in theirs]
    # two processes of the SAME code differ by more than three jobs of one process do, so the parent is run more than once, around
    # this run, and its runs' range is the yardstick
    result["off_against_parent"] = {"parent_runs": theirs, "parent_medians": medians, "off_median": off["median"],
                                    "off_median_inside_the_parent_runs_range_widened_by_the_spreads":
                                        bool(min(medians) - max(t["spread"] for t in theirs) - off["spread"] <= off["median"] <=
                                             max(medians) + max(t["spread"] for t in theirs) + off["spread"])}


def write(result, path):
    text = json.dumps(result, indent=1)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--wave", type=int, default=16)
    ap.add_argument("--in-flight", type=int, default=4)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--parent", nargs="+", help="results of tools/ocr_serve_timing.py --steps 1 on the parent commit, made before and after this run")
    ap.add_argument("--merge", help="a result of this tool: only hold its off leg against --parent and write it to --out")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.merge:
        with open(args.merge) as f:
            result = json.load(f)
        against_parent(result, args.parent)
        return write(result, args.out)
    from yomitoku_amd.mrc import DEFAULTS

    device = bench.rank_device(0)
    sds = bench.make_checkpoints("lite")
    sds = bench.calibrate_heads(sds, device, bench.Page(0, device))
    pages = bench.make_pages(list(range(args.pages)), device)
    host = [p.img for p in pages]
    ocr = ocr_serve_timing.build_ocr(device, sds, pages)
    shape = {"wave": args.wave, "in_flight": args.in_flight}
    result = {"pages_per_job": len(host), "reps": args.reps, **shape, **DEFAULTS, "device": torch.cuda.get_device_name(0)}
    result["device_ms_per_wave"] = stage_times([torch.from_numpy(img).to(device) for img in host[: args.wave]], dict(DEFAULTS))
    golden = np.ascontiguousarray(np.asarray(Image.open(GOLDEN).convert("RGB"))[:, :, ::-1])
    result["file_bytes"] = {"golden_page": file_sizes(golden), "bench_page": file_sizes(host[0])}
    legs = {"off": {"jpeg": "high"}, "on": {"jpeg": "high", "jpeg_mrc": True}}
    rates, failed, kinds = {name: [] for name in legs}, 0, {}
    for kwargs in legs.values():  # warm-up: shapes, workspaces, pinned rings, the render thread and its scratch
        ocr.serve(host, **shape, **kwargs)
    for rep in range(args.reps):
        order = list(legs)[rep % len(legs) :] + list(legs)[: rep % len(legs)]
        for name in order:
            rate, bad, out = ocr_serve_timing.timed_job(ocr, host, **shape, **legs[name])
            rates[name].append(rate)
            failed += bad
            files = [e[-1] for e in out if isinstance(e, tuple)]
            kinds[name] = {"pages_layered": sum(getattr(f, "mrc", False) is True for f in files),
                           "bytes_per_page": round(sum(f.nbytes if getattr(f, "mrc", False) is True else len(f.data) for f in files) / max(1, len(files)))}
    result["legs"] = {"ocr_jpeg_high": {name: {**ocr_serve_timing.summary(rates[name]), **kinds[name]} for name in legs}}
    off, on = result["legs"]["ocr_jpeg_high"]["off"], result["legs"]["ocr_jpeg_high"]["on"]
    on["median_minus_off_median"] = round(on["median"] - off["median"], 2)
    on["within_the_switch_off_spread"] = bool(off["median"] - on["median"] <= off["spread"])
    on["ms_per_page_more_than_off"] = round(1e3 / on["median"] - 1e3 / off["median"], 3)
    result["failed_entries"] = failed
    against_parent(result, args.parent)
    ocr.close()
    write(result, args.out)


if __name__ == "__main__":
    main()
