#!/usr/bin/env python3
"""What thresholding grey-valued pages on the device costs a searchable-PDF job and what it saves in bytes: bench.py's synthetic
1600 x 1200 pages taken as grey, through OCR.serve (run by hand on the GPU, not by the suite).

    python tools/binarize_serve_timing.py [--reps 3] [--wave 16] [--out profiles/binarize_serve.json]

Device time: one wave of grey-valued pages, HIP events around each C-ABI call of the new launches (median of 10 after a
warm-up), next to the "auto" path's test-and-pack launch on the same pages.
Jobs: OCR.serve(jpeg="high") pages/s on the grey-valued pages with the switch off, "otsu" and "adaptive": one warm-up job per leg,
then `reps` jobs per leg, the legs alternating within a repetition and each repetition starting with another leg; median and
spread per leg.  The yardstick is the switch-off leg of the same run.
Bytes: tests/golden/test_page.jpg taken as grey and the gradient page of tests/binarize_ref.py, as Group 4 under each method,
next to the grey JPEG at "high"."""
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

METHODS = ("otsu", "adaptive")


def as_grey(img):
    """A B G R page with its green plane in every channel: a grey-valued scan as load_image gives it."""
    return np.ascontiguousarray(np.stack([img[..., 1]] * 3, -1))


def file_bytes(page):
    from yomitoku_amd.jpeg import encode_jpeg

    out = {"height": int(page.shape[0]), "width": int(page.shape[1]), "grey_jpeg_q85": len(encode_jpeg(page, "high", grey="auto").data)}
    for method in METHODS:
        e = encode_jpeg(page, "high", bilevel=method)
        assert e.bilevel and e.method == method
        out["group4_" + method] = len(e.data)
        if method == "otsu":
            out["otsu_threshold"] = e.threshold
    return out


def stage_times(pages_dev, reps=10):
    """One wave of grey-valued device pages: median device milliseconds of every launch that thresholds, and of the "auto"
    path's test-and-pack on the same pages (HIP events around each C-ABI call)."""
    from yomitoku_amd import _lib
    from yomitoku_amd.ccitt import binarize_scratch_sizes, page_table, scratch_sizes

    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    blob, _, _, _ = page_table(pages_dev, capacities=[0] * len(pages_dev), tables=True)
    shapes = [t.shape for t in pages_dev]
    packed_b = scratch_sizes(shapes)[1]
    hist_b, sat_b = binarize_scratch_sizes(shapes)
    dev, n = pages_dev[0].device, len(pages_dev)
    answer, hist, sat, packed = (torch.empty(max(b, 8), dtype=torch.uint8, device=dev) for b in (8 * n, hist_b, sat_b, packed_b))
    blob_dev = torch.from_numpy(blob).to(dev)
    table = (blob_dev.data_ptr(), blob.size, n)
    most = max(int(t.shape[0]) * int(t.shape[1]) for t in pages_dev)
    tall, wide = max(int(t.shape[0]) for t in pages_dev), max(int(t.shape[1]) for t in pages_dev)
    thr = answer.data_ptr() + 4 * n
    calls = [
        ("auto_test_pack", lambda: lib.ymk_g4_test_pack(*table, most, answer.data_ptr(), packed.data_ptr(), packed_b, stream)),
        ("test", lambda: lib.ymk_bin_test_hist(*table, most, answer.data_ptr(), None, stream)),
        ("test_hist", lambda: lib.ymk_bin_test_hist(*table, most, answer.data_ptr(), hist.data_ptr(), stream)),
        ("otsu", lambda: lib.ymk_bin_otsu(n, hist.data_ptr(), thr, stream)),
        ("otsu_pack", lambda: lib.ymk_bin_otsu_pack(*table, most, thr, packed.data_ptr(), packed_b, stream)),
        ("adaptive_pack_3_launches", lambda: lib.ymk_bin_adaptive_pack(*table, tall, wide, sat.data_ptr(), sat_b, packed.data_ptr(), packed_b, stream)),
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
    assert (answer.view(torch.int32)[:n] == 0).all()
    out = {k: round(statistics.median(v), 3) for k, v in times.items()}
    out["scratch_mib"] = {"packed": round(packed_b / 2**20, 1), "histograms": round(hist_b / 2**20, 2), "tables": round(sat_b / 2**20, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--wave", type=int, default=16)
    ap.add_argument("--in-flight", type=int, default=4)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--out")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import binarize_ref

    device = bench.rank_device(0)
    sds = bench.make_checkpoints("lite")
    sds = bench.calibrate_heads(sds, device, bench.Page(0, device))
    pages = bench.make_pages(list(range(args.pages)), device)
    host = [as_grey(p.img) for p in pages]
    ocr = ocr_serve_timing.build_ocr(device, sds, pages)
    shape = {"wave": args.wave, "in_flight": args.in_flight}
    result = {"pages_per_job": len(host), "reps": args.reps, **shape, "device": torch.cuda.get_device_name(0)}
    golden = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "test_page.jpg")).convert("L"))
    gradient = binarize_ref.gradient_page()[0]
    result["bytes"] = {"golden_page_as_grey": file_bytes(np.ascontiguousarray(golden)), "gradient_page": file_bytes(gradient),
                       "bench_page_as_grey": file_bytes(host[0])}
    result["device_ms_per_wave"] = stage_times([torch.from_numpy(img).to(device) for img in host[: args.wave]])
    legs = {"off": {}, "otsu": {"jpeg_bilevel": "otsu"}, "adaptive": {"jpeg_bilevel": "adaptive"}}
    rates, failed, kinds = {name: [] for name in legs}, 0, {}
    for kwargs in legs.values():  # warm-up: shapes, workspaces, pinned rings, the render thread and its scratch
        ocr.serve(host, jpeg="high", **shape, **kwargs)
    for rep in range(args.reps):
        order = list(legs)[rep % len(legs) :] + list(legs)[: rep % len(legs)]
        for name in order:
            rate, bad, out = ocr_serve_timing.timed_job(ocr, host, jpeg="high", **shape, **legs[name])
            rates[name].append(rate)
            failed += bad
            good = [e for e in out if isinstance(e, tuple)]
            kinds[name] = {"group4_files": sum(getattr(e[-1], "bilevel", False) for e in good),
                           "bytes_per_page": round(statistics.mean(len(e[-1].data) for e in good))}
    result["legs"] = {name: {**ocr_serve_timing.summary(rates[name]), **kinds[name]} for name in legs}
    off = result["legs"]["off"]
    result["conditions"] = {"switch_off_spread": off["spread"]}
    for name in METHODS:
        leg = result["legs"][name]
        result["conditions"][name + "_median_minus_off_median"] = round(leg["median"] - off["median"], 2)
        result["conditions"][name + "_within_the_switch_off_spread"] = bool(off["median"] - leg["median"] <= off["spread"])
    result["failed_entries"] = failed
    ocr.close()
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
