#!/usr/bin/env python3
"""What lossless page files cost a searchable-PDF job and what they weigh: bench.py's textured 1600 x 1200 pages and the golden
page tiled to that size, through the coder's five launches and through OCR.serve (run by hand on the GPU, not by the suite).

    python tools/flate_serve_timing.py [--reps 3] [--wave 16] [--legs off,on] [--root TREE] [--out profiles/flate_serve.json]

Device time: one wave of pages; HIP events around each of the five launches (rows, tables, code, scan, gather; median of 5 after a
warm-up) and around the combined entry.
Bytes: the lossless file of a page of each kind next to its JPEG at "high".
Jobs: OCR.serve(jpeg="high") pages/s with the switch off and on: one warm-up job per leg, then `reps` jobs per leg, the legs taken
in turn and each repetition starting with another leg; median and spread per leg.
--legs off --root TREE: the switch-off leg alone with the package of another checkout (the parent commit's), which needs nothing
of this change: the same job before and after, to tell a difference from the box's run-to-run range."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _root() -> str:
    for k, a in enumerate(sys.argv):
        if a == "--root" and k + 1 < len(sys.argv):
            return os.path.abspath(sys.argv[k + 1])
    return HERE


ROOT = _root()
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # as `import yomitoku_amd` does and bench.py too: torch is imported first here
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import ocr_serve_timing  # noqa: E402

PHASES = ("rows", "tables", "code", "scan", "gather")


def file_bytes(page) -> dict:
    from yomitoku_amd.flate import encode_lossless_pages
    from yomitoku_amd.jpeg import encode_jpeg_pages

    flat = encode_lossless_pages([page])[0]
    jpeg = encode_jpeg_pages([page], "high", capacities=[4 * page.size])[0]
    return {"height": int(page.shape[0]), "width": int(page.shape[1]), "lossless": flat.nbytes, "jpeg_high": len(jpeg.data),
            "ratio": round(flat.nbytes / len(jpeg.data), 3), "bytes_per_pixel": round(flat.nbytes / (page.shape[0] * page.shape[1]), 3)}


def stage_times(pages_dev, reps=5) -> dict:
    """One wave of device pages: median device milliseconds of each of the five launches and of the combined entry."""
    from yomitoku_amd import _lib, flate

    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    c = flate._Coding(pages_dev, {})
    common = c._common(c.blob_dev, c.blob.size, c.n)
    p = lambda t: t.data_ptr()  # noqa: E731
    calls = [lambda: lib.ymk_flate_rows(*common, c.max_rows, c.max_row_segs, None, p(c.filt), p(c.tokens), p(c.segtok), p(c.segadler), p(c.hist), stream),
             lambda: lib.ymk_flate_tables(*common, None, p(c.hist), p(c.segadler), p(c.tables), p(c.head), p(c.sizes), stream),
             lambda: lib.ymk_flate_code(*common, c.max_rows, c.max_row_segs, p(c.tokens), p(c.segtok), p(c.tables), p(c.head), p(c.slots), p(c.segbits), stream),
             lambda: lib.ymk_flate_scan(*common, p(c.segbits), p(c.head), p(c.off), p(c.sizes), stream),
             lambda: lib.ymk_flate_gather(*common, p(c.slots), p(c.head), p(c.off), p(c.out), c.largest, stream)]
    times = {name: [] for name in PHASES + ("entry",)}
    for rep in range(reps + 1):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
        torch.cuda.synchronize()
        marks[0].record()
        for k, call in enumerate(calls):
            _lib.check(call(), PHASES[k])
            marks[k + 1].record()
        torch.cuda.synchronize()
        staged = c.out.clone()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        c.run()
        b.record()
        torch.cuda.synchronize()
        sizes = c.answers()
        assert all(n > 0 for n, _ in sizes) and all(torch.equal(staged[at : at + n], c.out[at : at + n]) for at, (n, _) in zip(c.offsets, sizes))
        if rep:  # the first pass warms up
            for k, name in enumerate(PHASES):
                times[name].append(marks[k].elapsed_time(marks[k + 1]))
            times["entry"].append(a.elapsed_time(b))
    out = {k: round(statistics.median(v), 3) for k, v in times.items()}
    out["sum_of_the_five_launches"] = round(sum(out[k] for k in PHASES), 3)
    out["bytes_per_page"] = round(statistics.mean(n for n, _ in sizes))
    shapes = [flate._shape(t) for t in pages_dev]
    sized = flate.scratch_sizes(shapes)
    out["scratch_mib"] = {"filtered": round(sized[1] / 2**20, 1), "tokens": round(sized[2] / 2**20, 1), "slots": round(sized[5] / 2**20, 1),
                          "files": round(c.out_bytes / 2**20, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--wave", type=int, default=16)
    ap.add_argument("--in-flight", type=int, default=4)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--legs", default="off,on")
    ap.add_argument("--root", default=HERE, help="the checkout whose package runs (default: this one)")
    ap.add_argument("--out")
    args = ap.parse_args()
    from PIL import Image

    device = bench.rank_device(0)
    sds = bench.make_checkpoints("lite")
    sds = bench.calibrate_heads(sds, device, bench.Page(0, device))
    pages = bench.make_pages(list(range(args.pages)), device)
    host = [np.ascontiguousarray(p.img) for p in pages]
    ocr = ocr_serve_timing.build_ocr(device, sds, pages)
    shape = {"wave": args.wave, "in_flight": args.in_flight}
    names = [n for n in args.legs.split(",") if n]
    result = {"root": os.path.relpath(ROOT, HERE), "pages_per_job": len(host), "reps": args.reps, **shape, "device": torch.cuda.get_device_name(0)}
    if "on" in names:
        golden = np.ascontiguousarray(np.array(Image.open(os.path.join(HERE, "tests", "golden", "test_page.jpg")).convert("RGB"))[:, :, ::-1])
        tiled = np.ascontiguousarray(np.tile(golden, (2, 3, 1))[:1600, :1200])
        result["bytes"] = {"golden_page": file_bytes(golden), "golden_page_tiled": file_bytes(tiled), "bench_page": file_bytes(host[0])}
        result["device_ms_per_wave"] = {
            "bench_pages": stage_times([torch.from_numpy(img).to(device) for img in host[: args.wave]]),
            "golden_pages_tiled": stage_times([torch.from_numpy(tiled).to(device) for _ in range(args.wave)])}
    legs = {name: ({"jpeg_lossless": True} if name == "on" else {}) for name in names}
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
            kinds[name] = {"lossless_files": sum(getattr(e[-1], "lossless", False) for e in good),
                           "bytes_per_page": round(statistics.mean(len(e[-1].data) for e in good))}
    result["legs"] = {name: {**ocr_serve_timing.summary(rates[name]), **kinds[name]} for name in legs}
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
