#!/usr/bin/env python3
"""What despeckling the Group 4 pages on the device costs a searchable-PDF job and what it saves in bytes: bench.py's synthetic
1600 x 1200 pages taken as grey, and the noisy golden page of tests/despeckle_ref.py tiled to that size, through OCR.serve (run
by hand on the GPU, not by the suite).

    python tools/despeckle_serve_timing.py [--reps 3] [--wave 16] [--out profiles/despeckle_serve.json]

Device time: one wave of pages thresholded by "otsu"; HIP events around each of a colour's four launches (ymk_cc_stage: label,
merge, areas, apply; median of 10 after a warm-up, each repetition on a fresh copy of the thresholded rows), around the whole
entry, and around the row coder (ymk_g4_code_rows) on the rows before and after - next to each other.
Jobs: OCR.serve(jpeg="high", jpeg_bilevel="otsu") pages/s with the switch off and on: one warm-up job per leg, then `reps` jobs
per leg, the legs alternating and each repetition starting with another leg; median and spread per leg.
Bytes: the Group 4 file of a page of each kind, and of the golden page as it is, under both methods, with and without."""
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

import bench  # noqa: E402
import ocr_serve_timing  # noqa: E402
from binarize_serve_timing import as_grey  # noqa: E402

STAGES = ("label", "merge", "areas", "apply")


def file_bytes(page):
    from yomitoku_amd.ccitt import encode_g4_pages

    out = {"height": int(page.shape[0]), "width": int(page.shape[1])}
    for method in ("otsu", "adaptive"):
        off, on = encode_g4_pages([page], binarize=method)[0], encode_g4_pages([page], binarize=method, despeckle=True)[0]
        d = on.despeckled
        out[method] = {"group4": len(off.data), "group4_despeckled": len(on.data), "ratio": round(len(on.data) / len(off.data), 3),
                       "black_components": d.black_components, "black_pixels": d.black_pixels, "white_components": d.white_components,
                       "white_pixels": d.white_pixels}
    return out


def stage_times(pages_dev, n_black=4, n_white=4, reps=10):
    """One wave of grey device pages thresholded by "otsu": median device milliseconds of every launch of both colours, of the
    entry as a whole, and of the row coder on the rows before and after."""
    from yomitoku_amd import _lib, ccitt, despeckle

    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    scratch = {}
    test = ccitt.start_binarize(pages_dev, scratch, "otsu")
    torch.cuda.synchronize()
    assert all(test.answers())
    rows0 = test.packed.clone()
    dev, n = pages_dev[0].device, len(pages_dev)
    shapes = [(int(t.shape[0]), int(t.shape[1])) for t in pages_dev]
    blob = despeckle.page_table(shapes, test.packed_at)
    label_b, area_b = despeckle.scratch_sizes(shapes)
    labels, areas = (torch.empty(b // 4, dtype=torch.int32, device=dev) for b in (label_b, area_b))
    counts = torch.zeros(4 * n, dtype=torch.int32, device=dev)
    blob_dev = torch.from_numpy(blob.reshape(-1)).to(dev)
    tall, wide = max(h for h, _ in shapes), max(w for _, w in shapes)
    buffers = (test.packed.data_ptr(), test.packed_bytes, labels.data_ptr(), label_b, areas.data_ptr(), area_b)
    table = (blob_dev.data_ptr(), blob.size, n, tall, wide)
    # the row coder's own table and scratch
    g4_blob, _, _, out_bytes = ccitt.page_table(pages_dev, test.packed_at)
    total_rows, _, slot_b, bits_b, _ = ccitt.scratch_sizes([t.shape for t in pages_dev])
    slots, rowbits = (torch.empty(max(b, 8), dtype=torch.uint8, device=dev) for b in (slot_b, bits_b))
    g4_dev = torch.from_numpy(g4_blob).to(dev)

    def code_rows():
        _lib.check(lib.ymk_g4_code_rows(g4_dev.data_ptr(), g4_blob.size, n, total_rows, tall, test.packed.data_ptr(), test.packed_bytes, slots.data_ptr(),
                                        slot_b, out_bytes, rowbits.data_ptr(), stream))

    calls = [("code_rows_before", code_rows)]
    for white, colour, size in ((0, "black", n_black), (1, "white", n_white)):
        for k, stage in enumerate(STAGES):
            calls.append((f"{colour}_{stage}", lambda k=k, white=white, size=size: _lib.check(
                lib.ymk_cc_stage(k, white, *table, *buffers, size, counts.data_ptr(), stream))))
    calls.append(("code_rows_after", code_rows))
    times = {name: [] for name, _ in calls}
    times["entry_both_colours"] = []
    for rep in range(reps + 1):
        test.packed.copy_(rows0)
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
        torch.cuda.synchronize()
        marks[0].record()
        for k, (_, call) in enumerate(calls):
            call()
            marks[k + 1].record()
        torch.cuda.synchronize()
        staged = test.packed.clone()
        test.packed.copy_(rows0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        _lib.check(lib.ymk_cc_despeckle_pages(*table, *buffers, n_black, n_white, counts.data_ptr(), stream))
        b.record()
        torch.cuda.synchronize()
        assert torch.equal(staged, test.packed)  # the stages in order are the entry
        if rep:  # the first pass warms up
            for k, (name, _) in enumerate(calls):
                times[name].append(marks[k].elapsed_time(marks[k + 1]))
            times["entry_both_colours"].append(a.elapsed_time(b))
    out = {k: round(statistics.median(v), 3) for k, v in times.items()}
    out["sum_of_the_eight_launches"] = round(sum(out[f"{c}_{s}"] for c in ("black", "white") for s in STAGES), 3)
    four = counts.view(-1, 4).sum(0).tolist()
    out["removed_per_wave"] = {"black_components": four[0], "black_pixels": four[1], "white_components": four[2], "white_pixels": four[3]}
    out["scratch_mib"] = {"labels": round(label_b / 2**20, 1), "areas": round(area_b / 2**20, 1)}
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
    import despeckle_ref

    device = bench.rank_device(0)
    sds = bench.make_checkpoints("lite")
    sds = bench.calibrate_heads(sds, device, bench.Page(0, device))
    pages = bench.make_pages(list(range(args.pages)), device)
    host = [as_grey(p.img) for p in pages]
    golden = despeckle_ref.golden_page(os.path.join(ROOT, "tests", "golden", "test_page.jpg"))
    noisy = despeckle_ref.noisy_page(golden)
    tiled = np.ascontiguousarray(np.tile(noisy, (2, 3))[:1600, :1200])
    ocr = ocr_serve_timing.build_ocr(device, sds, pages)
    shape = {"wave": args.wave, "in_flight": args.in_flight}
    result = {"pages_per_job": len(host), "reps": args.reps, **shape, "device": torch.cuda.get_device_name(0),
              "row_coder_ms_per_wave_in_profiles_ccitt_serve": 0.876}
    result["bytes"] = {"golden_page": file_bytes(np.ascontiguousarray(golden)), "noisy_golden_page": file_bytes(noisy),
                       "noisy_golden_page_tiled": file_bytes(tiled), "bench_page_as_grey": file_bytes(np.ascontiguousarray(host[0][..., 0]))}
    result["device_ms_per_wave"] = {
        "bench_pages": stage_times([torch.from_numpy(img).to(device) for img in host[: args.wave]]),
        "noisy_pages": stage_times([torch.from_numpy(tiled).to(device) for _ in range(args.wave)])}
    legs = {"off": {}, "on": {"jpeg_despeckle": True}}
    rates, failed, kinds = {name: [] for name in legs}, 0, {}
    for kwargs in legs.values():  # warm-up: shapes, workspaces, pinned rings, the render thread and its scratch
        ocr.serve(host, jpeg="high", jpeg_bilevel="otsu", **shape, **kwargs)
    for rep in range(args.reps):
        order = list(legs)[rep % len(legs) :] + list(legs)[: rep % len(legs)]
        for name in order:
            rate, bad, out = ocr_serve_timing.timed_job(ocr, host, jpeg="high", jpeg_bilevel="otsu", **shape, **legs[name])
            rates[name].append(rate)
            failed += bad
            good = [e for e in out if isinstance(e, tuple)]
            kinds[name] = {"group4_files": sum(getattr(e[-1], "bilevel", False) for e in good),
                           "bytes_per_page": round(statistics.mean(len(e[-1].data) for e in good))}
    result["legs"] = {name: {**ocr_serve_timing.summary(rates[name]), **kinds[name]} for name in legs}
    off, on = result["legs"]["off"], result["legs"]["on"]
    result["conditions"] = {"switch_off_spread": off["spread"], "on_median_minus_off_median": round(on["median"] - off["median"], 2),
                            "on_within_the_switch_off_spread": bool(off["median"] - on["median"] <= off["spread"])}
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
