#!/usr/bin/env python3
"""What Group 4 files save a searchable-PDF job of two-valued pages, and what the switch costs a job without such pages:
bench.py's synthetic 1600 x 1200 pages, as they are and thresholded at 128, through OCR.serve (run by hand on the GPU, not by
the suite).

    python tools/ccitt_serve_timing.py [--reps 3] [--wave 16] [--out profiles/ccitt_serve.json]

Bytes: the Group 4 file next to this tree's grey JPEG at "high", plain and with jpeg_optimize, for tests/golden/test_page.jpg
thresholded at 128 and for the bench's page 0 thresholded.
Device time: one wave of thresholded pages, HIP events around each C-ABI call of the new stages (median of 10 after a warm-up),
next to the JPEG stages for the same pages written as grey files and as colour files (tools/jpeg_serve_timing.py).
Jobs: OCR.serve(jpeg="high") pages/s, one warm-up job and then `reps` jobs per leg, the legs alternating within a repetition and
each repetition starting with another leg (a leg's place in the round is worth about as much as the switch), then one traced job
per leg for the render stage's mean visit:
  off        the bench's pages, the switch off
  on_none    the bench's pages, jpeg_bilevel="auto": no page qualifies, the test alone is paid
  two_off    the thresholded pages, the switch off (colour JPEG files of two-valued pages: today)
  two_on     the thresholded pages, jpeg_bilevel="auto"
Conditions (recorded, not fixed numbers): on_none's median within the spread of off's jobs below off's median; two_on's median
not below two_off's by more than that spread."""
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
import jpeg_serve_timing  # noqa: E402
import ocr_serve_timing  # noqa: E402


def thresholded(img):
    """A B G R page binarised at 128 on its green plane: every sample 0 or 255, B == G == R - a 1-bit scan as load_image gives it."""
    v = np.where(img[..., 1] < 128, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([v] * 3, -1))


def file_bytes(page):
    from yomitoku_amd.jpeg import encode_jpeg

    g4 = encode_jpeg(page, "high", bilevel="auto")
    grey = encode_jpeg(page, "high", grey="auto")
    opt = encode_jpeg(page, "high", grey="auto", optimize=True)
    assert g4.bilevel and grey.grey and opt.optimized
    return {"height": int(page.shape[0]), "width": int(page.shape[1]), "black_fraction": round(float((page[..., 0] == 0).mean()), 4),
            "group4": len(g4.data), "grey_jpeg_q85": len(grey.data), "grey_jpeg_q85_optimized": len(opt.data)}


def g4_stage_times(pages_dev, reps=10):
    """One wave of two-valued device pages: median device milliseconds of the four launches (HIP events around each C-ABI call)."""
    from yomitoku_amd import _lib
    from yomitoku_amd.ccitt import page_table, scratch_sizes

    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    blob, _, _, out_bytes = page_table(pages_dev)
    rows, packed_b, slot_b, bits_b, off_b = scratch_sizes([t.shape for t in pages_dev])
    dev, n = pages_dev[0].device, len(pages_dev)
    flags, packed, slots, rowbits, rowoff, out, lengths = (torch.empty(max(b, 8), dtype=torch.uint8, device=dev)
                                                           for b in (4 * n, packed_b, slot_b, bits_b, off_b, out_bytes, 4 * n))
    blob_dev = torch.from_numpy(blob).to(dev)
    table = (blob_dev.data_ptr(), blob.size, n)
    most = max(int(t.shape[0]) * int(t.shape[1]) for t in pages_dev)
    cap, tallest = int(blob.reshape(-1, 16)[:, 10].max()), max(int(t.shape[0]) for t in pages_dev)
    names = ("test_pack", "code_rows", "scan", "concat")
    times = {k: [] for k in names}
    for rep in range(reps + 1):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        torch.cuda.synchronize()
        marks[0].record()
        _lib.check(lib.ymk_g4_test_pack(*table, most, flags.data_ptr(), packed.data_ptr(), packed_b, stream))
        marks[1].record()
        _lib.check(lib.ymk_g4_code_rows(*table, rows, tallest, packed.data_ptr(), packed_b, slots.data_ptr(), slot_b, out_bytes, rowbits.data_ptr(),
                                        stream))
        marks[2].record()
        _lib.check(lib.ymk_g4_scan(*table, rows, packed_b, slot_b, out_bytes, rowbits.data_ptr(), rowoff.data_ptr(), lengths.data_ptr(), stream))
        marks[3].record()
        _lib.check(lib.ymk_g4_concat(*table, rows, packed_b, slots.data_ptr(), slot_b, rowoff.data_ptr(), lengths.data_ptr(), out.data_ptr(), out_bytes,
                                     cap, stream))
        marks[4].record()
        torch.cuda.synchronize()
        if rep:  # the first pass warms up
            for k, name in enumerate(names):
                times[name].append(marks[k].elapsed_time(marks[k + 1]))
    assert (flags.view(torch.int32) == 0).all() and (lengths.view(torch.int32) > 0).all()
    out = {k: round(statistics.median(v), 3) for k, v in times.items()}
    out["scratch_mib"] = {"packed": round(packed_b / 2**20, 1), "slots": round(slot_b / 2**20, 1), "files": round(out_bytes / 2**20, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--wave", type=int, default=16)
    ap.add_argument("--in-flight", type=int, default=4)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--out")
    args = ap.parse_args()
    device = bench.rank_device(0)
    sds = bench.make_checkpoints("lite")
    sds = bench.calibrate_heads(sds, device, bench.Page(0, device))
    pages = bench.make_pages(list(range(args.pages)), device)
    host = [p.img for p in pages]
    two = [thresholded(img) for img in host]
    ocr = ocr_serve_timing.build_ocr(device, sds, pages)
    shape = {"wave": args.wave, "in_flight": args.in_flight}
    result = {"pages_per_job": len(host), "reps": args.reps, **shape, "device": torch.cuda.get_device_name(0)}
    golden = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "test_page.jpg")).convert("RGB"))[:, :, ::-1]
    result["bytes"] = {"golden_page_thresholded": file_bytes(thresholded(golden)), "bench_page_thresholded": file_bytes(two[0])}
    wave_dev = [torch.from_numpy(img).to(device) for img in two[: args.wave]]
    result["device_ms_per_wave"] = {"group4": g4_stage_times(wave_dev),
                                    "jpeg_grey_files": jpeg_serve_timing.stage_times(wave_dev, "high", grey="auto"),
                                    "jpeg_colour_files": jpeg_serve_timing.stage_times(wave_dev, "high")}
    legs = {"off": (host, {}), "on_none": (host, {"jpeg_bilevel": "auto"}), "two_off": (two, {}), "two_on": (two, {"jpeg_bilevel": "auto"})}
    rates, failed, kinds = {name: [] for name in legs}, 0, {}
    for name, (src, kwargs) in legs.items():  # warm-up: shapes, workspaces, pinned rings, the render thread and its scratch
        ocr.serve(src, jpeg="high", **shape, **kwargs)
    for rep in range(args.reps):
        order = list(legs)[rep % len(legs) :] + list(legs)[: rep % len(legs)]
        for name in order:
            src, kwargs = legs[name]
            rate, bad, out = ocr_serve_timing.timed_job(ocr, src, jpeg="high", **shape, **kwargs)
            rates[name].append(rate)
            failed += bad
            good = [e for e in out if isinstance(e, tuple)]
            kinds[name] = {"group4_files": sum(getattr(e[-1], "bilevel", False) for e in good),
                           "bytes_per_page": round(statistics.mean(len(e[-1].data) for e in good))}
    result["legs"] = {name: {**ocr_serve_timing.summary(rates[name]), **kinds[name]} for name in legs}
    for name, (src, kwargs) in legs.items():
        stages = ocr_serve_timing.stage_busy(ocr, src, jpeg="high", **shape, **kwargs)["stages"]
        result["legs"][name]["render_stage"] = stages.get("render")
    off, none, two_off, two_on = (result["legs"][k] for k in ("off", "on_none", "two_off", "two_on"))
    result["conditions"] = {
        "switch_off_spread": off["spread"],
        "on_none_median_minus_off_median": round(none["median"] - off["median"], 2),
        "on_none_within_the_switch_off_spread": bool(off["median"] - none["median"] <= off["spread"]),
        "two_on_median_minus_two_off_median": round(two_on["median"] - two_off["median"], 2),
        "two_on_not_slower_than_two_off_by_more_than_the_spread": bool(two_off["median"] - two_on["median"] <= max(off["spread"], two_off["spread"])),
    }
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
