#!/usr/bin/env python3
"""What cutting and coding the figure crops on the device costs a job: bench.py's synthetic 1600 x 1200 pages with two figures
each - 400 x 300 and 800 x 600 pixels - through DocumentAnalyzer.serve (run by hand on the GPU, not by the suite).

    python tools/figures_serve_timing.py [--reps 3] [--wave 16] [--out profiles/figures_serve.json]

Device time: one wave of pages, 32 crops; HIP events around the crop launch (ymk_crop_u8) and around each of the encoder's three
launches on those crops (ymk_jpeg_coefficients / _entropy / _compact, quality 95, 4:2:0); median of `--event-reps` (20) after a
warm-up.  The crop launch moves the bytes the coefficient stage then reads.
Jobs: DocumentAnalyzer.serve pages/s with the switch off and on: one warm-up job per leg, then `reps` jobs per leg, the legs
alternating and each repetition starting with another leg; median and spread per leg.  bench.py's truth hand-over gives the
pages no figures, so the one used here adds the two boxes to every page's layout - in both legs: the aggregation sees the same
figures with the switch off."""
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

FIGURES = ((400, 300), (800, 600))  # (width, height) of the two figures of a page


def figure_boxes(h, w):
    """The two boxes on an h x w page: one below the other, clamped to the page."""
    out, y = [], 40
    for fw, fh in FIGURES:
        out.append([40, min(y, h - 1), min(40 + fw, w), min(y + fh, h)])
        y += fh + 40
    return out


def with_figures(handover_cls):
    from yomitoku_amd.schemas import Element, LayoutAnalyzerSchema

    class WithFigures(handover_cls):
        def layouts(self, wave, lays):
            out = []
            for (h, w), lay in zip(wave.sizes, super().layouts(wave, lays)):
                figures = [Element(id=None, box=b, score=1.0, role=None, contents=None) for b in figure_boxes(h, w)]
                out.append(LayoutAnalyzerSchema(paragraphs=lay.paragraphs, tables=lay.tables, figures=figures))
            return out

    return WithFigures


def stage_times(pages_dev, reps=20):
    """One wave of device pages: median device milliseconds of the crop launch and of the encoder's three launches on its crops."""
    from yomitoku_amd import _lib, figures, imaging
    from yomitoku_amd.jpeg import page_table, scratch_sizes

    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    rects = [[(b[0], b[1], b[2], b[3]) for b in figure_boxes(int(t.shape[0]), int(t.shape[1]))] for t in pages_dev]
    scratch = {}
    crops = figures.launch_crops(pages_dev, rects, scratch)  # sizes the buffer; the timed launches below reuse its table
    torch.cuda.synchronize()
    want = [t[y1:y2, x1:x2] for t, rs in zip(pages_dev, rects) for x1, y1, x2, y2 in rs]
    assert all(torch.equal(c, w) for c, w in zip(crops, want))
    dev = pages_dev[0].device
    recs, chunk = [], 0
    for t, rs in zip(pages_dev, rects):
        for x1, y1, x2, y2 in rs:
            rec = np.zeros(figures.CROP_WORDS, np.int32)
            rec[0:2] = figures.addr_words(t.data_ptr())
            rec[2:9] = (int(t.shape[0]), int(t.shape[1]), 3, x1, y1, x2 - x1, y2 - y1)
            rec[9:11] = figures.addr_words(crops[len(recs)].data_ptr())
            rec[11] = chunk
            chunk += -(-((y2 - y1) * (x2 - x1) * 3) // 16)
            recs.append(rec)
    crop_blob = np.concatenate(recs)
    crop_dev = imaging._stage_blob(crop_blob, dev)
    caps = [2 * c.numel() + figures.CAPACITY_ROOM for c in crops]
    blob, _, out_bytes = page_table(crops, 95, caps)
    mcus, blocks, intervals, coef_b, stream_b, iv_b = scratch_sizes([(int(c.shape[0]), int(c.shape[1]), 3) for c in crops])
    coef, bits, ivals, out, lengths = (torch.empty(n, dtype=torch.uint8, device=dev) for n in (coef_b, stream_b, iv_b, out_bytes, 4 * len(crops)))
    blob_dev = torch.from_numpy(blob).to(dev)
    names = ("crop", "coefficients", "entropy", "compact")
    times = {name: [] for name in names}
    for rep in range(reps + 1):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        torch.cuda.synchronize()
        marks[0].record()
        _lib.check(lib.ymk_crop_u8(crop_dev.data_ptr(), crop_blob.size, len(recs), chunk, stream))
        marks[1].record()
        _lib.check(lib.ymk_jpeg_coefficients(blob_dev.data_ptr(), blob.size, len(crops), mcus, coef.data_ptr(), blocks, stream))
        marks[2].record()
        _lib.check(lib.ymk_jpeg_entropy(blob_dev.data_ptr(), blob.size, len(crops), coef.data_ptr(), blocks, bits.data_ptr(), stream_b,
                                        ivals.data_ptr(), intervals, stream))
        marks[3].record()
        _lib.check(lib.ymk_jpeg_compact(blob_dev.data_ptr(), blob.size, len(crops), bits.data_ptr(), stream_b, blocks, ivals.data_ptr(),
                                        intervals, out.data_ptr(), out_bytes, lengths.data_ptr(), stream))
        marks[4].record()
        torch.cuda.synchronize()
        if rep:  # the first pass warms up
            for k, name in enumerate(names):
                times[name].append(marks[k].elapsed_time(marks[k + 1]))
    res = {k: round(statistics.median(v), 4) for k, v in times.items()}
    res["min"] = {k: round(min(v), 4) for k, v in times.items()}
    moved = sum(c.numel() for c in crops)
    res.update({"crops": len(crops), "crop_bytes": moved, "crop_gb_per_s_read_plus_written": round(2 * moved / (res["crop"] * 1e-3) / 1e9, 1),
                "file_bytes": int(lengths.view(torch.int32).clamp(min=0).sum().item()),
                "crop_below_coefficients": bool(res["crop"] < res["coefficients"])})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--event-reps", type=int, default=20)
    ap.add_argument("--wave", type=int, default=16)
    ap.add_argument("--in-flight", type=int, default=4)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--parent", nargs="+", help="results of this tool's --off-only run on the parent commit, made before and after this run")
    ap.add_argument("--off-only", action="store_true", help="the switch-off leg alone: what the parent commit can run")
    ap.add_argument("--result", help="a result of this tool to add --parent's comparison to: nothing is measured")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.result is None:
        result = measure(args)
    else:
        with open(args.result) as f:
            result = json.load(f)
    if args.parent:
        parents = []
        for path in args.parent:
            with open(path) as f:
                parents.append(json.load(f))
        mine, theirs = result["legs"]["off"], [p["legs"]["off"] for p in parents]
        medians = [t["median"] for t in theirs]
        # two processes of the SAME code differ by more than three jobs of one process do: the parent is run around this run
        result["off_against_parent"] = {"parent_runs": theirs, "parent_medians": medians, "off_median": mine["median"],
                                        "off_median_inside_the_parent_runs_range_widened_by_the_spreads":
                                            bool(min(medians) - max(t["spread"] for t in theirs) - mine["spread"] <= mine["median"])}
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


def measure(args):
    device = bench.rank_device(0)
    sds = bench.make_checkpoints("lite")
    sds = bench.calibrate_heads(sds, device, bench.Page(0, device))
    pages = bench.make_pages(list(range(args.pages)), device)
    host = [p.img for p in pages]
    doc = bench.build_analyzer(device, sds, "lite")
    doc.handover = with_figures(type(doc.handover))()
    doc.truth = pages
    shape = {"wave": args.wave, "in_flight": args.in_flight}
    result = {"pages_per_job": len(host), "reps": args.reps, **shape, "page": list(host[0].shape), "figures_per_page": [list(f) for f in FIGURES],
              "device": torch.cuda.get_device_name(0)}
    legs = {"off": {}} if args.off_only else {"off": {}, "on": {"figures": True}}
    if not args.off_only:
        result["device_ms_per_wave"] = stage_times([torch.from_numpy(img).to(device) for img in host[: args.wave]], args.event_reps)
    rates, failed, made = {name: [] for name in legs}, 0, {}
    for kwargs in legs.values():  # warm-up: shapes, workspaces, pinned rings, the render thread and its scratch
        doc.serve(host, **shape, **kwargs)
    for rep in range(args.reps):
        order = list(legs)[rep % len(legs) :] + list(legs)[: rep % len(legs)]
        for name in order:
            rate, bad, out = ocr_serve_timing.timed_job(doc, host, **shape, **legs[name])
            rates[name].append(rate)
            failed += bad
            if name == "on":
                files = [f for e in out if isinstance(e, tuple) for f in e[1]]
                made = {"files": len(files), "files_that_are_no_files": sum(not hasattr(f, "data") for f in files),
                        "bytes_per_page": round(sum(len(f.data) for f in files if hasattr(f, "data")) / max(len(out), 1))}
    result["legs"] = {name: ocr_serve_timing.summary(rates[name]) for name in legs}
    if "on" in legs:
        off, on = result["legs"]["off"], result["legs"]["on"]
        on.update(made)
        on["median_minus_off_median"] = round(on["median"] - off["median"], 2)
        on["within_the_switch_off_spread"] = bool(off["median"] - on["median"] <= off["spread"])
        on["ms_per_page_more_than_off"] = round(1e3 / on["median"] - 1e3 / off["median"], 3)
    result["failed_entries"] = failed
    bench.close_analyzer(doc)
    return result


if __name__ == "__main__":
    main()
