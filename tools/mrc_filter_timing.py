#!/usr/bin/env python3
"""What filtering the ink masks of layered pages costs a job and what it saves in bytes (run by hand on the GPU, not by the
suite).

    python tools/mrc_filter_timing.py [--reps 3] [--wave 16] [--out profiles/mrc_filter_serve.json] [--parent parent.json ...]
    python tools/mrc_filter_timing.py --merge result.json --parent before.json after.json --bench ours.json parents.json --out ...

Pages: tests/golden/test_page.jpg (842 x 596, at the defaults and at `side` 48), the noisy golden page of tests/despeckle_ref.py
tiled to 1600 x 1200, and bench.py's first synthetic 1600 x 1200 page, both at the defaults.
Bytes: mask, foreground and background of each page with neither switch, with each alone and with both.
Device time: a wave of 16 copies of the page; its ink by the separation's own launches; HIP events around each of the twelve
launches the filter adds (ymk_cc_stage for the two colours, ymk_cc_filter_stage for the blob pass; median of 10 after a warm-up,
each repetition on a fresh copy of the ink), around the whole entry, and - next to them - around the separation behind it
(ymk_mrc_pages on the caller's ink: cells, pull, flags, push) and the Group 4 row coder on the filtered rows.  Two more inks, for the
boxes kernel alone: the bench page's ink with a frame and a grid drawn through it - one component as large as the page -, and a
page that is all ink.
Jobs: pages/s of OCR.serve(jpeg="high", jpeg_mrc=...) on bench.py's pages with jpeg_mrc=True ("off": neither switch) and with
both switches at their defaults ("on"): one warm-up job per leg, then `reps` jobs per leg, the legs alternating and each
repetition starting with another leg; median and spread per leg.
--parent: results of tools/mrc_serve_timing.py made on the parent commit in the same session, before and after this run (its leg
"on" is this tool's "off" job): the off leg against the parent's run-to-run range.
--bench: files with the JSON line of `python bench.py --gpus 1`, this commit's and the parent's in turn, quoted as they are:
bench.py runs none of this code."""
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
STAGES = ("label", "merge", "areas", "apply")
BLOB_STAGES = ("label", "merge", "boxes", "apply")
BOTH = {"despeckle": True, "blobs": True}


def file_bytes(page, switches):
    """bytes of the three files of a page per set of switches, and what the filter removed"""
    from yomitoku_amd.jpeg import encode_jpeg_pages

    out = {"shape": list(page.shape)}
    for name, mrc in switches.items():
        got = encode_jpeg_pages([page], "high", mrc=mrc)[0]
        if getattr(got, "mrc", False) is not True:
            out[name] = {"plain_jpeg": len(got.data)}
            continue
        d = got.mask.despeckled
        out[name] = {"mask": len(got.mask.data), "foreground": len(got.foreground.data), "background": len(got.background.data), "total": got.nbytes}
        if d is not None:
            out[name]["removed"] = {k: getattr(d, k) for k in ("black_components", "black_pixels", "white_components", "white_pixels",
                                                               "blob_components", "blob_pixels")}
    return out


class _Rows:
    """packed rows of pages of one shape, one page behind the other: what despeckle.launch_filter and ccitt.launch_encode read"""

    def __init__(self, pages, packed, packed_at, packed_bytes):
        self.pages, self.packed, self.packed_at, self.packed_bytes = pages, packed, packed_at, packed_bytes


def _ink_of(pages_dev, params):
    """the pages' ink as the separation makes it, and the separation's buffers"""
    from yomitoku_amd.mrc import launch

    done = launch(pages_dev, params, {})
    torch.cuda.synchronize()
    return done


def filter_times(rows, filt, reps=10, separation=None):
    """median device milliseconds of the filter's launches on `rows` (a _Rows or a finished separation), of its entry, and of the
    launches it sits next to.  filt: {"black", "white", "side", "fill"}.  separation: a function that queues ymk_mrc_pages on the
    rows as they are, or None."""
    from yomitoku_amd import _lib, ccitt, despeckle

    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    pages = rows.pages
    dev, n = rows.packed.device, len(pages)
    shapes = [(int(t.shape[0]), int(t.shape[1])) for t in pages]
    blob = despeckle.page_table(shapes, rows.packed_at)
    label_b, area_b, box_b = despeckle.filter_scratch_sizes(shapes)
    labels, areas, boxes = (torch.empty(b // 4, dtype=torch.int32, device=dev) for b in (label_b, area_b, box_b))
    counts = torch.zeros(6 * n, dtype=torch.int32, device=dev)
    blob_dev = torch.from_numpy(blob.reshape(-1)).to(dev)
    tall, wide = max(h for h, _ in shapes), max(w for _, w in shapes)
    table = (blob_dev.data_ptr(), blob.size, n, tall, wide)
    two = (rows.packed.data_ptr(), rows.packed_bytes, labels.data_ptr(), label_b, areas.data_ptr(), area_b)
    rows0 = rows.packed.clone()
    g4_blob, _, _, out_bytes = ccitt.page_table(pages, rows.packed_at)
    total_rows, _, slot_b, bits_b, _ = ccitt.scratch_sizes([t.shape for t in pages])
    slots, rowbits = (torch.empty(max(b, 8), dtype=torch.uint8, device=dev) for b in (slot_b, bits_b))
    g4_dev = torch.from_numpy(g4_blob).to(dev)

    def code_rows():
        _lib.check(lib.ymk_g4_code_rows(g4_dev.data_ptr(), g4_blob.size, n, total_rows, tall, rows.packed.data_ptr(), rows.packed_bytes, slots.data_ptr(),
                                        slot_b, out_bytes, rowbits.data_ptr(), stream))

    calls = [("group4_code_rows_before", code_rows)]
    for white, colour, size in ((0, "black", filt["black"]), (1, "white", filt["white"])):
        if size:
            for k, stage in enumerate(STAGES):
                calls.append((f"{colour}_{stage}", lambda k=k, white=white, size=size: _lib.check(
                    lib.ymk_cc_stage(k, white, *table, *two, size, counts.data_ptr(), stream))))
    if filt["side"]:
        for k, stage in enumerate(BLOB_STAGES):
            calls.append((f"blob_{stage}", lambda k=k: _lib.check(
                lib.ymk_cc_filter_stage(k, *table, *two, boxes.data_ptr(), box_b, filt["side"], filt["fill"], counts.data_ptr(), stream))))
    added = [name for name, _ in calls[1:]]
    if separation is not None:
        calls.append(("separation_cells_pull_flags_push", separation))
    calls.append(("group4_code_rows_after", code_rows))
    times = {name: [] for name, _ in calls}
    times["entry"] = []
    for rep in range(reps + 1):
        rows.packed.copy_(rows0)
        counts.zero_()
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
        torch.cuda.synchronize()
        marks[0].record()
        for k, (_, call) in enumerate(calls):
            call()
            marks[k + 1].record()
        torch.cuda.synchronize()
        staged = rows.packed.clone()
        rows.packed.copy_(rows0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        _lib.check(lib.ymk_cc_filter_pages(*table, *two, boxes.data_ptr(), box_b, filt["black"], filt["white"], filt["side"], filt["fill"],
                                           counts.data_ptr(), stream))
        b.record()
        torch.cuda.synchronize()
        assert torch.equal(staged, rows.packed)  # the stages in order are the entry; the counts below are the entry's
        if rep:  # the first pass warms up
            for k, (name, _) in enumerate(calls):
                times[name].append(marks[k].elapsed_time(marks[k + 1]))
            times["entry"].append(a.elapsed_time(b))
    out = {k: round(statistics.median(v), 3) for k, v in times.items()}
    out["sum_of_the_added_launches"] = round(sum(out[k] for k in added), 3)
    out["largest_added_launch"] = max(added, key=lambda k: out[k])
    six = counts.view(-1, 6).sum(0).tolist()
    out["removed_per_wave"] = dict(zip(("black_components", "black_pixels", "white_components", "white_pixels", "blob_components", "blob_pixels"), six))
    out["scratch_mib"] = {"labels": round(label_b / 2**20, 1), "areas": round(area_b / 2**20, 1), "boxes": round(box_b / 2**20, 1)}
    rows.packed.copy_(rows0)
    return out


def page_times(page, mrc, wave):
    """a wave of copies of `page`: the filter's launches on its ink, next to the separation and the row coder"""
    from yomitoku_amd import _lib, despeckle
    from yomitoku_amd.mrc import check_mrc

    params = check_mrc(mrc)
    dev = torch.device("cuda", torch.cuda.current_device())
    pages_dev = [torch.from_numpy(page).to(dev) for _ in range(wave)]
    cells = {k: params[k] for k in ("bg_cell", "fg_cell")}
    done = _ink_of(pages_dev, cells)
    lib, n = _lib.load(), len(pages_dev)
    stream = torch.cuda.current_stream().cuda_stream
    luma_b, sat_b, packed_b, pyr_b, layers_b = done.buffers["sizes"]
    blob, pyr, flags = done.buffers["blob"], done.buffers["pyramids"], done.buffers["flags"]
    tall, wide = int(page.shape[0]), int(page.shape[1])

    def separation():
        _lib.check(lib.ymk_mrc_pages(blob.data_ptr(), n * 16, n, tall, wide, cells["bg_cell"], cells["fg_cell"], None, luma_b, None, sat_b,
                                     done.packed.data_ptr(), packed_b, None, pyr.data_ptr(), pyr_b, done.layers.data_ptr(), layers_b, flags.data_ptr(),
                                     stream))

    filt = despeckle.filter_params(params.get("despeckle"), params.get("blobs"))
    out = filter_times(done, filt, separation=separation)
    out["params"] = filt
    return out


def ink_times(mask, filt, wave):
    """the filter alone on a wave of copies of a bool mask"""
    from yomitoku_amd import despeckle

    dev = torch.device("cuda", torch.cuda.current_device())
    test = despeckle._Masks([torch.from_numpy(mask).to(dev)] * wave, dev)
    return filter_times(_Rows(test.pages, test.packed, test.packed_at, test.packed_bytes), filt)


def against_parent(result, paths):
    """the off leg against the parent commit's runs of the same job (tools/mrc_serve_timing.py there: its leg "on")"""
    if not paths:
        return
    theirs = []
    for path in paths:
        with open(path) as f:
            theirs.append(json.load(f)["legs"]["ocr_jpeg_high"]["on"])
    off = result["legs"]["off"]
    medians = [t["median"] for t in theirs]
    spread = max(t["spread"] for t in theirs)
    result["off_against_parent"] = {"parent_runs": [{k: t[k] for k in ("median", "spread", "rates") if k in t} for t in theirs],
                                    "parent_medians": medians, "parent_run_to_run_range": round(max(medians) - min(medians), 2),
                                    "parent_largest_spread_within_a_run": spread, "off_median": off["median"],
                                    "off_median_inside_the_parent_runs_range_widened_by_the_spreads":
                                        bool(min(medians) - spread - off["spread"] <= off["median"] <= max(medians) + spread + off["spread"])}


def bench_lines(result, paths):
    if not paths:
        return
    result["bench_py"] = {"this_commit": [], "parent_commit": []}  # the files in turn: this commit's, the parent's, this commit's, ...
    for k, path in enumerate(paths):
        with open(path) as f:
            lines = [json.loads(line) for line in f if line.lstrip().startswith("{")]
        line = {key: lines[-1].get(key) for key in ("metric", "value", "unit", "steps", "warmup", "ms_per_step")} if lines else None
        result["bench_py"]["parent_commit" if k % 2 else "this_commit"].append(line)


def earlier_form(result, path):
    """the two page-sized inks as a result of this tool had them with the boxes launch in its first form: one thread per pixel and
    one global add per run of lanes, and the blob apply launch without its count per block"""
    if not path:
        return
    with open(path) as f:
        old = json.load(f)["device_ms_per_wave"]
    result["page_sized_inks_with_the_first_form_of_the_boxes_and_apply_launches"] = {
        k: {s: old[k][s] for s in ("blob_label", "blob_merge", "blob_boxes", "blob_apply", "entry")} for k in ("bench_ink_with_a_frame_and_a_grid", "all_ink")}


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
    ap.add_argument("--parent", nargs="+", help="results of tools/mrc_serve_timing.py on the parent commit, made before and after this run")
    ap.add_argument("--bench", nargs="+", help="the output of bench.py on this commit and on the parent")
    ap.add_argument("--earlier", help="a result of this tool made with the first form of the boxes launch: its page-sized inks are quoted")
    ap.add_argument("--merge", help="a result of this tool: only hold its off leg against --parent, add --bench and write it to --out")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.merge:
        with open(args.merge) as f:
            result = json.load(f)
        against_parent(result, args.parent)
        bench_lines(result, args.bench)
        earlier_form(result, args.earlier)
        return write(result, args.out)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import despeckle_ref

    device = bench.rank_device(0)
    sds = bench.make_checkpoints("lite")
    sds = bench.calibrate_heads(sds, device, bench.Page(0, device))
    pages = bench.make_pages(list(range(args.pages)), device)
    host = [p.img for p in pages]
    golden = np.ascontiguousarray(np.asarray(Image.open(GOLDEN).convert("RGB"))[:, :, ::-1])
    noisy = despeckle_ref.noisy_page(despeckle_ref.golden_page(GOLDEN))
    tiled = np.ascontiguousarray(np.tile(noisy, (2, 3))[:1600, :1200])
    shape = {"wave": args.wave, "in_flight": args.in_flight}
    result = {"pages_per_job": len(host), "reps": args.reps, **shape, "device": torch.cuda.get_device_name(0),
              "for_scale_ms_per_wave": {"separation_in_profiles_mrc_serve": 0.40, "row_coder_in_profiles_ccitt_serve": 0.876}}
    switches = {"neither": True, "despeckle": {"despeckle": True}, "blobs": {"blobs": True}, "both": BOTH}
    at_48 = {"blobs_side_48": {"blobs": {"side": 48}}, "both_side_48": {"despeckle": True, "blobs": {"side": 48}}}
    result["file_bytes"] = {"golden_page": file_bytes(golden, {**switches, **at_48}), "noisy_golden_page_tiled": file_bytes(tiled, switches),
                            "bench_page": file_bytes(host[0], switches)}
    times = {"golden_page": page_times(golden, BOTH, args.wave), "golden_page_side_48": page_times(golden, at_48["both_side_48"], args.wave),
             "noisy_golden_page_tiled": page_times(tiled, BOTH, args.wave), "bench_page": page_times(host[0], BOTH, args.wave)}
    # one component as large as the page: the bench page's ink with a frame and a grid of 3-pixel lines every 100 pixels; all ink
    from yomitoku_amd.despeckle import unpack_rows

    done = _ink_of([torch.from_numpy(host[0]).to(device)], {"bg_cell": 2, "fg_cell": 8})
    ink = unpack_rows(done.mask_rows(0), host[0].shape[1]).cpu().numpy()
    grid = ink.copy()
    for k in range(0, max(grid.shape), 100):
        grid[k : k + 3, :] = True
        grid[:, k : k + 3] = True
    grid[-3:, :] = True
    grid[:, -3:] = True
    defaults = {"black": 4, "white": 4, "side": 128, "fill": 64}
    times["bench_ink_with_a_frame_and_a_grid"] = ink_times(grid, defaults, args.wave)
    times["all_ink"] = ink_times(np.ones(grid.shape, bool), defaults, args.wave)
    result["device_ms_per_wave"] = times
    ocr = ocr_serve_timing.build_ocr(device, sds, pages)
    legs = {"off": {"jpeg": "high", "jpeg_mrc": True}, "on": {"jpeg": "high", "jpeg_mrc": BOTH}}
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
    result["legs"] = {name: {**ocr_serve_timing.summary(rates[name]), **kinds[name]} for name in legs}
    off, on = result["legs"]["off"], result["legs"]["on"]
    on["median_minus_off_median"] = round(on["median"] - off["median"], 2)
    on["within_the_switch_off_spread"] = bool(off["median"] - on["median"] <= off["spread"])
    on["ms_per_page_more_than_off"] = round(1e3 / on["median"] - 1e3 / off["median"], 3)
    result["failed_entries"] = failed
    against_parent(result, args.parent)
    bench_lines(result, args.bench)
    earlier_form(result, args.earlier)
    ocr.close()
    write(result, args.out)


if __name__ == "__main__":
    main()
