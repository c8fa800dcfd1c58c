#!/usr/bin/env python3
"""What the device JPEG encoder saves a searchable-PDF job: bench.py's 64 synthetic 1600 x 1200 pages and its analyzer (run by
hand on the GPU, not by the suite).

    python tools/jpeg_serve_timing.py [--reps 3] [--wave 16] [--out profiles/jpeg_serve.json]
    python tools/jpeg_serve_timing.py --host-only --out FILE     # (c) and (a) alone; this form also runs when the file is copied
                                                                 # onto a checkout of the commit before the encoder
    python tools/jpeg_serve_timing.py --optimize --legs b --presets high --out profiles/jpeg_serve_optimized.json
                                                                 # (b) next to (o); without --optimize this form also runs on
                                                                 # a checkout of the commit before the optimised tables
    python tools/jpeg_serve_timing.py --legs b --presets high --subsampling 4:4:4 [--grey auto] [--grey-pages] --out FILE
                                                                 # (b) in another mode of the encoder; tools/jobs/jpeg_serve_modes.sh
                                                                 # runs the modes one after the other -> profiles/jpeg_serve_modes.json.
                                                                 # Without the three options this form also runs on a checkout
                                                                 # of the commit before the modes

Legs, each one job over all pages, pages/s = pages / wall time, median over the repetitions, for the presets "high" and "low":
  (c) plain   serve(pages): the headline path, 2 x reps jobs as a block of their own before the other legs.
  (a) host    serve(pages), then searchable_pdf_bytes(pages, results, q) on the caller's thread: Pillow resizes and encodes.
              A preset whose PDF the tree's writer cannot make is recorded with the error instead of a rate (the writer before
              the encoder raised on a scale that leaves fractions: "low" at 1600 wide).
  (b) device  serve(pages, jpeg=q), then searchable_pdf_bytes(encoded, results): the files come out of the render stage.
  (o) optimised  --optimize: (b) with jpeg_optimize=True - Huffman tables made for each page.
(a), (b) and (o) alternate within a repetition; --legs picks among c, a, b.
Also: the device time of the encoder's stages for one wave (HIP events around each C-ABI call, median of 10 after a warm-up; for
"low" the wall time of the Lanczos call), and bytes per page next to Pillow's own file for the same page; with --optimize the five
stages of the optimised path and the bytes of its files next to Pillow's `optimize=True` as well.
--subsampling / --grey: legs (b) and (o) and the stage times in that mode of the encoder (serve(jpeg_subsampling=, jpeg_grey=)); with
--grey auto the grey test's launch is timed as a stage of its own.  --grey-pages: the job's pages are made grey-valued (B = G = R =
the page's green plane) before anything runs - what a black-and-white scan is when load_image hands it over."""
import argparse
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # as `import yomitoku_amd` does and bench.py too: torch is imported first here
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import bench  # noqa: E402


def mode_kwargs(args, serve=True):
    """The keywords of --subsampling / --grey for serve() or encode_jpeg_pages(); none at the defaults (so that the tool also runs
    on a tree before the modes)."""
    out = {}
    if args.subsampling != "4:2:0":
        out["jpeg_subsampling" if serve else "subsampling"] = args.subsampling
    if args.grey != "off":
        out["jpeg_grey" if serve else "grey"] = args.grey
    return out


def page_modes(pages_dev, subsampling, grey, times=None, reps=10):
    """Word 15 of every page's record, as encode_jpeg_pages chooses it (None at the defaults); with grey "auto" the grey test's
    launch goes into times["grey_test"] (device milliseconds, HIP events around the C-ABI call)."""
    if subsampling == "4:2:0" and grey == "off":
        return None
    from yomitoku_amd import _lib, imaging
    from yomitoku_amd.jpeg import MODE_GREY, PAGE_WORDS, SUBSAMPLINGS, _addr_words, grey_pages

    as_grey = [False] * len(pages_dev)
    if grey == "auto":
        as_grey = grey_pages(pages_dev)
        rec = np.zeros((len(pages_dev), PAGE_WORDS), np.int32)
        for k, t in enumerate(pages_dev):
            rec[k, 0:2] = _addr_words(t.data_ptr())
            rec[k, 2:5] = (int(t.shape[0]), int(t.shape[1]), 3)
        blob_dev = imaging._stage_blob(rec.reshape(-1), pages_dev[0].device)
        diff = torch.empty(len(pages_dev), dtype=torch.int32, device=pages_dev[0].device)
        most = max(int(t.shape[0]) * int(t.shape[1]) for t in pages_dev)
        for rep in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            _lib.check(_lib.load().ymk_jpeg_pages_grey(blob_dev.data_ptr(), rec.size, len(pages_dev), most, diff.data_ptr(),
                                                       torch.cuda.current_stream().cuda_stream))
            b.record()
            torch.cuda.synchronize()
            if rep and times is not None:
                times.setdefault("grey_test", []).append(a.elapsed_time(b))
    return [MODE_GREY if g else SUBSAMPLINGS[subsampling] for g in as_grey]


def stage_times(pages_dev, preset, reps=10, subsampling="4:2:0", grey="off"):
    """One wave of device pages: median device milliseconds of the three encoder stages (HIP events around each C-ABI call),
    and - for a preset that shrinks - the wall time of the whole Lanczos call, host part (blob, upload) and wait included."""
    from yomitoku_amd import _lib
    from yomitoku_amd.jpeg import jpeg_preset, page_table, resize_pages, scratch_sizes

    lib, p = _lib.load(), jpeg_preset(preset)
    stream = torch.cuda.current_stream().cuda_stream
    times = {"resize_call_wall": [], "coefficients": [], "entropy": [], "compact": []}
    small = pages_dev
    if p["max_long_side"] is not None:
        sizes = []
        for t in pages_dev:
            h, w = int(t.shape[0]), int(t.shape[1])
            s = min(1.0, p["max_long_side"] / max(h, w))
            sizes.append((int(h * s), int(w * s)))
        for rep in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            small = resize_pages(pages_dev, sizes)
            torch.cuda.synchronize()
            if rep:  # the first pass builds the coefficient tables
                times["resize_call_wall"].append((time.perf_counter() - t0) * 1e3)
    modes = page_modes(small, subsampling, grey, times, reps)
    mode_kw = {} if modes is None else {"modes": modes}
    blob, _, out_bytes = page_table(small, p["jpeg_quality"], **mode_kw)
    mcus, blocks, intervals, coef_b, stream_b, iv_b = scratch_sizes([(int(t.shape[0]), int(t.shape[1]), 3) for t in small], **mode_kw)
    dev = small[0].device
    coef, bits, ivals, out, lengths = (torch.empty(n, dtype=torch.uint8, device=dev) for n in (coef_b, stream_b, iv_b, out_bytes, 4 * len(small)))
    blob_dev = torch.from_numpy(blob).to(dev)
    for rep in range(reps + 1):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        marks[0].record()
        _lib.check(lib.ymk_jpeg_coefficients(blob_dev.data_ptr(), blob.size, len(small), mcus, coef.data_ptr(), blocks, stream))
        marks[1].record()
        _lib.check(lib.ymk_jpeg_entropy(blob_dev.data_ptr(), blob.size, len(small), coef.data_ptr(), blocks, bits.data_ptr(), stream_b,
                                        ivals.data_ptr(), intervals, stream))
        marks[2].record()
        _lib.check(lib.ymk_jpeg_compact(blob_dev.data_ptr(), blob.size, len(small), bits.data_ptr(), stream_b, blocks, ivals.data_ptr(),
                                        intervals, out.data_ptr(), out_bytes, lengths.data_ptr(), stream))
        marks[3].record()
        torch.cuda.synchronize()
        if rep:  # the first pass warms up
            for k, name in enumerate(("coefficients", "entropy", "compact")):
                times[name].append(marks[k].elapsed_time(marks[k + 1]))
    return {k: round(statistics.median(v), 3) for k, v in times.items() if v}


def stage_times_optimized(pages_dev, preset, reps=10, subsampling="4:2:0", grey="off"):
    """stage_times for the five stages of the optimised path (the preset's shrink is not repeated here)."""
    from yomitoku_amd import _lib
    from yomitoku_amd.jpeg import jpeg_preset, page_table, resize_pages, scratch_sizes

    lib, p = _lib.load(), jpeg_preset(preset)
    stream = torch.cuda.current_stream().cuda_stream
    small = pages_dev
    if p["max_long_side"] is not None:
        sizes = []
        for t in pages_dev:
            h, w = int(t.shape[0]), int(t.shape[1])
            s = min(1.0, p["max_long_side"] / max(h, w))
            sizes.append((int(h * s), int(w * s)))
        small = resize_pages(pages_dev, sizes)
    n = len(small)
    modes = page_modes(small, subsampling, grey)
    mode_kw = {} if modes is None else {"modes": modes}
    blob, _, out_bytes = page_table(small, p["jpeg_quality"], optimize=True, **mode_kw)
    sized = scratch_sizes([(int(t.shape[0]), int(t.shape[1]), 3) for t in small], optimize=True, **mode_kw)
    mcus, blocks, intervals, coef_b, stream_b, iv_b, hist_b, tables_b, dht_b = sized
    dev = small[0].device
    coef, bits, ivals, hist, tables, dht, out, lengths = (torch.empty(b, dtype=torch.uint8, device=dev)
                                                          for b in (coef_b, stream_b, iv_b, hist_b, tables_b, dht_b, out_bytes, 4 * n))
    blob_dev = torch.from_numpy(blob).to(dev)
    table = (blob_dev.data_ptr(), blob.size, n)
    names = ("coefficients", "histogram", "optimal_tables", "entropy", "compact")
    times = {k: [] for k in names}
    for rep in range(reps + 1):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        torch.cuda.synchronize()
        marks[0].record()
        _lib.check(lib.ymk_jpeg_coefficients(*table, mcus, coef.data_ptr(), blocks, stream))
        marks[1].record()
        _lib.check(lib.ymk_jpeg_histogram(*table, coef.data_ptr(), blocks, intervals, hist.data_ptr(), stream))
        marks[2].record()
        _lib.check(lib.ymk_jpeg_optimal_tables(*table, hist.data_ptr(), tables.data_ptr(), dht.data_ptr(), stream))
        marks[3].record()
        _lib.check(lib.ymk_jpeg_entropy_opt(*table, coef.data_ptr(), blocks, tables.data_ptr(), bits.data_ptr(), stream_b, ivals.data_ptr(),
                                            intervals, stream))
        marks[4].record()
        _lib.check(lib.ymk_jpeg_compact_opt(*table, bits.data_ptr(), stream_b, blocks, ivals.data_ptr(), intervals, dht.data_ptr(),
                                            out.data_ptr(), out_bytes, lengths.data_ptr(), stream))
        marks[5].record()
        torch.cuda.synchronize()
        if rep:  # the first pass warms up
            for k, name in enumerate(names):
                times[name].append(marks[k].elapsed_time(marks[k + 1]))
    return {k: round(statistics.median(v), 3) for k, v in times.items()}


def main():
    from yomitoku_amd.utils.searchable_pdf import IMAGE_QUALITY_PRESETS, searchable_pdf_bytes

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--wave", type=int, default=16)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--presets", default="high,low")
    ap.add_argument("--host-only", action="store_true", help="legs (c) and (a) alone: nothing of the encoder is imported, so this "
                    "file also runs on a checkout of the commit before the encoder")
    ap.add_argument("--optimize", action="store_true", help="leg (o) next to (b), the optimised path's stage times and file sizes")
    ap.add_argument("--legs", default="c,a,b", help="which of the legs c, a, b to run (default: all three)")
    ap.add_argument("--subsampling", default="4:2:0", choices=["4:2:0", "4:2:2", "4:4:4"], help="the chroma of the device's colour files")
    ap.add_argument("--grey", default="off", choices=["off", "auto"], help="auto: grey-valued pages become grey files (one more launch and wait)")
    ap.add_argument("--grey-pages", action="store_true", help="make every page grey-valued (B = G = R) first")
    ap.add_argument("--out")
    args = ap.parse_args()
    device = bench.rank_device(0)
    sds = bench.make_checkpoints("lite")
    sds = bench.calibrate_heads(sds, device, bench.Page(0, device))
    pages = bench.make_pages(list(range(args.pages)), device)
    an = bench.build_analyzer(device, sds, "lite")
    an.truth = pages
    host = [p.img for p in pages]
    if args.grey_pages:
        host = [np.ascontiguousarray(np.stack([img[..., 1]] * 3, -1)) for img in host]
    presets = [q for q in args.presets.split(",") if q]
    legs = {"c", "a"} if args.host_only else {leg for leg in args.legs.split(",") if leg}
    if args.optimize and "b" not in legs:
        ap.error("--optimize measures (o) next to (b): --legs must name b")
    an.serve(host, wave=args.wave)  # warm-up: shapes, workspaces, pinned rings
    if "b" in legs:
        from yomitoku_amd.jpeg import encode_jpeg_pages

        for q in presets:  # the render thread, the wave slots' scratch, the Lanczos tables
            an.serve(host, wave=args.wave, jpeg=q, **mode_kwargs(args))
            if args.optimize:
                an.serve(host, wave=args.wave, jpeg=q, jpeg_optimize=True, **mode_kwargs(args))
    torch.cuda.synchronize()
    result = {"pages": args.pages, "wave": args.wave, "reps": args.reps, "device": torch.cuda.get_device_name(0),
              "legs": ", ".join(sorted(legs, key="cab".index)) + (", o" if args.optimize else ""), "presets": {}}
    if mode_kwargs(args) or args.grey_pages:
        result.update({"subsampling": args.subsampling, "grey": args.grey, "grey_pages": args.grey_pages})
    # (c) first, as a block of its own: nothing else between its jobs
    plain = []
    for _ in range(2 * args.reps if "c" in legs else 0):
        t0 = time.perf_counter()
        out = an.serve(host, wave=args.wave)
        torch.cuda.synchronize()
        plain.append(len(out) / (time.perf_counter() - t0))
    result["pages_per_s_plain"] = [round(v, 2) for v in plain]
    result["pages_per_s_plain_median"] = round(statistics.median(plain), 2) if plain else None
    failed = 0
    for q in presets:
        rates = {"host": [], "device": [], "optimized": []}
        pdf_bytes, host_error = {}, None
        for _ in range(args.reps):  # (a), (b) and (o) in turn
            if "a" in legs:
                t0 = time.perf_counter()
                out = an.serve(host, wave=args.wave)
                good = [(img, e) for img, e in zip(host, out) if not isinstance(e, BaseException)]
                try:
                    pdf_bytes["host"] = len(searchable_pdf_bytes([g[0] for g in good], [g[1] for g in good], q))
                    rates["host"].append(len(out) / (time.perf_counter() - t0))
                except Exception as exc:  # noqa: BLE001 - recorded: the leg has no rate on a tree whose writer cannot make this PDF
                    host_error = f"{type(exc).__name__}: {str(exc).splitlines()[0]}"
            for name, kwargs in (("device", {}), ("optimized", {"jpeg_optimize": True})):
                if "b" not in legs or (name == "optimized" and not args.optimize):
                    continue
                t0 = time.perf_counter()
                out = an.serve(host, wave=args.wave, jpeg=q, **kwargs, **mode_kwargs(args))
                good = [e for e in out if isinstance(e, tuple)]
                pdf_bytes[name] = len(searchable_pdf_bytes([e[1] for e in good], [e[0] for e in good]))
                rates[name].append(len(out) / (time.perf_counter() - t0))
                failed += len(out) - len(good)
        entry = {"pages_per_s_host_jpeg": [round(v, 2) for v in rates["host"]], "host_jpeg_error": host_error, "pdf_bytes": pdf_bytes,
                 "pages_per_s_host_jpeg_median": round(statistics.median(rates["host"]), 2) if rates["host"] else None}
        if "b" in legs:
            preset = IMAGE_QUALITY_PRESETS[q]
            wave_dev = [torch.from_numpy(img).to(device) for img in host[: args.wave]]
            files = encode_jpeg_pages(wave_dev, q, **mode_kwargs(args, serve=False))
            pil_sizes, pil_opt_sizes = [], []
            pil_kw = {} if args.subsampling == "4:2:0" else {"subsampling": args.subsampling}  # Pillow's file in the same mode
            for img in host[: args.wave]:
                image = Image.fromarray(np.ascontiguousarray(img[:, :, ::-1]))
                if args.grey == "auto" and args.grey_pages:
                    image, pil_kw = image.convert("L"), {}
                if preset["max_long_side"] is not None and max(image.size) > preset["max_long_side"]:
                    s = preset["max_long_side"] / max(image.size)
                    image = image.resize((int(image.size[0] * s), int(image.size[1] * s)), Image.LANCZOS)
                data = io.BytesIO()
                image.save(data, "JPEG", quality=preset["jpeg_quality"], **pil_kw)
                pil_sizes.append(len(data.getvalue()))
                if args.optimize:
                    data = io.BytesIO()
                    image.save(data, "JPEG", quality=preset["jpeg_quality"], optimize=True, **pil_kw)
                    pil_opt_sizes.append(len(data.getvalue()))
            entry.update({
                "pages_per_s_device_jpeg": [round(v, 2) for v in rates["device"]],
                "pages_per_s_device_jpeg_median": round(statistics.median(rates["device"]), 2),
                "device_ms_per_wave": stage_times(wave_dev, q, **({"subsampling": args.subsampling, "grey": args.grey} if mode_kwargs(args) else {})),
                "bytes_per_page_device": round(statistics.mean(len(f.data) for f in files)), "bytes_per_page_pillow": round(statistics.mean(pil_sizes)),
            })
            if args.optimize:
                files = encode_jpeg_pages(wave_dev, q, optimize=True, **mode_kwargs(args, serve=False))
                entry.update({
                    "pages_per_s_optimized_jpeg": [round(v, 2) for v in rates["optimized"]],
                    "pages_per_s_optimized_jpeg_median": round(statistics.median(rates["optimized"]), 2),
                    "optimized_ms_per_wave": stage_times_optimized(wave_dev, q, **({"subsampling": args.subsampling, "grey": args.grey} if mode_kwargs(args) else {})),
                    "bytes_per_page_optimized": round(statistics.mean(len(f.data) for f in files)),
                    "bytes_per_page_pillow_optimize": round(statistics.mean(pil_opt_sizes)),
                })
        result["presets"][q] = entry
    result["failed_entries"] = failed
    an.close()
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
