#!/usr/bin/env python3
"""What the device JPEG encoder saves a searchable-PDF job: bench.py's 64 synthetic 1600 x 1200 pages and its analyzer (run by
hand on the GPU, not by the suite).

    python tools/jpeg_serve_timing.py [--reps 3] [--wave 16] [--out profiles/jpeg_serve.json]
    python tools/jpeg_serve_timing.py --host-only --out FILE     # (c) and (a) alone; this form also runs when the file is copied
                                                                 # onto a checkout of the commit before the encoder

Legs, each one job over all pages, pages/s = pages / wall time, median over the repetitions, for the presets "high" and "low":
  (c) plain   serve(pages): the headline path, 2 x reps jobs as a block of their own before the other legs.
  (a) host    serve(pages), then searchable_pdf_bytes(pages, results, q) on the caller's thread: Pillow resizes and encodes.
              A preset whose PDF the tree's writer cannot make is recorded with the error instead of a rate (the writer before
              the encoder raised on a scale that leaves fractions: "low" at 1600 wide).
  (b) device  serve(pages, jpeg=q), then searchable_pdf_bytes(encoded, results): the files come out of the render stage.
(a) and (b) alternate within a repetition.
Also: the device time of the encoder's stages for one wave (HIP events around each C-ABI call, median of 10 after a warm-up; for
"low" the wall time of the Lanczos call), and bytes per page next to Pillow's own file for the same page."""
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


def stage_times(pages_dev, preset, reps=10):
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
    blob, _, out_bytes = page_table(small, p["jpeg_quality"])
    mcus, blocks, intervals, coef_b, stream_b, iv_b = scratch_sizes([(int(t.shape[0]), int(t.shape[1]), 3) for t in small])
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


def main():
    from yomitoku_amd.utils.searchable_pdf import IMAGE_QUALITY_PRESETS, searchable_pdf_bytes

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--wave", type=int, default=16)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--presets", default="high,low")
    ap.add_argument("--host-only", action="store_true", help="legs (c) and (a) alone: nothing of the encoder is imported, so this "
                    "file also runs on a checkout of the commit before the encoder")
    ap.add_argument("--out")
    args = ap.parse_args()
    device = bench.rank_device(0)
    sds = bench.make_checkpoints("lite")
    sds = bench.calibrate_heads(sds, device, bench.Page(0, device))
    pages = bench.make_pages(list(range(args.pages)), device)
    an = bench.build_analyzer(device, sds, "lite")
    an.truth = pages
    host = [p.img for p in pages]
    presets = [q for q in args.presets.split(",") if q]
    an.serve(host, wave=args.wave)  # warm-up: shapes, workspaces, pinned rings
    if not args.host_only:
        from yomitoku_amd.jpeg import encode_jpeg_pages

        for q in presets:  # the render thread, the wave slots' scratch, the Lanczos tables
            an.serve(host, wave=args.wave, jpeg=q)
    torch.cuda.synchronize()
    result = {"pages": args.pages, "wave": args.wave, "reps": args.reps, "device": torch.cuda.get_device_name(0),
              "legs": "c, a" if args.host_only else "c, a, b", "presets": {}}
    # (c) first, as a block of its own: nothing else between its jobs
    plain = []
    for _ in range(2 * args.reps):
        t0 = time.perf_counter()
        out = an.serve(host, wave=args.wave)
        torch.cuda.synchronize()
        plain.append(len(out) / (time.perf_counter() - t0))
    result["pages_per_s_plain"] = [round(v, 2) for v in plain]
    result["pages_per_s_plain_median"] = round(statistics.median(plain), 2)
    failed = 0
    for q in presets:
        rates = {"host": [], "device": []}
        pdf_bytes, host_error = {}, None
        for _ in range(args.reps):  # (a) and (b) in turn
            t0 = time.perf_counter()
            out = an.serve(host, wave=args.wave)
            good = [(img, e) for img, e in zip(host, out) if not isinstance(e, BaseException)]
            try:
                pdf_bytes["host"] = len(searchable_pdf_bytes([g[0] for g in good], [g[1] for g in good], q))
                rates["host"].append(len(out) / (time.perf_counter() - t0))
            except Exception as exc:  # noqa: BLE001 - recorded: the leg has no rate on a tree whose writer cannot make this PDF
                host_error = f"{type(exc).__name__}: {str(exc).splitlines()[0]}"
            if args.host_only:
                continue
            t0 = time.perf_counter()
            out = an.serve(host, wave=args.wave, jpeg=q)
            good = [e for e in out if isinstance(e, tuple)]
            pdf_bytes["device"] = len(searchable_pdf_bytes([e[1] for e in good], [e[0] for e in good]))
            rates["device"].append(len(out) / (time.perf_counter() - t0))
            failed += len(out) - len(good)
        entry = {"pages_per_s_host_jpeg": [round(v, 2) for v in rates["host"]], "host_jpeg_error": host_error, "pdf_bytes": pdf_bytes,
                 "pages_per_s_host_jpeg_median": round(statistics.median(rates["host"]), 2) if rates["host"] else None}
        if not args.host_only:
            preset = IMAGE_QUALITY_PRESETS[q]
            wave_dev = [torch.from_numpy(img).to(device) for img in host[: args.wave]]
            files = encode_jpeg_pages(wave_dev, q)
            pil_sizes = []
            for img in host[: args.wave]:
                image = Image.fromarray(np.ascontiguousarray(img[:, :, ::-1]))
                if preset["max_long_side"] is not None and max(image.size) > preset["max_long_side"]:
                    s = preset["max_long_side"] / max(image.size)
                    image = image.resize((int(image.size[0] * s), int(image.size[1] * s)), Image.LANCZOS)
                data = io.BytesIO()
                image.save(data, "JPEG", quality=preset["jpeg_quality"])
                pil_sizes.append(len(data.getvalue()))
            entry.update({
                "pages_per_s_device_jpeg": [round(v, 2) for v in rates["device"]],
                "pages_per_s_device_jpeg_median": round(statistics.median(rates["device"]), 2),
                "device_ms_per_wave": stage_times(wave_dev, q),
                "bytes_per_page_device": round(statistics.mean(len(f.data) for f in files)), "bytes_per_page_pillow": round(statistics.mean(pil_sizes)),
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
