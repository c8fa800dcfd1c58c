#!/usr/bin/env python3
"""What a visualize=True overlay costs, for profiles/visualize_overlay.json (run by hand on the GPU, not by the suite).

    python tools/overlay_timing.py [--out FILE]
    python tools/overlay_timing.py --wave [--out FILE]    the wave renderer, for profiles/visualize_overlay_wave.json (wave_leg)
    python tools/overlay_timing.py --tables [--out FILE]  a form page with tinted tables, as parse_pages(overlays=True) draws it (tables_leg)

One 1600 x 1200 page carrying 300 quads (closed polylines, t = 1), 300 labelled boxes (outline t = 2 + a 12 px label) and 300
text lines of 20 characters (18 px).  Reported, each the median of 20 runs after 3 warm-ups, one process, nothing else on the card:
  draw_overlay_device_ms   ymk_draw_overlay alone, HIP events around the launch
  build_and_bin_host_ms    building the command list, the atlas and the per-tile lists on the host
  render_wall_ms           Overlay.render on a device page: build + one H2D blob + clone + launch, host clock to a synchronise
  d2h_ms                   the finished image to a host array
  pillow_host_ms           Pillow's ImageDraw drawing the same content on a host copy of the page - how the reference draws
Built-in font on both sides, so the glyph work is the same."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, N, CHARS = 1600, 1200, 300, 20
RUNS, WARMUP = 20, 3


def content(seed=0):
    import numpy as np

    rng = np.random.default_rng(seed)
    x, y = rng.integers(0, W - 260, N), rng.integers(20, H - 40, N)
    bw, bh = rng.integers(60, 250, N), rng.integers(14, 32, N)
    quads = np.stack([np.stack([x, y], 1), np.stack([x + bw, y], 1), np.stack([x + bw, y + bh], 1), np.stack([x, y + bh], 1)], 1)
    bx, by = rng.integers(0, W - 400, N), rng.integers(20, H - 300, N)
    boxes = np.stack([bx, by, bx + rng.integers(50, 400, N), by + rng.integers(30, 300, N)], 1)
    alphabet = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
    lines = ["".join(alphabet[int(k)] for k in rng.integers(0, len(alphabet), CHARS)) for _ in range(N)]
    return quads, boxes, lines


def build_overlay(quads, boxes, lines, recorder=None):
    from yomitoku_amd.utils.visualizer import Overlay, load_font

    ov = (recorder or Overlay)()
    label, text = load_font(None, 12), load_font(None, 18)
    ov.polyline(quads, True, (0, 255, 0), 1)
    for k, b in enumerate(boxes.tolist()):
        ov.rectangle(b, (255, 0, 255), 2)
        ov.text((b[0], b[1]), f"paragraphs({k})", label, (255, 0, 0), anchor="ls")
    for q, s in zip(quads.tolist(), lines):
        ov.text((q[0][0], q[0][1] - 18), s, text, (0, 0, 255))
    return ov


def pillow_draw(page, quads, boxes, lines):
    from PIL import Image, ImageDraw, ImageFont

    img = Image.fromarray(page.copy())
    draw = ImageDraw.Draw(img)
    label, text = ImageFont.load_default(12), ImageFont.load_default(18)
    for q in quads.tolist():
        draw.line([tuple(p) for p in q] + [tuple(q[0])], fill=(0, 255, 0), width=1)
    for k, b in enumerate(boxes.tolist()):
        draw.rectangle(b, outline=(255, 0, 255), width=2)
        draw.text((b[0], b[1]), f"paragraphs({k})", font=label, fill=(255, 0, 0), anchor="ls")
    for q, s in zip(quads.tolist(), lines):
        draw.text((q[0][0], q[0][1] - 18), s, font=text, fill=(0, 0, 255))
    import numpy as np

    return np.asarray(img)


def median_ms(fn, sync=None):
    out = []
    for _ in range(RUNS + WARMUP):
        if sync:
            sync()
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(out[WARMUP:]), 3)


WAVE_PAGES = 16


def wave_leg(out_path):
    """serve(overlays=True)'s renderer on a wave of WAVE_PAGES such pages x 2 canvases (every canvas carries the whole content):
      layout_device_ms / draw_pages_device_ms   ymk_overlay_layout / ymk_draw_overlay_pages for the WAVE, HIP events around each call
      record_and_build_host_ms_per_page         the run recorder + build_wave for the wave, per page (two canvases)
      render_wave_wall_ms                       render_wave: clone, blob, both launches, D2H of all canvases, owned copies
    next to the per-page path's own rows re-measured in the same process (one launch and one host build per CANVAS)."""
    import torch

    from yomitoku_amd import _lib
    from yomitoku_amd.utils import visualizer as V
    from yomitoku_amd.utils.synth import synthetic_page

    assert torch.cuda.is_available(), "overlay_timing.py measures on the GPU"
    lib = _lib.load()
    page_dev = torch.from_numpy(synthetic_page(0, H, W)).to("cuda:0")
    quads, boxes, lines = content()
    sync = torch.cuda.synchronize
    n_canvases = 2 * WAVE_PAGES

    def record():
        return [build_overlay(quads, boxes, lines, V.RunOverlay) for _ in range(n_canvases)]

    V.build_wave(record()[:1], [(H, W)])  # the glyphs enter the store once per process
    sizes = [(H, W)] * n_canvases
    data = V.build_wave(record(), sizes)
    buf = torch.empty(data["bytes"], dtype=torch.uint8, device="cuda:0")
    for off in data["table"][:, 0].tolist():
        buf[off : off + H * W * 3] = page_dev.reshape(-1)
    staged = V.draw_wave(buf, record(), sizes)
    stream = _lib.current_stream_ptr()

    def timed(fn, name, call_args):
        out = []
        for _ in range(RUNS + WARMUP):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(fn(*call_args, stream), name)
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return round(statistics.median(out[WARMUP:]), 4)

    # the per-page path, one canvas: the rows of profiles/visualize_overlay.json again, same process
    ov = build_overlay(quads, boxes, lines)
    one = ov.build(H, W)
    canvas = page_dev.clone()
    staged_one = V.stage_commands(canvas, one["cmds"], one["atlas"], lists=(one["tile_offsets"], one["tile_cmds"]))
    kernel = []
    for _ in range(RUNS + WARMUP):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        V.launch_staged(canvas, staged_one)
        b.record()
        b.synchronize()
        kernel.append(a.elapsed_time(b))
    slot = [None]
    result = {
        "page": [H, W], "wave_pages": WAVE_PAGES, "canvases": n_canvases, "commands_per_canvas": int(len(data["cmds"]) // n_canvases),
        "commands": int(len(data["cmds"])), "text_runs": int(len(data["runs"])), "characters": int(len(data["codes"])),
        "tiles": int(data["tiles"]), "runs": RUNS, "warmup": WARMUP,
        "layout_device_ms": timed(lib.ymk_overlay_layout, "ymk_overlay_layout", staged["layout_args"]),
        "draw_pages_device_ms": timed(lib.ymk_draw_overlay_pages, "ymk_draw_overlay_pages", staged["draw_args"]),
        "record_and_build_host_ms_per_page": round(median_ms(lambda: V.build_wave(record(), sizes)) / WAVE_PAGES, 3),
        "render_wave_wall_ms": median_ms(lambda: V.render_wave([page_dev] * n_canvases, record(), slot), sync),
        "per_page_path_same_process": {
            "draw_overlay_device_ms_per_canvas": round(statistics.median(kernel[WARMUP:]), 4),
            "build_and_bin_host_ms_per_canvas": median_ms(lambda: build_overlay(quads, boxes, lines).build(H, W)),
            "render_wall_ms_per_canvas": median_ms(lambda: build_overlay(quads, boxes, lines).render(page_dev), sync),
        },
        "device": torch.cuda.get_device_name(0),
    }
    result["draw_pages_device_ms_per_canvas"] = round(result["draw_pages_device_ms"] / n_canvases, 4)
    result["layout_device_ms_per_canvas"] = round(result["layout_device_ms"] / n_canvases, 4)
    text = json.dumps(result, indent=1)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(text)


def form_results(seed=0):
    """What TableSemanticParser returns for a dense form, without running the networks: 4 tables of 12 x 6 cells (the first row
    headers, every cell sharing its border rows and columns with its neighbours), a kv item per cell of the first data column,
    one grid and its graph per table, a word per cell."""
    from types import SimpleNamespace as NS

    from yomitoku_amd.utils.graph import OrderedDiGraph

    tables, dags, words = [], [], []
    rows, cols, cw, ch = 12, 6, 90, 28
    for t in range(4):
        ox, oy = 40 + (t % 2) * 580, 60 + (t // 2) * 760
        cells, dag = {}, OrderedDiGraph()
        for r in range(rows):
            for c in range(cols):
                b = [ox + c * cw, oy + r * ch, ox + (c + 1) * cw, oy + (r + 1) * ch]
                cid = f"r{r}c{c}"
                cells[cid] = NS(id=cid, box=b, role="header" if r == 0 else ("empty" if (r + c) % 5 == 0 else "cell"), contents="")
                dag.add_node(cid, bbox=b)
                words.append(NS(points=[[b[0] + 4, b[1] + 6], [b[2] - 4, b[1] + 6], [b[2] - 4, b[3] - 4], [b[0] + 4, b[3] - 4]],
                                content=f"w{t}{r}{c}", direction="horizontal"))
        for r in range(rows):
            for c in range(cols):
                if c + 1 < cols:
                    dag.add_edge(f"r{r}c{c}", f"r{r}c{c + 1}", dir="R")
                    dag.add_edge(f"r{r}c{c + 1}", f"r{r}c{c}", dir="L")
                if r + 1 < rows:
                    dag.add_edge(f"r{r}c{c}", f"r{r + 1}c{c}", dir="D")
                    dag.add_edge(f"r{r + 1}c{c}", f"r{r}c{c}", dir="U")
        box = [ox, oy, ox + cols * cw, oy + rows * ch]
        cells["grp0"] = NS(id="grp0", box=box, role="group", contents="")
        kv = [NS(id=f"kv{r}", key=[f"r{r}c0"], value=f"r{r}c1") for r in range(1, rows)]
        tables.append(NS(id=f"t{t}", box=box, cells=cells, kv_items=kv, grids=[NS(box=box)]))
        dags.append(dag)
    paragraphs = [NS(id=f"p{k}", box=[40 + 290 * k, 20, 300 + 290 * k, 50]) for k in range(4)]
    return NS(tables=tables, paragraphs=paragraphs, words=words), dags


def tables_leg(out_path):
    """The render step of TableSemanticParser.parse_pages(overlays=True) for a wave of WAVE_PAGES form pages (form_results), two
    canvases per page, through the functions parse_pages calls (the drawings' content helpers on RunOverlay, build_wave, the
    two launches):
      draw_pages_device_ms               ymk_draw_overlay_pages for the WAVE, HIP events around the call
      record_and_build_host_ms_per_page  recording both drawings of a page + its share of build_wave
      layer_records / flushes            how many records of a layout canvas paint the layer, and how many flushes composite it"""
    import torch

    from yomitoku_amd import _lib
    from yomitoku_amd.utils import visualizer as V
    from yomitoku_amd.utils.synth import synthetic_page

    assert torch.cuda.is_available(), "overlay_timing.py measures on the GPU"
    lib = _lib.load()
    page_dev = torch.from_numpy(synthetic_page(0, H, W)).to("cuda:0")
    results, dags = form_results()
    font = V.load_font(None, 12)

    def record():
        out = []
        for _ in range(WAVE_PAGES):
            layout, ocr = V.RunOverlay(), V.RunOverlay()
            V._semantic_layout_commands(layout, results, dags)
            V._semantic_ocr_commands(ocr, results, font, 12, (255, 0, 0))
            out += [layout, ocr]
        return out

    n_canvases = 2 * WAVE_PAGES
    sizes = [(H, W)] * n_canvases
    V.build_wave(record()[:2], sizes[:2])  # the glyphs enter the store once per process
    data = V.build_wave(record(), sizes)
    buf = torch.empty(data["bytes"], dtype=torch.uint8, device="cuda:0")
    for off in data["table"][:, 0].tolist():
        buf[off : off + H * W * 3] = page_dev.reshape(-1)
    staged = V.draw_wave(buf, record(), sizes)
    stream = _lib.current_stream_ptr()
    times = []
    for _ in range(RUNS + WARMUP):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(lib.ymk_draw_overlay_pages(*staged["draw_args"], stream), "ymk_draw_overlay_pages")
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    first = data["table"][0]
    layout_cmds = data["cmds"][int(first[3]) : int(first[3]) + int(first[4])]
    result = {
        "page": [H, W], "wave_pages": WAVE_PAGES, "canvases": n_canvases, "tables_per_page": len(results.tables),
        "cells_per_page": sum(len(t.cells) for t in results.tables), "words_per_page": len(results.words),
        "commands": int(len(data["cmds"])), "layout_canvas_commands": int(len(layout_cmds)),
        "layer_records": int(((layout_cmds[:, 0] & V.TO_LAYER) != 0).sum()), "flushes": int((layout_cmds[:, 0] == V.FLUSH).sum()),
        "runs": RUNS, "warmup": WARMUP,
        "draw_pages_device_ms": round(statistics.median(times[WARMUP:]), 4),
        "record_and_build_host_ms_per_page": round(median_ms(lambda: V.build_wave(record(), sizes)) / WAVE_PAGES, 3),
        "device": torch.cuda.get_device_name(0),
    }
    result["draw_pages_device_ms_per_canvas"] = round(result["draw_pages_device_ms"] / n_canvases, 4)
    text = json.dumps(result, indent=1)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--wave", action="store_true", help="the wave renderer of serve(overlays=True): profiles/visualize_overlay_wave.json")
    ap.add_argument("--tables", action="store_true", help="a form page with tinted tables: profiles/visualize_table_overlays.json")
    args = ap.parse_args()
    if args.wave:
        return wave_leg(args.out)
    if args.tables:
        return tables_leg(args.out)
    import torch

    from yomitoku_amd.utils.synth import synthetic_page
    from yomitoku_amd.utils.visualizer import launch_staged, stage_commands

    assert torch.cuda.is_available(), "overlay_timing.py measures on the GPU"
    page = synthetic_page(0, H, W)
    page_dev = torch.from_numpy(page).to("cuda:0")
    quads, boxes, lines = content()
    sync = torch.cuda.synchronize

    ov = build_overlay(quads, boxes, lines)
    data = ov.build(H, W)
    canvas = page_dev.clone()
    staged = stage_commands(canvas, data["cmds"], data["atlas"], lists=(data["tile_offsets"], data["tile_cmds"]))
    kernel = []
    for _ in range(RUNS + WARMUP):  # the same canvas again and again: the work per pixel does not depend on its colour
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch_staged(canvas, staged)
        b.record()
        b.synchronize()
        kernel.append(a.elapsed_time(b))
    per_tile = data["tile_offsets"][1:] - data["tile_offsets"][:-1]
    result = {
        "page": [H, W], "quads": N, "labelled_boxes": N, "text_lines": N, "chars_per_line": CHARS,
        "commands": int(len(data["cmds"])), "list_entries": int(len(data["tile_cmds"])), "tiles": int(len(per_tile)),
        "tiles_with_commands": int((per_tile > 0).sum()), "longest_tile_list": int(per_tile.max()), "atlas_bytes": int(data["atlas"].size),
        "runs": RUNS, "warmup": WARMUP,
        "draw_overlay_device_ms": round(statistics.median(kernel[WARMUP:]), 4),
        "build_and_bin_host_ms": median_ms(lambda: build_overlay(quads, boxes, lines).build(H, W)),
        "render_wall_ms": median_ms(lambda: build_overlay(quads, boxes, lines).render(page_dev), sync),
        "d2h_ms": median_ms(lambda: canvas.cpu().numpy(), sync),
        "pillow_host_ms": median_ms(lambda: pillow_draw(page, quads, boxes, lines)),
        "device": torch.cuda.get_device_name(0),
    }
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
