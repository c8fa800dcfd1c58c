"""Multi-page serving on ONE GPU from ONE process: host pages in, every page's result out, in page order.

The reference's unit of use is "file in -> all page results out" (cli/main.py:105-137): the page loop calls the
analyzer once per page and a failing file is logged and skipped (cli/main.py:555-564).  On an MI355X one page at a time
leaves the device mostly idle, so `DocumentAnalyzer.serve` runs the page loop as a STAGE PIPELINE over waves of pages:

    caller thread   decode (paths) -> pinned staging ring -> H2D on the copy stream              (PageStager)
    detect          DBNet forwards over the wave, maps back in one DMA per forward               HIP stream
    boxes           DB box extraction, C++, GIL released                                         host
    crops           per-page mini-batches (bucketing, width budget) + the crop kernels           HIP stream
    recognize       ONE grouped PARSeq forward with one greedy loop per wave; TWO lanes (below)   HIP stream x 2
    decode          token decode, un-permutation                                                 host
    layout          RT-DETRv2 layout forward over the wave                                       HIP stream
    tables          layout boxes (host), table-structure forward over all table crops            HIP stream
    cells           row / column / span filters, cell grids                                      host
    finish          word -> cell / paragraph aggregation and reading order, per page             host
    render          serve(overlays=True) / serve(jpeg=...) only: both overlay images and / or the
                    JPEG file of every page of the wave                                           HIP stream

The host halves are their own stages on purpose: a thread that owns a network only ever launches - it never sits in box
logic or string decoding while its stream runs dry (measured: with crop planning / decode inside the recognise stage
and the table grid logic inside the layout stage the GPU was idle 16 % of a job, in 10-20 ms holes).
Every network exists once, except the recogniser, which has a second PARSeq handle (a replica of the first's weights,
~50 MB for the --lite model): the grouped forward is the longest stage and half of it is the greedy loop - ~100 dependent,
nearly empty launches - so two lanes let wave k + 1's encoder fill the chip while wave k's loop idles through its steps.  A
model handle is only ever used by one thread, which is what include/ymk.h asks for; six compute streams plus the copy
stream fit the eight hardware queues the package asks the HIP runtime for.  Wave k + 1 is in the detector while wave k decodes text and its tables are parsed; up to `in_flight`
waves are between upload and aggregation (a ring of pinned map buffers per wave slot), which bounds host and device
memory.

`render` is not one of the nine: its thread and stream are started by the first job that asks for overlays or JPEG files, and
only the waves of such a job visit it - after `finish` has aggregated them, before their slot is handed back.  It draws all
canvases of a wave (as many per page as the analyzer draws: two, OCR one) with two launches (utils/visualizer.py: render_wave) and / or encodes the wave's clean pages
as the job's PageFiles (`wave.job.files`; yomitoku_amd/jpeg.py: encode_page_files) says: as JPEG files with three launches - five with `optimize` -, its two-valued pages as Group 4 files with four
more under `bilevel="auto"` (yomitoku_amd/ccitt.py) - or its grey-valued pages, thresholded, with `"otsu"` (six
more) or `"adaptive"` (seven more); `mrc` separates the pages that leaves into an ink mask and two layers in front of those
launches (yomitoku_amd/mrc.py: the page-skew step's luminance and ink, cells, a pull per level, flags, push) and hands the layers
to the JPEG launches and the masks to the Group 4 launches; a job with `figures` has the crops of every page's `schema.figures` cut
from the wave's pages by one launch and coded by the JPEG launches as pages of their own (yomitoku_amd/figures.py:
crop_figure_files), the stage's third product; a job with none of the three runs exactly the stages above.

`serve(deskew=...)` adds no stage either: the skew of every page of a wave is estimated and undone on the copy stream, behind the
wave's uploads and before the event every stage waits for (yomitoku_amd/deskew.py: launch; five launches and the binariser's three),
so the stages above see the corrected pages; the decision reaches the host through pinned words that are read when the wave's
entries are written.

Garbage collection: a full (generation-2) pass of CPython's cyclic collector walks every live container object of the
process while holding the GIL - measured 100-180 ms with the results of a few hundred pages alive, six times in a
4 s job - and every stage thread that needs the interpreter to issue its next launch stalls behind it (the GPU idles;
this, not the launch rate, is what held one process at 48 pages/s where two reached 66).  `serve` therefore defers
generation-2 collections for the duration of a job (`defer_full_gc=True`: the young generations keep running, the
previous thresholds come back when the job ends).

Failure isolation: a stage that raises marks its wave failed; the pages of a failed wave are re-run as single-page
waves through the same pipeline, and a page that fails alone gets the exception object as its result - the job goes
on (the reference's per-file `except: log, continue`).  Results equal `DocumentAnalyzer.__call__` page by page
(tests/test_serving_gpu.py).

What the pipeline asks of an analyzer is written down in `StageAnalyzer` (below), the base class of DocumentAnalyzer,
TableSemanticParser and OCR: it holds the chain plumbing, the OCR chain and the render stage once, each analyzer adds its table
chain, `finish` and the drawings of a page.  The stage plan is data (`CHAINS`), and an analyzer says which chains it has:
`OCR.serve` declares `chains = ("ocr",)` and runs detect ... decode, finish and render alone - no layout, tables or cells
thread, no stream for them, `finish` after one arrival, one picture per page in the render stage."""

from __future__ import annotations

import contextlib
import gc
import logging
import os
import queue
import sys
import threading
import time
from collections import deque
from concurrent.futures import Future, ThreadPoolExecutor
from typing import Iterable, List, Optional

import numpy as np
import torch

from . import imaging
from .data.staging import PageStager
from .jpeg import check_jpeg_preset, encode_page_files  # noqa: F401 - check_jpeg_preset: the public entries and the tests take it from here

logger = logging.getLogger(__name__)

_STOP = object()


class Wave:
    """The pages that share device batches, and what the stages have produced for them so far."""

    __slots__ = ("seq", "ids", "imgs", "pages", "ring", "uploaded", "maps", "sizes", "dets", "rec_plan", "recs", "lay_raw",
                 "lay_parsed", "tab_raw", "lays", "error", "failed_stage", "layout_done", "joined", "retry", "job", "results", "dags", "skew")

    def __init__(self, seq=0, ids=(), imgs=(), pages=(), ring=0, uploaded=None, retry=False, job=None):
        self.seq, self.ids, self.imgs, self.pages, self.ring, self.uploaded = seq, list(ids), list(imgs), list(pages), ring, uploaded
        self.job = job  # the serve() call this wave belongs to: a late wave of an aborted job must not write into the next one
        self.results = None  # per page, what `finish` made of it (schema or exception): only kept for the render stage
        self.dags = None  # TableSemanticParser, overlays jobs: per page the grid graphs `finish` parsed, for the render stage
        self.skew = None  # serve(deskew=...): the wave's launched skew step (yomitoku_amd/deskew.py); `pages` are the corrected ones
        self.sizes = [tuple(int(v) for v in p.shape[:2]) for p in self.pages]
        self.maps = self.dets = self.rec_plan = self.recs = self.lay_raw = self.lay_parsed = self.tab_raw = self.lays = None
        self.error: Optional[BaseException] = None
        self.failed_stage = None
        self.layout_done = threading.Event()
        self.joined = 0
        self.retry = retry

    def __len__(self):
        return len(self.ids)

    def fail(self, stage, exc):
        if self.error is None:
            self.error, self.failed_stage = exc, stage


class _Job:
    """One serve() call: where results go and how many waves are still out."""

    def __init__(self, n_hint=0, overlays=False, options=None, files=None, deskew=None, figures=None):
        self.results = {}
        self.figures = figures  # None, or the record of check_figures: the entries get the page's PageFigures, made in the render stage too
        self.deskew = deskew  # None, or the parameters of check_deskew: the pages are turned upright behind their upload
        self.options = options  # what the analyzer's serve() wants its stages to know about THIS job (read through wave.job)
        self.overlays = bool(overlays)  # entries are (schema, the analyzer's pictures...): the waves visit the render stage
        self.files = files  # None, or the PageFiles of check_jpeg_preset: the entries end with the page's file, made in the render stage too
        self.cond = threading.Condition()
        self.outstanding = 0
        self.retries: "deque" = deque()  # (page id, host page) to re-run alone
        self.waves = 0
        self.retried_pages = 0


@contextlib.contextmanager
def _full_gc_deferred(on: bool):
    """Generation-2 collections of the cyclic collector postponed while the block runs (module doc)."""
    if not on or not gc.isenabled():
        yield
        return
    t0, t1, t2 = gc.get_threshold()
    gc.set_threshold(t0, t1, 1 << 30)
    try:
        yield
    finally:
        gc.set_threshold(t0, t1, t2)


_switch_lock = threading.Lock()
_switch_users = 0
_switch_saved = None


@contextlib.contextmanager
def _switch_interval(seconds):
    """CPython's thread switch interval shortened while the block runs.  The stage threads are launch-latency-bound: one
    returning from a 50 us library call must not wait 5 ms (the default interval) behind another stage's Python loop before
    it can issue its next launch.  None / 0 leaves the interpreter alone.  The setting is process-wide, so it is reference
    counted: the first job in saves the interpreter's value, the LAST job out restores it - two pipelines serving at once
    (two analyzers, two threads) cannot restore out of order and leave the short interval behind."""
    global _switch_users, _switch_saved
    if not seconds:
        yield
        return
    with _switch_lock:
        if _switch_users == 0:
            _switch_saved = sys.getswitchinterval()
        _switch_users += 1
        sys.setswitchinterval(min(float(seconds), sys.getswitchinterval()))
    try:
        yield
    finally:
        with _switch_lock:
            _switch_users -= 1
            if _switch_users == 0 and _switch_saved is not None:
                sys.setswitchinterval(_switch_saved)
                _switch_saved = None


def _run_stage(stream, wave, fn, *args):
    """One stage visit: `fn(*args)` on `stream` after the wave's upload, waited for.  The one place that guards device memory: when
    the stage raises, kernels it already queued may still read the wave's pages / pinned maps / crops, which the caller is about
    to hand back with the slot - they are drained first (best effort: the device may be the problem), then the exception goes
    on.  `stream` None (a host stage, or the host-only pipeline): the plain call."""
    if stream is None:
        return fn(*args)
    try:
        with torch.cuda.stream(stream):
            stream.wait_event(wave.uploaded)
            out = fn(*args)
            stream.synchronize()
        return out
    except BaseException:
        try:
            stream.synchronize()
        except Exception:  # noqa: BLE001
            pass
        raise


# The stage plan, once: per chain its stages in order as (stage, the analyzer's method, launches on the GPU?).  A wave enters
# every chain its analyzer declares at the chain's first stage; the chains join in `finish`.
CHAINS = {
    "ocr": (("detect", "_stage_detect", True), ("boxes", "_stage_boxes", False), ("crops", "_stage_crops", True),
            ("recognize", "_stage_recognize", True), ("decode", "_stage_decode", False)),
    "layout": (("layout", "_stage_layout", True), ("tables", "_stage_tables", True), ("cells", "_stage_cells", False)),
}


def _declared_chains(analyzer):
    """The analyzer's `chains` - a tuple out of CHAINS' names; an analyzer that says nothing runs both - checked: a ValueError
    for none, an unknown or a repeated name, and for `split_text_across_cells` (the words are cut at the cells of the
    layout chain) without "layout"."""
    chains = tuple(getattr(analyzer, "chains", tuple(CHAINS)))
    unknown = [c for c in chains if c not in CHAINS]
    if not chains or unknown or len(set(chains)) != len(chains):
        raise ValueError(f"chains must be a non-empty tuple out of {tuple(CHAINS)} without repeats, got {chains!r}")
    if getattr(analyzer, "split_text_across_cells", False) and "layout" not in chains:
        raise ValueError(f"split_text_across_cells needs the layout chain, the analyzer declares chains={chains!r}")
    return chains


class PagePipeline:
    def __init__(self, analyzer, wave: int = 16, in_flight: int = 4, defer_full_gc: bool = True, stage_priority=None,
                 rec_lanes: int = 2):
        """rec_lanes: recogniser forwards in flight.  The grouped PARSeq forward is two phases with opposite appetites - the
        ViT encoder (large GEMMs) and the greedy loop (~100 dependent, nearly empty launches) - and it is the longest stage;
        with two lanes (each its own PARSeq handle and HIP stream, the second a replica of the first's weights) wave k + 1's
        encoder fills the chip while wave k's loop idles through its steps.  Forced to 1 with `rec_orientation_fallback`
        (its retry forwards run on the module's own model from the decode path).
        stage_priority: {"detect" | "recognize" | "layout": HIP stream priority (0 default, -1 high)}; also read from
        YMK_STAGE_PRIORITY="recognize:-1,..." (measurement knob)."""
        self.analyzer = analyzer
        self.defer_full_gc = bool(defer_full_gc)
        # thread switch interval for the duration of a job (YMK_SWITCH_INTERVAL overrides; 0 = leave the interpreter's)
        self.switch_interval = float(os.environ.get("YMK_SWITCH_INTERVAL", 2e-4))
        self.stage_priority = dict(stage_priority or {})
        rec = getattr(analyzer, "text_recognizer", None)
        self.rec_lanes_asked = int(rec_lanes)  # what the caller asked for: an analyzer's serve() rebuilds the pipeline when it changes
        self.rec_lanes = 1 if getattr(rec, "rec_orientation_fallback", False) else max(1, int(os.environ.get("YMK_REC_LANES", rec_lanes)))
        for item in filter(None, os.environ.get("YMK_STAGE_PRIORITY", "").split(",")):
            name, _, value = item.partition(":")
            self.stage_priority.setdefault(name.strip(), int(value))
        self.wave = max(1, int(wave))
        self.in_flight = max(1, int(in_flight))
        self.device = torch.device(analyzer.text_detector.device)
        # a HIP device always, for DocumentAnalyzer (BaseModule refuses anything else); the host-only form exists so that
        # the orchestration (ordering, back-pressure, retries) can be tested with stub stages on a box without a GPU
        self._gpu = self.device.type == "cuda"
        self.stager = PageStager(self.device, slots=self.wave * (self.in_flight + 1)) if self._gpu else None
        self._rings: "queue.Queue" = queue.Queue()
        for r in range(self.in_flight):
            self._rings.put(r)
        self.chains = _declared_chains(analyzer)
        self._job: Optional[_Job] = None
        self._seq = 0
        self.trace = None  # a list: every stage appends (stage, wave seq, pages, t_start, t_end) - tools/serve_trace.py
        self._serve_lock = threading.Lock()
        self._render_q: "queue.Queue" = queue.Queue()
        self._render_thread = None  # started by the first job that asks for overlays
        self._deskew_scratch = {}  # serve(deskew=...): the step's device buffers, made by the first such job
        self._deskew_pinned = {}  # wave slot -> the pinned buffer its choice words come back through
        # (stage, function, launches on the GPU?, next stages), built from CHAINS for the chains the analyzer declares: every
        # chain is entered at its first stage (_launch) and all of them join in `finish`.  A stage of a chain that is not
        # declared has no thread, no stream and no queue, and its method is never looked up
        plan = []
        for chain in self.chains:
            stages = CHAINS[chain]
            for (name, method, on_gpu), after in zip(stages, stages[1:] + (("finish",),)):
                fn = self._boxes if name == "boxes" else getattr(analyzer, method)  # `boxes` may wait for the layout chain
                plan.append((name, fn, on_gpu, (after[0],)))
        plan.append(("finish", self._finish, False, ()))
        self._entries = tuple(CHAINS[chain][0][0] for chain in self.chains)  # where _launch puts a wave
        self._q = {spec[0]: queue.Queue() for spec in plan}
        self._workers = {spec[0]: (self.rec_lanes if spec[0] == "recognize" else 1) for spec in plan}
        self._threads = [threading.Thread(target=self._loop, args=spec + (lane,), name=f"ymk-{spec[0]}-{lane}" if self._workers[spec[0]] > 1 else f"ymk-{spec[0]}",
                                          daemon=True) for spec in plan for lane in range(self._workers[spec[0]])]
        for t in self._threads:
            t.start()

    # ------------------------------------------------------------------ stage threads
    def _loop(self, name, fn, on_gpu, outs, lane=0):
        stream = None
        if self._workers[name] > 1:  # a stage with several lanes tells its function which one is calling
            inner = fn

            def fn(wave):
                return inner(wave, lane)

        if on_gpu and self._gpu:
            torch.cuda.set_device(self.device)
            stream = torch.cuda.Stream(device=self.device, priority=self.stage_priority.get(name, 0))
        q_in = self._q[name]
        while True:
            wave = q_in.get()
            if wave is _STOP:
                return
            if name == "finish":
                wave.joined += 1
                if wave.joined < len(self.chains):  # arrives once from every chain the analyzer declares
                    continue
            if wave.error is None or name == "finish":
                t_start = time.perf_counter()
                try:
                    _run_stage(stream, wave, fn, wave)
                except BaseException as exc:  # noqa: BLE001 - delivered to the page's result slot
                    wave.fail(name, exc)
                    if name == "finish":  # cannot happen short of a bug in _finish itself: never lose a page or a slot
                        for idx in wave.ids:
                            wave.job.results.setdefault(idx, exc)
                        if wave.pages is not None:
                            self._release(wave)
                if self.trace is not None:
                    self.trace.append((name, wave.seq, len(wave), t_start, time.perf_counter()))
            if name == "cells":
                wave.layout_done.set()
            for out in outs:
                self._q[out].put(wave)

    def _boxes(self, wave):
        a = self.analyzer
        a._stage_boxes(wave)
        if getattr(a, "split_text_across_cells", False):
            wave.layout_done.wait()
            if wave.error is None:
                a._stage_split(wave)

    def _render_loop(self):
        """The render stage: waves of overlays and / or jpeg jobs, after aggregation.  Turns every page's schema into (schema,
        the analyzer's pictures...) - ocr and layout overlay; OCR: the ocr overlay alone -, (schema, EncodedJpeg) or (schema,
        pictures..., EncodedJpeg), each with the page's PageFigures behind it in a figures job; a page whose
        drawing or encoding fails - or every page of the wave, when the launches fail - gets the exception."""
        stream = None
        if self._gpu:
            torch.cuda.set_device(self.device)
            stream = torch.cuda.Stream(device=self.device)
        while True:
            wave = self._render_q.get()
            if wave is _STOP:
                return
            t_start = time.perf_counter()
            job, results = wave.job, wave.results
            try:
                skews = self._skews(wave)
                products = []  # per product of the job, per page: a tuple of entry members, or the exception
                for wanted, fn in ((job.overlays, "_stage_render"), (job.files is not None, "_stage_jpeg"),
                                   (job.figures is not None, "_stage_figures")):
                    if not wanted:
                        continue
                    try:
                        products.append(_run_stage(stream, wave, getattr(self.analyzer, fn), wave, results))
                    except BaseException as exc:  # noqa: BLE001 - delivered to the pages' result slots
                        logger.error("wave %d failed in the render stage: %s: %s", wave.seq, type(exc).__name__, exc)
                        products.append([exc] * len(wave))
                for k, idx in enumerate(wave.ids):
                    failed = next((made[k] for made in products if isinstance(made[k], BaseException)), None)
                    if isinstance(results[k], BaseException):
                        job.results[idx] = results[k]
                    elif failed is not None:
                        logger.error("page %d failed in the render stage: %s: %s", idx, type(failed).__name__, failed)
                        job.results[idx] = failed
                    else:
                        job.results[idx] = (results[k],) + tuple(m for made in products for m in made[k]) + (() if skews is None else (skews[k],))
                if self.trace is not None:
                    self.trace.append(("render", wave.seq, len(wave), t_start, time.perf_counter()))
            finally:
                wave.results = None
                self._release(wave)

    def _start_render(self):
        if self._render_thread is None or not self._render_thread.is_alive():
            self._render_thread = threading.Thread(target=self._render_loop, name="ymk-render", daemon=True)
            self._render_thread.start()

    def _release(self, wave):
        job = wave.job
        wave.pages = wave.maps = wave.rec_plan = wave.skew = None  # the device pages, the pinned map views and the crop tensors go back
        self._rings.put(wave.ring)
        with job.cond:
            job.outstanding -= 1
            job.cond.notify_all()

    def _finish(self, wave):
        job = wave.job
        if wave.error is not None:
            if len(wave) > 1:
                logger.warning("wave of %d pages failed in stage %s (%s: %s); re-running its pages one by one", len(wave),
                               wave.failed_stage, type(wave.error).__name__, wave.error)
                with job.cond:
                    job.retries.extend(zip(wave.ids, wave.imgs))
            else:
                logger.error("page %d failed in stage %s: %s: %s", wave.ids[0], wave.failed_stage, type(wave.error).__name__,
                             wave.error)
                job.results[wave.ids[0]] = wave.error
        else:
            done = []
            for k, idx in enumerate(wave.ids):
                try:
                    done.append(self.analyzer._stage_finish(wave, k))
                except Exception as exc:  # noqa: BLE001 - aggregation is per page: only this page fails
                    logger.error("page %d failed in aggregation: %s: %s", idx, type(exc).__name__, exc)
                    done.append(exc)
            if job.overlays or job.files is not None or job.figures is not None:  # the render stage writes the entries and hands the slot back
                wave.results = done
                self._render_q.put(wave)
                return
            skews = self._skews(wave)
            for k, (idx, entry) in enumerate(zip(wave.ids, done)):
                job.results[idx] = entry if skews is None or isinstance(entry, BaseException) else (entry, skews[k])
        self._release(wave)

    @staticmethod
    def _skews(wave):
        """Per page of a deskew job's wave its PageSkew, else None.  The choice words were copied to pinned memory on the copy
        stream before the wave's `uploaded` event, which every stage stream has waited for and been waited for since: no wait."""
        return None if wave.skew is None else wave.skew.skews()

    # ------------------------------------------------------------------ caller side
    def _launch(self, job, ids, imgs, retry=False, ring=None, waited=0.0):
        """`ring`: a wave slot the caller already holds (serve() takes the slot BEFORE it pulls the wave's sources; `waited`:
        how long it waited for it), or None: taken here."""
        t_start = time.perf_counter() - waited
        if ring is None:
            ring = self._rings.get()  # blocks while `in_flight` waves are out: back-pressure on decoding and staging
        t_ring = time.perf_counter()
        try:
            if self._gpu:
                pages = [self.stager.upload(img, wait=False) for img in imgs]
                skew = None
                if job.deskew is not None:
                    # behind the uploads on the copy stream, before the event every stage waits for: the chains see the corrected
                    # pages and nothing downstream changes.  Device scratch: one set (the step is serialised on this stream); the
                    # pinned choice words: one per wave slot, read when the wave's entries are written
                    from .deskew import launch as launch_deskew

                    with torch.cuda.device(self.device), torch.cuda.stream(self.stager.stream):
                        skew = launch_deskew(pages, job.deskew, self._deskew_scratch, pin_scratch=self._deskew_pinned.setdefault(ring, {}))
                    pages, skew.corrected = skew.corrected, None  # the wave holds them; the uploaded originals go back now
                uploaded = torch.cuda.Event()
                uploaded.record(self.stager.stream)
            else:
                pages, uploaded, skew = list(imgs), None, None
        except BaseException:
            self._rings.put(ring)
            raise
        self._seq += 1
        if self.trace is not None:
            self.trace.append(("wait_slot", self._seq, len(ids), t_start, t_ring))
            self.trace.append(("stage_h2d", self._seq, len(ids), t_ring, time.perf_counter()))
        wave = Wave(self._seq, ids, imgs, pages, ring, uploaded, retry, job)
        wave.skew = skew
        with job.cond:
            job.outstanding += 1
            job.waves += 1
        for name in self._entries:
            self._q[name].put(wave)

    def serve(self, sources: Iterable, with_source: bool = False, overlays: bool = False, options=None, files=None,
              deskew=False, figures=None) -> List:
        """sources: uint8 H x W x 3 BGR arrays and / or image file paths (a multi-frame file contributes one entry per
        frame).  Returns one entry per page, in order: the DocumentAnalyzerSchema, or the exception that page (or
        file) raised.  with_source=True: (source index, frame index within the source, entry) triples instead - what a
        caller that writes `<file>_p<page>.json` per page needs (cli/main.py:122-137).
        overlays=True: a page's entry is (DocumentAnalyzerSchema, ocr overlay, layout overlay) - the two uint8 H x W x 3 images
        `analyze_pages` returns for the page with visualize=True everywhere, as arrays the caller owns; a failed page's entry
        stays the bare exception.  The waves of such a job pass through the render stage, whose thread the first such job
        starts; a job without overlays runs what it always ran.
        files: None, or the PageFiles of the job (yomitoku_amd/jpeg.py: check_jpeg_preset makes it of the public entries' `jpeg...`
        options): a page's entry ends with its page file - (schema, EncodedJpeg), or (schema, ocr overlay, layout overlay,
        EncodedJpeg); an EncodedBilevel or an EncodedMrc where the record gives the page one - encoded in the render stage from
        the clean page, never from a canvas.
        deskew: False, True, or a dict with any of max_angle, step, min_angle in degrees (yomitoku_amd/deskew.py: check_deskew;
        anything else is a ValueError before a source is read): every page's skew is estimated and undone on the device behind
        its upload, so words, boxes, overlays and page files are those of the corrected page, and a page's entry ends with its
        PageSkew - (schema, PageSkew), (schema, ..., EncodedJpeg, PageSkew); a failed page's entry stays the bare exception.  A
        page that is re-run alone is estimated again from its host original.  Needs a HIP device.
        figures: None, or the record of the job's figure crops (yomitoku_amd/figures.py: check_figures makes it of the public
        entry's `figures`): the crops of the page's `schema.figures` are cut from the clean - with deskew: corrected - page in the
        render stage and coded as JPEG files, and the entry gets the page's PageFigures behind the page file and in front of
        the PageSkew - (schema, PageFigures), (schema, ocr overlay, layout overlay, EncodedJpeg, PageFigures, PageSkew).
        options: carried on the job for the analyzer's own stages (TableSemanticParser: template / grid_only / kv_only); the
        pipeline does not look at it."""
        from .data.functions import load_image
        from .deskew import check_deskew

        deskew = check_deskew(deskew)
        if deskew is not None and not self._gpu:
            raise ValueError("deskew needs a HIP device: this pipeline has none (there is no host fallback)")
        with self._serve_lock, _full_gc_deferred(self.defer_full_gc), _switch_interval(self.switch_interval):
            job = self._job = _Job(overlays=overlays, options=options, files=files, deskew=deskew, figures=figures)
            if job.overlays or job.files is not None or job.figures is not None:
                self._start_render()
            n = 0
            origin = []  # page id -> (source index, frame index)
            pend_ids, pend_imgs = [], []

            held = [None, 0.0]  # the wave slot taken for the wave being collected, and how long the caller waited for it

            def flush():
                nonlocal pend_ids, pend_imgs
                if pend_ids:
                    ids, imgs, pend_ids, pend_imgs = pend_ids, pend_imgs, [], []
                    ring, held[0] = held[0], None
                    try:
                        self._launch(job, ids, imgs, ring=ring, waited=held[1] if ring is not None else 0.0)
                    except Exception as exc:  # noqa: BLE001 - e.g. a page that is not uint8 H x W x 3
                        if len(ids) == 1:
                            job.results[ids[0]] = exc
                        else:
                            with job.cond:
                                job.retries.extend(zip(ids, imgs))

            def drain_retries():
                while True:
                    with job.cond:
                        if not job.retries:
                            return
                        idx, img = job.retries.popleft()
                        job.retried_pages += 1
                    try:
                        self._launch(job, [idx], [img], retry=True)
                    except Exception as exc:  # noqa: BLE001
                        job.results[idx] = exc

            # The slot of a wave is taken BEFORE the wave's first source is pulled: `sources` may be a generator that claims
            # work from a shared counter (distributed.PageDealer) - a rank must not claim pages it has no room for yet, or the
            # end of a sharded job is as ragged as a static deal.  (A slot held while nothing is pending is given back below.)
            it = enumerate(sources)
            try:
                while True:
                    if not pend_ids and held[0] is None:
                        drain_retries()
                        t_wait = time.perf_counter()
                        held[0] = self._rings.get()
                        held[1] = time.perf_counter() - t_wait
                    try:
                        si, src = next(it)
                    except StopIteration:
                        break
                    if isinstance(src, np.ndarray):
                        frames = [src]
                    else:
                        try:
                            frames = list(load_image(src))
                        except Exception as exc:  # noqa: BLE001 - cli/main.py:555-564: log, go on with the next file
                            logger.error("cannot load %s: %s: %s", src, type(exc).__name__, exc)
                            job.results[n] = exc
                            origin.append((si, 0))
                            n += 1
                            continue
                    for fi, frame in enumerate(frames):
                        origin.append((si, fi))
                        pend_ids.append(n)
                        pend_imgs.append(frame)
                        n += 1
                        if len(pend_ids) == self.wave:
                            flush()
                flush()
            finally:
                # the source list ended on a wave boundary - or the source iterator raised (a generator over a network store,
                # KeyboardInterrupt): the exception goes to the caller, the slot goes back first, or `in_flight` such failures
                # would block every later job.  Waves already launched finish on their own and release theirs (_release)
                if held[0] is not None:
                    self._rings.put(held[0])
                    held[0] = None
            while True:
                drain_retries()
                with job.cond:
                    if job.outstanding == 0 and not job.retries:
                        break
                    job.cond.wait(timeout=0.05)
            self.last_job = {"pages": n, "waves": job.waves, "retried_pages": job.retried_pages}
            if with_source:
                return [(origin[i][0], origin[i][1], job.results[i]) for i in range(n)]
            return [job.results[i] for i in range(n)]

    def close(self):
        for name, q in self._q.items():
            for _ in range(self._workers[name]):
                q.put(_STOP)
        for t in self._threads:
            t.join(timeout=10)
        if self._render_thread is not None:
            self._render_q.put(_STOP)
            self._render_thread.join(timeout=10)
            self._render_thread = None


def _chain_priorities():
    spec = os.environ.get("YMK_CHAIN_PRIORITY", "")  # e.g. "layout:-1,ocr:0" (measurement knob)
    out = {}
    for item in filter(None, spec.split(",")):
        name, _, value = item.partition(":")
        out[name.strip()] = int(value)
    return out


class StageAnalyzer:
    """What `PagePipeline` asks of its analyzer, and the part of it that DocumentAnalyzer, TableSemanticParser and OCR share.
    The pipeline is duck-typed (the tests drive it with stubs); a real analyzer derives from this class and adds its table
    chain - or, like OCR, declares that it has none.

    Attributes the pipeline reads: `text_detector.device`, `text_recognizer` (its `rec_orientation_fallback` forces one
    recogniser lane), `split_text_across_cells` (True: `boxes` waits for the wave's `cells`, then calls `_stage_split(wave)`;
    needs the layout chain) and `chains`:

        chains              stage threads and streams                     who
        ("ocr", "layout")   all nine; `finish` after both chains          the default: DocumentAnalyzer, TableSemanticParser
        ("ocr",)            detect ... decode, finish; no layout chain    OCR

    An analyzer without the attribute runs both chains.  The stages of a chain that is not declared have no thread, no HIP
    stream and no queue, and their methods are never looked up: an analyzer need not have them.

    Stage methods, each called with the `Wave` by the stage's one thread (GPU: on that thread's HIP stream, after the wave's
    upload; the stream is waited for before the wave moves on):

        stage      chain   launches  reads                                  writes              defined
        detect     ocr     GPU       pages, ring                            maps                here
        boxes      ocr     host      maps, sizes                            dets                here
        crops      ocr     GPU       pages, dets                            rec_plan            here
        recognize  ocr     GPU       rec_plan; called (wave, lane)          rec_plan            here
        decode     ocr     host      rec_plan                               recs, rec_plan=None here
        layout     layout  GPU       pages                                  lay_raw             subclass
        tables     layout  GPU       pages, lay_raw, ids (hand-over)        lay_parsed, tab_raw subclass
        cells      layout  host      tab_raw, lay_parsed                    lays                subclass

    `_stage_finish(wave, k)` (host, subclass) returns page k's schema from dets / recs / lay_parsed / lays / imgs and the job
    (`wave.job.options`, `wave.job.overlays`); `_stage_render(wave, results)` (GPU, here; overlays jobs only) returns per page
    its pictures - pictures per page: as many as `_page_drawings(wave, k, results)` (subclass) records, the same for every page
    of an analyzer (DocumentAnalyzer and TableSemanticParser two, OCR one) -, from those drawings and `wave.pages`; `_stage_jpeg(wave, results)` (GPU,
    here; jobs with page files only) returns per page a 1-tuple with its page file, from `wave.pages` and `wave.job.files`;
    `_stage_figures(wave, results)` (GPU, here; figures jobs only) per page a 1-tuple with its PageFigures, from `wave.pages`,
    `results[k].figures` and `wave.job.figures`.  `_nets()`
    (subclass): the modules whose `model.close()` releases the analyzer's device memory.

    `handover`: None, or an object that sees - and may replace - what one stage hands to the next, AFTER the stage has
    produced it at full cost (`_handed`; yomitoku_amd.testing.Handover): measurements and tests with seeded weights, whose
    detections are noise.  A hook the object lacks - or a data attribute of that name - passes the value through."""

    split_text_across_cells = False
    chains = tuple(CHAINS)  # both: an analyzer without a layout chain says ("ocr",)

    def _init_chains(self):
        """The constructors' shared part: the two chains of a page or wave (OCR; layout / tables) run on one thread and HIP
        stream each; `concurrent_chains` False runs them one after the other on the caller's thread and stream (profiling: a
        kernel's timing then brackets that kernel alone; same results)."""
        self._pool = ThreadPoolExecutor(max_workers=2)
        self._streams = {}
        self.concurrent_chains = True
        # HIP stream priority per chain (0 = default, -1 = high).  Measured on the analyzer bench: raising either chain
        # LOWERS the throughput (66.9 -> 62.3 layout high, 64.2 ocr high), so the default is no priority
        self.chain_priority = _chain_priorities()
        self.handover = None
        self._render_pinned = {}  # wave slot -> [pinned buffer the slot's canvases come back through] (serve(overlays=True))
        self._jpeg_scratch = {}  # wave slot -> the encoder's device and pinned buffers, made when the slot first needs them (serve(jpeg=...))
        self._figures_scratch = {}  # wave slot -> the figure crops' and their encoder's buffers, likewise (serve(figures=...))
        self._pipeline = None

    # ---- the two concurrent chains, each on its own HIP stream
    def _submit(self, name, fn, *args):
        """A chain as a future: on its own thread + HIP stream, or - concurrent_chains False - run right here."""
        if self.concurrent_chains:
            return self._pool.submit(self._on_stream, name, fn, *args)
        f = Future()
        try:
            f.set_result(fn(*args))
        except BaseException as exc:  # noqa: BLE001 - delivered by f.result(), like a pool future
            f.set_exception(exc)
        return f

    def _on_stream(self, name, fn, *args):
        dev = self.text_detector.device
        stream = self._streams.get(name)
        if stream is None:
            stream = self._streams[name] = torch.cuda.Stream(device=dev, priority=self.chain_priority.get(name, 0))
        stream.wait_stream(torch.cuda.default_stream(dev))  # the page upload was issued there
        with torch.cuda.stream(stream):
            out = fn(*args)
            stream.synchronize()
        return out

    def _handed(self, what, wave, value):
        fn = getattr(self.handover, what, None)  # a hook is a method: an attribute of that name that holds data is none
        return fn(wave, value) if callable(fn) else value

    # ---- the OCR chain
    def _stage_detect(self, wave):
        """DBNet forwards over same-size pages of the wave; the maps come back into the wave slot's pinned buffers."""
        wave.maps = self._handed("maps", wave, self.text_detector.forward_pages(wave.pages, ring=wave.ring))

    def _stage_boxes(self, wave):
        """DB box extraction (C++, GIL released), the pages of the wave concurrently."""
        wave.dets = self._handed("boxes", wave, self.text_detector.extract_boxes(wave.maps, wave.sizes))

    def _stage_crops(self, wave):
        """Per-page mini-batches (bucketing, width budget) and the crop kernels that build their tensors."""
        wave.rec_plan = self.text_recognizer.plan_pages(wave.pages, [d.points for d in wave.dets])

    def _stage_recognize(self, wave, lane=0):
        """One grouped PARSeq forward over the mini-batches of all pages of the wave, on the recogniser handle of `lane`
        (serve keeps two forwards in flight: TextRecognizer.replica_model); with `rec_orientation_fallback` the decode
        happens here too, because the retry runs further forwards."""
        self.text_recognizer.forward_plan(wave.rec_plan, self.text_recognizer.replica_model(lane))
        if self.text_recognizer.rec_orientation_fallback:
            self._stage_decode(wave)

    def _stage_decode(self, wave):
        """Token decode and un-permutation on the host."""
        if wave.recs is None:
            wave.recs = self.text_recognizer.finish_plan(wave.rec_plan)
            wave.rec_plan = None

    def _ocr_drawing(self, wave, k):
        """The OCR picture of page k of a finished wave, recorded for the wave renderer: the detection quads, then the
        recognised strings in the recogniser's configured font, size and colour."""
        from .utils import visualizer as V

        ocr = V.RunOverlay()
        V._det_commands(ocr, wave.dets[k].points)
        cfg = self.text_recognizer._cfg.visualize
        V._rec_commands(ocr, wave.recs[k], V.load_font(cfg.font, cfg.font_size), cfg.font_size, tuple(cfg.color[::-1]))
        return ocr

    def _stage_render(self, wave, results, pinned=None):
        """Overlays: per page of the wave its pictures as owned host arrays - as many as `_page_drawings` records for a page, in
        that order (the same number for every page of an analyzer: DocumentAnalyzer and TableSemanticParser two, OCR one);
        an exception for a page whose drawing raised, None for a page that had already failed.  All canvases of the wave are
        drawn by the wave renderer (utils/visualizer.py: render_wave) on the calling thread's stream and come back through
        `pinned` - by default the wave slot's pinned buffer."""
        from .utils.visualizer import render_wave

        out = [None] * len(wave)
        live, drawings = [], []
        for k in range(len(wave)):
            if isinstance(results[k], BaseException):
                continue
            try:
                made = tuple(self._page_drawings(wave, k, results[k]))
            except Exception as exc:  # noqa: BLE001 - only this page fails
                out[k] = exc
                continue
            drawings.append(made)
            live.append(k)
        wave.dags = None
        if live:
            n = len(drawings[0])  # pictures per page: what the analyzer draws (OCR one, the others two)
            assert all(len(made) == n for made in drawings), "an analyzer draws the same number of pictures for every page"
            if pinned is None:
                pinned = self._render_pinned.setdefault(wave.ring, [None])
            images = render_wave([wave.pages[k] for k in live for _ in range(n)], [d for made in drawings for d in made], pinned)
            for j, k in enumerate(live):
                out[k] = tuple(images[n * j : n * (j + 1)])
        return out

    def _stage_jpeg(self, wave, results, scratch=None):
        """Page files: per page of the wave a 1-tuple with its EncodedJpeg (an EncodedBilevel, an EncodedMrc or an EncodedLossless
        where `wave.job.files`, the job's PageFiles, gives the page one), an exception for a page
        that could not be encoded, None for a page that had already failed.  All pages of the wave are encoded together on
        the calling thread's stream (yomitoku_amd/jpeg.py: encode_page_files) from `wave.pages` - the clean pages: the
        overlays are drawn on copies - with `scratch`, by default the wave slot's."""
        out = [None] * len(wave)
        live = [k for k in range(len(wave)) if not isinstance(results[k], BaseException)]
        if live:
            if scratch is None:
                scratch = self._jpeg_scratch.setdefault(wave.ring, {})
            files = encode_page_files([wave.pages[k] for k in live], wave.job.files, scratch=scratch)
            for k, made in zip(live, files):
                out[k] = made if isinstance(made, BaseException) else (made,)
        return out

    def _stage_figures(self, wave, results, scratch=None):
        """Figure crops: per page of the wave a 1-tuple with its PageFigures - the crops of `results[k].figures`, cut from
        `wave.pages[k]` (the clean and, with deskew, corrected page) and coded as `wave.job.figures` says -, an exception for a page
        that is no page, None for a page that had already failed.  All pages of the wave go through one call on the calling
        thread's stream (yomitoku_amd/figures.py: crop_figure_files) with `scratch`, by default the wave slot's own."""
        from .figures import crop_figure_files

        out = [None] * len(wave)
        live = [k for k in range(len(wave)) if not isinstance(results[k], BaseException)]
        if live:
            if scratch is None:
                scratch = self._figures_scratch.setdefault(wave.ring, {})
            made = crop_figure_files([wave.pages[k] for k in live], [[f.box for f in results[k].figures] for k in live],
                                     wave.job.figures, scratch=scratch)
            for k, one in zip(live, made):
                out[k] = one if isinstance(one, BaseException) else (one,)
        return out

    # ---- one wave at a time (`analyze_pages`, `parse_pages`): the same stage methods as two concurrent chains
    def _recognize_wave(self, wave):
        self._stage_crops(wave)
        self._stage_recognize(wave)
        self._stage_decode(wave)

    def _layout_wave(self, wave):
        self._stage_layout(wave)
        self._stage_tables(wave)
        self._stage_cells(wave)

    def _ocr_wave(self, wave):
        self._stage_detect(wave)
        self._stage_boxes(wave)
        if not self.split_text_across_cells:
            self._recognize_wave(wave)

    def _run_wave(self, imgs, start, job=None):
        """`imgs` (pages `start`... of a call) uploaded and through every stage before `finish`: the finished Wave."""
        dev = self.text_detector.device
        pages = [img if isinstance(img, torch.Tensor) else imaging.page_to_device(img, dev) for img in imgs]
        wave = Wave(ids=range(start, start + len(imgs)), imgs=imgs, pages=pages, job=job)
        f_ocr = self._submit("ocr", self._ocr_wave, wave)
        f_lay = self._submit("layout", self._layout_wave, wave)
        f_ocr.result()
        f_lay.result()
        if self.split_text_across_cells:
            self._stage_split(wave)
            self._submit("ocr", self._recognize_wave, wave).result()
        return wave

    # ---- the pipeline of this analyzer
    def _serve(self, sources, wave, in_flight, defer_full_gc, with_source, rec_lanes, overlays, options=None, files=None, deskew=False,
               figures=None):
        """What the public `serve()`s share: the pipeline is built on first use and rebuilt when its shape changes."""
        pipe = self._pipeline
        if pipe is None or (pipe.wave, pipe.in_flight, pipe.rec_lanes_asked) != (max(1, int(wave)), max(1, int(in_flight)), int(rec_lanes)):
            if pipe is not None:
                pipe.close()
            pipe = self._pipeline = PagePipeline(self, wave=wave, in_flight=in_flight, rec_lanes=rec_lanes)
        pipe.defer_full_gc = bool(defer_full_gc)
        return pipe.serve(sources, with_source=with_source, overlays=overlays, options=options, files=files, deskew=deskew, figures=figures)

    def close(self, release_models: bool = True):
        """Stop the pipeline threads, drop the render buffers, release the extra recogniser handles and - `release_models` -
        the device memory of the four nets (weights and the reserved workspaces: tens of GB per analyzer).  The analyzer stays
        usable: a net rebuilds its handle from the state dict it holds the next time it is called."""
        if self._pipeline is not None:
            self._pipeline.close()
            self._pipeline = None
        self._render_pinned.clear()
        self._jpeg_scratch.clear()
        self._figures_scratch.clear()
        self.text_recognizer.close_replicas()
        if release_models:
            for module in self._nets():
                module.model.close()
