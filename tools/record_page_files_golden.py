#!/usr/bin/env python3
"""What the page-file entries launch, wait for and write, recorded on a HIP device: the fixture that holds a change of
yomitoku_amd/jpeg.py, ccitt.py, mrc.py or deskew.py to the same device work in the same order and to the same bytes.

    python tools/record_page_files_golden.py                 # writes tests/golden/page_files_calls.json
    python tools/record_page_files_golden.py --out FILE

Only the public entries are called - `encode_jpeg_pages`, `encode_g4_pages`, `encode_mrc_pages`, `deskew_pages` - so the tool
runs unchanged on any commit that has them: record on the commit a change starts from, test on the change
(tests/test_page_files_calls_gpu.py imports `record_all` from here).  While a case runs, what `yomitoku_amd._lib.load()`
returns is a proxy that logs the name of every stream-taking entry in `LAUNCHES`, and `torch.cuda.Stream.synchronize` logs
"wait".  Per case the file holds that sequence and per page its entry: the class name, the fields that are not bytes, and
the sha256 and length of every file's bytes (an EncodedMrc: of its three parts) - or the exception's class and text.  Data only.
"""
import argparse
import contextlib
import dataclasses
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "page_files_calls.json")
PRESET = "low"  # max_long_side 1500: the two strips are larger
LAUNCHES = ("ymk_g4_test_pack", "ymk_bin_test_hist", "ymk_bin_otsu", "ymk_bin_otsu_pack", "ymk_bin_adaptive_pack", "ymk_mrc_pages",
            "ymk_pil_resize_u8", "ymk_jpeg_pages_grey", "ymk_jpeg_encode_pages", "ymk_jpeg_encode_pages_opt", "ymk_g4_encode_pages",
            "ymk_dsk_pages")
KINDS = ("jpeg-colour", "jpeg-grey", "resized", "group4", "layered", "exception")


def batch() -> list:
    """The eight pages: colour, grey-valued colour, grey (odd width), two-valued, white, a strip larger than the preset with ink,
    a white one, and an array that is no page."""
    from yomitoku_amd.utils.synth import synthetic_page_with_truth

    page = synthetic_page_with_truth(3, 600, 640)[0]
    colour = np.ascontiguousarray(page[0:96, 0:128])
    assert (colour[..., 0] != colour[..., 1]).any(), "the colour crop has no pixel with B != G"
    green = page[..., 1]
    return [colour,
            np.ascontiguousarray(np.stack([green[100:260, 60:260]] * 3, axis=-1)),
            np.ascontiguousarray(green[100:220, 60:393]),
            np.where(green[0:96, 0:128] < 128, 0, 255).astype(np.uint8),
            np.full((64, 48, 3), 255, np.uint8),
            np.ascontiguousarray(np.tile(page[200:208], (1, 3, 1))),
            np.full((8, 1600, 3), 255, np.uint8),
            np.zeros((16, 16, 3), np.float32)]


STRIPS = (5, 6)  # the two pages of `batch()` that the preset resizes


def kinds_of(pages) -> list:
    """Per page, by the definitions (tests/ccitt_ref.py, binarize_ref.py, mrc_ref.py) on the CPU, what the cases can make of it."""
    from yomitoku_amd.utils.searchable_pdf import IMAGE_QUALITY_PRESETS
    from tests import binarize_ref, ccitt_ref, mrc_ref

    long_side = IMAGE_QUALITY_PRESETS[PRESET]["max_long_side"]
    out = []
    for p in pages:
        if p.dtype != np.uint8:
            out.append({"exception"})
            continue
        kinds, large = set(), max(p.shape[:2]) > long_side
        layered = mrc_ref.separate(p)[0] == 1
        if ccitt_ref.is_bilevel(p):
            kinds.add("group4")
        if layered:
            kinds.add("layered")
        if large and not layered:
            kinds.add("resized")
        if p.ndim == 3 and not large:
            kinds.add("jpeg-grey" if binarize_ref.is_grey_valued(p) else "jpeg-colour")
        out.append(kinds)
    return out


def check_batch(pages):
    found = set().union(*kinds_of(pages))
    assert found >= set(KINDS), f"the batch lacks {sorted(set(KINDS) - found)}"


class _Logged:
    """The loaded library with the entries of LAUNCHES logging their names."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in LAUNCHES:
            return fn

        def logged(*args):
            self._log.append(name)
            return fn(*args)

        return logged


@contextlib.contextmanager
def recording():
    """-> the list that the launches and waits made inside the block are appended to."""
    import torch

    from yomitoku_amd import _lib

    log, real, wait = [], _lib.load(), torch.cuda.Stream.synchronize

    def synchronize(self):
        log.append("wait")
        return wait(self)

    _lib._lib, torch.cuda.Stream.synchronize = _Logged(real, log), synchronize
    try:
        yield log
    finally:
        _lib._lib, torch.cuda.Stream.synchronize = real, wait


def _digest(data) -> dict:
    return {"sha256": hashlib.sha256(bytes(data)).hexdigest(), "length": len(data)}


def describe(entry) -> dict:
    """An entry as data: an exception's class and text; else the class name, the plain fields, the digest of `data`, and the
    same of every part that is itself such an object."""
    import torch

    if isinstance(entry, BaseException):
        return {"exception": type(entry).__name__, "text": str(entry)}
    if isinstance(entry, torch.Tensor):
        return {"class": "Tensor", "shape": list(entry.shape), **_digest(entry.cpu().numpy().tobytes())}
    out = {"class": type(entry).__name__}
    for f in dataclasses.fields(entry):
        value = getattr(entry, f.name)
        if f.name == "data":
            out.update(_digest(value))
        elif dataclasses.is_dataclass(value):
            out[f.name] = describe(value)
        elif isinstance(value, np.ndarray):
            out[f.name] = value.tolist()
        else:
            out[f.name] = value
    return out


def cases(pages) -> list:
    """(name, [function of a scratch dict -> the entries, ...]): the functions of one case share one scratch dict."""
    from yomitoku_amd.ccitt import encode_g4_pages
    from yomitoku_amd.deskew import deskew_pages
    from yomitoku_amd.jpeg import encode_jpeg_pages
    from yomitoku_amd.mrc import encode_mrc_pages

    few = [p for k, p in enumerate(pages) if k not in STRIPS]

    def jpeg(which, **kw):
        return lambda scratch: encode_jpeg_pages(which, PRESET, scratch=scratch, **kw)

    def skewed(scratch):
        corrected, skews = deskew_pages(pages[:1] + pages[2:3], scratch=scratch)
        return list(corrected) + list(skews)

    layered = dict(bilevel="adaptive", mrc=True, optimize=True, subsampling="4:4:4")
    return [("defaults", [jpeg(pages)]),
            ("optimize", [jpeg(pages, optimize=True)]),
            ("grey_auto", [jpeg(pages, grey="auto")]),
            ("grey_auto_no_strips", [jpeg(few, grey="auto")]),
            ("bilevel_auto_grey_auto_no_strips", [jpeg(few, bilevel="auto", grey="auto")]),
            ("bilevel_otsu", [jpeg(pages, bilevel="otsu")]),
            ("bilevel_adaptive_mrc_optimize_444", [jpeg(pages, **layered)]),
            ("mrc_cells_1_4", [jpeg(pages, mrc={"bg_cell": 1, "fg_cell": 4})]),
            ("one_scratch_two_cases", [jpeg(pages, **layered), jpeg(pages, grey="auto")]),
            ("g4_plain", [lambda scratch: encode_g4_pages(pages, scratch=scratch)]),
            ("g4_otsu", [lambda scratch: encode_g4_pages(pages, scratch=scratch, binarize="otsu")]),
            ("encode_mrc_pages", [lambda scratch: encode_mrc_pages(pages, PRESET, scratch=scratch)]),
            ("deskew_two_pages", [skewed])]


def record_all(check: bool = False) -> dict:
    """{case: {"calls": [...], "entries": [...]}} of every case, on the current HIP device.  check: hold the batch to `KINDS`
    by the definitions first, on the CPU."""
    pages = batch()
    if check:
        check_batch(pages)
    out = {}
    for name, runs in cases(pages):
        scratch, entries = {}, []
        with recording() as log:
            for run in runs:
                entries += [describe(e) for e in run(scratch)]
        out[name] = {"calls": list(log), "entries": entries}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    recorded = record_all(check=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(recorded, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, case in recorded.items():
        print(f"{name}: {' '.join(case['calls'])}")
        print("   ", [e.get("class", e.get("exception")) for e in case["entries"]])


if __name__ == "__main__":
    main()
