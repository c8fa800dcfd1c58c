"""What tests/test_conv_views_gpu.py and tests/test_conv_planes_gpu.py share: the float64 reference of one convolution launch,
the kernel-route switches and their reset, the launch table of a call, and the checks on sentinels and max|y| records."""
from __future__ import annotations

import contextlib
import ctypes

import torch
import torch.nn.functional as F

ACT64 = {"none": lambda t: t, "relu": torch.relu, "silu": F.silu, "gelu": F.gelu, "sigmoid": torch.sigmoid}

TOL_EXACT = 3e-6  # of max|ref|: one launch of the exact fp32 kernels against float64 (tests/test_conv_split_gpu.py)
TOL_F16 = 4e-6    # the same on two fp16 planes

# the short list of exact-kernel routes that covers every epilogue: the library's choice (split-K at these sizes), conv_igemm
# only, the widest and the narrowest split-K shape, and conv_igemm with the LDS-staged, the direct and the default epilogue
ROUTES = [("auto", {}), ("no_splitk", {"no_splitk": 1}), ("splitk0", {"splitk_force": 0}), ("splitk4", {"splitk_force": 4}),
          ("fast3-staged", {"no_splitk": 1, "conv_fast": 3}), ("fast7-direct", {"no_splitk": 1, "conv_fast": 7}),
          ("fast27", {"no_splitk": 1, "conv_fast": 27})]
ROUTE_IDS = [r[0] for r in ROUTES]
RESET = (("splitk_force", -1), ("no_splitk", 0), ("conv_variant", 0), ("conv_fast", 27), ("conv_split", -1), ("conv_split_tile", 0),
         ("gemm_row_limit", 0), ("act_planes", 1))


@contextlib.contextmanager
def options(opts):
    """ymk_debug_option switches for the block; every one this module knows is back at its default afterwards."""
    from yomitoku_amd import _lib

    try:
        for key, val in opts.items():
            _lib.debug_option(key, val)
        yield
    finally:
        for key, val in RESET:
            _lib.debug_option(key, val)


def conv_ref64(x, wt, scale=None, bias=None, res=None, stride=1, pad=0, dil=1, act="none", res_post=False):
    """float64 on the CPU: act(scale * conv(x) + bias + res), or res + act(...) with res_post; res NCHW or a [cout] vector."""
    r = F.conv2d(x.double(), wt.double(), None, stride, pad, dil)
    if scale is not None:
        r = r * scale.double().view(1, -1, 1, 1)
    if bias is not None:
        r = r + bias.double().view(1, -1, 1, 1)
    rr = None if res is None else (res.double().view(1, -1, 1, 1) if res.dim() == 1 else res.double())
    if rr is not None and not res_post:
        r = r + rr
    r = ACT64[act](r)
    if rr is not None and res_post:
        r = r + rr
    return r


def rel_err(got, ref):
    return float((got.double().cpu() - ref).abs().max()) / float(ref.abs().max())


def launches(fn):
    """(fn(), [(ms, flop, bytes, mfma_products)] of the convolution launches fn made)."""
    from yomitoku_amd import _lib

    lib = _lib.load()
    _lib.check(lib.ymk_prof_begin(), "ymk_prof_begin")
    try:
        out = fn()
    finally:
        ms, fl, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        _lib.check(lib.ymk_prof_end(ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(n)), "ymk_prof_end")
    return out, _lib.prof_launch_table()


def is_sentinel(t):
    from tests import hipops

    return t.view(torch.int32) == hipops.SENTINEL


def check_outside_untouched(buf, c0, c):
    """every word of the NHWC buffer outside channels c0 .. c0 + c - 1 still holds the sentinel"""
    s = is_sentinel(buf)
    assert bool(s[..., :c0].all()) and bool(s[..., c0 + c:].all()), "a store landed outside the output view"


def record_value(rec):
    """the record's maximum (as int bits) after checking that nothing but word 0 of its 32 lines was written"""
    lines = rec.cpu().view(32, 32)
    assert int(lines[:, 1:].abs().max()) == 0, "a word off the record's 32 lines was written"
    return int(lines[:, 0].max())


def check_record(rec, stored):
    """the record equals, as an integer, the bit pattern of max|y| over the values the launch stored (an identity: amax_fold
    keeps the largest bit pattern of |v| of what a thread stores, amax_commit takes maxima)"""
    want = int(stored.float().abs().max().view(torch.int32)) if stored.numel() else 0
    got = record_value(rec)
    assert got == want, f"record {got:#x} != bits of max|y| {want:#x}"
