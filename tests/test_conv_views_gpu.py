"""Single launches of the convolution kernels with everything ConvK carries that ymk_op_conv2d pins (ymk_op_conv2d_view):
leading dimensions that differ from the channel count (Tensor::slice_c views), a residual row broadcast to every pixel, the
residual behind the activation, rectangular kernels and strides (the PARSeq patchify), the row predicate of the grouped greedy
loop and the max|y| record a launch leaves for its consumer - each against torch.nn.functional.conv2d in float64 on the CPU
(3e-6 of max|ref| on the exact kernels, 4e-6 on two fp16 planes), bit for bit against the same data passed contiguously, and
with a sentinel in every word the launch must not write."""
import functools

import pytest
import torch

from tests.conv_ref import (ROUTE_IDS, ROUTES, TOL_EXACT, TOL_F16, check_outside_untouched, check_record, conv_ref64, is_sentinel,
                            launches, options, record_value, rel_err)

pytestmark = pytest.mark.gpu

KERNELS = {  # name -> (k, stride, pad, dil, act)
    "1x1": (1, 1, 0, 1, "silu"),
    "3x3p1": (3, 1, 1, 1, "relu"),
    "3x3s2": (3, 2, 1, 1, "none"),
    "3x3d2": (3, 1, 2, 2, "gelu"),
}
# (channels, (first channel, ld)) of the input views; (cout, output view, residual view): the DBNet fuse slice, a 36-channel
# slice that is 16-byte but not 128-byte aligned, and an odd leading dimension that forces the scalar stores
IN_VIEWS = [(32, (32, 96)), (36, (4, 96))]
OUT_VIEWS = [(64, (64, 256), (4, 72)), (36, (4, 256), (8, 48)), (36, (0, 37), (1, 41))]


@functools.lru_cache(maxsize=None)
def _operands(cin, cout, kname, n=2, h=9, w=11, seed=5):
    """x, weight, scale, bias, residual and the float64 reference of one layer, computed once and shared (never modified)"""
    k, stride, pad, dil, act = KERNELS[kname]
    g = torch.Generator().manual_seed(seed + 1000 * cin + cout)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    sc, bi = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    ref0 = conv_ref64(x, wt, sc, bi, None, stride, pad, dil)
    res = torch.randn(ref0.shape, generator=g)
    return x, wt, sc, bi, res, conv_ref64(x, wt, sc, bi, res, stride, pad, dil, act)


def _check_view_case(dev, cin, in_view, cout, out_view, res_view, kname, tol, shape=(2, 9, 11), compare_op=True):
    from tests import hipops

    k, stride, pad, dil, act = KERNELS[kname]
    x, wt, sc, bi, res, ref = _operands(cin, cout, kname, *shape)
    xd, rd = x.to(dev), res.to(dev)
    y, buf, rec = hipops.conv2d_view(xd, wt, sc, bi, rd, stride, pad, dil, act, in_view=in_view, out_view=out_view,
                                     res_view=res_view, record=True)
    yc, _, recc = hipops.conv2d_view(xd, wt, sc, bi, rd, stride, pad, dil, act, record=True)
    err = rel_err(y, ref)
    print(f"view {kname} cin={cin}@{in_view} cout={cout}@{out_view} res@{res_view}: err {err:.2e}")
    assert not bool(torch.isnan(y).any()), "NaN: a channel outside the input or residual view entered a product (or a word of the view was not written)"
    assert err < tol, err
    assert torch.equal(y, yc), "a leading dimension moves addresses, not arithmetic"
    check_outside_untouched(buf, out_view[0], cout)
    check_record(rec, y)
    check_record(recc, yc)
    if compare_op:  # ld == c: the new entry point and ymk_op_conv2d are the same launch
        assert torch.equal(yc, hipops.conv2d(xd, wt, sc, bi, rd, stride, pad, dil, act))
    else:  # fp16-split kernels: the caller's max|x| record instead of the pass over the view - the same scale, the same bits
        yr = hipops.conv2d_view(xd, wt, sc, bi, rd, stride, pad, dil, act, in_view=in_view, out_view=out_view, res_view=res_view,
                                amax_in=hipops.amax_record(float(x.abs().max()), dev))[0]
        assert torch.equal(yr, y), "a record of the true max|x| and the measured maximum give one scale"


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("kname", list(KERNELS))
def test_views_on_the_exact_kernels(dev, kname, route):
    with options(route[1]):
        for cin, in_view in IN_VIEWS:
            for cout, out_view, res_view in OUT_VIEWS:
                _check_view_case(dev, cin, in_view, cout, out_view, res_view, kname, TOL_EXACT)


def test_view_entry_equals_conv2d_on_every_case_of_the_operator_suite(dev):
    """ymk_op_conv2d_view at ld == c against ymk_op_conv2d, bit for bit, on tests/test_ops_gpu.py::CASES"""
    from tests import hipops
    from tests.test_ops_gpu import CASES

    for case in CASES:
        n, cin, h, w, cout, k, stride, pad, dil = case
        g = torch.Generator().manual_seed(23)
        x = torch.randn(n, cin, h, w, generator=g).to(dev)
        wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
        sc, bi = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
        oh, ow = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1, (w + 2 * pad - dil * (k - 1) - 1) // stride + 1
        res = torch.randn(n, cout, oh, ow, generator=g).to(dev)
        want = hipops.conv2d(x, wt, sc, bi, res, stride, pad, dil, "relu")
        got, _, rec = hipops.conv2d_view(x, wt, sc, bi, res, stride, pad, dil, "relu", record=True)
        assert torch.equal(got, want), case
        check_record(rec, got)


# ---- the fp16-split kernels: only launches that fill the chip reach them (>= 256 blocks of 128 x 64)
SPLIT_SHAPE = (1, 150, 220)  # M = 33 000
SPLIT_CASES = [  # tile, kernel, shape, cin, in view, cout, out view, res view
    (3, "1x1", SPLIT_SHAPE, 64, (32, 128), 64, (64, 256), (4, 72)),
    (3, "3x3p1", SPLIT_SHAPE, 64, (32, 128), 64, (64, 256), (4, 72)),
    (21, "1x1", SPLIT_SHAPE, 64, (32, 128), 64, (64, 256), (4, 72)),
    (21, "3x3p1", SPLIT_SHAPE, 64, (32, 128), 64, (64, 256), (4, 72)),
    (21, "3x3d2", SPLIT_SHAPE, 64, (32, 128), 64, (64, 256), (4, 72)),
    (21, "3x3s2", (1, 300, 440), 32, (32, 96), 64, (64, 256), (4, 72)),   # 150 x 220 outputs again
    (21, "3x3p1", SPLIT_SHAPE, 36, (4, 96), 36, (4, 256), (8, 48)),        # a partial channel tile in every tap
    (3, "1x1", SPLIT_SHAPE, 36, (4, 96), 36, (0, 37), (1, 41)),            # scalar stores on a strided output
    (30, "1x1", SPLIT_SHAPE, 128, (32, 192), 128, (64, 256), (4, 136)),
    (30, "1x1", SPLIT_SHAPE, 36, (4, 96), 36, (4, 256), (8, 48)),
]


@pytest.mark.parametrize("case", SPLIT_CASES, ids=[f"tile{c[0]}-{c[1]}-c{c[3]}-o{c[5]}@{c[6][1]}" for c in SPLIT_CASES])
def test_views_on_the_fp16_split_kernels(dev, case):
    from yomitoku_amd import _lib

    tile, kname, shape, cin, in_view, cout, out_view, res_view = case
    astat0 = _lib.stat("astat_launches")
    with options({"conv_split": 16, "conv_split_tile": tile}):
        _, table = launches(lambda: _check_view_case(dev, cin, in_view, cout, out_view, res_view, kname, TOL_F16, shape, compare_op=False))
    assert len(table) == 3 and all(row[3] == 3.0 for row in table), f"not the fp16-split family: {table}"
    assert (_lib.stat("astat_launches") - astat0 == 3) == (tile == 30), "the A-stationary kernel ran exactly where it was asked for"


# ---- one residual row for every pixel
@pytest.mark.parametrize("route", [("prefetch", {"no_splitk": 1, "conv_fast": 27}), ("no-prefetch", {"no_splitk": 1, "conv_fast": 25}),
                                   ("auto", {}), ("direct", {"no_splitk": 1, "conv_fast": 7})], ids=lambda r: r[0])
@pytest.mark.parametrize("cout,out_view,res_view", [(64, (64, 256), (4, 72)), (64, None, None), (36, (0, 37), (1, 41))],
                         ids=["vector-view", "vector", "scalar"])
def test_broadcast_residual(dev, cout, out_view, res_view, route):
    from tests import hipops

    x, wt, sc, bi, _, _ = _operands(32, cout, "3x3p1")
    row = torch.randn(cout, generator=torch.Generator().manual_seed(3)) * 2.0
    ref = conv_ref64(x, wt, sc, bi, row, 1, 1, 1, "relu")
    with options(route[1]):
        y, buf, rec = hipops.conv2d_view(x.to(dev), wt, sc, bi, row, 1, 1, 1, "relu", out_view=out_view, res_view=res_view, record=True)
        full = hipops.conv2d_view(x.to(dev), wt, sc, bi, row.view(1, -1, 1, 1).expand(ref.shape).contiguous(), 1, 1, 1, "relu")[0]
    err = rel_err(y, ref)
    print(f"res_ld 0, cout {cout} @ {out_view}, {route[0]}: err {err:.2e}")
    assert err < TOL_EXACT and not bool(torch.isnan(y).any())
    assert torch.equal(y, full), "one broadcast row and the same row stored per pixel are the same sum"
    if out_view:
        check_outside_untouched(buf, out_view[0], cout)
    check_record(rec, y)


# ---- y = res + act(conv)
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("act", ["none", "relu", "silu", "gelu", "sigmoid"])
def test_residual_behind_the_activation(dev, act, route):
    """res_post on the vector stores (cout 64), the scalar stores (cout 36 at ld 37) and, through the routes, the direct
    epilogue: the residual has the outputs' own standard deviation, so act(v + r) and act(v) + r are far apart."""
    from tests import hipops

    for cout, out_view, res_view in ((64, None, (4, 72)), (36, (0, 37), (1, 41))):
        x, wt, sc, bi, res, _ = _operands(32, cout, "3x3p1")
        ref = conv_ref64(x, wt, sc, bi, res, 1, 1, 1, act, res_post=True)
        other = conv_ref64(x, wt, sc, bi, res, 1, 1, 1, act, res_post=False)
        if act != "none":
            assert rel_err(other, ref) > 1e-2  # the two orders differ by far more than the tolerance
        with options(route[1]):
            y, buf, rec = hipops.conv2d_view(x.to(dev), wt, sc, bi, res.to(dev), 1, 1, 1, act, res_post=True, out_view=out_view,
                                             res_view=res_view, record=True)
        err = rel_err(y, ref)
        print(f"res_post {act} cout {cout} {route[0]}: err {err:.2e}")
        assert err < TOL_EXACT, err
        check_record(rec, y)


@pytest.mark.parametrize("tile,cin,cout", [(30, 128, 128), (3, 64, 64), (21, 64, 64)])
@pytest.mark.parametrize("act", ["silu", "sigmoid"])
def test_residual_behind_the_activation_on_the_fp16_split_kernels(dev, act, tile, cin, cout):
    from tests import hipops

    g = torch.Generator().manual_seed(41)
    x = torch.randn(1, cin, 150, 220, generator=g)
    wt = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    bi = torch.randn(cout, generator=g)
    res = torch.randn(1, cout, 150, 220, generator=g)
    ref = conv_ref64(x, wt, None, bi, res, act=act, res_post=True)
    with options({"conv_split": 16, "conv_split_tile": tile}):
        (y, _, rec), table = launches(lambda: hipops.conv2d_view(x.to(dev), wt, None, bi, res.to(dev), act=act, res_post=True,
                                                                 res_view=(4, cout + 8), record=True))
    err = rel_err(y, ref)
    print(f"res_post {act} tile {tile}: err {err:.2e}")
    assert [row[3] for row in table] == [3.0]
    assert err < TOL_F16, err
    check_record(rec, y)


# ---- rectangular kernels and strides
@pytest.mark.parametrize("cout", [192, 384])
@pytest.mark.parametrize("width", [104, 100])  # 100: the last, partial patch is dropped
def test_patchify_4x8(dev, width, cout):
    """The PARSeq-tiny patch embedding: a 3-channel image as NHWC4, kernel 4 x 8, stride (4, 8), the 4-channel stem kernel."""
    from tests import hipops

    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, 3, 32, width, generator=g)
    wt = torch.randn(cout, 3, 4, 8, generator=g) / 96 ** 0.5
    bi = torch.randn(cout, generator=g)
    ref = conv_ref64(x, wt, None, bi, None, (4, 8))
    assert ref.shape == (2, cout, 8, width // 8)
    y, _, rec = hipops.conv2d_view(x.to(dev), wt, None, bi, None, (4, 8), record=True)
    err = rel_err(y, ref)
    print(f"patchify 32 x {width} -> {cout}: err {err:.2e}")
    assert y.shape == ref.shape and err < TOL_EXACT, err
    check_record(rec, y)


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_rectangular_kernel_and_stride(dev, route):
    from tests import hipops

    g = torch.Generator().manual_seed(14)
    x = torch.randn(2, 64, 9, 11, generator=g)
    wt = torch.randn(64, 64, 1, 3, generator=g) / 192 ** 0.5
    sc, bi = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g)
    ref = conv_ref64(x, wt, sc, bi, None, (1, 2), 1, 1, "silu")  # one pad for both axes: two rows of pure bias above and below
    with options(route[1]):
        y, buf, rec = hipops.conv2d_view(x.to(dev), wt, sc, bi, None, (1, 2), 1, 1, "silu", in_view=(32, 128), out_view=(4, 72), record=True)
    err = rel_err(y, ref)
    print(f"1 x 3, stride (1, 2), {route[0]}: err {err:.2e}")
    assert y.shape == ref.shape == (2, 64, 11, 6) and err < TOL_EXACT, err
    check_outside_untouched(buf, 4, 64)
    check_record(rec, y)


# ---- the row predicate of the grouped greedy loop
def _groups(m, run0, run, tail):
    """Three interleaved groups; group 1 (the one the tests close) also owns one contiguous run and the tail of M, besides its
    scattered single rows."""
    rg = torch.arange(m, dtype=torch.int32) % 3
    rg[run0:run0 + run] = 1
    rg[m - tail:] = 1
    return rg


@functools.lru_cache(maxsize=None)
def _linear(m, cin=64, cout=96):
    g = torch.Generator().manual_seed(19)
    x = torch.randn(1, cin, 1, m, generator=g)
    wt = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    bi = torch.randn(cout, generator=g)
    res = torch.randn(1, cout, 1, m, generator=g)
    return x, wt, bi, res, conv_ref64(x, wt, None, bi, res, act="gelu")


def _check_row_predicate(dev, m, run0, run, tail, tol, max_tile):
    from tests import hipops

    x, wt, bi, res, ref = _linear(m)
    xd, rd = x.to(dev), res.to(dev)
    rg = _groups(m, run0, run, tail).to(dev)
    kw = dict(act="gelu", in_view=(32, 128), out_view=(32, 160), res_view=(4, 104), record=True)

    def run_with(open_words):
        return hipops.conv2d_view(xd, wt, None, bi, rd, row_group=rg, group_open=torch.tensor(open_words, dtype=torch.int32, device=dev), **kw)

    plain, _, rec_plain = hipops.conv2d_view(xd, wt, None, bi, rd, **kw)
    y, buf, rec = run_with([1, 0, 1])
    rows = y[0, :, 0, :].t().contiguous().cpu()  # [m][cout]
    want = ref[0, :, 0, :].t()
    closed = (rg.cpu() == 1)
    untouched = is_sentinel(rows).all(dim=1)
    partly = is_sentinel(rows).any(dim=1) & ~untouched
    assert not bool(partly.any()), "a row was written in part"
    assert not bool((untouched & ~closed).any()), "a row of an open group was skipped"
    scale = float(want.abs().max())
    stored = ~untouched
    err = float((rows[stored].double() - want[stored]).abs().max()) / scale
    print(f"row predicate M={m}: {int(untouched.sum())} of {int(closed.sum())} closed rows untouched, err of the stored rows {err:.2e}")
    assert err < tol, "every row is untouched or right - no third state"
    assert int(untouched.sum()) >= (run - 2 * max_tile + 1 if run >= 2 * max_tile else 0), "whole tiles of closed rows must be skipped"
    check_outside_untouched(buf, 32, 96)
    check_record(rec, rows[stored])      # the record covers the stored rows only
    _, buf0, rec0 = run_with([0, 0, 0])
    assert bool(is_sentinel(buf0).all()) and record_value(rec0) == 0, "every group closed: nothing is written"
    y1, _, rec1 = run_with([1, 1, 1])
    assert torch.equal(y1, plain) and record_value(rec1) == record_value(rec_plain), "every group open: the launch without a predicate"
    return y, rec, run_with


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_row_predicate_on_the_exact_kernels(dev, route):
    with options(route[1]):
        _check_row_predicate(dev, 300, 10, 270, 17, TOL_EXACT, 128)


@pytest.mark.parametrize("split,tile", [(0, 0), (16, 3), (16, 30)], ids=["exact", "f16-staged", "f16-astat-asked"])
def test_row_predicate_on_chip_filling_launches(dev, split, tile):
    """M = 33 000: the 128-row exact tile and the register-staged fp16 kernel (the A-stationary one runs no row predicate: asked
    for, the predicated launch lands on the register-staged kernel, the plain one it is compared with on the A-stationary)."""
    with options({"conv_split": split, "conv_split_tile": tile}):
        _, table = launches(lambda: _check_row_predicate(dev, 33000, 1000, 700, 300, TOL_F16 if split else TOL_EXACT, 256))
    assert all(row[3] == (3.0 if split else 0.0) for row in table), table


@pytest.mark.parametrize("route", ROUTES[1:4], ids=ROUTE_IDS[1:4])
def test_row_chunks_equal_the_unchunked_launch(dev, route):
    """gemm() cuts its rows into chunks ("gemm_row_limit" 1024: three chunks of M = 2500) and hands every chunk `row_group + m0`;
    rows are independent, so wherever the chunks run the kernel of the whole launch - conv_igemm (any tile: one fmaf chain in k
    order per output) or one forced split-K shape - every bit and every skipped row agree.  (Left to its own choice the library
    may run a smaller chunk on another kernel, which reorders the K sums: tests/test_parseq_gpu.py.)"""
    from yomitoku_amd import _lib

    with options(route[1]):
        y, rec, run_with = _check_row_predicate(dev, 2500, 900, 800, 300, TOL_EXACT, 128)
        _lib.debug_option("gemm_row_limit", 1024)
        (yc, _, recc), chunked = launches(lambda: run_with([1, 0, 1]))
    assert len(chunked) == 3, "three chunks of at most 1024 rows"
    assert torch.equal(yc.view(torch.int32), y.view(torch.int32)), "row chunks change nothing (sentinels included)"
    assert record_value(recc) == record_value(rec)


# ---- records on the launches the cases above do not reach
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("m,cout", [(5, 37), (300, 37), (5, 64)], ids=["tiny-ragged", "ragged", "tiny"])
def test_record_is_the_maximum_of_what_was_stored(dev, m, cout, route):
    """A ragged Cout (scalar stores), an M far below one tile, and - through the routes - split-K, whose partial sums are larger
    than the outputs here (the bias pulls every output towards zero) and must not reach the record."""
    from tests import hipops

    g = torch.Generator().manual_seed(29)
    x = torch.randn(1, 256, 1, m, generator=g) + 4.0
    wt = (torch.rand(cout, 256, 1, 1, generator=g) + 0.5) / 16.0
    bi = -conv_ref64(x, wt).mean(dim=(0, 2, 3)).float()  # outputs centred on zero: every partial sum over K is far larger
    ref = conv_ref64(x, wt, None, bi)
    with options(route[1]):
        y, _, rec = hipops.conv2d_view(x.to(dev), wt, None, bi, None, in_view=(0, 260), out_view=(3, cout + 8), record=True)
    err = float((y.double().cpu() - ref).abs().max()) / float(conv_ref64(x, wt).abs().max())
    print(f"record M={m} cout={cout} {route[0]}: err {err:.2e}")
    assert err < TOL_EXACT, err  # (relative to the accumulated sum: the bias cancels it)
    check_record(rec, y)
