"""fp16 planes in HBM (Tensor::planes): a producer convolution whose epilogue writes its outputs as the two scaled fp16 planes
the k x k consumer multiplies with, run as DBNetModel::bottleneck runs the pair (ymk_op_conv_planes_pair).  The test decodes the
intermediate itself from the layout ymk_f16_planes.h documents - per pixel and 32-channel slice 32 high halves, then 32 low
halves; value = (hi + lo) / sa, sa = 2^(141 - e), e the record's biased exponent clamped to 27 .. 227 - and holds
  the producer   to 4e-6 of max|ref| (the launch's own error) + 2^-22 of the record's value B (the cut: |x sa - hi - lo| <=
                 2^-22 |x sa| and |x| <= B) against float64,
  the consumer   to 4e-6 of max|ref| against float64 computed FROM THE DECODED PLANES (the producer's error is not counted twice),
  the record     to the bound pl_a max|x| + pl_b, which must cover every decoded value."""
import functools

import pytest
import torch

from tests.conv_ref import TOL_F16, conv_ref64, launches, options, record_value, rel_err

pytestmark = pytest.mark.gpu

H, W = 150, 220  # M = 33 000: the smallest launches the fp16-split kernels take (256 blocks of 128 x 64), no multiple of 128


def _bits_to_float(bits):
    return float(torch.tensor(bits, dtype=torch.int32).view(torch.float32))


def _decode(mid, rec):
    """raw intermediate [n, h, w, c] (device) + its record -> (values NCHW float64, hi, lo as fp16 [n, h, w, c / 32, 32], sa, B)"""
    bits = record_value(rec)
    e = min(max(bits >> 23, 27), 227)
    sa = 2.0 ** (141 - e)
    n, h, w, c = mid.shape
    halves = mid.cpu().contiguous().view(torch.float16).view(n, h, w, c // 32, 2, 32)
    hi, lo = halves[..., 0, :], halves[..., 1, :]
    assert bool(torch.isfinite(hi).all()) and bool(torch.isfinite(lo).all()), "an infinite or NaN half"
    val = ((hi.double() + lo.double()) / sa).reshape(n, h, w, c).permute(0, 3, 1, 2).contiguous()
    return val, hi, lo, sa, _bits_to_float(bits)


def _layer(g, cout, cin, k, bias_sign=0.0, positive=False):
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    sc = torch.rand(cout, generator=g) + 0.5
    bi = torch.randn(cout, generator=g) * (0.3 if bias_sign else 1.0) + bias_sign
    if positive:
        wt, bi = wt.abs(), bi.abs()
    return wt, sc, bi


@functools.lru_cache(maxsize=None)
def _input(h=H, w=W, seed=31):
    return torch.randn(1, 64, h, w, generator=torch.Generator().manual_seed(seed))


def _run_pair(dev, x, w1, p1, w2, p2, amax_in=None, expect=1, check_consumer=True, label=""):
    """One call of the pair with every check that holds for any qualifying pair; -> dict of what the callers look at further."""
    from tests import hipops
    from yomitoku_amd import _lib

    wr0, rd0 = _lib.stat("planes_written_launches"), _lib.stat("planes_read_launches")
    (y, mid, rec, taken, pl_a, pl_b), table = launches(lambda: hipops.conv_planes_pair(x.to(dev), w1, w2, p1, p2, amax_in=amax_in))
    assert taken == expect, f"planes_taken {taken}"
    assert _lib.stat("planes_written_launches") - wr0 == expect and _lib.stat("planes_read_launches") - rd0 == expect
    host = lambda p: {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in p.items()}
    p1, p2 = host(p1), host(p2)
    ref1 = conv_ref64(x, w1, p1.get("scale"), p1.get("bias"), p1.get("residual"), p1.get("stride", 1), p1.get("padding", 0),
                      p1.get("dilation", 1), p1.get("act", "none"))
    if taken:
        assert [row[3] for row in table] == [3.0, 3.0], f"both launches on the fp16-split kernels: {table}"
        val, hi, lo, sa, B = _decode(mid, rec)
    else:
        val, hi, lo, sa = mid.cpu().double().permute(0, 3, 1, 2).contiguous(), None, None, None
        B = 0.0  # fp32 values: no cut
        assert record_value(rec) == int(mid.abs().max().cpu().view(torch.int32)), "without planes the record is the measured maximum"
    s1 = float(ref1.abs().max())
    err1 = float((val - ref1).abs().max())
    allowed1 = TOL_F16 * s1 + 2.0 ** -22 * B
    out = dict(y=y, mid=mid, rec=rec, pl_a=pl_a, pl_b=pl_b, val=val, hi=hi, lo=lo, sa=sa, B=B, ref1=ref1, table=table, err1=err1 / s1)
    msg = f"{label}: producer err {err1 / s1:.2e} of max|ref| (allowed {allowed1 / s1:.2e}), B / max|ref| = {B / s1:.3g}"
    if check_consumer:
        ref2 = conv_ref64(val, w2, p2.get("scale"), p2.get("bias"), p2.get("residual"), p2.get("stride", 1), p2.get("padding", 0),
                          p2.get("dilation", 1), p2.get("act", "none"))
        out["err2"] = rel_err(y, ref2)
        msg += f", consumer err {out['err2']:.2e}"
    print(msg, "| launches (ms, flop, bytes, products):", [tuple(f"{v:.3g}" for v in row) for row in table])
    assert err1 <= allowed1, (err1, allowed1)
    if taken:
        assert B >= float(val.abs().max()), "the record is a bound of what the planes hold"
    if check_consumer:
        assert out["err2"] < TOL_F16, out["err2"]
    return out


def _check_bound(out, x, w1, sc, bi, max_in=None):
    """pl_a, pl_b against the test's own float64 values; the record within one ulp of float32(max_in pl_a + pl_b)"""
    a = float((w1.double().abs().sum(dim=(1, 2, 3)) * (sc.double().abs() if sc is not None else 1.0)).max())
    b = float(bi.double().abs().max()) if bi is not None else 0.0
    assert a <= out["pl_a"] <= 1.002 * a and b <= out["pl_b"] <= 1.002 * b, (a, out["pl_a"], b, out["pl_b"])
    max_in = float(x.abs().max()) if max_in is None else max_in
    want = torch.tensor(max_in * float(out["pl_a"]) + float(out["pl_b"]), dtype=torch.float64).float()
    got = torch.tensor(out["B"], dtype=torch.float32)
    assert abs(int(got.view(torch.int32)) - int(want.view(torch.int32))) <= 1, (float(got), float(want))


CONSUMERS = {"pad1": dict(stride=1, padding=1, dilation=1), "stride2": dict(stride=2, padding=1, dilation=1),
             "dil2": dict(stride=1, padding=2, dilation=2)}
PRODUCERS = {"1x1-64": (64, 1, 0), "1x1-96": (96, 1, 0), "3x3-64": (64, 3, 1)}  # cout1, k, pad


@pytest.mark.parametrize("consumer,producer", [("pad1", "1x1-64"), ("stride2", "1x1-64"), ("dil2", "1x1-64"), ("pad1", "1x1-96"), ("pad1", "3x3-64")])
def test_planes_hold_the_producer_and_feed_the_consumer(dev, consumer, producer):
    """Producers on the LDS-DMA kernel (64 columns; the 3 x 3) and on the register-staged kernel (96 columns: three 32-channel
    slices, the last one alone in the second 64-column half), every consumer geometry; the stored halves bit for bit against
    half(y sa), half(y sa - hi) of the fp32 run; both runs bit-identical on repeat."""
    from tests import hipops

    cout1, k1, pad1 = PRODUCERS[producer]
    x = _input(300, 440) if consumer == "stride2" else _input()  # stride 2: the consumer too must fill the chip
    g = torch.Generator().manual_seed(37)
    w1, sc1, bi1 = _layer(g, cout1, 64, k1)
    w2, sc2, bi2 = _layer(g, 64, cout1, 3)
    p1 = dict(padding=pad1, act="relu", scale=sc1, bias=bi1)
    p2 = dict(CONSUMERS[consumer], act="relu", scale=sc2, bias=bi2)
    with options({}):
        out = _run_pair(dev, x, w1, p1, w2, p2, label=f"{producer} -> 3x3 {consumer}")
        _check_bound(out, x, w1, sc1, bi1)
        again = hipops.conv_planes_pair(x.to(dev), w1, w2, p1, p2)
        assert torch.equal(again[0], out["y"]) and torch.equal(again[1].view(torch.int32), out["mid"].view(torch.int32))
        with options({"act_planes": 0}):
            (y0, mid0, _, taken0, _, _), table0 = launches(lambda: hipops.conv_planes_pair(x.to(dev), w1, w2, p1, p2))
            again0 = hipops.conv_planes_pair(x.to(dev), w1, w2, p1, p2)
    assert taken0 == 0 and torch.equal(again0[0], y0) and torch.equal(again0[1], mid0)
    ref = conv_ref64(out["ref1"], w2, sc2, bi2, None, p2["stride"], p2["padding"], p2["dilation"], "relu")
    print(f"end to end against float64 from x: planes {rel_err(out['y'], ref):.2e}, fp32 intermediate {rel_err(y0, ref):.2e}")
    same_family = [row[3] for row in table0] == [3.0, 3.0]
    print("stored halves against half(y sa), half(y sa - hi) of the fp32 run:", "compared" if same_family else f"not comparable {table0}")
    if same_family:  # the same fp16-split arithmetic produced y (the kernels of the family are bit-equal: tests/test_conv_split_gpu.py)
        ys = mid0.cpu() * out["sa"]
        hi = ys.half()
        lo = (ys - hi.float()).half()
        n, h, w, c = ys.shape
        assert torch.equal(hi.view(n, h, w, c // 32, 32).view(torch.int16), out["hi"].contiguous().view(torch.int16)), "high plane"
        assert torch.equal(lo.view(n, h, w, c // 32, 32).view(torch.int16), out["lo"].contiguous().view(torch.int16)), "low plane"


@pytest.mark.parametrize("bias_sign", [-1.5, 1.5], ids=["negative-bias", "positive-bias"])
@pytest.mark.parametrize("act", ["none", "relu", "silu", "gelu"])
def test_producer_activations_stay_under_the_bound(dev, act, bias_sign):
    g = torch.Generator().manual_seed(43)
    w1, sc1, bi1 = _layer(g, 64, 64, 1, bias_sign)
    w2, sc2, bi2 = _layer(g, 64, 64, 3)
    with options({}):
        out = _run_pair(dev, _input(), w1, dict(act=act, scale=sc1, bias=bi1), w2, dict(padding=1, act="none", scale=sc2, bias=bi2),
                        label=f"{act}, bias {bias_sign:+}")
    _check_bound(out, _input(), w1, sc1, bi1)


@pytest.mark.parametrize("log2m", [0, -20, 20])
def test_constant_input_reaches_the_bound(dev, log2m):
    """x = +m everywhere, weights, scale and bias non-negative, no activation: every output of the heaviest channel is
    (pl_a m + pl_b) / 1.001 - the largest value the planes' scale must hold without overflowing."""
    m = 2.0 ** log2m
    g = torch.Generator().manual_seed(47)
    w1, sc1, _ = _layer(g, 64, 64, 1, positive=True)
    bi1 = torch.full((64,), 0.5 * m)
    w2, sc2, bi2 = _layer(g, 64, 64, 3)
    x = torch.full((1, 64, H, W), m)
    with options({}):
        out = _run_pair(dev, x, w1, dict(scale=sc1, bias=bi1), w2, dict(padding=1, scale=sc2, bias=bi2 * m), label=f"constant 2^{log2m}")
    _check_bound(out, x, w1, sc1, bi1)
    top = float(out["val"].abs().max())
    assert top >= out["B"] / 1.002, "the case must reach the bound it exists for"


@pytest.mark.parametrize("loose", [0, 4, 8])
def test_loose_input_record(dev, loose):
    """The caller's record 2^loose above the true max|x| (pooled tensors inherit their source's record): the bound, the scale
    and with them the cut grow by the same factor - the producer tolerance is derived from B as read from the record."""
    from tests import hipops

    g = torch.Generator().manual_seed(53)
    w1, sc1, bi1 = _layer(g, 64, 64, 1)
    w2, sc2, bi2 = _layer(g, 64, 64, 3)
    x = _input()
    claimed = float(x.abs().max()) * 2.0 ** loose
    with options({}):
        out = _run_pair(dev, x, w1, dict(act="relu", scale=sc1, bias=bi1), w2, dict(padding=1, act="relu", scale=sc2, bias=bi2),
                        amax_in=hipops.amax_record(claimed, dev), label=f"record 2^{loose} loose")
    _check_bound(out, x, w1, sc1, bi1, max_in=claimed)


def test_outlier_leaves_the_rest_its_accuracy(dev):
    """One element 2^12 above the rest: the scale follows it, every other value keeps 11 + 11 bits - the outputs that do not see
    the outlier stay within 4e-6 of float64 computed from x."""
    g = torch.Generator().manual_seed(59)
    w1, sc1, bi1 = _layer(g, 64, 64, 1)
    w2, sc2, bi2 = _layer(g, 64, 64, 3)
    x = _input().clone()
    x[0, 3, 5, 7] = 4096.0
    p2 = dict(padding=1, act="none", scale=sc2, bias=bi2)
    with options({}):
        out = _run_pair(dev, x, w1, dict(act="none", scale=sc1, bias=bi1), w2, p2, label="outlier")
    ref = conv_ref64(out["ref1"], w2, sc2, bi2, None, 1, 1, 1)
    far = torch.ones_like(ref, dtype=torch.bool)
    far[0, :, 4:7, 6:9] = False  # the 1 x 1 keeps the outlier in its pixel, the 3 x 3 spreads it to the eight around
    err = float(((out["y"].double().cpu() - ref).abs() * far).max()) / float((ref.abs() * far).max())
    far1 = torch.ones_like(out["ref1"], dtype=torch.bool)
    far1[0, :, 5, 7] = False
    s1 = float((out["ref1"].abs() * far1).max())
    err1 = float(((out["val"] - out["ref1"]).abs() * far1).max()) / s1
    print(f"outlier: outputs that do not see it {err:.2e}; intermediate off the outlier's pixel {err1:.2e}, B / max = {out['B'] / s1:.3g}")
    assert err < TOL_F16, err
    # off the pixel the cut is relative to each value (2^-22 |v|) until its low half goes subnormal (2^-25 / sa = 2^-39 B at most)
    assert err1 < TOL_F16 + 2.0 ** -22 + 2.0 ** -39 * out["B"] / s1, err1


@pytest.mark.parametrize("why", ["producer-residual", "cout1-48", "consumer-1x1", "act_planes-0"])
def test_pairs_that_do_not_qualify_run_with_an_fp32_intermediate(dev, why):
    g = torch.Generator().manual_seed(61)
    cout1 = 48 if why == "cout1-48" else 64
    k2 = 1 if why == "consumer-1x1" else 3
    w1, sc1, bi1 = _layer(g, cout1, 64, 1)
    w2, sc2, bi2 = _layer(g, 64, cout1, k2)
    p1 = dict(act="relu", scale=sc1, bias=bi1)
    if why == "producer-residual":
        p1["residual"] = torch.randn(1, cout1, H, W, generator=g)
    with options({"act_planes": 0} if why == "act_planes-0" else {}):
        _run_pair(dev, _input(), w1, p1, w2, dict(padding=k2 // 2, act="relu", scale=sc2, bias=bi2), expect=0, label=why)
