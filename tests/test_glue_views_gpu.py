"""Single launches of the memory-bound NHWC kernels between the convolutions (layout change, pooling, resize, broadcast add) and
of the max|x| passes (k_absmax, k_amax_merge), in the forms the models launch them: channel slices of wider buffers, more work
than one pass of the grid-stride loop, 1-pixel and odd geometry.  References: tests/glue_ref.py (float64 or exact; checked
against torch on the CPU by tests/test_glue_ref_host.py).  Every operand view lies in a buffer whose spare words are NaN, every
output buffer is SENTINEL in every word before the launch: a read beside a view poisons the result, a write beside one shows."""
import numpy as np
import pytest
import torch

from tests import glue_ref, hipops
from tests.hipops import AMAX_REC_WORDS, SENTINEL
from tests.test_det_ops_gpu import POOL_SHAPES

pytestmark = pytest.mark.gpu

EPS = 2.0**-24  # half an ulp of 1: the relative error of one fp32 rounding


def _x(shape, seed=0):
    """unit-normal data; the second image clearly different (a kernel that mixes the images up fails)"""
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape)))
    if shape[0] > 1:
        x[1] += 4.0
    return x


def _forms(c):
    """(input view, output view) per launch: contiguous - the pools' form in the models -, one side in a wider buffer, both
    sides in different ones (a kernel that swaps the two leading dimensions has nowhere to hide)"""
    a, b = (4, c + 8), (8, c + 20)
    return [(None, None), (a, None), (None, b), (a, b), (b, a)]


def _check_buffer(ybuf, view, c, what, finite=True):
    """every word of the output buffer outside the view still SENTINEL, every word inside written (and finite)"""
    c0 = (view or (0, c))[0]
    words = ybuf.cpu().view(torch.int32)
    outside = torch.ones(words.shape[-1], dtype=torch.bool)
    outside[c0:c0 + c] = False
    assert (words[..., outside] == SENTINEL).all(), f"{what}: a word outside the output view was written"
    inside = words[..., c0:c0 + c]
    assert (inside != SENTINEL).all(), f"{what}: a word of the output view was not written"
    vals = inside.view(torch.float32)
    assert not torch.isnan(vals).any(), f"{what}: NaN in the output (a read outside the input view)"
    if finite:
        assert torch.isfinite(vals).all(), what


# ---------------------------------------------------------------------------------------------------------------- max-pool
@pytest.mark.parametrize("c", [4, 64, 260])
@pytest.mark.parametrize("hw", [(1, 1), (1, 2), (2, 1), (5, 7), (6, 8), (33, 47)])
def test_maxpool_views(dev, hw, c):
    """MaxPool2d(3, 2, 1) bit for bit (a maximum rounds nothing) over 1-pixel, even, odd and multi-block sizes in every view
    form; once with every value negative (-1 - |randn|: a window padded with 0 instead of -inf fails on every border pixel),
    once with -inf among the values (-inf is a value, not "no value")."""
    x = _x((2, c) + hw)
    for k, (iv, ov) in enumerate(_forms(c)):
        y, ybuf = hipops.pool_view("maxpool", x.to(dev), iv, ov)
        assert torch.equal(y.cpu().double(), glue_ref.maxpool3x3s2(x)), (iv, ov)
        _check_buffer(ybuf, ov, c, f"maxpool {hw} {iv} {ov}")
    iv, ov = _forms(c)[3]
    neg = -1.0 - x.abs()
    y, ybuf = hipops.pool_view("maxpool", neg.to(dev), iv, ov)
    assert torch.equal(y.cpu().double(), glue_ref.maxpool3x3s2(neg)) and (y <= -1.0).all()
    _check_buffer(ybuf, ov, c, "maxpool, negative data")
    inf = x.clone()
    inf.view(-1)[::3] = float("-inf")
    inf[0, :, 0, 0] = float("-inf")  # with a 1-pixel image: a window holding nothing else
    y, ybuf = hipops.pool_view("maxpool", inf.to(dev), iv, ov)
    assert torch.equal(y.cpu().double(), glue_ref.maxpool3x3s2(inf))
    _check_buffer(ybuf, ov, c, "maxpool, -inf present", finite=False)


# ---------------------------------------------------------------------------------------------------------------- average pool, nearest x2
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_avgpool_and_nearest_views(dev, shape):
    """AvgPool2d(2, 2, 0, ceil_mode=True) within 1e-6 max|x| (the bound and its derivation: test_det_ops_gpu.py - three fp32
    additions and an exact division, 1.8e-7) and nearest x2 bit for bit, the shapes of that test in every view form."""
    x = _x(shape)
    c = shape[1]
    want = glue_ref.avgpool2x2_ceil(x)
    worst = 0.0
    for iv, ov in _forms(c):
        y, ybuf = hipops.pool_view("avgpool", x.to(dev), iv, ov)
        assert y.shape == want.shape
        err = (y.cpu().double() - want).abs().max().item() / x.abs().max().item()
        worst = max(worst, err)
        assert err < 1e-6, (iv, ov, err)
        _check_buffer(ybuf, ov, c, f"avgpool {shape} {iv} {ov}")
        up, ubuf = hipops.pool_view("nearest", x.to(dev), iv, ov)
        assert torch.equal(up.cpu(), glue_ref.nearest2x(x)), (iv, ov)
        _check_buffer(ubuf, ov, c, f"nearest {shape} {iv} {ov}")
    print(f"avgpool views {shape}: {worst:.2e} of max|x|")


@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (20, 21)])
def test_nearest_rtdetr_form(dev, hw):
    """RT-DETR's FPN: columns 256 .. 511 of one 512-wide concat buffer up-sampled into columns 0 .. 255 of another."""
    x = _x((2, 256) + hw)
    up, ubuf = hipops.pool_view("nearest", x.to(dev), (256, 512), (0, 512))
    assert torch.equal(up.cpu(), glue_ref.nearest2x(x))
    _check_buffer(ubuf, (0, 512), 256, f"nearest {hw}, the RT-DETR form")


# ---------------------------------------------------------------------------------------------------------------- bilinear
def _bilinear_tol(x, add=None):
    return 8 * EPS * (x.abs().max().item() + (add.abs().max().item() if add is not None else 0.0))


BILINEAR_CASES = [((7, 9), (7, 9)), ((7, 9), (14, 18)), ((7, 9), (28, 36)), ((10, 14), (20, 28)), ((10, 14), (40, 56)),
                  ((9, 12), (18, 25)), ((20, 27), (40, 53)), ((40, 53), (20, 27)), ((65, 66), (130, 131)), ((1, 1), (4, 4)), ((1, 5), (3, 20))]


@pytest.mark.parametrize("hw,size", BILINEAR_CASES)
def test_bilinear_views(dev, hw, size):
    """F.interpolate(bilinear, align_corners=False) (+ add) against the float64 interpolation over the kernel's documented fp32
    source coordinates (glue_ref.bilinear): x1 (bit-equal to the input), x2 and x4, four non-integer ratios (one of them
    down-sampling), a 1-pixel source and a single source row; with and without `add`, `add` once in a view of its own.
    Tolerance 8 * 2^-24 * (max|x| + max|add|).  Every intermediate of hy (hx a + lx b) + ly (hx c + lx d) is a convex
    combination of values no larger than max|x| (up to the roundings counted here), so one fp32 rounding costs at most 2^-24
    max|x|, and there are seven: the two weights 1 - ly and 1 - lx, the two products and the sum of a source row (three for
    the row pair, whose errors hy and ly weigh with hy + ly = 1), the two outer products and their sum - plus one for `add`, on
    a value of at most max|x| + max|add|.  Fused multiply-adds only remove roundings.  The source coordinates themselves are
    NOT part of the tolerance: the kernel has to round the product and the difference of (o + 0.5) * s - 0.5 separately, as
    documented.  (Contracted into one FMA they move by an ulp of a coordinate; this test measured 9.6e-7 max|x| at 65 x 66 ->
    130 x 131 for that form, twice the bound, and 1.0e-7 for the documented one.)"""
    c = 12
    x = _x((2, c) + hw, 7)
    add = _x((2, c) + size, 11)
    want = glue_ref.bilinear(x, size)
    worst = 0.0
    for k, (iv, ov) in enumerate(_forms(c)):
        y, ybuf = hipops.upsample_bilinear_view(x.to(dev), size, None, iv, ov)
        err = (y.cpu().double() - want).abs().max().item()
        worst = max(worst, err / x.abs().max().item())
        assert err <= _bilinear_tol(x), (iv, ov, err, _bilinear_tol(x))
        _check_buffer(ybuf, ov, c, f"bilinear {hw} -> {size} {iv} {ov}")
        if hw == size:
            assert torch.equal(y.cpu(), x), "x1 is the identity"
        av = (None, (4, c + 12))[k % 2]
        ya, abuf = hipops.upsample_bilinear_view(x.to(dev), size, add.to(dev), iv, ov, av)
        err = (ya.cpu().double() - (want + add.double())).abs().max().item()
        assert err <= _bilinear_tol(x, add), (iv, ov, av, err, _bilinear_tol(x, add))
        _check_buffer(abuf, ov, c, f"bilinear + add {hw} -> {size} {iv} {ov} {av}")
    print(f"bilinear {hw} -> {size}: {worst:.2e} of max|x| (bound {8 * EPS:.2e})")


def test_bilinear_dbnet_form(dev):
    """DBNet's concat: three contiguous 64-channel maps up-sampled x4, x4 and x2 (from 5 x 6, 5 x 6, 10 x 12) into columns 0, 64
    and 128 of one 20 x 24 x 256 buffer; columns 192 .. 255 (the fourth map's, a convolution's) stay untouched throughout."""
    size = (20, 24)
    srcs = [_x((2, 64, 5, 6), 1), _x((2, 64, 5, 6), 2), _x((2, 64, 10, 12), 3)]
    buf = None
    for k, x in enumerate(srcs):
        y, buf = hipops.upsample_bilinear_view(x.to(dev), size, None, None, (64 * k, 256), into=buf)
        words = buf.cpu().view(torch.int32)
        assert (words[..., 64 * (k + 1):] == SENTINEL).all(), f"launch {k} wrote beyond its slice"
    got = buf.cpu()
    assert (got.view(torch.int32)[..., 192:] == SENTINEL).all()
    for k, x in enumerate(srcs):  # also: a later launch left the earlier slices alone
        part = got[..., 64 * k:64 * (k + 1)].permute(0, 3, 1, 2).double()
        err = (part - glue_ref.bilinear(x, size)).abs().max().item()
        print(f"bilinear, DBNet slice {k}: {err / x.abs().max().item():.2e} of max|x|")
        assert err <= _bilinear_tol(x), (k, err)


# ---------------------------------------------------------------------------------------------------------------- layout change, broadcast add
@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (32, 100)])
@pytest.mark.parametrize("n", [1, 3])
def test_nchw3_to_nhwc4(dev, n, hw):
    """The first kernel of every forward, bit for bit: channel 3 exactly +0.0; the three planes are distinct constants plus noise
    and the images differ, so a channel or image swap shows."""
    x = torch.randn(n, 3, *hw, generator=torch.Generator().manual_seed(n + sum(hw))) * 0.1
    x += torch.tensor([1.0, 2.0, 3.0]).view(1, 3, 1, 1) + 10.0 * torch.arange(n).view(n, 1, 1, 1)
    y = hipops.nchw3_to_nhwc4(x.to(dev)).cpu()
    assert torch.equal(y.view(torch.int32), glue_ref.nchw3_to_nhwc4(x).view(torch.int32))


def _add_bcast_case(m, rows_mod, d):
    g = torch.Generator().manual_seed(m + rows_mod + d)
    a = torch.randn(m, d, generator=g)
    b = torch.randn(rows_mod, d, generator=g) + torch.arange(rows_mod, dtype=torch.float32).view(-1, 1)  # distinct rows
    return a, b


@pytest.mark.parametrize("m,rows_mod,d", [(6, 3, 256), (400, 400, 256), (401 * 3, 401, 256), (7, 1, 4)])
def test_add_bcast(dev, m, rows_mod, d):
    """out[r] = a[r] + b[r % rows_mod] (AIFI's position embedding over the batch; the decoder's query embedding with rows_mod =
    m), bit-equal to the fp32 sum = the float64 sum rounded once."""
    a, b = _add_bcast_case(m, rows_mod, d)
    out = hipops.add_bcast(a.to(dev), b.to(dev)).cpu()
    assert torch.equal(out, glue_ref.add_bcast(a, b).float())


# ---------------------------------------------------------------------------------------------------------------- grid-stride passes
GRID_ITEMS = 4096 * 256  # the launchers cap the grid at 4096 blocks of 256 threads: beyond, the grid-stride loops go round again


@pytest.fixture(scope="module")
def big_pool_input():
    return torch.randn(1, 256, 259, 255, generator=torch.Generator().manual_seed(259))


@pytest.mark.parametrize("kind", ["maxpool", "avgpool"])
def test_pool_grid_stride(dev, big_pool_input, kind):
    """256 channels, 259 x 255 -> 130 x 128: 1 064 960 float4 items of output, a ragged 16 384 into the second pass."""
    x = big_pool_input
    ov = (8, 276)
    y, ybuf = hipops.pool_view(kind, x.to(dev), None, ov)
    assert y.shape[2:] == (130, 128) and y[0].numel() // 4 > GRID_ITEMS and (y[0].numel() // 4) % GRID_ITEMS != 0
    if kind == "maxpool":
        assert torch.equal(y.cpu(), glue_ref.maxpool3x3s2(x, torch.float32))
    else:
        err = (y.cpu().double() - glue_ref.avgpool2x2_ceil(x)).abs().max().item() / x.abs().max().item()
        print(f"avgpool 259 x 255: {err:.2e} of max|x|")
        assert err < 1e-6
    _check_buffer(ybuf, ov, 256, f"{kind}, grid-stride")


def test_nearest_grid_stride(dev):
    x = _x((1, 256, 65, 64))
    up, ubuf = hipops.pool_view("nearest", x.to(dev), (256, 512), (0, 512))
    assert up.shape[2:] == (130, 128) and up.numel() // 4 > GRID_ITEMS
    assert torch.equal(up.cpu(), glue_ref.nearest2x(x))
    _check_buffer(ubuf, (0, 512), 256, "nearest, grid-stride")


def test_bilinear_grid_stride(dev):
    """64 channels, 129 x 128 -> 258 x 256 (1 056 768 items) into columns 64 .. 127 of a 256-wide buffer."""
    x = _x((1, 64, 129, 128))
    size = (258, 256)
    y, ybuf = hipops.upsample_bilinear_view(x.to(dev), size, None, None, (64, 256))
    assert y.numel() // 4 > GRID_ITEMS and (y.numel() // 4) % GRID_ITEMS != 0
    err = (y.cpu().double() - glue_ref.bilinear(x, size)).abs().max().item()
    print(f"bilinear 129 x 128 -> 258 x 256: {err / x.abs().max().item():.2e} of max|x|")
    assert err <= _bilinear_tol(x)
    _check_buffer(ybuf, (64, 256), 64, "bilinear, grid-stride")


def test_add_bcast_grid_stride(dev):
    m, rows_mod, d = 41 * 401, 401, 256
    assert m * d // 4 > GRID_ITEMS and (m * d // 4) % GRID_ITEMS != 0
    a, b = _add_bcast_case(m, rows_mod, d)
    out = hipops.add_bcast(a.to(dev), b.to(dev)).cpu()
    assert torch.equal(out, glue_ref.add_bcast(a, b).float())


def test_nchw3_to_nhwc4_grid_stride(dev):
    n, h, w = 2, 725, 725
    assert n * h * w > GRID_ITEMS and (n * h * w) % GRID_ITEMS != 0
    x = torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(725)) * 0.1
    x += torch.tensor([1.0, 2.0, 3.0]).view(1, 3, 1, 1) + 10.0 * torch.arange(n).view(n, 1, 1, 1)
    y = hipops.nchw3_to_nhwc4(x.to(dev)).cpu()
    assert torch.equal(y.view(torch.int32), glue_ref.nchw3_to_nhwc4(x).view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- k_absmax
def _bits(v):
    return int(np.array([abs(v)], dtype=np.float32).view(np.uint32)[0])


def _u32(t):
    return t.cpu().to(torch.int64) & 0xFFFFFFFF


def _absmax_blocks(items):
    return min(1024, (items + 1023) // 1024)  # absmax_launch (ymk_conv_split.hip)


def _absmax_positions(items, contiguous):
    """The float4 items whose place in k_absmax's loops differs: the ends, the middle, around one, three and four grid strides
    and - contiguous form, unrolled by four - the last item an unrolled pass reads and the first and last the tail loop reads.
    Thread i (< stride) reads items i + k stride; its pass r (items k = 4r .. 4r + 3) is unrolled iff i + (4r + 3) stride < items."""
    stride = 256 * _absmax_blocks(items)
    cand = {0, items - 1, items // 2, stride - 1, stride, 3 * stride - 1, 3 * stride, 3 * stride + 1, 4 * stride - 1, 4 * stride, 4 * stride + 1}
    if contiguous:
        j = np.arange(items, dtype=np.int64)
        unrolled = (j % stride) + (4 * (j // stride // 4) + 3) * stride < items
        if unrolled.any():
            cand.add(int(j[unrolled].max()))
        if (~unrolled).any():
            cand |= {int(j[~unrolled].min()), int(j[~unrolled].max())}
    return sorted(p for p in cand if 0 <= p < items)


def _records(dev, slot0=0, next0=0x3F800000):
    """(slot, next): every word but word 0 a pattern of its own, slot's word 0 as given (0: a fresh record), next's non-zero"""
    pat = torch.arange(AMAX_REC_WORDS, dtype=torch.int32) * 1000003 + 12345
    slot, nxt = pat.clone(), pat.clone() + 7
    slot[0], nxt[0] = slot0, next0
    return slot.to(dev), nxt.to(dev), pat


def _absmax_check(slot, nxt, pat, want_bits, what):
    s, n = _u32(slot), _u32(nxt)
    assert int(s[0]) == want_bits, f"{what}: record {int(s[0]):#x}, max|x| {want_bits:#x}"
    assert int(n[0]) == 0, f"{what}: word 0 of the next record not cleared"
    assert torch.equal(s[1:], _u32(pat)[1:]) and torch.equal(n[1:], _u32(pat + 7)[1:]), f"{what}: another word of a record changed"


ABSMAX_FORMS = {  # name -> (c, first channel, leading dimension, pixel counts)
    # contiguous (c = ld = 4, as absmax_record passes it): 1, 255, 1023, 1024, 1025, 3079 items around the one-block, two-block and
    # unroll boundaries, and two unrolled passes of the capped 1024-block grid plus a tail of more than a stride
    "contiguous": (4, 0, 4, [1, 255, 1023, 1024, 1025, 3079, 2 * 1024 * 1024 + 256 * 1024 + 5]),
    # strided (a slice of a concat buffer): 16 and 9 float4 per pixel, item counts around the same boundaries and above the cap
    "c64_ld96": (64, 32, 96, [1, 16, 64, 65, 193, 65537]),
    "c36_ld96": (36, 4, 96, [1, 29, 114, 343, 116510]),
}


@pytest.mark.parametrize("form", list(ABSMAX_FORMS))
def test_absmax_positions(dev, form):
    """The record is the fp32 bit pattern of max|x|, wherever the maximum sits: |x| < 1 everywhere but one planted +-M that
    moves through the position classes of the loops (_absmax_positions) and the four lanes of a float4.  Strided forms: NaN in
    every spare word - one NaN read makes the record a NaN pattern, above every number.  Each launch also clears word 0 of the
    next record from a non-zero value and leaves every other word of both records alone."""
    c, c0, ld, sizes = ABSMAX_FORMS[form]
    c4 = c // 4
    for pixels in sizes:
        items = pixels * c4
        g = torch.Generator().manual_seed(pixels)
        vals = (torch.rand(pixels, c, generator=g) * 2 - 1) * 0.999
        buf = torch.full((pixels, ld), float("nan"))
        buf[:, c0:c0 + c] = vals
        buf = buf.to(dev).view(-1)
        base = _bits(vals.abs().max().item())
        slot, nxt, pat = _records(dev)
        hipops.absmax(buf, pixels, c, (c0, ld), slot, nxt)
        _absmax_check(slot, nxt, pat, base, f"{form} {pixels}: unplanted")
        cases = [(0, 0), (items - 1, 3)] + [(items // 2, e) for e in range(4)]
        cases += [(p, k % 4) for k, p in enumerate(_absmax_positions(items, ld == c))]
        for k, (item, lane) in enumerate(cases):
            m = (-1.0) ** k * (3.0 + k)
            at = (item // c4) * ld + c0 + (item % c4) * 4 + lane
            keep = buf[at].clone()
            buf[at] = m
            slot, nxt, pat = _records(dev)
            hipops.absmax(buf, pixels, c, (c0, ld), slot, nxt)
            _absmax_check(slot, nxt, pat, _bits(m), f"{form} {pixels} pixels: {m} at item {item} lane {lane}")
            buf[at] = keep


def test_absmax_values_and_accumulation(dev):
    """A negative maximum; -0.0 alone (the record stays 0); denormals alone (their bit pattern, nothing flushed); a second launch
    into a record that already holds a larger value keeps it, into one holding a smaller value raises it."""
    def run(vals, slot0=0):
        buf = torch.tensor(vals, dtype=torch.float32).to(dev)
        slot, nxt, pat = _records(dev, slot0)
        hipops.absmax(buf, buf.numel() // 4, 4, (0, 4), slot, nxt)
        assert torch.equal(_u32(slot)[1:], _u32(pat)[1:]) and int(_u32(nxt)[0]) == 0
        return int(_u32(slot)[0])

    assert run([0.5, -0.75, 0.25, 0.125] * 3) == _bits(0.75)
    assert run([-0.0] * 8) == 0
    tiny = [1e-45, -3e-45, 2e-45, 0.0] * 2
    assert run(tiny) == 2  # -3e-45 is the denormal with bit pattern 2
    assert run([1e-39, 0.0, -0.0, 0.0]) == _bits(1e-39)
    assert run([0.5, -0.75, 0.25, 0.125], slot0=_bits(2.0)) == _bits(2.0)
    assert run([0.5, -0.75, 0.25, 0.125], slot0=_bits(0.5)) == _bits(0.75)


# ---------------------------------------------------------------------------------------------------------------- k_amax_merge
def test_amax_merge(dev):
    """dst word 0 of every line = the larger of the two records' (lines larger in dst, larger in src, equal, zero in one or
    both); words 1 .. 31 of src's lines hold a large pattern that must not leak; everything else is unchanged; a null record
    makes the call a no-op."""
    g = torch.Generator().manual_seed(32)
    d0 = torch.rand(32, generator=g) * 8
    s0 = torch.rand(32, generator=g) * 8
    s0[4:8] = d0[4:8]          # equal
    d0[8:12] = 0.0             # zero in dst
    s0[12:16] = 0.0            # zero in src
    d0[16:18] = s0[16:18] = 0  # zero in both
    d0[20], s0[20] = 1e30, 1e-30
    dst = (torch.arange(AMAX_REC_WORDS, dtype=torch.int32) * 7919 + 3) & 0x3FFFFFFF
    src = torch.full((AMAX_REC_WORDS,), 0x7F7FFFFF, dtype=torch.int32)  # FLT_MAX's pattern beside every value
    dst[::32] = d0.view(torch.int32)
    src[::32] = s0.view(torch.int32)
    want = dst.clone()
    want[::32] = torch.maximum(d0, s0).view(torch.int32)
    assert (want[::32] != dst[::32]).sum() >= 8 and (want[::32] == dst[::32]).sum() >= 8
    dd, sd = dst.to(dev), src.to(dev)
    hipops.amax_merge(dd, sd)
    assert torch.equal(dd.cpu(), want) and torch.equal(sd.cpu(), src)
    assert glue_ref.record_value(dd) == max(d0.max().item(), s0.max().item())
    dd = dst.to(dev)
    hipops.amax_merge(dd, None)
    hipops.amax_merge(None, sd)
    assert torch.equal(dd.cpu(), dst) and torch.equal(sd.cpu(), src)


# ---------------------------------------------------------------------------------------------------------------- the bound inherited records rely on
def _asf_weights(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(16, 64, generator=g) / 16, torch.randn(64, 16, generator=g) / 8, torch.randn(3, 3, generator=g) / 3, 1.5,
            torch.randn(4, 64, generator=g) / 8)


def _amax(t):
    return t.double().abs().max().item()


@pytest.mark.parametrize("data", ["random", "k0", "k10", "k-10"])
def test_outputs_stay_within_the_record_they_inherit(dev, data):
    """The models hand a producer's max|x| record on to the output of these kernels instead of measuring again (`p.amax =
    c1.amax` after the max-pool, `src.amax = cur.amax` after the average pool, one record for the parts of DBNet's `fuse`,
    amax_merge after nearest x2, `fused.amax = fuse.amax` after ASF).  That is sound if max|out| <= max|in|: exactly for the
    max-pool, nearest x2 (copies), the average pool (fp32 sums of <= 4 values of magnitude <= M round to at most 4 M, itself a
    float, and the division by 4, 2 or 1 is exact) and ASF (out = score * fuse, score = 1 / (1 + e) <= 1).  Bilinear is a convex
    combination only up to the rounding of 1 - l: max|out| <= max|in| (1 + 8 * 2^-24), the roundings counted in
    test_bilinear_views.  On random data and on a constant tensor whose value is the largest float below a power of two
    (nextafter(2^k, 0), k = 0, 10, -10), where any excess crosses a binade.
    Why a few ulp are enough: f16_plane_scales scales a tensor so that its record lands in [2^14, 2^15), and fp16 ends at
    65504 - just below 2^16.  A value up to twice the record still fits; an excess of 5e-7 of it is four orders of magnitude
    inside that headroom, so no inherited record can saturate a plane."""
    shape, c = (2, 64, 9, 11), 64
    if data == "random":
        x = _x(shape, 21)
        fuse = _x((2, 256, 9, 11), 22)
        ax = _x(shape, 23)
    else:
        v = float(np.nextafter(np.float32(2.0 ** int(data[1:])), np.float32(0)))
        x = torch.full(shape, v)
        x[1] = -v
        fuse = torch.full((2, 256, 9, 11), v)
        fuse[1] = -v
        ax = torch.full(shape, 30.0)  # every gate saturates: score rounds to 1
    m = _amax(x)
    for kind in ("maxpool", "avgpool", "nearest"):
        for iv, ov in _forms(c)[::3]:
            y, _ = hipops.pool_view(kind, x.to(dev), iv, ov)
            assert _amax(y.cpu()) <= m, (kind, _amax(y.cpu()), m)
    for size in ((9, 11), (18, 22), (36, 44), (20, 27), (5, 6), (37, 41)):
        y, _ = hipops.upsample_bilinear_view(x.to(dev), size, None, None, (64, 256))
        got = _amax(y.cpu())
        print(f"bilinear {data} -> {size}: max|out| / max|in| - 1 = {got / m - 1:.2e}")
        assert got <= m * (1 + 8 * EPS), (size, got, m)
    w1, w2, sp33, sp11, watt = _asf_weights(5)
    if data != "random":
        watt = watt.abs() + 1.0
    out = hipops.dbnet_asf(ax.to(dev), fuse.to(dev), w1, w2, sp33, sp11, watt).cpu()
    assert torch.isfinite(out).all() and _amax(out) <= _amax(fuse), (_amax(out), _amax(fuse))
    if data != "random":
        assert _amax(out) == _amax(fuse), "the saturated gate passes the constant through"


# ---------------------------------------------------------------------------------------------------------------- refusals
BAD_VIEWS = [("ld < c", lambda c: (0, c - 4)), ("ld % 4", lambda c: (0, c + 2)), ("first channel 2: not 16-byte aligned", lambda c: (2, c + 8))]


def _refused(err, buf, what):
    assert err, f"{what}: accepted"
    assert (buf.cpu().view(torch.int32) == SENTINEL).all(), f"{what}: refused, but the output buffer was written"


@pytest.mark.parametrize("kind", ["maxpool", "avgpool", "nearest"])
def test_pool_entries_refuse_what_the_kernels_trust(dev, kind):
    """ld < c, ld % 4 != 0, a view that starts at channel 2, c % 4 != 0 - on the input and on the output side: an error with a
    message, and not a word of the output buffer written.  (These entries derive the output size from the input themselves;
    the launch functions' own shape checks are what the models' calls meet.)"""
    c = 8
    x = _x((2, c, 5, 7)).to(dev)
    for what, view in BAD_VIEWS:
        _refused(*hipops.pool_view(kind, x, view(c), None, unchecked=True), f"{kind}, input: {what}")
        _refused(*hipops.pool_view(kind, x, None, view(c), unchecked=True), f"{kind}, output: {what}")
    _refused(*hipops.pool_view(kind, _x((2, 6, 5, 7)).to(dev), (0, 8), (0, 8), unchecked=True), f"{kind}: c % 4")
    err, buf = hipops.pool_view(kind, x, (4, c + 8), (8, c + 20), unchecked=True)
    assert err is None and not (buf.cpu().view(torch.int32) == SENTINEL).all(), "a good view passes the same path"
    lib, stream = hipops._lib.load(), hipops._lib.current_stream_ptr()
    name = hipops.GLUE_VIEW_OPS[kind][0]
    y = torch.zeros(2 * 10 * 14 * c, device=dev)
    for args in ((None, 2, 5, 7, c, c, y.data_ptr(), c), (x.data_ptr(), 2, 5, 7, c, c, None, c), (x.data_ptr(), 0, 5, 7, c, c, y.data_ptr(), c),
                 (x.data_ptr(), 2, 0, 7, c, c, y.data_ptr(), c), (x.data_ptr(), 2, 5, -1, c, c, y.data_ptr(), c)):
        assert getattr(lib, name)(*args, stream) != 0 and lib.ymk_last_error(), (kind, args[1:6])
    torch.cuda.synchronize()
    assert not y.cpu().any()


def test_bilinear_entry_refuses_what_the_kernel_trusts(dev):
    """As above for x, y and add; and an output size that does not follow from anything: oh or ow below 1."""
    c = 8
    x = _x((2, c, 5, 7)).to(dev)
    add = _x((2, c, 10, 14)).to(dev)
    for what, view in BAD_VIEWS:
        _refused(*hipops.upsample_bilinear_view(x, (10, 14), None, view(c), None, unchecked=True), f"bilinear, input: {what}")
        _refused(*hipops.upsample_bilinear_view(x, (10, 14), None, None, view(c), unchecked=True), f"bilinear, output: {what}")
        _refused(*hipops.upsample_bilinear_view(x, (10, 14), add, None, None, view(c), unchecked=True), f"bilinear, add: {what}")
    err, buf = hipops.upsample_bilinear_view(x, (10, 14), add, (4, c + 8), (8, c + 20), (4, c + 12), unchecked=True)
    assert err is None and not (buf.cpu().view(torch.int32) == SENTINEL).all()
    lib, stream = hipops._lib.load(), hipops._lib.current_stream_ptr()
    y = torch.zeros(2 * 10 * 14 * c, device=dev)
    for oh, ow in ((0, 14), (10, 0), (-3, 14)):
        assert lib.ymk_op_upsample_bilinear_view(x.data_ptr(), 2, 5, 7, c, c, oh, ow, None, 0, y.data_ptr(), c, stream) != 0, (oh, ow)
        assert lib.ymk_last_error()
    assert lib.ymk_op_upsample_bilinear_view(None, 2, 5, 7, c, c, 10, 14, None, 0, y.data_ptr(), c, stream) != 0
    assert lib.ymk_op_upsample_bilinear_view(x.data_ptr(), 2, 5, 7, c, c, 10, 14, None, 0, None, c, stream) != 0
    assert lib.ymk_op_upsample_bilinear_view(x.data_ptr(), 0, 5, 7, c, c, 10, 14, None, 0, y.data_ptr(), c, stream) != 0
    torch.cuda.synchronize()
    assert not y.cpu().any()


def test_flat_entries_refuse_what_the_kernels_trust(dev):
    """nchw3_to_nhwc4: an output that is not 16-byte aligned, an empty image, null; add_bcast: d % 4, rows_mod < 1, a pointer
    two floats off; absmax: ld < c, ld % 4, first channel 2, no pixels - the records untouched; all with a message."""
    lib, stream = hipops._lib.load(), hipops._lib.current_stream_ptr()
    x = torch.randn(2, 3, 5, 7).to(dev)
    _refused(*hipops.nchw3_to_nhwc4(x, unchecked=True, offset=2), "nchw3_to_nhwc4: misaligned output")
    err, y = hipops.nchw3_to_nhwc4(x, unchecked=True)
    assert err is None
    y = torch.zeros(2 * 5 * 7 * 4, device=dev)
    for args in ((None, 2, 5, 7, y.data_ptr()), (x.data_ptr(), 2, 5, 7, None), (x.data_ptr(), 0, 5, 7, y.data_ptr()), (x.data_ptr(), 2, 0, 7, y.data_ptr()),
                 (x.data_ptr(), 2, 5, 0, y.data_ptr())):
        assert lib.ymk_op_nchw3_to_nhwc4(*args, stream) != 0 and lib.ymk_last_error(), args[1:4]
    a, b = torch.randn(6, 8).to(dev), torch.randn(3, 8).to(dev)
    _refused(*hipops.add_bcast(a, b, unchecked=True, d=6), "add_bcast: d % 4")
    _refused(*hipops.add_bcast(a, b, unchecked=True, offset=2), "add_bcast: misaligned output")
    err, out = hipops.add_bcast(a, b, unchecked=True)
    assert err is None
    out = torch.zeros(6 * 8, device=dev)
    for args in ((a.data_ptr(), b.data_ptr(), 0, 6, 8, out.data_ptr()), (a.data_ptr(), b.data_ptr(), 3, 0, 8, out.data_ptr()),
                 (None, b.data_ptr(), 3, 6, 8, out.data_ptr()), (a.data_ptr(), None, 3, 6, 8, out.data_ptr()), (a.data_ptr(), b.data_ptr(), 3, 6, 8, None),
                 (a.data_ptr() + 8, b.data_ptr(), 3, 5, 8, out.data_ptr()), (a.data_ptr(), b.data_ptr() + 8, 2, 6, 8, out.data_ptr())):
        assert lib.ymk_op_add_bcast(*args, stream) != 0 and lib.ymk_last_error(), args[2:5]
    buf = torch.rand(64 * 24).to(dev)
    for c, view, pixels in ((8, (0, 4), 64), (8, (0, 10), 64), (8, (2, 16), 64), (6, (0, 8), 64), (8, (0, 8), 0)):
        slot, nxt, pat = _records(dev)
        assert hipops.absmax(buf, pixels, c, view, slot, nxt, unchecked=True), (c, view, pixels)
        assert torch.equal(slot.cpu()[1:], pat[1:]) and int(slot.cpu()[0]) == 0 and int(_u32(nxt)[0]) == 0x3F800000
    slot, nxt, pat = _records(dev)
    assert lib.ymk_op_absmax(None, 64, 8, 8, slot.data_ptr(), nxt.data_ptr(), stream) != 0
    assert lib.ymk_op_absmax(buf.data_ptr(), 64, 8, 8, None, nxt.data_ptr(), stream) != 0
    assert lib.ymk_op_absmax(buf.data_ptr(), 64, 8, 8, slot.data_ptr(), None, stream) != 0
    assert int(slot.cpu()[0]) == 0 and int(_u32(nxt)[0]) == 0x3F800000
    torch.cuda.synchronize()
    assert not y.cpu().any() and not out.cpu().any()
