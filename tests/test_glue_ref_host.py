"""CPU checks of tests/glue_ref.py against torch's own operators, so that tests/test_glue_views_gpu.py does not rest on an
untested reference."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import glue_ref
from tests.hipops import AMAX_REC_WORDS

SHAPES = [(2, 4, 1, 1), (1, 4, 1, 2), (1, 4, 2, 1), (2, 8, 5, 7), (2, 8, 6, 8), (1, 4, 33, 47), (2, 4, 1, 10), (2, 4, 5, 1)]


def _x(shape, seed=0):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape)))
    if shape[0] > 1:
        x[1] += 4.0
    return x


@pytest.mark.parametrize("shape", SHAPES)
def test_pool_and_nearest_references_match_torch(shape):
    """Max-pool (also on all-negative data and with -inf present: the border is -inf, never 0), average pool (divisor = taps
    inside) and nearest x2 are torch's float64 operators bit for bit."""
    x = _x(shape)
    neg = -1.0 - x.abs()
    inf = x.clone()
    inf.view(-1)[::3] = float("-inf")
    for t in (x, neg, inf):
        want = F.max_pool2d(t.double(), 3, 2, 1)
        got = glue_ref.maxpool3x3s2(t)
        assert got.dtype == torch.float64 and torch.equal(got, want)
    assert (glue_ref.maxpool3x3s2(neg) <= -1.0).all()
    got = glue_ref.avgpool2x2_ceil(x)
    want = F.avg_pool2d(x.double(), 2, 2, 0, ceil_mode=True)
    assert got.shape == want.shape and (got - want).abs().max().item() <= 2.0**-50 * x.abs().max().item()
    assert torch.equal(glue_ref.nearest2x(x), F.interpolate(x, scale_factor=2, mode="nearest"))


def test_layout_and_broadcast_add_references():
    x = _x((3, 3, 5, 7))
    y = glue_ref.nchw3_to_nhwc4(x)
    assert y.shape == (3, 5, 7, 4) and torch.equal(y[..., :3].permute(0, 3, 1, 2), x)
    assert torch.equal(y[..., 3].view(torch.int32), torch.zeros(3, 5, 7, dtype=torch.int32))  # +0.0, not -0.0
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(7, 8, generator=g), torch.randn(3, 8, generator=g)
    want = a.double() + b.double().repeat(3, 1)[:7]
    assert torch.equal(glue_ref.add_bcast(a, b), want)
    assert torch.equal(glue_ref.add_bcast(a, b[:1]), a.double() + b[0].double())
    # one fp32 addition is the float64 sum rounded once
    assert torch.equal(glue_ref.add_bcast(a, b).float(), a + b.repeat(3, 1)[:7])


@pytest.mark.parametrize("shape,size", [((2, 4, 7, 9), (7, 9)), ((2, 4, 7, 9), (14, 18)), ((2, 4, 7, 9), (28, 36)), ((2, 4, 10, 14), (20, 28)),
                                        ((2, 4, 10, 14), (40, 56)), ((1, 4, 1, 1), (4, 4)), ((1, 4, 5, 6), (20, 24))])
def test_bilinear_reference_is_torch_float64_at_integer_ratios(shape, size):
    """x1, x2, x4: (o + 0.5) * s - 0.5 is exact in fp32 (s a power of two, the sums short), so the fp32 coordinates are the
    float64 ones and the reference equals F.interpolate on float64 input bit for bit; x1 returns the input."""
    x = _x(shape)
    got = glue_ref.bilinear(x, size)
    want = F.interpolate(x.double(), size=size, mode="bilinear", align_corners=False)
    assert torch.equal(got, want)
    if tuple(size) == tuple(shape[2:]):
        assert torch.equal(got, x.double())
    add = _x((shape[0], shape[1]) + tuple(size), 3)
    assert torch.equal(glue_ref.bilinear(x, size, add), want + add.double())


# (input h x w, output size, the distance measured on the CPU as a fraction of max|x|)
NONINTEGER = [((9, 12), (18, 25), 2.0e-7), ((20, 27), (40, 53), 8.2e-7), ((40, 53), (20, 27), 8.3e-7), ((65, 66), (130, 131), 2.3e-6)]


@pytest.mark.parametrize("hw,size,measured", NONINTEGER)
def test_bilinear_reference_distance_from_torch_float64(hw, size, measured):
    """At non-integer ratios the fp32 source coordinates are rounded (an ulp of a coordinate near 64 is 7.6e-6 of a pixel), so
    "the formula in fp32 coordinates" and torch's float64 operator - which computes the coordinates in float64 - differ.  The
    distance is a property of the two references alone; measured on the CPU with this test's data (two images of eight
    channels, unit normal, the second shifted by 4), as a fraction of max|x|:
        9 x 12 -> 18 x 25      2.0e-7
        20 x 27 -> 40 x 53     8.2e-7
        40 x 53 -> 20 x 27     8.3e-7
        65 x 66 -> 130 x 131   2.3e-6
    (unshifted unit-normal data, whose max|x| is half as large, gives about twice these fractions) and asserted below twice
    the measured value.  This bounds how far the coordinate rounding takes the kernel's documented formula from the operator
    the model was trained with; the GPU test compares with the fp32-coordinate reference and needs no slack for it."""
    x = _x((2, 8) + hw, 1)
    got = glue_ref.bilinear(x, size)
    want = F.interpolate(x.double(), size=size, mode="bilinear", align_corners=False)
    d = (got - want).abs().max().item() / x.abs().max().item()
    print(f"bilinear reference {hw} -> {size}: {d:.2e} of max|x| from torch float64")
    assert 0 < d < 2 * measured


def test_bilinear_reference_edges():
    """A 1-pixel source is constant; 1 x 5 -> 3 x 20 has a single source row (i1 = i0 = 0); the weights are in [0, 1], sum to
    one within an ulp and the source indices stay inside the image."""
    x = _x((1, 4, 1, 1))
    assert torch.equal(glue_ref.bilinear(x, (4, 4)), x.double().expand(1, 4, 4, 4))
    x = _x((2, 4, 1, 5))
    got = glue_ref.bilinear(x, (3, 20))
    want = F.interpolate(x.double(), size=(3, 20), mode="bilinear", align_corners=False)
    assert (got - want).abs().max().item() <= 2.0**-22 * x.abs().max().item()
    assert torch.equal(got[:, :, 0], got[:, :, 2])
    for n_in, n_out in ((1, 4), (5, 20), (65, 130), (53, 27), (129, 258)):
        i0, i1, hgh, l = glue_ref.bilinear_axis(n_in, n_out)
        assert 0 <= int(i0.min()) and int(i1.max()) <= n_in - 1 and ((i1 - i0 == 1) | (i0 == n_in - 1)).all()
        assert (l >= 0).all() and (l < 1).all() and (hgh > 0).all() and (hgh <= 1).all()
        assert ((hgh + l) - 1).abs().max().item() <= 2.0**-24
        assert torch.equal(hgh.float().double(), hgh) and torch.equal(l.float().double(), l)  # fp32 values


def test_record_value():
    rec = torch.zeros(AMAX_REC_WORDS, dtype=torch.int32)
    assert glue_ref.record_value(rec) == 0.0
    vals = np.array([0.5, 3.25, 1e-40, 0.0], dtype=np.float32)
    for line, v in zip((0, 7, 20, 31), vals):
        rec[line * 32] = int(np.array([v]).view(np.int32)[0])
    rec[7 * 32 + 1] = 0x7F000000  # words 1..31 of a line are not part of the record
    assert glue_ref.record_value(rec) == 3.25
    rec[31 * 32] = int(np.array([np.inf], dtype=np.float32).view(np.int32)[0])
    assert glue_ref.record_value(rec) == float("inf")
