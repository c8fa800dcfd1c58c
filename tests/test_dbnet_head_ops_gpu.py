"""The DBNet++ head kernels one at a time, each against a plain float64 restatement on the CPU computed from the fp32 inputs the
kernel received: the binarize head's ConvTranspose2d(64, 64, 2, 2) + BatchNorm + ReLU as a 1 x 1 panel with the scattering
EPI_DECONV2X2 epilogue (with the model's own panel packing, make_deconv2x2_panel, on every route and operand precision the
convolution path has), the final ConvTranspose2d(64, 1, 2, 2) + sigmoid (k_deconv_to1), and the adaptive-scale-fusion block
(k_gap_partial / k_gap_final, k_asf_gate, k_asf_mean, k_asf_apply: ScaleChannelSpatialAttention + the per-scale multiply of
ScaleFeatureSelection, models/layers/dbnet_feature_attention.py)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _deconv_reference(x, w, scale, bias):
    """relu(conv_transpose2d(x, w, stride=2) * scale + bias) in float64."""
    y = F.conv_transpose2d(x.double(), w.double(), stride=2)
    return torch.relu(y * scale.double().view(1, -1, 1, 1) + bias.double().view(1, -1, 1, 1))


def _deconv_operands(n, cin, h, w, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g)
    x[-1] += 1.0  # the images differ
    wt = torch.randn(cin, cout, 2, 2, generator=g) / cin ** 0.5
    scale, bias = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.5
    return x, wt, scale, bias


@pytest.mark.parametrize("cout", [32, 64, 128])
def test_deconv2x2_epilogue_small_m_exact_fp32(dev, cout):
    """A grid-starved launch (M = 35 rows: the split-K kernel, exact fp32 operands) with an odd width.  Tolerance 3e-6 of
    max|y|: a k-ordered fmaf chain of 64 terms, as tests/test_conv_split_gpu.py bounds the exact kernels."""
    from tests import hipops

    x, wt, scale, bias = _deconv_operands(1, 64, 5, 7, cout, 40 + cout)
    y = hipops.deconv2x2(x.to(dev), wt, scale, bias, act="relu").cpu()
    ref = _deconv_reference(x, wt, scale, bias)
    assert y.shape == ref.shape
    err = (y.double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"deconv small M cout={cout}: {err:.2e}")
    assert err < 3e-6


# conv_split code, conv_split_tile, mfma products per fp32-grade product of the launch that must have run, tolerance / max|y|
BIG_RUNS = ([(0, 0, 0.0, 3e-6)] + [(16, t, 3.0, 4e-6) for t in (0, 1, 3, 21, 30)]
            + [(3, 0, 6.0, 4e-6), (2, 0, 3.0, 2.0 ** -14), (3, 1, 6.0, 4e-6), (2, 1, 3.0, 2.0 ** -14)])


def test_deconv2x2_epilogue_chip_filling_every_route(dev):
    """The binarize head's shape at a chip-filling M (2 x 150 x 201 = 60 300 rows, odd width; cin = 64, cout = 64: a 256-column
    panel) under every operand precision and forced tile of the split path: exact fp32 ("conv_split" 0), two fp16 planes (16)
    on the automatic tile and on tiles 1, 3, 21 and 30 - which the A-stationary kernel refuses for this epilogue, so
    the launch falls back to the register-staged kernel - and three / two bf16 planes (3 / 2) on the automatic tile and on
    tile 1.  ymk_prof_launch_table names the
    kernel family that ran.  Tolerances as tests/test_conv_split_gpu.py asserts them: 3e-6 of max|y| for exact fp32, 4e-6 for
    two fp16 planes and three bf16 planes, 2^-14 for two bf16 planes (products to 2^-16)."""
    import ctypes

    from tests import hipops
    from yomitoku_amd import _lib

    lib = _lib.load()
    x, wt, scale, bias = _deconv_operands(2, 64, 150, 201, 64, 50)
    ref = _deconv_reference(x, wt, scale, bias)
    top = ref.abs().max().item()
    xd = x.to(dev)
    errs = {}
    try:
        for split, tile, products, tol in BIG_RUNS:
            _lib.debug_option("conv_split", split)
            _lib.debug_option("conv_split_tile", tile)
            _lib.check(lib.ymk_prof_begin())
            y = hipops.deconv2x2(xd, wt, scale, bias, act="relu")
            ms, fl, ln = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
            _lib.check(lib.ymk_prof_end(ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(ln)))
            rows = _lib.prof_launch_table()
            assert len(rows) == 1 and rows[0][3] == products, (split, tile, rows)
            errs[(split, tile)] = (y.cpu().double() - ref).abs().max().item() / top
            print(f"deconv chip-filling conv_split={split} tile={tile}: {errs[(split, tile)]:.2e}")
            assert errs[(split, tile)] < tol, (split, tile, errs[(split, tile)])
    finally:
        _lib.debug_option("conv_split", -1)
        _lib.debug_option("conv_split_tile", 0)


@pytest.mark.parametrize("cout", [32, 128])
def test_deconv2x2_epilogue_chip_filling_other_widths(dev, cout):
    """The same chip-filling rows with a 128- and a 512-column panel, exact fp32 and the models' default (two fp16 planes)."""
    from tests import hipops
    from yomitoku_amd import _lib

    x, wt, scale, bias = _deconv_operands(2, 64, 150, 201, cout, 60 + cout)
    ref = _deconv_reference(x, wt, scale, bias)
    top = ref.abs().max().item()
    xd = x.to(dev)
    try:
        for split, tol in ((0, 3e-6), (16, 4e-6)):
            _lib.debug_option("conv_split", split)
            err = (hipops.deconv2x2(xd, wt, scale, bias, act="relu").cpu().double() - ref).abs().max().item() / top
            print(f"deconv chip-filling cout={cout} conv_split={split}: {err:.2e}")
            assert err < tol
    finally:
        _lib.debug_option("conv_split", -1)


def test_deconv2x2_to1_sigmoid(dev):
    """sigmoid(conv_transpose2d(x, w[64][1][2][2], stride=2) + bias) in float64, N = 2 with odd H and W and 66 246 input pixels
    (> 65 536: the grid-stride loop of the 16-lane groups runs).  Tolerance 1e-6 absolute: the kernel's dot products of 64 terms
    sum 4 per lane then over a 16-lane tree (7 levels): <= 7 * 2^-24 * sum|x w| ~ 4e-7 * 4 here, times sigmoid' <= 1/4, plus
    expf and the reciprocal (2^-23)."""
    from tests import hipops

    g = torch.Generator().manual_seed(70)
    x = torch.randn(2, 64, 181, 183, generator=g)
    x[1] -= 0.5
    w = torch.randn(64, 1, 2, 2, generator=g) / 16
    bias = -0.3
    y = hipops.deconv2x2_to1_sigmoid(x.to(dev), w, bias).cpu()
    ref = torch.sigmoid(F.conv_transpose2d(x.double(), w.double(), stride=2) + bias)
    assert y.shape == ref.shape
    err = (y.double() - ref).abs().max().item()
    print(f"deconv_to1: {err:.2e}")
    assert err < 1e-6


def _asf_reference(ax, fuse, w1, w2, sp33, sp11, watt):
    """ScaleChannelSpatialAttention.forward + the per-scale multiply of ScaleFeatureSelection.forward, in float64."""
    ax, fuse = ax.double(), fuse.double()
    gap = ax.mean(dim=(2, 3))                                              # channel_wise: AdaptiveAvgPool2d(1)
    gate = torch.sigmoid(torch.relu(gap @ w1.double().t()) @ w2.double().t())   # conv 1x1 -> ReLU -> conv 1x1, .sigmoid()
    gx = gate[:, :, None, None] + ax                                       # global_x + x
    mean = gx.mean(dim=1, keepdim=True)
    sp = torch.sigmoid(sp11 * torch.relu(F.conv2d(mean, sp33.double().view(1, 1, 3, 3), padding=1)))   # spatial_wise
    score = torch.sigmoid(F.conv2d(sp + gx, watt.double().view(4, 64, 1, 1)))                      # attention_wise
    return torch.cat([score[:, i:i + 1] * fuse[:, 64 * i:64 * (i + 1)] for i in range(4)], dim=1)


@pytest.mark.parametrize("hw", [(7, 9), (7, 300), (200, 150)])
def test_dbnet_asf_chain(dev, hw):
    """The ASF block over n = 2 images whose channel means differ clearly (a gate applied to the wrong image fails), at
    63 pixels (fewer than GAP_CHUNKS = 256: most chunks empty), 7 x 300 and 200 x 150; cmid = 16.  Tolerance 2e-6 of max|out|:
    out = score * fuse with score = sigmoid(a), sigmoid' <= 1/4, and a = the attention row . (x + gate + sp) summed in fp32 over
    64 terms (a 16-lane tree) - about 4e-7 |watt| . |x + gate + sp|, a few 1e-7 with these weights; the gate's own error (the
    fp32 mean over up to 30 000 pixels, through two small 1 x 1 layers whose rows sum to below 1 in magnitude) is smaller."""
    from tests import hipops

    h, w = hw
    g = torch.Generator().manual_seed(80 + h * w)
    ax = torch.randn(2, 64, h, w, generator=g)
    ax[0] -= 1.0
    ax[1] += 2.0
    fuse = torch.randn(2, 256, h, w, generator=g)
    w1 = torch.randn(16, 64, generator=g) / 16
    w2 = torch.randn(64, 16, generator=g) / 8
    sp33 = torch.randn(3, 3, generator=g) / 3
    sp11 = 1.5
    watt = torch.randn(4, 64, generator=g) / 8
    out = hipops.dbnet_asf(ax.to(dev), fuse.to(dev), w1, w2, sp33, sp11, watt).cpu()
    ref = _asf_reference(ax, fuse, w1, w2, sp33, sp11, watt)
    err = (out.double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"asf {h}x{w}: {err:.2e}")
    assert err < 2e-6
    # the two images' gates really differ: swapping the images' gates would move the output far beyond the tolerance
    gap = ax.double().mean(dim=(2, 3))
    gate = torch.sigmoid(torch.relu(gap @ w1.double().t()) @ w2.double().t())
    assert (gate[0] - gate[1]).abs().max().item() > 1e-2
