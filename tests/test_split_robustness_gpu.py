"""Model-level robustness of the fp16-plane arithmetic ("Next round" item 2).

The default product path multiplies fp32 operands as two scaled fp16 planes (ymk_conv_split.hip); the scale of the
activations is ONE power of two per launch, taken from the max|x| record the producer of the tensor left behind (static
bounds for LayerNorm outputs).  Seeded checkpoints have well-behaved channels, trained ones do not: a LayerNorm gain or a
folded BatchNorm scale can sit 2^10 - 2^12 above its peers, a dead channel can have a vanishing running variance.  These
tests plant exactly that in the checkpoints and compare the whole nets - split path on, as the product runs it - with the
CPU oracle (reference numerics: models/parseq.py:159-311, models/dbnet_plus.py:200-230, models/rtdetr*.py) at the usual
tolerances (probability maps / logits 1e-3, boxes 1e-4), and with the exact-fp32 kernels on the discrete outputs (token ids,
AR step counts).  Inside each, `amax_check` re-measures every recorded maximum: none may lie below the truth."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


class _AmaxCheck:
    """ymk_debug_option("amax_check", 1) around a block; afterwards: records checked / below the truth / loose."""

    def __enter__(self):
        from yomitoku_amd import _lib

        self.lib = _lib
        self.before = _lib.amax_check_counters()
        _lib.debug_option("amax_check", int(__import__("os").environ.get("YMK_AMAX_CHECK_LEVEL", 1)))
        return self

    def __exit__(self, *exc):
        self.lib.debug_option("amax_check", 0)
        now = self.lib.amax_check_counters()
        self.checked, self.below, self.loose = (int(a - b) for a, b in zip(now[:3], self.before[:3]))
        return False


def _scale_rows(t, rows, factor):
    t = t.clone()
    t[rows] = t[rows] * factor
    return t


def test_parseq_with_a_layernorm_gain_outlier_and_a_loud_qkv_row(dev):
    """One LayerNorm gain channel x 2^10 (block 3, norm1: its output - the q|k|v GEMM's input - then carries a channel 1000
    times above the rest, and the STATIC bound sqrt(D) max|gamma| + max|beta| stacks a further ~2^2 on top), one q row of the
    next block's qkv x 2^8 (the attention's fp16 planes take their scale from the qkv record, which that row now owns), and one
    fc1 row x 2^8 (a loud hidden unit in front of fc2)."""
    from oracle.parseq import parseq_forward
    from tests.test_parseq_gpu import _net
    from yomitoku_amd.utils.synth import parseq_state_dict, synthetic_line_batch

    sd = parseq_state_dict(1235, eos_bias=5.5)
    sd["encoder.blocks.3.norm1.weight"] = _scale_rows(sd["encoder.blocks.3.norm1.weight"], [17], 2.0 ** 10)
    sd["encoder.blocks.4.attn.qkv.weight"] = _scale_rows(sd["encoder.blocks.4.attn.qkv.weight"], [5], 2.0 ** 8)
    sd["encoder.blocks.4.attn.qkv.bias"] = _scale_rows(sd["encoder.blocks.4.attn.qkv.bias"], [5], 2.0 ** 8)
    sd["encoder.blocks.6.mlp.fc1.weight"] = _scale_rows(sd["encoder.blocks.6.mlp.fc1.weight"], [100], 2.0 ** 8)
    ocfg, net = _net(dev, sd)
    x = synthetic_line_batch(23, 128, 256)  # 128 lines x 256 tokens: every encoder GEMM fills the chip (the split path)
    ref, steps = parseq_forward(sd, ocfg, x, return_steps=True)
    with _AmaxCheck() as chk:
        out = net(x.to(dev)).cpu()
        got_steps = net.last_ar_steps
    net.set_conv_split(0)
    exact = net(x.to(dev)).cpu()
    exact_steps = net.last_ar_steps
    net.close()
    print("records checked", chk.checked, "below", chk.below, "loose", chk.loose, "max|logit|", float(ref.abs().max()),
          "split vs oracle", float((out - ref).abs().max()), "exact vs oracle", float((exact - ref).abs().max()))
    assert chk.checked >= 10 and chk.below == 0  # (a launch that carries its LayerNorm, or the whole MLP, has no input tensor to re-measure)
    assert got_steps == exact_steps == steps and out.shape == ref.shape
    assert torch.equal(out.argmax(-1), exact.argmax(-1)), "the fp16 planes moved a token the exact-fp32 kernels decode"
    assert torch.equal(out.argmax(-1), ref.argmax(-1))
    # a gain of 2^10 amplifies fp32's OWN rounding: the exact-fp32 kernels sit 6e-3 from the CPU oracle on this checkpoint
    # (measured; an fmaf chain against oneDNN's blocked sums), so the bar is what exact fp32 achieves, not the 1e-3 of
    # well-conditioned checkpoints - the planes must not be further from the oracle than the exact kernels are
    e_exact = (exact - ref).abs().max().item()
    assert e_exact < 5e-2
    assert (out - ref).abs().max().item() < max(1e-3, 1.5 * e_exact)
    assert (out - exact).abs().max().item() < max(1e-3, 1.5 * e_exact)


def _dbnet_outlier_checkpoint():
    from yomitoku_amd.utils.synth import dbnet_state_dict

    sd = dbnet_state_dict(1234)
    # a folded BatchNorm channel 2^12 above its peers in the middle of a bottleneck (the next 3 x 3 reads it), and one more at
    # the output of a stage (every consumer of the residual stream and the FPN lateral read it)
    sd["backbone.body.layer2.1.bn1.weight"] = _scale_rows(sd["backbone.body.layer2.1.bn1.weight"], [9], 2.0 ** 12)
    sd["backbone.body.layer1.2.bn3.weight"] = _scale_rows(sd["backbone.body.layer1.2.bn3.weight"], [40], 2.0 ** 6)
    # a dead channel: vanishing running variance (scale = gamma / sqrt(var + eps) = 316 gamma) around a zero mean
    v = sd["backbone.body.layer3.0.bn2.running_var"].clone()
    v[3] = 1e-12
    sd["backbone.body.layer3.0.bn2.running_var"] = v
    return sd


def test_dbnet_with_a_folded_bn_outlier_and_a_dead_channel(dev):
    from oracle.dbnet import dbnet_forward
    from yomitoku_amd.nets import DBNet

    sd = _dbnet_outlier_checkpoint()
    net = DBNet().load_state_dict(sd).to(dev)
    x = torch.randn(2, 3, 640, 960, generator=torch.Generator().manual_seed(31))
    ref = dbnet_forward(sd, x)["binary"]
    with _AmaxCheck() as chk:
        out = net(x.to(dev))["binary"].cpu()
    net.set_conv_split(0)
    exact = net(x.to(dev))["binary"].cpu()
    net.close()
    print("records checked", chk.checked, "below", chk.below, "loose", chk.loose, "split vs oracle", float((out - ref).abs().max()),
          "exact vs oracle", float((exact - ref).abs().max()), "map mean / std", float(ref.mean()), float(ref.std()))
    assert chk.checked >= 40 and chk.below == 0
    assert 0.02 < ref.mean().item() < 0.98 and ref.std().item() > 0.02  # not saturated: the comparison means something
    assert (out - ref).abs().max().item() < 1e-3
    assert (out - exact).abs().max().item() < 1e-3
    # the binarised map the box extraction sees (threshold 0.3): the same pixels, up to those within 1e-4 of the threshold
    near = (ref - 0.3).abs() < 1e-4
    assert torch.equal((out > 0.3) | near, (ref > 0.3) | near)


def test_rtdetr_with_a_folded_bn_outlier(dev):
    from oracle.rtdetr import rtdetr_forward
    from tests.test_rtdetr_gpu import _net, assert_same_detections
    from yomitoku_amd.utils.synth_rtdetr import rtdetr_state_dict

    sd = rtdetr_state_dict(1242, num_classes=6)
    sd["backbone.res_layers.1.blocks.0.branch2a.norm.weight"] = _scale_rows(sd["backbone.res_layers.1.blocks.0.branch2a.norm.weight"], [7], 2.0 ** 12)
    v = sd["backbone.res_layers.2.blocks.1.branch2b.norm.running_var"].clone()
    v[11] = 1e-12
    sd["backbone.res_layers.2.blocks.1.branch2b.norm.running_var"] = v
    net = _net(dev, sd, 6)
    x = torch.rand(2, 3, 640, 640, generator=torch.Generator().manual_seed(19))
    ref = rtdetr_forward(sd, x)
    with _AmaxCheck() as chk:
        out = net(x.to(dev))
    lg, bx = out["pred_logits"].cpu().numpy(), out["pred_boxes"].cpu().numpy()
    net.close()
    print("records checked", chk.checked, "below", chk.below, "loose", chk.loose)
    assert chk.checked >= 20 and chk.below == 0
    assert np.isfinite(lg).all() and np.isfinite(bx).all()
    assert_same_detections(lg, bx, ref["pred_logits"].numpy(), ref["pred_boxes"].numpy())


def test_an_all_zero_input_takes_the_clamped_scale(dev):
    """max|x| = 0 (a record that was never raised: an all-zero tensor - what a black page is after a ReLU) must give
    bias-only outputs, not NaNs from a 0 x inf scale pair: the f16_scales clamp (ymk_conv_split.hip) - at operator level on
    the three fp16 kernels, and through a whole DBNet on an all-zero input tensor against the oracle."""
    from oracle.dbnet import dbnet_forward
    from tests import hipops
    from yomitoku_amd import _lib
    from yomitoku_amd.nets import DBNet
    from yomitoku_amd.utils.synth import dbnet_state_dict

    g = torch.Generator().manual_seed(3)
    wt = torch.randn(128, 64, 3, 3, generator=g) / 24.0
    sc, bi = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g)
    x = torch.zeros(2, 64, 160, 160)
    try:
        _lib.debug_option("conv_split", 16)
        for tile in (0, 3, 21):
            _lib.debug_option("conv_split_tile", tile)
            y = hipops.conv2d(x.to(dev), wt, sc, bi, None, 1, 1, 1, "none").cpu()
            assert torch.equal(y, bi.view(1, -1, 1, 1).expand_as(y)), tile
    finally:
        _lib.debug_option("conv_split", -1)
        _lib.debug_option("conv_split_tile", 0)
    sd = dbnet_state_dict(1234)
    net = DBNet().load_state_dict(sd).to(dev)
    xz = torch.zeros(1, 3, 640, 960)
    out = net(xz.to(dev))["binary"].cpu()
    net.close()
    ref = dbnet_forward(sd, xz)["binary"]
    assert torch.isfinite(out).all() and (out - ref).abs().max().item() < 1e-3


def test_black_and_white_pages_through_the_whole_analyzer(dev):
    """Pages without content - all black, all white - through DocumentAnalyzer.serve next to ordinary pages: constant inputs
    drive whole activation tensors to a single value (records at the extremes of their range); every page must come back as a
    schema, equal to its own `__call__`, with every recorded maximum at or above the truth."""
    from tests.test_pipeline_gpu import _assert_same_schema
    from tests.test_serving_gpu import _analyzer
    from yomitoku_amd.utils.synth import synthetic_page_with_truth

    an = _analyzer()
    pages = [np.zeros((1200, 1600, 3), np.uint8), synthetic_page_with_truth(61, 1200, 1600)[0], np.full((1200, 1600, 3), 255, np.uint8),
             synthetic_page_with_truth(62, 1200, 1600)[0]]
    singles = [an(p)[0].model_dump() for p in pages]
    with _AmaxCheck() as chk:
        out = an.serve(pages, wave=4, in_flight=1)
    an.close()
    assert chk.below == 0 and chk.checked >= 100
    for want, got in zip(singles, out):
        assert not isinstance(got, BaseException), got
        _assert_same_schema(want, got.model_dump())
