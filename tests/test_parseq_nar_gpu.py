"""PARSeq's non-autoregressive mode (`decode_ar: 0`, models/parseq.py:253-262) on the device: one decoder pass over all
positions with <bos> as the only context, then the refinement passes.  Checked against tests/golden/parseq_ref_nar.npz -
what the REFERENCE class returned for the same seeded checkpoints and inputs (tools/pin_parseq_nar.py; the seeds were
chosen there so that every row up to a sample's first <eos> has a top-1 / top-2 margin >= 1e-2, ten times the logit
tolerance: the token comparison is meaningful).  Tolerances are those of tests/test_parseq_gpu.py: tokens exact,
logits < 1e-3.  The cross-attention kernel of the pass is also tested alone against fp64 (tolerance of the fp64
attention test in tests/test_seq_ops_gpu.py: 2e-5 of max|ref|)."""
import ast
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3
GOLD = os.path.join(os.path.dirname(__file__), "golden")
COUNTERS = ("allocs_in_forward", "arena_grows_in_forward", "lazy_panel_builds", "syncs_in_forward")


def _gold():
    return np.load(os.path.join(GOLD, "parseq_ref_nar.npz"))


def _net(dev, z, tag, decode_ar=0, **over):
    from yomitoku_amd.nets import PARSeq
    from yomitoku_amd.utils.synth import parseq_state_dict

    c = ast.literal_eval(str(z[f"{tag}_cfg"]))
    kw = ast.literal_eval(str(z[f"{tag}_ckpt"]))
    cfg = {
        "num_tokens": c["num_tokens"], "max_label_length": c["max_label_length"], "refine_iters": c["refine_iters"],
        "decode_ar": decode_ar, "repetition_stop": True, "data": {"img_size": [32, 800]},
        "encoder": {"patch_size": list(c["patch"]), "num_heads": c["heads"], "embed_dim": c["dim"], "mlp_ratio": 4, "depth": c["enc_depth"]},
        "decoder": {"embed_dim": c["dim"], "num_heads": c["heads"], "mlp_ratio": 4, "depth": 1},
    }
    cfg.update(over)
    return PARSeq(cfg).load_state_dict(parseq_state_dict(**kw)).to(dev)


def _check_against_golden(z, tag, lg):
    stride = int(z["stride"])
    assert lg.shape[:2] == z[f"{tag}_ids"].shape
    top = np.abs(lg.max(-1).values.numpy() - z[f"{tag}_top"]).max()
    smp = np.abs(lg[:, :, ::stride].numpy() - z[f"{tag}_sample"]).max()
    print(f"{tag}: max |d top logit| {top:.2e}, max |d sampled logit| {smp:.2e}, golden margin {float(z[f'{tag}_margin']):.4f}")
    assert top < LOGIT_TOL and smp < LOGIT_TOL
    assert np.array_equal(lg.argmax(-1).numpy().astype(np.int64), z[f"{tag}_ids"].astype(np.int64))


TAGS = ["lite_r1", "lite_r0", "lite_r2", "wide_r1"]


@pytest.mark.parametrize("tag", TAGS)
def test_matches_reference_golden(dev, tag):
    """Logits within 1e-3, tokens identical, all 101 rows returned, no greedy steps."""
    z = _gold()
    assert float(z[f"{tag}_margin"]) >= 1e-2
    net = _net(dev, z, tag)
    logits = net(torch.from_numpy(z["x"]).to(dev))
    assert logits.shape[1] == 101 and net.last_ar_steps == 0
    _check_against_golden(z, tag, logits.cpu())


@pytest.mark.parametrize("split", [0, None])
def test_exact_fp32_and_default_planes_both_hold_the_tolerance(dev, split):
    z = _gold()
    for tag in ("lite_r1", "wide_r1"):
        net = _net(dev, z, tag)
        net.set_conv_split(split)
        _check_against_golden(z, tag, net(torch.from_numpy(z["x"]).to(dev)).cpu())


@pytest.mark.parametrize("tag", ["lite_r1", "lite_r0", "wide_r1"])
def test_grouped_forward_equals_single_group_calls(dev, tag):
    """ymk_parseq_forward_groups with four groups of different widths (ragged memory tables): every group gets what its own
    single-group call gets (same tokens; logits to the last bits - the kernel shape choice of a GEMM follows its row count,
    as in tests/test_parseq_gpu.py), out_len = 101 and ar_steps = 0 per group; the golden batch is one of the groups."""
    from yomitoku_amd.utils.synth import synthetic_line_batch

    z = _gold()
    net = _net(dev, z, tag)
    xs = [synthetic_line_batch(31, 3, 160), torch.from_numpy(z["x"]), synthetic_line_batch(32, 1, 800), synthetic_line_batch(33, 4, 72)]
    logits, out_lens, steps = net.forward_groups([x.to(dev) for x in xs])
    assert list(out_lens) == [101] * len(xs) and list(steps) == [0] * len(xs) and net.last_ar_steps == 0
    lg = logits.cpu()
    assert lg.shape[0] == sum(x.shape[0] for x in xs) and bool(torch.isfinite(lg).all())
    row = 0
    for i, x in enumerate(xs):
        got = lg[row : row + x.shape[0]]
        one = net(x.to(dev)).cpu()
        assert one.shape == got.shape
        assert torch.equal(one.argmax(-1), got.argmax(-1))
        assert (one - got).abs().max().item() < 1e-4
        if i == 1:
            _check_against_golden(z, tag, got)
        row += x.shape[0]
    again, _, _ = net.forward_groups([x.to(dev) for x in xs])
    assert torch.equal(again.cpu(), lg), "grouped forward must be bit-identical on repeat"


def test_counters_nar_forwards_rise_and_a_reserved_forward_does_no_forbidden_work(dev):
    from yomitoku_amd import _lib
    from yomitoku_amd.utils.synth import synthetic_line_batch

    z = _gold()
    net = _net(dev, z, "lite_r1")
    xs = [synthetic_line_batch(41 + i, b, w).to(dev) for i, (b, w) in enumerate([(3, 160), (2, 800), (5, 72)])]
    net.reserve(16, 32, 800)
    before = {k: _lib.stat(k) for k in COUNTERS}
    n0 = _lib.stat("nar_forwards")
    net(xs[0])
    assert _lib.stat("nar_forwards") == n0 + 1
    for _ in range(5):  # 80 grouped calls: more than the 64 staging slots of the row tables, so slots are taken again
        for _ in range(16):  # back to back, nothing waited for in between
            net.forward_groups(xs)
        torch.cuda.synchronize()
    net.forward_groups(xs[::-1])
    torch.cuda.synchronize()
    assert _lib.stat("nar_forwards") == n0 + 82
    after = {k: _lib.stat(k) for k in COUNTERS}
    assert after == before, {k: after[k] - before[k] for k in COUNTERS}


def test_an_ar_model_in_the_same_process_still_reproduces_its_golden(dev):
    """The modes do not leak into each other: decode_ar = 1 next to a live decode_ar = 0 model, forwards interleaved."""
    from yomitoku_amd.nets import PARSeq
    from yomitoku_amd.utils.synth import parseq_state_dict

    z = _gold()
    nar = _net(dev, z, "lite_r1")
    g = np.load(os.path.join(GOLD, "parseq_ref_eos.npz"))
    cfg = {"num_tokens": 7121, "max_label_length": 100, "refine_iters": 1, "decode_ar": 1, "repetition_stop": True,
           "data": {"img_size": [32, 800]},
           "encoder": {"patch_size": [4, 8], "num_heads": 6, "embed_dim": 192, "mlp_ratio": 4, "depth": 12},
           "decoder": {"embed_dim": 192, "num_heads": 6, "mlp_ratio": 4, "depth": 1}}
    ar = PARSeq(cfg).load_state_dict(parseq_state_dict(**ast.literal_eval(str(g["ckpt"])))).to(dev)
    nar(torch.from_numpy(z["x"]).to(dev))
    lg = ar(torch.from_numpy(g["x"]).to(dev)).cpu()
    assert ar.last_ar_steps == int(g["steps"]) and lg.shape[:2] == g["ids"].shape
    assert np.array_equal(lg.argmax(-1).numpy().astype(np.int32), g["ids"])
    assert np.abs(lg.max(-1).values.numpy() - g["top"]).max() < LOGIT_TOL
    assert np.abs(lg[:, :, ::97].numpy() - g["sample"]).max() < LOGIT_TOL
    _check_against_golden(z, "lite_r1", nar(torch.from_numpy(z["x"]).to(dev)).cpu())
    assert nar.last_ar_steps == 0


def test_any_other_decode_ar_is_refused(dev):
    from yomitoku_amd._lib import YmkError

    z = _gold()
    with pytest.raises(YmkError, match="decode_ar"):
        _net(dev, z, "lite_r0", decode_ar=2)


# ---------------------------------------------------------------------------------------------- the kernel alone
def _nar_attn(q, k, v, heads, lens, dev):
    """q [lq][D] shared; k / v [sum lens][D] (ragged) -> o [b][lq][D] through ymk_op_nar_cross_attention."""
    from yomitoku_amd import _lib

    lib = _lib.load()
    lq, d = q.shape
    b = len(lens)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    qd, kd, vd = (t.float().contiguous().to(dev) for t in (q, k, v))
    koff = torch.from_numpy(off).to(dev)
    klen = torch.tensor(lens, dtype=torch.int32, device=dev)
    o = torch.full((b, lq, d), float("nan"), device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.ymk_op_nar_cross_attention(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), b, heads, lq, max(lens),
                                                  d // heads, ctypes.c_float((d // heads) ** -0.5), koff.data_ptr(), klen.data_ptr(),
                                                  _lib.current_stream_ptr()), "ymk_op_nar_cross_attention")
    return o.cpu()


def _ref64(q, k, v, heads, lens):
    q, k, v = q.double().numpy(), k.double().numpy(), v.double().numpy()
    lq, d = q.shape
    hd = d // heads
    out = np.zeros((len(lens), lq, d))
    row = 0
    for i, n in enumerate(lens):
        for h in range(heads):
            sl = slice(h * hd, (h + 1) * hd)
            s = q[:, sl] @ k[row : row + n, sl].T * hd**-0.5
            p = np.exp(s - s.max(-1, keepdims=True))
            out[i, :, sl] = (p / p.sum(-1, keepdims=True)) @ v[row : row + n, sl]
        row += n
    return out


@pytest.mark.parametrize("heads,hd,lq,lens", [
    (6, 32, 101, [1, 37, 800, 8, 13]),    # one key; not a multiple of the 8-key tile (nor of the 4-key step); the longest memory; one tile
    (8, 64, 101, [800, 1, 99, 400]),      # one query per lane, two query blocks per sample
    (8, 32, 51, [5, 64]),
    (8, 48, 101, [131, 7]),               # parseq-small
    (8, 46, 51, [50, 9, 200]),            # the legacy parseq-tiny: rows only 8 B aligned, padded to 48 in LDS
    (8, 96, 101, [800, 3, 22]),           # parseq-large: 4-key tiles
])
def test_nar_cross_attention_against_fp64(dev, heads, hd, lq, lens):
    g = torch.Generator().manual_seed(hd * 1000 + lq)
    d = heads * hd
    q = torch.randn(lq, d, generator=g) * 2.0  # sharper softmax: exercises the running-max rescale
    k, v = torch.randn(sum(lens), d, generator=g), torch.randn(sum(lens), d, generator=g)
    ref = _ref64(q, k, v, heads, lens)
    got = _nar_attn(q, k, v, heads, lens, dev).double().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"heads {heads} hd {hd} lq {lq} lens {lens}: max err / max|ref| {err:.2e}")
    assert err < 2e-5


def test_nar_cross_attention_uniform_form_equals_the_ragged_one(dev):
    """Without tables sample i reads rows i * lk ..: the same bits as the table form on the same rows."""
    from yomitoku_amd import _lib

    g = torch.Generator().manual_seed(5)
    heads, hd, lq, lk, b = 6, 32, 101, 96, 3
    d = heads * hd
    q, k, v = torch.randn(lq, d, generator=g), torch.randn(b * lk, d, generator=g), torch.randn(b * lk, d, generator=g)
    ragged = _nar_attn(q, k, v, heads, [lk] * b, dev)
    lib = _lib.load()
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    o = torch.empty((b, lq, d), device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.ymk_op_nar_cross_attention(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), b, heads, lq, lk, hd,
                                                  ctypes.c_float(hd**-0.5), None, None, _lib.current_stream_ptr()),
                   "ymk_op_nar_cross_attention")
    assert torch.equal(o.cpu(), ragged)


# ---------------------------------------------------------------------------------------------- through the public classes
def _nar_yaml(tmp_path):
    p = tmp_path / "text_recognizer_nar.yaml"
    p.write_text("decode_ar: 0\n")
    return str(p)


def test_text_recognizer_with_decode_ar_0_on_the_sample_line(dev, tmp_path):
    from yomitoku_amd.data.functions import load_image
    from yomitoku_amd.text_recognizer import TextRecognizer
    from yomitoku_amd.utils.synth import parseq_state_dict

    (img,) = load_image(os.path.join(GOLD, "sample_text.jpg"))
    rec = TextRecognizer(model_name="parseq-tiny-dynw-v4", path_cfg=_nar_yaml(tmp_path), from_pretrained=False, device="cuda:0",
                         dynamic_width=True, batch_bucketing=True, source_downscale=True)
    rec.model.load_state_dict(parseq_state_dict(1235, eos_bias=6.0))
    assert int(rec._cfg.decode_ar) == 0 and int(rec.model.params()["decode_ar"]) == 0
    line = [[[0, 0], [90, 0], [90, 37], [0, 37]], [[3, 4], [60, 4], [60, 33], [3, 33]], [[30, 2], [88, 6], [86, 36], [28, 30]]]
    got, _ = rec(img, line)
    assert rec.model.last_ar_steps == 0
    assert len(got.contents) == len(got.scores) == len(got.directions) == len(got.points) == 3 and got.points == line
    assert all(isinstance(c, str) for c in got.contents) and all(0.0 <= s <= 1.0 for s in got.scores)
    many = rec.recognize_pages([img, img], [line, line[::-1]])
    assert many[0].contents == got.contents and many[1].contents == got.contents[::-1]
    assert many[1].points == line[::-1]


def test_serve_two_pages_with_decode_ar_0_keeps_the_page_order(dev, tmp_path):
    from tests.test_pipeline_gpu import _assert_same_schema
    from yomitoku_amd import DocumentAnalyzer
    from yomitoku_amd.utils.synth import dbnet_state_dict, parseq_state_dict, synthetic_page_with_truth
    from yomitoku_amd.utils.synth_rtdetr import rtdetr_state_dict

    configs = {
        "ocr": {"text_detector": {"from_pretrained": False},
                "text_recognizer": {"model_name": "parseq-tiny-dynw-v4", "path_cfg": _nar_yaml(tmp_path), "from_pretrained": False,
                                    "dynamic_width": True, "batch_bucketing": True, "source_downscale": True}},
        "layout_analyzer": {"layout_parser": {"from_pretrained": False}, "table_structure_recognizer": {"from_pretrained": False}},
    }
    an = DocumentAnalyzer(configs=configs, device="cuda:0")
    an.text_detector.model.load_state_dict(dbnet_state_dict(1234, out_bias=-2.0))
    an.text_recognizer.model.load_state_dict(parseq_state_dict(1235, eos_bias=6.0))
    an.layout.layout_parser.model.load_state_dict(rtdetr_state_dict(1240, num_classes=6, score_bias=-2.0))
    an.layout.table_structure_recognizer.model.load_state_dict(rtdetr_state_dict(1241, num_classes=3, score_bias=-1.0))
    assert int(an.text_recognizer.model.params()["decode_ar"]) == 0
    imgs = [synthetic_page_with_truth(3, 1000, 1400)[0], synthetic_page_with_truth(4, 1400, 1000)[0]]
    singles = [an(img)[0].model_dump() for img in imgs]
    assert sum(len(s["words"]) for s in singles) > 0 and an.text_recognizer.model.last_ar_steps == 0
    out = an.serve(imgs, wave=2, in_flight=2)
    assert len(out) == 2 and not any(isinstance(o, Exception) for o in out)
    for want, got in zip(singles, out):
        _assert_same_schema(want, got.model_dump())
    an.close()
