"""Planned workspaces ("workspace_reuse", include/ymk.h) on the device.

The mode changes WHERE a forward's activations live, never what is computed: every output must be `torch.equal` to the
bump arena's, for every net, in both arithmetic modes ("conv_split" 16 and 0), across shape changes inside a reservation,
and - the check that catches a buffer released one launch too early - with "workspace_poison" filling every released
range with NaN bit patterns at the moment of its release.  The goldens of the four nets hold in the mode within the
tolerances their own tests state; a serve job keeps the four "in_forward" counters at zero; the plan is never larger than
the bump arena's sum and never smaller than the live bound.  Nothing here asserts a ratio."""
import ast
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTERS = ("allocs_in_forward", "arena_grows_in_forward", "lazy_panel_builds", "syncs_in_forward")


def _stats():
    from yomitoku_amd import _lib

    return {k: _lib.stat(k) for k in ("workspace_planned_forwards", "ws_plan_bytes_last", "ws_bump_bytes_last", "ws_live_bound_last")}


def _tensors(out):
    if isinstance(out, dict):
        return [out[k] for k in sorted(out)]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in _tensors(o)]
    return [out if torch.is_tensor(out) else torch.as_tensor(out)]


def _same(want, got, what):
    a, b = _tensors(want), _tensors(got)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape, what
        if torch.is_floating_point(y):
            assert torch.isfinite(y).all(), f"{what}: non-finite output"
        assert torch.equal(x.cpu(), y.cpu()), f"{what}: planned workspace output differs from the bump arena's"


def _compare(make, calls, split, reserve=None):
    """Two handles with the same weights, bump and planned.  `calls`: functions net -> output, run in order on both (the
    bump handle is the reference for every call: a fresh bump result per shape); then all of them again with poison on."""
    from yomitoku_amd import _lib

    bump, plan = make(), make()
    for net in (bump, plan):
        net.set_conv_split(split)
    plan.set_workspace_reuse(True)
    try:
        if reserve is not None:
            bump.reserve(*reserve)
            plan.reserve(*reserve)
            print(f"reserve{reserve}: bump {bump.workspace_bytes} planned {plan.workspace_bytes}")
            assert 0 < plan.workspace_bytes < bump.workspace_bytes
        held = plan.workspace_bytes
        want = []
        for call in calls:
            s0 = _stats()["workspace_planned_forwards"]
            want.append(call(bump))
            assert _stats()["workspace_planned_forwards"] == s0, "a bump-arena forward counted as planned"
        for poison in (0, 1):
            _lib.debug_option("workspace_poison", poison)
            for i, call in enumerate(calls):
                s0 = _stats()["workspace_planned_forwards"]
                got = call(plan)
                torch.cuda.synchronize()
                st = _stats()
                assert st["workspace_planned_forwards"] == s0 + 1
                print(f"call {i} poison {poison}: live {st['ws_live_bound_last']} plan {st['ws_plan_bytes_last']} bump {st['ws_bump_bytes_last']}")
                assert 0 < st["ws_live_bound_last"] <= st["ws_plan_bytes_last"] < st["ws_bump_bytes_last"]
                _same(want[i], got, f"call {i}, conv_split {split}, poison {poison}")
        if reserve is not None:
            assert plan.workspace_bytes == held, "a forward inside the reservation resized the planned workspace"
    finally:
        _lib.debug_option("workspace_poison", 0)
        bump.close()
        plan.close()


# ---------------------------------------------------------------------------------------------------------------- DBNet
def _x(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("split", [16, 0])
def test_dbnet_is_bit_identical(dev, split):
    from yomitoku_amd.nets import DBNet
    from yomitoku_amd.utils.synth import dbnet_state_dict

    sd = dbnet_state_dict(1234)
    a, b = _x((2, 3, 160, 128), 1).to(dev), _x((1, 3, 96, 128), 2).to(dev)
    calls = [lambda n: n(a)["binary"], lambda n: n(b)["binary"], lambda n: n(a)["binary"]]
    _compare(lambda: DBNet().load_state_dict(sd).to(dev), calls, split, reserve=(2, 160, 128))


# ---------------------------------------------------------------------------------------------------------------- RT-DETR
@pytest.mark.parametrize("split", [16, 0])
@pytest.mark.parametrize("tag,nc,size,nq,seed", [("layout", 6, 640, 300, 1240), ("table", 3, 640, 300, 1241), ("cell", 6, 960, 1500, 1244)])
def test_rtdetr_is_bit_identical(dev, tag, nc, size, nq, seed, split):
    from tests.test_rtdetr_gpu import _net
    from yomitoku_amd.utils.synth_rtdetr import rtdetr_state_dict

    sd = rtdetr_state_dict(seed, num_classes=nc, eval_size=(size, size))
    g = torch.Generator().manual_seed(7)
    a, b = torch.rand(2, 3, size, size, generator=g).to(dev), torch.rand(1, 3, size, size, generator=g).to(dev)
    calls = [lambda n: n(a), lambda n: n(b), lambda n: n(a)]
    _compare(lambda: _net(dev, sd, nc, size, nq), calls, split, reserve=(2, size, size))


# ---------------------------------------------------------------------------------------------------------------- PARSeq
def _parseq_cfg(decode_ar=1, refine_iters=1, patch=(4, 8), dim=192, heads=6, depth=12, num_tokens=7121):
    return {
        "num_tokens": num_tokens, "max_label_length": 100, "refine_iters": refine_iters, "decode_ar": decode_ar,
        "repetition_stop": True, "data": {"img_size": [32, 800]},
        "encoder": {"patch_size": list(patch), "num_heads": heads, "embed_dim": dim, "mlp_ratio": 4, "depth": depth},
        "decoder": {"embed_dim": dim, "num_heads": heads, "mlp_ratio": 4, "depth": 1},
    }


def _parseq_calls(dev, shapes_a, shapes_b):
    from yomitoku_amd.utils.synth import synthetic_line_batch

    def batch(seed, shapes):
        return [synthetic_line_batch(seed + i, b, w).to(dev) for i, (b, w) in enumerate(shapes)]

    xa, xb = batch(11, shapes_a), batch(31, shapes_b)

    def run(xs):
        def call(net):
            if len(xs) == 1:
                lg = net(xs[0])
                return lg, torch.tensor([net.last_ar_steps])
            lg, lens, steps = net.forward_groups(xs)
            # rows beyond a group's out_len are not results (refine_iters = 0 only): compare what the call returns as valid
            rows, row = [], 0
            for x, n in zip(xs, lens):
                rows.append(lg[row : row + x.shape[0], :n])
                row += x.shape[0]
            return rows, torch.tensor(lens), torch.tensor(steps)

        return call

    return [run(xa), run(xb), run(xa)]


GROUPS = [(5, 160), (2, 800), (9, 72), (1, 96)]


@pytest.mark.parametrize("split", [16, 0])
@pytest.mark.parametrize("decode_ar", [1, 0])
@pytest.mark.parametrize("grouped", [False, True])
def test_parseq_tiny_is_bit_identical(dev, decode_ar, grouped, split):
    """parseq-tiny-dynw geometry: the greedy loop (fused decoder step, host flag, published-row tables) and `decode_ar: 0`,
    as one mini-batch and as a grouped call with four mini-batches of different widths."""
    from yomitoku_amd.nets import PARSeq
    from yomitoku_amd.utils.synth import parseq_state_dict

    sd = parseq_state_dict(1235, eos_bias=5.5)
    cfg = _parseq_cfg(decode_ar=decode_ar)
    calls = _parseq_calls(dev, GROUPS if grouped else [(5, 160)], [(3, 64), (3, 64)] if grouped else [(2, 96)])
    _compare(lambda: PARSeq(cfg).load_state_dict(sd).to(dev), calls, split, reserve=(17, 32, 800))


@pytest.mark.parametrize("split", [16, 0])
@pytest.mark.parametrize("dim,heads,patch,refine", [(384, 8, (16, 16), 1), (768, 12, (8, 8), 1), (384, 8, (16, 16), 0)])
def test_parseq_wide_geometries_are_bit_identical(dev, dim, heads, patch, refine, split):
    """D = 384 and 768 at reduced depth: the per-op decoder path (no fused step), the stored AR logits, and - refine_iters 0 -
    the copy of the AR logits to the output."""
    from yomitoku_amd.nets import PARSeq
    from yomitoku_amd.utils.synth import parseq_state_dict

    sd = parseq_state_dict(78, eos_bias=6.0, patch=patch, enc_dim=dim, dec_dim=dim, num_tokens=7312, enc_depth=2)
    cfg = _parseq_cfg(refine_iters=refine, patch=patch, dim=dim, heads=heads, depth=2, num_tokens=7312)
    calls = _parseq_calls(dev, [(3, 320), (2, 96)], [(2, 160)])
    _compare(lambda: PARSeq(cfg).load_state_dict(sd).to(dev), calls, split, reserve=(5, 32, 800))


def test_mode_switch_on_a_live_handle(dev):
    """set_workspace_reuse on a finalized model: plans and reservations are dropped, the next reserve re-sizes the slab (it
    shrinks), results stay the same; switching back grows it again."""
    from yomitoku_amd.nets import DBNet
    from yomitoku_amd.utils.synth import dbnet_state_dict

    net = DBNet().load_state_dict(dbnet_state_dict(1234)).to(dev)
    x = _x((2, 3, 160, 128), 1).to(dev)
    net.reserve(2, 160, 128)
    want, big = net(x)["binary"].clone(), net.workspace_bytes
    s0 = _stats()["workspace_planned_forwards"]
    net.set_workspace_reuse(True)
    net.reserve(2, 160, 128)
    small = net.workspace_bytes
    assert 0 < small < big
    assert torch.equal(net(x)["binary"], want) and _stats()["workspace_planned_forwards"] == s0 + 1
    net.set_workspace_reuse(False)
    assert torch.equal(net(x)["binary"], want) and _stats()["workspace_planned_forwards"] == s0 + 1
    assert net.workspace_bytes == big
    net.close()


def test_a_model_parameter_wins_over_the_process_default(dev):
    from yomitoku_amd import _lib
    from yomitoku_amd.nets import DBNet
    from yomitoku_amd.utils.synth import dbnet_state_dict

    sd = dbnet_state_dict(1234)
    x = _x((1, 3, 96, 128), 2).to(dev)
    follows, refuses = DBNet().load_state_dict(sd).to(dev), DBNet().load_state_dict(sd).to(dev)
    refuses.set_workspace_reuse(False)
    want = follows(x)["binary"].clone()
    try:
        _lib.debug_option("workspace_reuse", 1)
        s0 = _stats()["workspace_planned_forwards"]
        assert torch.equal(follows(x)["binary"], want)
        assert _stats()["workspace_planned_forwards"] == s0 + 1
        assert torch.equal(refuses(x)["binary"], want)
        assert _stats()["workspace_planned_forwards"] == s0 + 1
    finally:
        _lib.debug_option("workspace_reuse", 0)
    follows.close()
    refuses.close()


# ---------------------------------------------------------------------------------------------------------------- goldens
def test_dbnet_golden_holds(dev):
    from tests.test_dbnet_gpu import PROB_TOL
    from yomitoku_amd.nets import DBNet
    from yomitoku_amd.utils.synth import dbnet_state_dict

    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "dbnet_ref_64x96.npz"))
    net = DBNet().load_state_dict(dbnet_state_dict(int(z["seed"])))
    net.set_workspace_reuse(True)
    s0 = _stats()["workspace_planned_forwards"]
    out = net.to(dev)(torch.from_numpy(z["x"]).to(dev))["binary"].cpu().numpy()
    assert _stats()["workspace_planned_forwards"] == s0 + 1
    assert np.abs(out - z["prob"]).max() < PROB_TOL
    net.close()


@pytest.mark.parametrize("tag", ["layout", "table", "cell"])
def test_rtdetr_goldens_hold(dev, tag):
    from tests.test_rtdetr_gpu import GOLD, _net, assert_same_detections
    from yomitoku_amd.utils.synth_rtdetr import rtdetr_state_dict

    z = np.load(os.path.join(GOLD, f"rtdetr_ref_{tag}.npz"))
    seed, nc, size, nq = int(z["seed"]), int(z["num_classes"]), int(z["size"]), int(z["num_queries"])
    sd = rtdetr_state_dict(seed, num_classes=nc, eval_size=(size, size), enc_score_gain=1.0 if size == 640 else 12.0)
    net = _net(dev, sd, nc, size, nq)
    net.set_workspace_reuse(True)
    s0 = _stats()["workspace_planned_forwards"]
    x = torch.rand(1, 3, size, size, generator=torch.Generator().manual_seed(int(z["x_seed"])))
    out = net(x.to(dev))
    assert _stats()["workspace_planned_forwards"] == s0 + 1
    assert_same_detections(out["pred_logits"].cpu().numpy(), out["pred_boxes"].cpu().numpy(), z["logits"], z["boxes"])
    net.close()


@pytest.mark.parametrize("tag", ["eos", "rep"])
def test_parseq_goldens_hold(dev, tag):
    from tests.test_parseq_gpu import GOLD, LOGIT_TOL, _net
    from yomitoku_amd.utils.synth import parseq_state_dict

    z = np.load(os.path.join(GOLD, f"parseq_ref_{tag}.npz"))
    _, net = _net(dev, parseq_state_dict(**ast.literal_eval(str(z["ckpt"]))))
    net.set_workspace_reuse(True)
    s0 = _stats()["workspace_planned_forwards"]
    lg = net(torch.from_numpy(z["x"]).to(dev)).cpu()
    assert _stats()["workspace_planned_forwards"] == s0 + 1
    assert net.last_ar_steps == int(z["steps"])
    assert lg.shape[:2] == z["ids"].shape
    assert np.array_equal(lg.argmax(-1).numpy().astype(np.int32), z["ids"])
    assert np.abs(lg.max(-1).values.numpy() - z["top"]).max() < LOGIT_TOL
    assert np.abs(lg[:, :, ::97].numpy() - z["sample"]).max() < LOGIT_TOL
    net.close()


def test_parseq_nar_goldens_hold(dev):
    from tests.test_parseq_nar_gpu import TAGS, _check_against_golden, _gold, _net

    z = _gold()
    for tag in TAGS:
        net = _net(dev, z, tag)
        net.set_workspace_reuse(True)
        s0 = _stats()["workspace_planned_forwards"]
        logits = net(torch.from_numpy(z["x"]).to(dev))
        assert _stats()["workspace_planned_forwards"] == s0 + 1
        assert logits.shape[1] == 101 and net.last_ar_steps == 0
        _check_against_golden(z, tag, logits.cpu())
        net.close()


# ---------------------------------------------------------------------------------------------------------------- contract
def test_serve_job_keeps_the_forward_contract(dev):
    """DocumentAnalyzer(workspace_reuse=True).serve over pages with tables (two table boxes per page handed to the table
    stage, so that its forwards run whatever the seeded layout net detects): the results of the default analyzer, the four
    "in_forward" counters untouched, planned forwards counted - and none counted for the default analyzer."""
    from tests.test_pipeline_gpu import _assert_same_schema
    from tests.test_serving_gpu import _analyzer
    from yomitoku_amd import _lib
    from yomitoku_amd.testing import Handover
    from yomitoku_amd.utils.synth import synthetic_page_with_truth

    class Tables(Handover):
        crops = 0

        def table_boxes(self, wave, boxes):
            Tables.crops += 2 * len(boxes)
            return [[[80, 90, 620, 500], [300, 520, 900, 880]] for _ in boxes]

    shapes = [(1000, 1400), (1400, 1000), (1200, 1600), (1000, 1400), (1400, 1000)]
    imgs = [synthetic_page_with_truth(3 + i, h, w)[0] for i, (h, w) in enumerate(shapes)]

    s0 = _stats()["workspace_planned_forwards"]
    an = _analyzer()
    an.handover = Tables()
    want = an.serve(imgs, wave=3, in_flight=2)
    assert not any(isinstance(o, Exception) for o in want), want
    assert Tables.crops == 2 * len(imgs), "the table stage did not see every page"
    assert _stats()["workspace_planned_forwards"] == s0, "the default analyzer ran planned forwards"
    held_default = [n.workspace_bytes for n in (an.text_detector.model, an.text_recognizer.model, an.layout.layout_parser.model,
                                                an.layout.table_structure_recognizer.model)]
    want = [r.model_dump() for r in want]
    an.close()

    before = {k: _lib.stat(k) for k in COUNTERS}
    an = _analyzer(workspace_reuse=True)
    an.handover = Tables()
    nets = (an.text_detector.model, an.text_recognizer.model, an.layout.layout_parser.model, an.layout.table_structure_recognizer.model)
    assert all(n._workspace_reuse is True for n in nets)
    got = an.serve(imgs, wave=3, in_flight=2)
    assert not any(isinstance(o, Exception) for o in got), got
    assert an.text_recognizer._replicas.get(1) is not None and an.text_recognizer._replicas[1]._workspace_reuse is True
    again = an.serve(imgs[::-1], wave=3, in_flight=2)  # other waves, other shapes: re-planned on the host inside the reservations
    after = {k: _lib.stat(k) for k in COUNTERS}
    assert after == before, {k: after[k] - before[k] for k in COUNTERS}
    assert _stats()["workspace_planned_forwards"] > s0
    for w, g in zip(want, got):
        _assert_same_schema(w, g.model_dump(), score_rtol=0.0)
    for w, g in zip(want[::-1], again):
        _assert_same_schema(w, g.model_dump(), score_rtol=0.0)
    held = [n.workspace_bytes for n in nets]
    print("workspace bytes per net, default analyzer:", held_default, "planned:", held)
    assert all(0 < p < d for p, d in zip(held, held_default))
    an.close()
