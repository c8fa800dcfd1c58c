"""PARSeq "retire_rows" (include/ymk.h): a row leaves the greedy loop after the step whose raw arg-max is its own <eos>.

With the switch on, token ids up to and including each row's first <eos>, the score over them and the step counts are what
they are with it off; logits behind a row's first <eos> may differ (no repetition cut there, last bits of the refinement's
fp16-plane products).  A row that only the repetition detector stopped is not retired.  Checked on whole forwards (grouped,
switch on against off; the repetition-stopped rows of tests/golden/parseq_ref_rep.npz against the oracle), on the three kernels
one launch at a time (k_greedy_step, k_parseq_dec_step_rows, the row-max vocabulary head) and through TextRecognizer."""
import ast
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle.parseq import detect_repeat_onset
from tests import hipops
from tests.test_parseq_decstep_gpu import GUARD, SENT, Case, _same_bits
from tests.test_parseq_gpu import LOGIT_TOL
from yomitoku_amd import _lib

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
COUNTERS = ("allocs_in_forward", "arena_grows_in_forward", "lazy_panel_builds", "syncs_in_forward")


@pytest.fixture(autouse=True)
def _reset_dec_rows():
    yield
    _lib.debug_option("dec_rows", 0)


def _net(dev, sd, retire, **cfg_over):
    from oracle.parseq import PRESETS, make_cfg
    from yomitoku_amd.nets import PARSeq

    ocfg = make_cfg(**{**PRESETS["parseq-tiny-dynw-v4"], **cfg_over})
    cfg = {
        "num_tokens": ocfg.num_tokens, "max_label_length": ocfg.max_label_length, "refine_iters": ocfg.refine_iters,
        "decode_ar": 1, "retire_rows": retire, "repetition_stop": ocfg.repetition_stop, "data": {"img_size": [32, 800]},
        "encoder": {"patch_size": list(ocfg.patch), "num_heads": ocfg.enc_heads, "embed_dim": ocfg.enc_dim,
                    "mlp_ratio": 4, "depth": ocfg.enc_depth},
        "decoder": {"embed_dim": ocfg.dec_dim, "num_heads": ocfg.dec_heads, "mlp_ratio": 4, "depth": 1},
    }
    net = PARSeq(cfg).load_state_dict(sd).to(dev)
    assert net.params()["retire_rows"] == retire
    return ocfg, net


def _first_eos(ids_row):
    """index of the first <eos> (id 0) of a row of token ids, or its last index when it holds none"""
    hit = (ids_row == 0).nonzero()
    return int(hit[0]) if hit.numel() else ids_row.numel() - 1


# ------------------------------------------------------------------------------------------- whole forwards: switch on against off
SHAPES = [(7, 160), (3, 800), (9, 72), (1, 96), (6, 320), (5, 64)]


def test_grouped_forward_switch_on_against_off(dev):
    """Six mini-batches in one greedy loop, two nets.  Step counts and valid rows are equal; ids are equal up to and including
    each row's first <eos>, probabilities there within LOGIT_TOL (the bound the PARSeq forward has against the oracle); a
    repeat with the switch on is bit-identical.  On the CPU oracle these batches stop after 7, 7, 58, 17, 12 and 7 steps while
    e.g. seven of the nine rows of the third emit their <eos> by step 13: rows retire long before their mini-batch closes."""
    from yomitoku_amd.nets import PARSeq
    from yomitoku_amd.utils.synth import parseq_state_dict, synthetic_line_batch

    sd = parseq_state_dict(1235, eos_bias=5.5)
    xs = [synthetic_line_batch(23 + i, b, w).to(dev) for i, (b, w) in enumerate(SHAPES)]
    _, off = _net(dev, sd, 0)
    _, on = _net(dev, sd, 1)
    lg_off, len_off, st_off = off.forward_groups(xs)
    lg_on, len_on, st_on = on.forward_groups(xs)
    assert list(st_on) == list(st_off) and list(len_on) == list(len_off)
    ids_off, p_off = (t.cpu() for t in PARSeq.token_stats(lg_off))
    ids_on, p_on = (t.cpu() for t in PARSeq.token_stats(lg_on))
    early, row, worst = 0, 0, 0.0
    for (b, _), st in zip(SHAPES, st_off):
        for r in range(row, row + b):
            e = _first_eos(ids_off[r])
            early += int(e + 1 + 3 <= st)  # the row's own <eos> is out at least three steps before its mini-batch stops
            assert torch.equal(ids_on[r, :e + 1], ids_off[r, :e + 1]), f"row {r}: ids differ at or before the first <eos> ({e})"
            worst = max(worst, (p_on[r, :e + 1] - p_off[r, :e + 1]).abs().max().item())
        row += b
    behind = int((ids_on != ids_off).sum())
    print(f"retire on/off: steps {list(st_off)}, rows retired >= 3 steps early: {early}, worst |dp| up to <eos>: {worst:.3e}, "
          f"ids that differ behind an <eos>: {behind}")
    assert early >= 1, "no row retires early: these batches prove nothing"
    assert worst < LOGIT_TOL
    again, _, _ = on.forward_groups(xs)
    assert torch.equal(again.cpu(), lg_on.cpu()), "the forward with retired rows must be bit-identical on repeat"
    off.close()
    on.close()


def test_repetition_stopped_rows_are_not_retired(dev):
    """tests/golden/parseq_ref_rep.npz as one mini-batch of three rows, all stopped by the repetition detector (no arg-max
    <eos> at all), two of them two steps before the third: they hold <eos> in `tok` but keep running, and their later
    arg-maxes are unmasked context of the refinement.  Next to a longer mini-batch, with the switch on, every logit within
    out_len equals the oracle's (LOGIT_TOL, same arg-max) - which it does not if has_eos were the retirement condition: the
    two rows would then show <eos> in `raw` from their stop on and the refinement would mask those keys."""
    from oracle.parseq import PRESETS, make_cfg, parseq_forward
    from yomitoku_amd.utils.synth import parseq_state_dict, synthetic_line_batch

    z = np.load(os.path.join(GOLD, "parseq_ref_rep.npz"))
    sd = parseq_state_dict(**ast.literal_eval(str(z["ckpt"])))
    ocfg, net = _net(dev, sd, 1)
    xa = torch.from_numpy(z["x"])
    # the premise, from the oracle's greedy loop alone (detector off, so that the logits carry no cut row): within the steps
    # the batch runs no row's arg-max is <eos>, every row trips the detector, and some row does so before the last step
    ar_steps = int(z["steps"])
    free = make_cfg(**{**PRESETS["parseq-tiny-dynw-v4"], "refine_iters": 0, "repetition_stop": False})
    raw = parseq_forward(sd, free, xa).argmax(-1)[:, :ar_steps]
    assert not bool((raw == 0).any())
    stops = [min(j for j in range(1, ar_steps + 1) if detect_repeat_onset(r[:j], ocfg.rep_period_max, ocfg.rep_min_run_p1,
                                                                          ocfg.rep_min_repeats) is not None)
             for r in raw.tolist()]
    assert min(stops) < max(stops) == ar_steps, stops
    cands = [synthetic_line_batch(40 + i, 1, w) for i, w in enumerate((96, 240, 480, 800))]
    steps = []
    for c in cands:
        net(c.to(dev))
        steps.append(net.last_ar_steps)
    xb = cands[int(np.argmax(steps))]
    assert ar_steps < max(steps) < 101, steps
    xs = [xa, xb]
    logits, out_lens, got_steps = net.forward_groups([x.to(dev) for x in xs])
    assert list(got_steps) == [ar_steps, max(steps)]
    lg, row = logits.cpu(), 0
    for k, x in enumerate(xs):
        ref, ref_steps = parseq_forward(sd, ocfg, x, return_steps=True)
        got = lg[row:row + x.shape[0], :out_lens[k]]
        assert ref_steps == got_steps[k] and got.shape == ref.shape
        err = (got - ref).abs().max().item()
        print(f"retire on, group {k}: {ref_steps} steps, max|dlogit| vs the oracle {err:.3e}")
        assert torch.equal(got.argmax(-1), ref.argmax(-1)) and err < LOGIT_TOL
        row += x.shape[0]
    net.close()


# ------------------------------------------------------------------------------------------------------- k_greedy_step, one launch
EOS, VOCAB = 0, 400
BOS, PAD = VOCAB, VOCAB + 1
REP = (1, 8, 8, 3)
NUM_STEPS = 26


def _fill(seq, n, base):
    """seq continued to n tokens with tokens that occur nowhere else"""
    return list(seq) + [base + i for i in range(n - len(seq))]


SEQS = {
    # arg-max <eos> at step 2, then a run that trips the detector (it stays armed behind an <eos>)
    "eos_then_run": _fill([5, 6, EOS] + [1] * 9, NUM_STEPS, 100),
    # only the detector stops it (period 2, three units, complete at step 5); the arg-max is never <eos>
    "rep_only": _fill([1, 2] * 3, NUM_STEPS, 140),
    "never_done": _fill([], NUM_STEPS, 180),
    # the detector stops it at step 5, the arg-max turns <eos> at step 8
    "rep_then_eos": _fill([3, 4] * 3 + [50, 51, EOS], NUM_STEPS, 220),
    "eos_first": _fill([EOS], NUM_STEPS, 260),
}


def _greedy_step(logits, step, tok, raw, state, not_done, retire, prev_not_done=None, gid=None, gopen=None, ng=1):
    lib = _lib.load()
    with torch.cuda.device(tok.device):
        _lib.check(lib.ymk_op_greedy_step_retire(logits.data_ptr(), logits.shape[1], VOCAB, step, NUM_STEPS, tok.data_ptr(),
                                                 raw.data_ptr(), tok.shape[1], state.data_ptr(), EOS, *REP, not_done.data_ptr(),
                                                 _lib.ptr(prev_not_done), _lib.ptr(gid), _lib.ptr(gopen), ng, 0, retire,
                                                 tok.shape[0], _lib.current_stream_ptr()), "ymk_op_greedy_step_retire")


def _simulate(seqs, retire, gid, ng, ld_tok):
    """The reference's loop row by row (oracle/parseq.py: parseq_forward) with the grouped forward's freezing and the retired
    rows; yields (tok, raw, state, not_done, gopen) after every step."""
    rep_on, pmax, p1, mr = REP
    B = len(seqs)
    tok = [[BOS] + [PAD] * (ld_tok - 1) for _ in range(B)]
    raw = [[77] * ld_tok for _ in range(B)]
    state = [[0, 0, -1, 0] for _ in range(B)]
    not_done = [0] * NUM_STEPS
    gopen = [[0] * ng for _ in range(NUM_STEPS)]
    for step in range(NUM_STEPS):
        if step > 0 and not_done[step - 1] == 0:
            yield tok, raw, state, not_done, gopen
            continue
        for b in range(B):
            g = gid[b] if gid is not None else 0
            st = state[b]
            if (gid is not None and step > 0 and gopen[step - 1][g] == 0) or (retire and st[3]):
                raw[b][step] = EOS
                continue
            am = seqs[b][step]
            raw[b][step] = am
            if retire and am == EOS:
                st[3] = 1
            j = step + 1
            if j < NUM_STEPS:
                tok[b][j] = am
                if rep_on and not st[1] and am != EOS:
                    hit = detect_repeat_onset(tok[b][1:j + 1], pmax, p1, mr)
                    if hit is not None:
                        st[2], st[1] = hit[0] + hit[1], 1
                        tok[b][j] = EOS
                if tok[b][j] == EOS:
                    st[0] = 1
            if not st[0]:
                not_done[step] = 1
                if gid is not None:
                    gopen[step][g] = 1
        yield tok, raw, state, not_done, gopen


def _drive(dev, names, retire, gid=None, ng=1):
    seqs = [SEQS[n] for n in names]
    B, ld_tok = len(seqs), NUM_STEPS + 3
    tok, state = hipops.init_decode(B, ld_tok, BOS, PAD, dev)
    raw = torch.full((B, ld_tok), 77, dtype=torch.int32, device=dev)
    not_done = torch.zeros(NUM_STEPS, dtype=torch.int32, device=dev)
    gopen = torch.zeros(NUM_STEPS, ng, dtype=torch.int32, device=dev)
    gid_d = None if gid is None else torch.tensor(gid, dtype=torch.int32, device=dev)
    idx = torch.tensor(seqs, dtype=torch.int64, device=dev)
    logits = torch.empty(B, VOCAB, device=dev)
    last = None
    for step, want in enumerate(_simulate(seqs, retire, gid, ng, ld_tok)):
        logits.fill_(-1.0)
        logits.scatter_(1, idx[:, step:step + 1], 5.0)
        _greedy_step(logits, step, tok, raw, state, not_done[step:step + 1], retire,
                     prev_not_done=not_done[step - 1:step] if step > 0 else None, gid=gid_d,
                     gopen=gopen if gid is not None else None, ng=ng)
        got = (tok.cpu().tolist(), raw.cpu().tolist(), state.cpu().tolist(), not_done.cpu().tolist(), gopen.cpu().tolist())
        for name, a, b in zip(("tok", "raw", "state", "not_done", "gopen"), got, want):
            assert a == b, f"retire {retire}, step {step}: {name} differs: got {a} want {b}"
        last = want
    return last


def test_greedy_step_retires_on_the_raw_arg_max_only(dev):
    """Every buffer after every step against the restatement, switch off and on.  On: the row whose arg-max is <eos> at step 2
    gets raw = <eos> from step 3, and tok, the detector's words and the cut stay put although the later arg-maxes form a run.
    Off: they advance and the detector fires behind the <eos> (the documented difference).  The row only the detector stops
    keeps advancing in both modes, until its arg-max itself is <eos>."""
    names = list(SEQS)
    i = {n: names.index(n) for n in names}
    tok0, raw0, st0, nd0, _ = _drive(dev, names, 0)
    tok1, raw1, st1, nd1, _ = _drive(dev, names, 1)
    assert nd0 == nd1  # the open-row words: a retired row held an <eos> before, it never voted anyway
    r = i["eos_then_run"]
    assert st1[r] == [1, 0, -1, 1] and raw1[r][3:NUM_STEPS] == [EOS] * (NUM_STEPS - 3) and tok1[r][4:NUM_STEPS] == [PAD] * (NUM_STEPS - 4)
    # off: six of the 1s are three units of (1, 1) - the detector fires at step 8 with the cut behind the <eos>
    assert st0[r] == [1, 1, 5, 0] and raw0[r][3:12] == [1] * 9 and tok0[r][4:10] == [1] * 5 + [EOS]
    r = i["rep_only"]
    assert st0[r] == st1[r] == [1, 1, 2, 0] and raw0[r] == raw1[r] and tok0[r] == tok1[r]
    assert raw1[r][:NUM_STEPS] == SEQS["rep_only"] and tok1[r][6] == EOS and tok1[r][7:NUM_STEPS] == SEQS["rep_only"][6:NUM_STEPS - 1]
    r = i["rep_then_eos"]
    assert st1[r] == [1, 1, 2, 1] and st0[r] == [1, 1, 2, 0]
    assert raw1[r][:9] == raw0[r][:9] == SEQS["rep_then_eos"][:9] and raw1[r][9:NUM_STEPS] == [EOS] * (NUM_STEPS - 9)
    assert raw0[r][9:NUM_STEPS] == SEQS["rep_then_eos"][9:]
    assert st1[i["eos_first"]] == [1, 0, -1, 1] and st1[i["never_done"]] == [0, 0, -1, 0]


def test_greedy_step_group_rule_still_freezes_rows_that_are_not_retired(dev):
    """Two mini-batches: the second holds the two detector-stopped rows and closes after step 5; from step 6 on its rows are
    frozen by the group rule in both modes, although neither has been retired."""
    names = ["eos_then_run", "never_done", "rep_only", "rep_then_eos"]
    for retire in (0, 1):
        tok, raw, st, _, gopen = _drive(dev, names, retire, gid=[0, 0, 1, 1], ng=2)
        assert [gopen[s][1] for s in range(7)] == [1, 1, 1, 1, 1, 0, 0] and gopen[NUM_STEPS - 1][0] == 1
        for r in (2, 3):
            assert st[r] == [1, 1, 2, 0] and raw[r][6:NUM_STEPS] == [EOS] * (NUM_STEPS - 6)


# ------------------------------------------------------------------------------------------- the decoder step with retired rows
def _dec_step(case, dev, rows, state=None, gid=None, gopen=None, ng=1):
    """one launch of the fused step at `rows` samples per block -> (out_full, skv_full, skv_before) on the host"""
    lib = _lib.load()
    tok, skv, out, mem = case.buffers(dev)
    before = skv.cpu()
    w, B, NS, (D, H, Fd) = case.w, case.B, case.NS, case.geom
    host = [w[n].detach().float().cpu().contiguous() for n in hipops.DEC_STEP_WEIGHTS]
    norms = [w[f"{n}.{k}"].detach().float().cpu().contiguous() for n in hipops.DEC_STEP_NORMS for k in ("weight", "bias")]
    ln = (ctypes.c_void_p * 10)(*[t.data_ptr() for t in norms])
    emb, posq, qs = (t.detach().float().cpu().contiguous() for t in (w["emb"], w["pos_queries"], case.qsa))
    dv = lambda t: None if t is None else t.to(dev)  # noqa: E731
    state_d, gid_d, gopen_d = dv(state), dv(gid), dv(gopen)
    assert int(tok[:, case.step].min()) >= 0 and int(tok[:, case.step].max()) < emb.shape[0] and mem.shape[0] >= B * case.L
    assert state is None or (state.dtype == torch.int32 and state.shape == (B, 4))
    assert gid is None or (gid.shape == (B,) and gopen.shape == (NS, ng) and 0 <= int(gid.min()) and int(gid.max()) < ng)
    _lib.debug_option("dec_rows", rows)
    with torch.cuda.device(dev):
        _lib.check(lib.ymk_op_parseq_dec_step_state(D, H, Fd, *[t.data_ptr() for t in host], ln, emb.data_ptr(), emb.shape[0],
                                                    posq.data_ptr(), qs.data_ptr(), tok.data_ptr(), skv[:B].data_ptr(), mem.data_ptr(),
                                                    None, None, None, _lib.ptr(gid_d), _lib.ptr(gopen_d), ng, _lib.ptr(state_d),
                                                    case.step, B, case.L, NS, out[:B].data_ptr(), _lib.current_stream_ptr()),
                   "ymk_op_parseq_dec_step_state")
    torch.cuda.synchronize()
    return out.cpu(), skv.cpu(), before


@pytest.mark.parametrize("geom", [(192, 6, 768), (64, 2, 128)], ids=str)
def test_dec_step_retired_rows_keep_their_slots_and_live_rows_their_bits(dev, geom):
    """Eleven rows, six retired (state[b][3] = 1; the other words of a row's state carry values the kernel must not look at):
    at 1, 2, 3 and 4 rows per block there are blocks of retired rows only, mixed blocks and a short last block.  A retired
    row's `out` and cache row keep the sentinel bit for bit, a live row equals the launch without a state bit for bit.  Then
    with a closed mini-batch on top: a row is live when its mini-batch is open AND it is not retired."""
    B, NS, step, ng = 11, 26, 6, 3
    case = Case(geom, NS, step, L=16, B=B)
    retired = torch.zeros(B, dtype=torch.bool)
    retired[[0, 1, 2, 3, 5, 10]] = True
    state = torch.tensor([[1, b % 2, b - 1, int(retired[b])] for b in range(B)], dtype=torch.int32)
    gid = torch.tensor([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2], dtype=torch.int32)
    gopen = torch.ones(NS, ng, dtype=torch.int32)
    gopen[step - 1, 2] = 0  # mini-batch 2 (rows 8, 9, 10) closed at the previous step; rows 8 and 9 are not retired
    gopen[step, :] = 0
    for rows in (1, 2, 3, 4):
        plain_out, plain_skv, _ = _dec_step(case, dev, rows)
        for live, kw in ((~retired, {}), (~retired & (gid != 2), dict(gid=gid, gopen=gopen, ng=ng))):
            out, skv, before = _dec_step(case, dev, rows, state=state, **kw)
            assert _same_bits(out[:B][live], plain_out[:B][live]) and _same_bits(skv[:B][live], plain_skv[:B][live]), rows
            assert _same_bits(out[:B][~live], torch.full_like(out[:B][~live], SENT)), f"dec_rows {rows}: a dead row's out was written"
            assert _same_bits(skv[:B][~live], before[:B][~live]), f"dec_rows {rows}: a dead row's cache was written"
            assert _same_bits(out[B:], torch.full_like(out[B:], SENT)) and _same_bits(skv[B:], before[B:])
    assert GUARD >= 1
    # a state without a retired row changes nothing
    out, skv, _ = _dec_step(case, dev, 2, state=torch.tensor([[1, 1, 3, 0]] * B, dtype=torch.int32))
    plain_out, plain_skv, _ = _dec_step(case, dev, 2)
    assert _same_bits(out, plain_out) and _same_bits(skv, plain_skv)


# ------------------------------------------------------------------------------------------------- the row-max vocabulary head
HEAD_SENT = 0x7FA5A5A5  # a NaN bit pattern no kernel produces


def _rowmax_head(x, w, bias, split, pairs, row_group=None, group_open=None, state=None, amax_in=None):
    lib = _lib.load()
    M, K = x.shape
    wh, bh = w.float().cpu().contiguous(), bias.float().cpu().contiguous()
    dead = None if state is None else state.data_ptr() + 12  # word 3 of each row's four
    assert row_group is None or (row_group.numel() == M and 0 <= int(row_group.min()) and int(row_group.max()) < group_open.numel())
    assert state is None or (state.dtype == torch.int32 and state.shape == (M, 4) and state.is_contiguous())
    assert pairs.shape == (M, 2 * ((w.shape[0] + 63) // 64)) and pairs.is_contiguous()
    with torch.cuda.device(x.device):
        _lib.check(lib.ymk_op_rowmax_head(x.data_ptr(), M, K, wh.data_ptr(), w.shape[0], bh.data_ptr(), split, _lib.ptr(row_group),
                                          _lib.ptr(group_open), dead, 4, _lib.ptr(amax_in), pairs.data_ptr(),
                                          _lib.current_stream_ptr()), "ymk_op_rowmax_head")
    return pairs.cpu()


@pytest.mark.parametrize("form", ["fp32_64_row_tiles", "f16_astat_128_row_tiles"])
def test_rowmax_head_skips_tiles_of_dead_rows_only(dev, form):
    """The head's M tiles (64 rows in the exact fp32 kernel, which small forwards run; 128 in the A-stationary fp16 kernel, the
    one a wave's loop runs): a tile all of whose rows are retired or sit in a closed mini-batch keeps the sentinel, every
    other tile is written whole and equals the launch without a predicate bit for bit - with the retired words alone, and
    together with a closed mini-batch whose rows are not retired."""
    if form == "fp32_64_row_tiles":
        M, C, split, T = 230, 200, 0, 64
    else:
        M, C, split, T = 700, 7119, 16, 128
    K = 192
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, K, generator=g).to(dev)
    w = torch.randn(C, K, generator=g) / K ** 0.5
    bias = 0.1 * torch.randn(C, generator=g)
    amax = hipops.amax_record(float(x.abs().max()), dev) if split else None
    ntile = (M + T - 1) // T
    tile_of = torch.arange(M) // T
    fresh = lambda: torch.full((M, 2 * ((C + 63) // 64)), HEAD_SENT, dtype=torch.int32, device=dev).view(torch.float32)  # noqa: E731
    a0 = _lib.stat("astat_launches")
    plain = _rowmax_head(x, w, bias, split, fresh(), amax_in=amax).view(torch.int32)
    if split:
        assert _lib.stat("astat_launches") == a0 + 1, "this launch should take the A-stationary kernel (the loop's head at wave size)"
    assert not bool((plain == HEAD_SENT).any())
    # the arg-max the pairs encode is the arg-max of the product (lowest column among equal maxima)
    ref = (x.cpu().double() @ w.double().t() + bias.double())
    pv = plain.view(torch.float32).reshape(M, -1, 2)
    col = pv[:, :, 1].contiguous().view(torch.int32)
    best = pv[:, :, 0].argmax(dim=1)
    am = col[torch.arange(M), best].long()
    top2 = ref.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3  # rows whose winner no rounding can change
    assert torch.equal(am[clear], ref.argmax(dim=1)[clear])

    dead = torch.zeros(M, dtype=torch.bool)
    dead[tile_of == 0] = True                    # a tile of retired rows only
    dead[T:T + T // 2] = True                    # a mixed tile
    dead[tile_of == ntile - 1] = True            # the short last tile, all retired
    state = torch.tensor([[1, 0, -1, int(d)] for d in dead.tolist()], dtype=torch.int32, device=dev)
    group = (tile_of == ntile - 2).int()         # mini-batch 1 = the rows of the tile before the last: closed, none retired
    gopen = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    for with_group in (False, True):
        needed = ~dead & ((group == 0) if with_group else torch.ones(M, dtype=torch.bool))
        kw = dict(row_group=group.to(dev), group_open=gopen) if with_group else {}
        got = _rowmax_head(x, w, bias, split, fresh(), state=state, amax_in=amax, **kw).view(torch.int32)
        for tl in range(ntile):
            rows = tile_of == tl
            if bool(needed[rows].any()):
                assert torch.equal(got[rows], plain[rows]), f"tile {tl} (needed) differs from the launch without a predicate"
            else:
                assert bool((got[rows] == HEAD_SENT).all()), f"tile {tl} holds no needed row and was written"
        assert ntile >= 4 and not bool(needed[tile_of == 0].any()) and bool(needed[tile_of == 1].any())
        assert bool(needed[tile_of == ntile - 2].any()) != with_group


# ------------------------------------------------------------------------------------------------------------ the product's switch
def test_text_recognizer_retires_rows_by_default_with_the_same_results(dev):
    """TextRecognizer.__call__ on one synthetic sheet of 48 lines (the bench's recogniser checkpoint): the module turns the
    switch on unless told otherwise; contents are identical with it off, scores within LOGIT_TOL; no forward allocated, grew
    its workspace, built a weight copy or waited (ymk_stat)."""
    from yomitoku_amd import imaging
    from yomitoku_amd.text_recognizer import TextRecognizer
    from yomitoku_amd.utils.synth import parseq_state_dict, synthetic_line_sheet

    sd = parseq_state_dict(seed=1235, eos_bias=6.1)
    sheet, quads = synthetic_line_sheet(seed=5, n_lines=48)
    page = imaging.page_to_device(sheet, dev)
    before = {k: _lib.stat(k) for k in COUNTERS}
    res = {}
    for name, kw in (("on", {}), ("off", {"retire_rows": False})):
        rec = TextRecognizer(model_name="parseq-tiny-dynw-v4", from_pretrained=False, device=str(dev), dynamic_width=True,
                             batch_bucketing=True, **kw)
        rec.model.load_state_dict(sd)
        assert rec.model.params()["retire_rows"] == (1 if name == "on" else 0)
        res[name] = rec(page, quads)[0]
        rec.model.close()
    after = {k: _lib.stat(k) for k in COUNTERS}
    assert res["on"].contents == res["off"].contents and len(res["on"].contents) == 48
    assert len(set(res["on"].contents)) > 10  # the sheet decodes to many different strings
    d = np.abs(np.asarray(res["on"].scores) - np.asarray(res["off"].scores)).max()
    print(f"TextRecognizer retire on/off: max|dscore| = {d:.3e}")
    assert d < LOGIT_TOL
    assert after == before, {k: after[k] - before[k] for k in COUNTERS}
