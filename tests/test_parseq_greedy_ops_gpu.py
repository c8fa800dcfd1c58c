"""The bookkeeping kernels of PARSeq's greedy decode (yomitoku_amd/csrc/ymk_seq.hip) one launch at a time: the arg-max family
(k_row_argmax, k_row_maxprob, k_greedy_step on full rows and on (max, column) pairs), the greedy step driven as a loop against a
plain-Python restatement of the reference's loop (oracle/parseq.py: parseq_forward, detect_repeat_onset), k_refine_prep,
k_rep_cut, k_ctx_embed_ln, k_init_decode, k_tile_rows and k_add_pos.  Integer results are compared exactly; the two
floating-point results (the arg-max's probability, the context LayerNorm) against float64 with the tolerance
4 x max|fp32 CPU - fp64| of the same expression on the same case."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle.parseq import detect_repeat_onset
from tests import hipops
from yomitoku_amd import _lib

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")


# ------------------------------------------------------------------------------------------------------------ arg-max family
ARGMAX_C = (1, 2, 255, 256, 257, 513, 7121, 8192, 8193, 8449)  # the last two: rows too long for the register path


def _argmax_rows(C, g):
    """(rows [n, C] fp32, names): random rows and planted ties.  The expected index is torch.argmax on the CPU."""
    rows, names = [], []

    def add(name, r):
        rows.append(r.float())
        names.append(name)

    for i in range(32):
        add(f"random{i}", torch.randn(C, generator=g) * (1.0 + i % 5))
    base = lambda: torch.randn(C, generator=g).clamp_(-3, 3)  # noqa: E731
    r = base(); r[0] = 9.0; add("max_at_0", r)
    r = base(); r[C - 1] = 9.0; add("max_at_last", r)
    add("all_equal", torch.full((C,), 0.75))
    add("all_neg_inf", torch.full((C,), NEG_INF))
    r = torch.full((C,), NEG_INF); r[C - 1] = -5.0; add("one_finite_at_last", r)
    if C >= 2:
        r = -base().abs() - 1.0; r[C // 2] = -0.0; r[C - 1] = 0.0; add("neg_zero_then_pos_zero", r)
        r = -base().abs() - 1.0; r[C // 3] = 0.0; r[C - 1] = -0.0; add("pos_zero_then_neg_zero", r)
        r = base(); r[1] = 9.0; r[C - 1] = 9.0; add("tie_first_last", r)
        # rows as k_rep_cut writes them, and a spread of 200 (most terms of the softmax sum underflow to zero)
        r = torch.full((C,), -30.0); r[0] = 30.0; add("rep_cut_row", r)
        r = torch.full((C,), -30.0); r[C - 1] = 30.0; add("rep_cut_row_last", r)
        r = torch.full((C,), -100.0) + torch.rand(C, generator=g); r[C // 2] = 100.0; add("spread_200", r)
    if C > 256:
        c = min(7, C - 257)
        r = base(); r[c] = 9.0; r[c + 256] = 9.0; add("tie_within_a_threads_stripe", r)
        # thread 3 holds column 259, thread 5 column 5: the LDS tree meets the higher column in the lower slot
        if C > 259:
            r = base(); r[5] = 9.0; r[259] = 9.0; add("tie_across_threads_low_slot_high_column", r)
    if C >= 255:
        r = base(); r[200] = 9.0; r[100] = 9.0; r[254] = 9.0; add("tie_across_threads", r)
    return torch.stack(rows), names


@pytest.mark.parametrize("C", ARGMAX_C)
def test_argmax_family_agrees_with_torch(dev, C):
    """row_argmax, token_stats and greedy_step (full rows) return torch.argmax's index on every row - first maximal column, +0.0
    and -0.0 equal, 0 for a row of -inf - and token_stats' probability is 1 / sum(exp(x - max)) to 4 x the fp32 CPU error
    over the rows of a C, and per row to the relative rounding bound of its own chain of operations."""
    rows, names = _argmax_rows(C, torch.Generator().manual_seed(C))
    want = torch.argmax(rows, dim=1).to(torch.int32)
    x = rows.to(dev)
    n = rows.shape[0]
    bad = lambda got: [(names[i], int(got[i]), int(want[i])) for i in range(n) if int(got[i]) != int(want[i])]  # noqa: E731

    got = hipops.row_argmax(x).cpu()
    assert not bad(got), f"row_argmax (name, got, want): {bad(got)}"
    ids, probs = hipops.token_stats(x)
    ids, probs = ids.cpu(), probs.cpu()
    assert not bad(ids), f"token_stats (name, got, want): {bad(ids)}"

    tok = torch.full((n, 4), 77, dtype=torch.int32, device=dev)
    raw = torch.full((n, 4), 77, dtype=torch.int32, device=dev)
    state = torch.tensor([[0, 0, -1, 0]] * n, dtype=torch.int32, device=dev)
    not_done = torch.zeros(1, dtype=torch.int32, device=dev)
    hipops.greedy_step(x, C, 0, 4, tok, raw, state, not_done, eos_id=C + 5, rep=(0, 8, 8, 3))
    raw, tok = raw.cpu(), tok.cpu()
    assert not bad(raw[:, 0]), f"greedy_step raw (name, got, want): {bad(raw[:, 0])}"
    assert torch.equal(tok[:, 1], want) and torch.equal(raw[:, 1:], torch.full((n, 3), 77, dtype=torch.int32))

    fin = torch.tensor([not nm.startswith("all_neg_inf") for nm in names])  # (-inf) - (-inf): no probability to speak of
    x64 = rows[fin].double()
    p64 = 1.0 / torch.exp(x64 - x64.max(dim=1, keepdim=True).values).sum(dim=1)
    x32 = rows[fin]
    p32 = 1.0 / torch.exp(x32 - x32.max(dim=1, keepdim=True).values).sum(dim=1)
    e32 = (p32.double() - p64).abs().max().item()
    err = (probs[fin].double() - p64).abs().max().item()
    print(f"token_stats C={C}: gpu_err={err:.3e} e32={e32:.3e}")
    assert torch.isfinite(probs[fin]).all()
    assert err <= 4 * e32, f"probability: {err:.3e} > 4 * {e32:.3e}"
    # The absolute bound above is set by the rows with p near 1; the long flat rows (p ~ 1 / C) need a bound of their own.
    # Per row, relative, from the arithmetic alone: x - max (one rounding), expf (1 ulp), a thread's chain of ceil(C / 256)
    # additions of positive terms, the 8 levels of the LDS tree, the division - each at most one ulp (2^-23) of the result.
    rel = ((probs[fin].double() - p64).abs() / p64).max().item()
    bound = (math.ceil(C / 256) + 8 + 3) * 2.0 ** -23
    print(f"token_stats C={C}: worst relative error {rel:.3e}, bound {bound:.3e}")
    assert rel <= bound, f"probability, relative: {rel:.3e} > {bound:.3e}"


@pytest.mark.parametrize("order", ["tile_order", "shuffled"])
@pytest.mark.parametrize("C", [1, 2, 112, 255, 256])
def test_greedy_step_on_partial_pairs(dev, C, order):
    """partials = 1: C (max, column-as-int-bits) pairs per row, one per 64-column tile of the vocabulary head.  The result is the
    arg-max of the expanded row: equal maxima resolve to the lowest COLUMN, wherever its pair sits."""
    g = torch.Generator().manual_seed(100 + C)
    T = 64
    rows = [torch.randn(C * T, generator=g) for _ in range(8)]
    rows.append(torch.full((C * T,), 0.5))
    rows.append(torch.full((C * T,), NEG_INF))
    r = torch.randn(C * T, generator=g).clamp_(-3, 3); r[C * T - 1] = 9.0; rows.append(r)
    if C >= 2:
        r = torch.randn(C * T, generator=g).clamp_(-3, 3); r[T + 3] = 9.0; r[(C - 1) * T + 1] = 9.0; r[(C - 1) * T + 9] = 9.0; rows.append(r)
        r = -torch.rand(C * T, generator=g) - 1.0; r[(C // 2) * T + 5] = -0.0; r[(C - 1) * T + 2] = 0.0; rows.append(r)
    rows = torch.stack(rows).float()
    n = rows.shape[0]
    want = torch.argmax(rows, dim=1).to(torch.int32)
    tiles = rows.reshape(n, C, T)
    mx = tiles.max(dim=2).values
    col = (torch.argmax(tiles, dim=2) + T * torch.arange(C)[None, :]).to(torch.int32)
    if order == "shuffled":
        perm = torch.randperm(C, generator=g)
        mx, col = mx[:, perm], col[:, perm]
    pairs = torch.stack([mx.contiguous().view(torch.int32), col], dim=2).contiguous().view(torch.float32).reshape(n, 2 * C)
    tok = torch.full((n, 4), 77, dtype=torch.int32, device=dev)
    raw = torch.full((n, 4), 77, dtype=torch.int32, device=dev)
    state = torch.tensor([[0, 0, -1, 0]] * n, dtype=torch.int32, device=dev)
    not_done = torch.zeros(1, dtype=torch.int32, device=dev)
    hipops.greedy_step(pairs.to(dev), C, 0, 4, tok, raw, state, not_done, eos_id=C * T + 5, rep=(0, 8, 8, 3), partials=1)
    assert torch.equal(raw.cpu()[:, 0], want), (raw.cpu()[:, 0].tolist(), want.tolist())
    assert torch.equal(tok.cpu()[:, 1], want)


# ------------------------------------------------------------------------------------------------------ the greedy step as a loop
EOS, VOCAB = 0, 400  # one-hot rows of 400 logits: two columns per thread of the reduction
BOS, PAD = VOCAB, VOCAB + 1
FILL0 = 40  # filler tokens FILL0, FILL0 + 1, ...: all different, so they never repeat


def _fill(seq, n):
    """seq continued to n tokens with tokens that occur nowhere else."""
    return list(seq) + [FILL0 + i for i in range(n - len(seq))]


def _sequences(num_steps, pmax, p1, mr):
    """name -> the arg-max a row produces at steps 0 .. num_steps - 1, and name -> the (fired, cut) the detector must reach for
    the rows whose outcome is plain to see (units of distinct tokens)."""
    seqs, expect = {}, {}
    for p in range(1, 9):
        thr = p1 if p == 1 else mr
        unit = list(range(1, p + 1))
        short = (unit * (thr - 1) + [30])[:num_steps]  # one unit short of the threshold, then something else
        seqs[f"p{p}_short"] = _fill(short, num_steps)
        if p * thr < num_steps:
            seqs[f"p{p}_at"] = (unit * num_steps)[:num_steps]  # reaches the threshold, then goes on repeating (the row is rep_done)
            if p >= 2:
                expect[f"p{p}_at"] = (p <= pmax, p)
                expect[f"p{p}_short"] = (False, -1)
    seqs["equal_pairs"] = _fill([7] * 12, num_steps)          # a run of one token: period 1 against period 2 on the unit (7, 7)
    seqs["equal_pairs_short"] = _fill([7, 7, 7, 31, 7, 7], num_steps)
    pre = [21, 22, 23, 24, 25]
    seqs["prefix_then_p3"] = _fill(pre + [1, 2, 3] * mr, num_steps)
    expect["prefix_then_p3"] = (3 <= pmax and len(pre) + 3 * mr < num_steps, len(pre) + 3)
    seqs["eos_early"] = _fill([5, 6, EOS, 1, 1, 1, 1, 1, 1, 1, 1, 1], num_steps)   # <eos>, then a run: the detector stays armed
    seqs["eos_run"] = _fill([5] + [EOS] * 10, num_steps)                        # a run of <eos> is no repetition
    seqs["eos_first"] = _fill([EOS], num_steps)
    seqs["never_done"] = _fill([], num_steps)
    seqs["repeat_at_the_end"] = _fill([], num_steps - 2 * mr) + [9, 10] * mr    # completes at the last step: nothing left to write
    return seqs, expect


def _simulate(seqs, num_steps, rep, gid, ng, ld_tok):
    """The reference's loop (oracle/parseq.py: parseq_forward) row by row, with the grouped forward's freezing; yields the
    buffers after every step: (tok, raw, state, not_done, gopen) as nested lists."""
    rep_on, pmax, p1, mr = rep
    B = len(seqs)
    tok = [[BOS] + [PAD] * (ld_tok - 1) for _ in range(B)]
    raw = [[77] * ld_tok for _ in range(B)]
    state = [[0, 0, -1, 0] for _ in range(B)]
    not_done = [0] * num_steps
    gopen = [[0] * ng for _ in range(num_steps)]
    for step in range(num_steps):
        if step > 0 and not_done[step - 1] == 0:  # every row holds an <eos>: a speculative step changes nothing
            yield tok, raw, state, not_done, gopen
            continue
        for b in range(B):
            g = gid[b] if gid is not None else 0
            if gid is not None and step > 0 and gopen[step - 1][g] == 0:  # the row's own loop has stopped
                raw[b][step] = EOS
                continue
            st = state[b]
            am = seqs[b][step]
            raw[b][step] = am
            j = step + 1
            if j < num_steps:
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


def _drive(dev, seqs, num_steps, rep, gid=None, ng=1):
    """Runs the kernel step by step on one-hot logits and compares every buffer with the restatement after every step.
    Returns the final (tok, raw, state) of the restatement."""
    B = len(seqs)
    ld_tok = num_steps + 3  # three columns behind the row: the last step must write nothing there
    tok, state = hipops.init_decode(B, ld_tok, BOS, PAD, dev)
    raw = torch.full((B, ld_tok), 77, dtype=torch.int32, device=dev)
    not_done = torch.zeros(num_steps, dtype=torch.int32, device=dev)
    gopen = torch.zeros(num_steps, ng, dtype=torch.int32, device=dev)
    gid_d = None if gid is None else torch.tensor(gid, dtype=torch.int32, device=dev)
    idx = torch.tensor(seqs, dtype=torch.int64, device=dev)  # [B, num_steps]
    logits = torch.empty(B, VOCAB, device=dev)
    last = None
    for step, want in enumerate(_simulate(seqs, num_steps, rep, gid, ng, ld_tok)):
        logits.fill_(-1.0)
        logits.scatter_(1, idx[:, step:step + 1], 5.0)
        hipops.greedy_step(logits, VOCAB, step, num_steps, tok, raw, state, not_done[step:step + 1], eos_id=EOS, rep=rep,
                           prev_not_done=not_done[step - 1:step] if step > 0 else None, gid=gid_d,
                           gopen=gopen if gid is not None else None, ng=ng)
        got = (tok.cpu().tolist(), raw.cpu().tolist(), state.cpu().tolist(), not_done.cpu().tolist(), gopen.cpu().tolist())
        for name, a, b in zip(("tok", "raw", "state", "not_done", "gopen"), got, want):
            if a != b:
                rows = [i for i in range(len(a)) if a[i] != b[i]]
                raise AssertionError(f"step {step}: {name} differs in rows {rows[:5]}: got {[a[i] for i in rows[:2]]} want {[b[i] for i in rows[:2]]}")
        last = want
    return last


REP_CONFIGS = {"default": (1, 8, 8, 3), "alt": (1, 4, 5, 2), "off": (0, 8, 8, 3)}


@pytest.mark.parametrize("num_steps", [26, 101, 256, 300])
@pytest.mark.parametrize("config", list(REP_CONFIGS))
def test_greedy_loop_matches_the_reference_loop(dev, num_steps, config):
    """Tokens, raw arg-maxes, {has_eos, rep_done, rep_cut} and the open-row word after EVERY step, for runs one short of and
    exactly at the detector's threshold at every period, at both threshold sets; num_steps <= 256 walks the row in LDS, 300 in
    global memory."""
    rep = REP_CONFIGS[config]
    seqs, expect = _sequences(num_steps, *rep[1:])
    names = list(seqs)
    tok, raw, state, _, _ = _drive(dev, [seqs[n] for n in names], num_steps, rep)
    # the restatement itself reaches what the sequences were built for
    for name, (fired, cut) in expect.items():
        st = state[names.index(name)]
        assert (st[1], st[2]) == ((1, cut) if fired and rep[0] else (0, -1)), (name, st)
    assert state[names.index("never_done")][0] == 0


@pytest.mark.parametrize("num_steps", [26, 300])
def test_greedy_loop_grouped_rows_freeze(dev, num_steps):
    """Three mini-batches in one loop; the rows of the middle one all reach an <eos> early: from the next step on they get raw =
    <eos> and nothing else of theirs moves, while live rows set their own group's word only."""
    rep = REP_CONFIGS["default"]
    seqs, _ = _sequences(num_steps, *rep[1:])
    order = [("never_done", 0), ("p2_at", 0), ("eos_early", 1), ("eos_first", 1), ("p3_at", 1), ("p1_short", 2), ("eos_run", 2),
             ("equal_pairs", 1), ("prefix_then_p3", 2)]
    tok, raw, state, not_done, gopen = _drive(dev, [seqs[n] for n, _ in order], num_steps, rep, gid=[g for _, g in order], ng=3)
    closed = [s for s in range(num_steps) if gopen[s][1] == 0]
    assert closed and closed[0] < 12 and gopen[num_steps - 1][0] == 1  # group 1 closed early, group 0 never
    assert raw[2][closed[0] + 1:num_steps] == [EOS] * (num_steps - closed[0] - 1)


def test_speculative_greedy_steps_change_nothing(dev):
    """Every row holds an <eos> after step 3: the steps issued behind it (prev_not_done -> 0) leave every buffer as it was."""
    num_steps = 26
    seqs = [_fill([1, 2, EOS], num_steps), _fill([EOS], num_steps), _fill([4, 4, 4, EOS], num_steps)]
    tok, raw, state, not_done, _ = _drive(dev, seqs, num_steps, REP_CONFIGS["default"])
    assert not_done[:5] == [1, 1, 1, 0, 0] and all(r[4:num_steps] == [77] * (num_steps - 4) for r in raw)


# ---------------------------------------------------------------------------------------------------------------- refine_prep
@pytest.mark.parametrize("B", [1, 63, 64, 65])
@pytest.mark.parametrize("S", [1, 2, 26, 101])
def test_refine_prep(dev, S, B):
    g = torch.Generator().manual_seed(S * 100 + B)
    bos, eos, ld = 500, 0, S + 3
    raw = torch.randint(1, 400, (B, ld), generator=g, dtype=torch.int32)
    for b in range(B):  # no <eos> | first | last position the kernel reads | two | random
        kind = b % 5
        if kind == 1:
            raw[b, 0] = eos
        elif kind == 2:
            raw[b, max(S - 2, 0)] = eos
        elif kind == 3:
            raw[b, S // 3] = eos
            raw[b, (2 * S) // 3] = eos
        elif kind == 4:
            raw[b, torch.randint(0, ld, (2,), generator=g)] = eos
    raw[:, S - 1:] = eos  # never read: tok2[t] = raw[t - 1] for t <= S - 1

    def want(gid=None, gsteps=None):
        tok2 = torch.full((B, ld), 77, dtype=torch.int32)
        tok2[:, 0] = bos
        tok2[:, 1:S] = raw[:, :S - 1]
        kpm = (tok2[:, :S] == eos).int().cumsum(-1) > 0
        if gid is not None:
            kpm |= torch.arange(S)[None, :] >= gsteps[gid.long()][:, None]
        full = torch.full((B, ld), 77, dtype=torch.uint8)
        full[:, :S] = kpm.to(torch.uint8)
        return tok2, full

    tok2, kpm = hipops.refine_prep(raw.to(dev), S, bos, eos)
    wt, wk = want()
    assert torch.equal(tok2.cpu(), wt) and torch.equal(kpm.cpu(), wk)
    # grouped: positions >= the mini-batch's own step count are masked whatever the buffer holds there (no <eos> needed)
    gsteps = torch.tensor([1, max(1, S // 2), S], dtype=torch.int32)
    gid = torch.randint(0, 3, (B,), generator=g, dtype=torch.int32)
    tok2, kpm = hipops.refine_prep(raw.to(dev), S, bos, eos, gid=gid.to(dev), gsteps=gsteps.to(dev))
    wt, wk = want(gid, gsteps)
    assert torch.equal(tok2.cpu(), wt) and torch.equal(kpm.cpu(), wk)


# -------------------------------------------------------------------------------------------------------------------- rep_cut
@pytest.mark.parametrize("eos", [0, 3])
@pytest.mark.parametrize("C", [7121, 257])
def test_rep_cut(dev, C, eos):
    S, rows = 5, 6  # one row behind S: a cut of S must do nothing although the memory is there
    cuts = [-1, 0, S - 1, S, 2, -1]
    B = len(cuts)
    g = torch.Generator().manual_seed(C)
    x = torch.randn(B, rows, C, generator=g)
    state = torch.tensor([[1, 1, c, 0] for c in cuts], dtype=torch.int32)
    want = x.clone()
    for b, c in enumerate(cuts):
        if 0 <= c < S:
            want[b, c, :] = -30.0
            want[b, c, eos] = 30.0
    xd = x.to(dev)
    hipops.rep_cut(xd, S, state.to(dev), eos)
    assert torch.equal(xd.cpu().view(torch.int32), want.view(torch.int32))


# --------------------------------------------------------------------------------------------------------------- ctx_embed_ln
@pytest.mark.parametrize("form", ["first_row", "step_row", "all_rows"])
@pytest.mark.parametrize("D", [32, 192, 368, 1024])
def test_ctx_embed_ln(dev, D, form):
    """content rows sqrt(D) emb[tok] (+ pos_queries[pos - 1]) -> LayerNorm: position 0 alone (no positional term), one later
    position (the per-step form) and all S positions (the refinement's form); rows not asked for keep the sentinel."""
    g = torch.Generator().manual_seed(D)
    B, S, ntok, eps = 3, 7, 19, 1e-5
    out_rows = S + 2
    pos0, npos = {"first_row": (0, 1), "step_row": (4, 1), "all_rows": (0, S)}[form]
    tok = torch.randint(0, ntok, (B, S + 1), generator=g, dtype=torch.int32)
    emb = torch.randn(ntok, D, generator=g) / math.sqrt(D)
    posq = 0.5 * torch.randn(S, D, generator=g)
    gam, bet = 1.0 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)

    def ref(dt):
        x = math.sqrt(D) * emb.to(dt)[tok[:, :S].long()]
        x[:, 1:] = posq.to(dt)[None, :S - 1] + x[:, 1:]
        return F.layer_norm(x, (D,), gam.to(dt), bet.to(dt), eps)

    r64, r32 = ref(torch.float64), ref(torch.float32)
    out = torch.full((B, out_rows, D), -777.25, device=dev)
    hipops.ctx_embed_ln(tok.to(dev), pos0, npos, emb.to(dev), posq.to(dev), gam.to(dev), bet.to(dev), eps, out)
    out = out.cpu()
    sel = slice(pos0, pos0 + npos)
    e32 = (r32[:, sel].double() - r64[:, sel]).abs().max().item()
    err = (out[:, sel].double() - r64[:, sel]).abs().max().item()
    print(f"ctx_embed_ln D={D} {form}: gpu_err={err:.3e} e32={e32:.3e}")
    assert err <= 4 * e32, f"{err:.3e} > 4 * {e32:.3e}"
    keep = torch.ones(out_rows, dtype=torch.bool)
    keep[sel] = False
    assert torch.equal(out[:, keep], torch.full_like(out[:, keep], -777.25))


def test_ctx_embed_ln_refuses_rows_wider_than_1024(dev):
    D = 1028
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    out = torch.full((1, 2, D), -777.25, device=dev)
    with pytest.raises(_lib.YmkError, match="D <= 1024"):
        hipops.ctx_embed_ln(torch.zeros(1, 2, dtype=torch.int32, device=dev), 0, 1, z(3, D), z(2, D), z(D), z(D), 1e-5, out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((1, 2, D), -777.25))


# ------------------------------------------------------------------------------------------ init_decode, tile_rows, add_pos_embed
@pytest.mark.parametrize("ld_tok,B", [(4, 70001), (26, 10101), (101, 2603), (26, 3)])
def test_init_decode(dev, ld_tok, B):
    """B * ld_tok beyond 1024 blocks x 256 threads: the stride loop runs (and a small batch that it does not need)."""
    assert B == 3 or B * ld_tok > 1024 * 256
    tok, state = hipops.init_decode(B, ld_tok, 7119, 7120, dev)
    want = torch.full((B, ld_tok), 7120, dtype=torch.int32)
    want[:, 0] = 7119
    assert torch.equal(tok.cpu(), want)
    assert torch.equal(state.cpu(), torch.tensor([[0, 0, -1, 0]], dtype=torch.int32).expand(B, 4))


@pytest.mark.parametrize("rows,D,B", [(26, 32, 1), (7, 4, 3), (101, 192, 5), (101, 64, 330)])
def test_tile_rows(dev, rows, D, B):
    """the last case is beyond 2048 blocks x 256 float4: the stride loop runs."""
    src = torch.randn(rows, D, generator=torch.Generator().manual_seed(rows))
    got = hipops.tile_rows(src.to(dev), B).cpu()
    assert torch.equal(got, src[None].expand(B, rows, D))


@pytest.mark.parametrize("B,gh,gw,full_gw,D", [(2, 3, 5, 9, 8), (3, 8, 100, 100, 192), (74, 8, 37, 100, 192)])
def test_add_pos_embed(dev, B, gh, gw, full_gw, D):
    """x[b, r, c] += pos[r * full_gw + c]: a cropped width (gw < full_gw), the full width, and a total beyond 4096 blocks x 256
    float4 (the stride loop)."""
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, gh, gw, D, generator=g)
    pos = torch.randn(gh * full_gw, D, generator=g)
    assert B != 74 or B * gh * gw * D // 4 > 4096 * 256
    got = hipops.add_pos_embed(x.to(dev), pos.to(dev), full_gw).cpu()
    want = x + pos.reshape(gh, full_gw, D)[None, :, :gw]
    assert torch.equal(got, want)
