"""The fused PARSeq decoder step (yomitoku_amd/csrc/ymk_decstep.hip: k_parseq_dec_step_rows) one launch at a time against a
float64 restatement of one query step, written from oracle/parseq.py::decode: content row -> norm_c -> K|V (appended to the
cache), self attention of query `step` over cache rows 0..step, cross attention over the sample's own memory rows, MLP with
exact-erf GELU, decoder.norm.

Everything the kernel reads is fp32 data the test made: random weights (LayerNorm gammas near 1), random earlier cache rows,
random memory K|V, and the qsa table - built in float64 from norm_q and the self attention's query projection, then rounded
to fp32 for the op.  The reference evaluates the same fp32 inputs in float64.

Tolerance: no constant.  The same restatement also runs in float32 on the CPU; with e32 = max|fp32 - fp64| of a case the
kernel must satisfy max|gpu - fp64| <= 4 * e32, for `out` and for the appended K|V row alike (beyond plain fp32 arithmetic
the kernel differs by its summation order, __expf in the two softmaxes and gelu_f32: all of fp32 rounding's own size).

Observed on an MI355X, largest gpu_err / e32 over all cases of a geometry (D, H, F):
    (192, 6, 768) 1.23    (256, 8, 1024) 0.98    (128, 8, 256) 1.38    (64, 2, 128) 2.20    (32, 8, 64) 3.24    (256, 4, 512) 1.33
(28 cases each; the 3.24 is the K|V row of a two-sample case at D = 32 - 128 values, e32 = 3.6e-7; `out` alone: 1.23, 0.98,
1.32, 1.94, 2.41, 1.27).

Every case runs dec_rows = 1, 2, 3, 4 and asks for the same bits from all four; buffers carry guard rows behind the batch and
a sentinel in every cache row the step must not touch."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import hipops
from yomitoku_amd import _lib

pytestmark = pytest.mark.gpu

GEOMS = [(192, 6, 768), (256, 8, 1024), (128, 8, 256), (64, 2, 128), (32, 8, 64), (256, 4, 512)]
NTOK = 41
NS_MAX = 101
SENT = -777.25
GUARD = 4  # rows behind the batch in out / skv: a block's dead rows must not be written
FACTOR = 4.0

_weights = {}
_ratios = {}


def _w(geom):
    """fp32 host weights of one geometry (made once, never changed) + the fp32 qsa table for NS_MAX positions."""
    if geom in _weights:
        return _weights[geom]
    D, H, Fd = geom
    g = torch.Generator().manual_seed(1000 + D + 7 * H + Fd)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    w = {}
    for name in ("self_attn", "cross_attn"):
        w[f"{name}.in_proj_weight"] = rn(3 * D, D) / math.sqrt(D)
        w[f"{name}.in_proj_bias"] = 0.1 * rn(3 * D)
        w[f"{name}.out_proj.weight"] = rn(D, D) / math.sqrt(D)
        w[f"{name}.out_proj.bias"] = 0.1 * rn(D)
    w["linear1.weight"] = rn(Fd, D) / math.sqrt(D)
    w["linear1.bias"] = 0.1 * rn(Fd)
    w["linear2.weight"] = rn(D, Fd) / math.sqrt(Fd)
    w["linear2.bias"] = 0.1 * rn(D)
    for n in hipops.DEC_STEP_NORMS:
        w[f"{n}.weight"] = 1.0 + 0.1 * rn(D)
        w[f"{n}.bias"] = 0.1 * rn(D)
    w["emb"] = rn(NTOK, D) / math.sqrt(D)
    w["pos_queries"] = 0.5 * rn(NS_MAX, D)
    # qsa = W_q norm_q(pos_queries) + b_q of the self attention, in float64, rounded to fp32 for the op
    pq = w["pos_queries"].double()
    qn = F.layer_norm(pq, (D,), w["norm_q.weight"].double(), w["norm_q.bias"].double(), 1e-5)
    qsa = F.linear(qn, w["self_attn.in_proj_weight"][:D].double(), w["self_attn.in_proj_bias"][:D].double()).float()
    _weights[geom] = (w, qsa)
    return _weights[geom]


def _attend(q, kv, H):
    """q [D], kv [n, 2D] (K | V) -> [D]: softmax(q_h . K_h / sqrt(hd)) V_h per head."""
    D = q.shape[0]
    hd = D // H
    k = kv[:, :D].reshape(-1, H, hd)
    v = kv[:, D:].reshape(-1, H, hd)
    s = torch.einsum("hd,nhd->hn", q.reshape(H, hd), k) / math.sqrt(hd)
    return torch.einsum("hn,nhd->hd", torch.softmax(s, dim=-1), v).reshape(D)


def _ref_step(w, qsa, H, tok_col, step, skv_prev, mems, dt):
    """One query step for every sample in dtype dt -> (out [B, D], kv [B, 2D]).  tok_col [B] = tok[:, step], skv_prev
    [B, step, 2D] the cache rows 0..step-1, mems: per sample its memory K|V [len, 2D]."""
    c = lambda t: t.to(dt)  # noqa: E731
    ln = lambda x, n: F.layer_norm(x, (x.shape[-1],), c(w[n + ".weight"]), c(w[n + ".bias"]), 1e-5)  # noqa: E731
    D = qsa.shape[1]
    B = tok_col.shape[0]
    pq = c(w["pos_queries"])
    content = math.sqrt(D) * c(w["emb"])[tok_col.long()]
    if step > 0:
        content = pq[step - 1] + content
    kv = F.linear(ln(content, "norm_c"), c(w["self_attn.in_proj_weight"])[D:], c(w["self_attn.in_proj_bias"])[D:])
    rows = torch.cat([c(skv_prev), kv[:, None]], dim=1)
    sa = torch.stack([_attend(c(qsa)[step], rows[b], H) for b in range(B)])
    query = pq[step] + F.linear(sa, c(w["self_attn.out_proj.weight"]), c(w["self_attn.out_proj.bias"]))
    qc = F.linear(ln(query, "norm1"), c(w["cross_attn.in_proj_weight"])[:D], c(w["cross_attn.in_proj_bias"])[:D])
    ca = torch.stack([_attend(qc[b], c(mems[b]), H) for b in range(B)])
    query = query + F.linear(ca, c(w["cross_attn.out_proj.weight"]), c(w["cross_attn.out_proj.bias"]))
    h = F.gelu(F.linear(ln(query, "norm2"), c(w["linear1.weight"]), c(w["linear1.bias"])))
    query = query + F.linear(h, c(w["linear2.weight"]), c(w["linear2.bias"]))
    return ln(query, "decoder.norm"), kv


@pytest.fixture(autouse=True)
def _reset_dec_rows():
    yield
    _lib.debug_option("dec_rows", 0)


class Case:
    """The fp32 inputs of one step: tokens, earlier cache rows, memory (dense: L rows per sample; lens: the ragged form)."""

    def __init__(self, geom, NS, step, L, B, lens=None, seed=0):
        D, H, Fd = geom
        self.geom, self.NS, self.step, self.L, self.B, self.lens = geom, NS, step, L, B, lens
        self.w, qsa = _w(geom)
        self.w = dict(self.w, pos_queries=self.w["pos_queries"][:NS].contiguous())
        self.qsa = qsa[:NS].contiguous()
        g = torch.Generator().manual_seed(seed * 7919 + D + 3 * NS + 5 * step + 11 * L + 13 * B)
        self.tok = torch.randint(0, NTOK, (B, NS), generator=g, dtype=torch.int32)
        self.skv_prev = torch.randn(B, step, 2 * D, generator=g)
        if lens is None:
            mem = torch.randn(B * L, 2 * D, generator=g)
            self.mems = [mem[b * L:(b + 1) * L] for b in range(B)]
            self.mem_off = self.mem_len = None
        else:
            assert len(lens) == B and max(lens) <= L and min(lens) >= 1
            # a few rows nobody owns in front and between the samples: an offset taken as b * L reads the wrong rows
            off, o = [], 3
            for n in lens:
                off.append(o)
                o += n + 2
            mem = torch.randn(o, 2 * D, generator=g)
            self.mems = [mem[a:a + n] for a, n in zip(off, lens)]
            self.mem_off = torch.tensor(off, dtype=torch.int32)
            self.mem_len = torch.tensor(lens, dtype=torch.int32)
        self.mem = mem
        self._ref = None

    def ref(self):
        """(out64, kv64, e32_out, e32_kv), computed once."""
        if self._ref is None:
            H = self.geom[1]
            a = (self.w, self.qsa, H, self.tok[:, self.step], self.step, self.skv_prev, self.mems)
            o64, k64 = _ref_step(*a, torch.float64)
            o32, k32 = _ref_step(*a, torch.float32)
            self._ref = (o64, k64, (o32.double() - o64).abs().max().item(), (k32.double() - k64).abs().max().item())
        return self._ref

    def buffers(self, dev):
        """fresh device buffers with guard rows: (tok, skv_full, out_full, memkv)."""
        B, NS, D = self.B, self.NS, self.geom[0]
        skv = torch.full((B + GUARD, NS, 2 * D), SENT)
        skv[:B, :self.step] = self.skv_prev
        out = torch.full((B + GUARD, D), SENT)
        return self.tok.to(dev), skv.to(dev), out.to(dev), self.mem.to(dev)

    def launch(self, dev, rows, **kw):
        """one launch at `rows` samples per block -> (out_full, skv_full, skv_before) on the host."""
        tok, skv, out, mem = self.buffers(dev)
        before = skv.cpu()
        _lib.debug_option("dec_rows", rows)
        kw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()}
        hipops.parseq_dec_step(self.w, self.geom[1], self.qsa, tok, skv[:self.B], mem, out[:self.B], self.step, self.L,
                               mem_off=None if self.mem_off is None else self.mem_off.to(dev),
                               mem_len=None if self.mem_len is None else self.mem_len.to(dev), **kw)
        torch.cuda.synchronize()
        return out.cpu(), skv.cpu(), before


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check(case, dev):
    """dec_rows 1..4 give the same bits; untouched rows keep their bits; out and the new cache row are within FACTOR * e32 of
    float64.  Returns the dec_rows = 1 (out, skv) for bit comparisons by the caller."""
    B, step = case.B, case.step
    o64, k64, e_out, e_kv = case.ref()
    first = None
    for rows in (1, 2, 3, 4):
        out, skv, before = case.launch(dev, rows)
        keep = torch.ones(skv.shape[:2], dtype=torch.bool)
        keep[:B, step] = False
        assert _same_bits(skv[keep], before[keep]), f"dec_rows {rows}: a cache row other than row {step} of the batch changed"
        assert _same_bits(out[B:], torch.full_like(out[B:], SENT)), f"dec_rows {rows}: out written behind the batch"
        if first is None:
            first = (out, skv)
        else:
            assert _same_bits(out, first[0]) and _same_bits(skv, first[1]), f"dec_rows {rows} differs from dec_rows 1 in bits"
    out, skv = first
    g_out = (out[:B].double() - o64).abs().max().item()
    g_kv = (skv[:B, step].double() - k64).abs().max().item()
    r_out, r_kv = g_out / e_out, g_kv / e_kv
    print(f"decstep geom={case.geom} NS={case.NS} step={step} L={case.L} B={B} ragged={case.lens is not None}: "
          f"out gpu_err={g_out:.3e} e32={e_out:.3e} ratio={r_out:.2f} | kv gpu_err={g_kv:.3e} e32={e_kv:.3e} ratio={r_kv:.2f}")
    _ratios[case.geom] = max(_ratios.get(case.geom, 0.0), r_out, r_kv)
    assert g_out <= FACTOR * e_out, f"out: {g_out:.3e} > {FACTOR} * {e_out:.3e}"
    assert g_kv <= FACTOR * e_kv, f"K|V row: {g_kv:.3e} > {FACTOR} * {e_kv:.3e}"
    return first


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_steps_cross_the_wave_and_batch_edges(dev, geom):
    """step 0 (no positional term, one key row), 1, 15 / 16 / 17 (the 16 virtual waves each get their first row, then the
    first of them its second) and NS - 1 (101 key rows: up to seven per virtual wave, a second batch of four)."""
    for NS in (26, 101):
        for step in (0, 1, 15, 16, 17, NS - 1):
            _check(Case(geom, NS, step, L=15, B=3), dev)
    print(f"decstep worst ratio so far geom={geom}: {_ratios[geom]:.2f}")


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_memory_lengths(dev, geom):
    for L in (1, 15, 16, 65, 277, 1024):
        _check(Case(geom, 26, 5, L=L, B=2), dev)
    print(f"decstep worst ratio so far geom={geom}: {_ratios[geom]:.2f}")


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_ragged_memory(dev, geom):
    """mem_off / mem_len: lengths mixed from 1 to L; every sample must read ITS rows."""
    _check(Case(geom, 26, 17, L=277, B=6, lens=[1, 277, 16, 65, 2, 130]), dev)
    _check(Case(geom, 26, 0, L=20, B=3, lens=[17, 1, 20]), dev)


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_batch_sizes_against_rows_per_block(dev, geom):
    """B in {1, 2, 3, 5, 9} x dec_rows 1..4: B not a multiple of the rows per block, a last block with dead rows."""
    for B in (1, 2, 3, 5, 9):
        _check(Case(geom, 26, 16, L=65, B=B), dev)


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_grouped_rows_freeze_and_live_rows_keep_their_bits(dev, geom):
    """Three mini-batches, the middle one closed at step - 1: its rows' out and cache row keep the sentinel bit for bit, the
    live rows equal the ungrouped launch bit for bit - at every rows-per-block (blocks of frozen rows only, and mixed ones)."""
    B, NS, step, ng = 7, 26, 6, 3
    case = Case(geom, NS, step, L=16, B=B)
    plain_out, plain_skv = _check(case, dev)
    gid = torch.tensor([0, 0, 1, 1, 1, 2, 2], dtype=torch.int32)
    gopen = torch.ones(NS, ng, dtype=torch.int32)
    gopen[step - 1, 1] = 0
    gopen[step, :] = 0      # only row step - 1 may be looked at
    gopen[step - 2, :] = 0
    live = gid != 1
    for rows in (1, 2, 3, 4):
        out, skv, before = case.launch(dev, rows, gid=gid, gopen=gopen, ng=ng)
        assert _same_bits(out[:B][live], plain_out[:B][live]) and _same_bits(skv[:B][live], plain_skv[:B][live]), rows
        assert _same_bits(out[:B][~live], torch.full_like(out[:B][~live], SENT)), f"dec_rows {rows}: a frozen row's out was written"
        assert _same_bits(skv[:B][~live], before[:B][~live]), f"dec_rows {rows}: a frozen row's cache was written"
        assert _same_bits(out[B:], torch.full_like(out[B:], SENT)) and _same_bits(skv[B:], before[B:])
    # at step 0 no mini-batch can have closed: the tables are not consulted
    case0 = Case(geom, NS, 0, L=16, B=B)
    p0, s0 = _check(case0, dev)
    out, skv, _ = case0.launch(dev, 2, gid=gid, gopen=torch.zeros(NS, ng, dtype=torch.int32), ng=ng)
    assert _same_bits(out, p0) and _same_bits(skv, s0)


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_speculative_step_changes_nothing(dev, geom):
    case = Case(geom, 26, 3, L=15, B=5)
    plain_out, plain_skv = _check(case, dev)
    for rows in (1, 4):
        out, skv, before = case.launch(dev, rows, prev_not_done=torch.zeros(1, dtype=torch.int32))
        assert _same_bits(out, torch.full_like(out, SENT)) and _same_bits(skv, before), rows
        out, skv, _ = case.launch(dev, rows, prev_not_done=torch.ones(1, dtype=torch.int32))
        assert _same_bits(out, plain_out) and _same_bits(skv, plain_skv), rows


@pytest.mark.parametrize("D,H,Fd,L", [(368, 8, 768, 15), (260, 5, 768, 15), (192, 6, 1028, 15), (192, 6, 768, 1025)],
                         ids=["D368_H8", "D260", "F1028", "L1025"])
def test_unsupported_geometries_are_refused_and_nothing_is_launched(dev, D, H, Fd, L):
    g = torch.Generator().manual_seed(5)
    NS, B = 26, 2
    w = {n: torch.randn(*s, generator=g) * 0.05 for n, s in (
        ("self_attn.in_proj_weight", (3 * D, D)), ("self_attn.in_proj_bias", (3 * D,)), ("self_attn.out_proj.weight", (D, D)),
        ("self_attn.out_proj.bias", (D,)), ("cross_attn.in_proj_weight", (3 * D, D)), ("cross_attn.in_proj_bias", (3 * D,)),
        ("cross_attn.out_proj.weight", (D, D)), ("cross_attn.out_proj.bias", (D,)), ("linear1.weight", (Fd, D)),
        ("linear1.bias", (Fd,)), ("linear2.weight", (D, Fd)), ("linear2.bias", (D,)), ("emb", (NTOK, D)), ("pos_queries", (NS, D)))}
    for n in hipops.DEC_STEP_NORMS:
        w[n + ".weight"], w[n + ".bias"] = torch.ones(D), torch.zeros(D)
    tok = torch.zeros(B, NS, dtype=torch.int32, device=dev)
    skv = torch.full((B, NS, 2 * D), SENT, device=dev)
    out = torch.full((B, D), SENT, device=dev)
    mem = torch.randn(B * L, 2 * D, generator=g).to(dev)
    with pytest.raises(_lib.YmkError, match="unsupported geometry"):
        hipops.parseq_dec_step(w, H, torch.zeros(NS, D), tok, skv, mem, out, 1, L)
    torch.cuda.synchronize()
    assert _same_bits(out.cpu(), torch.full((B, D), SENT)) and _same_bits(skv.cpu(), torch.full((B, NS, 2 * D), SENT))
