"""What tests/test_attention_views_gpu.py and tests/test_attn_ref_host.py share: plain float64 references of one attention launch
and of LayerNorm, and the builders of the ragged and masked inputs.  The references are written out - scores, the row maximum,
exp, the row sum - so that torch's own softmax and attention stay an independent check of them (the host test)."""
from __future__ import annotations

import functools

import torch

TOL = 2e-5  # of max|ref| for attention, absolute for LayerNorm: the project's bound (tests/test_seq_ops_gpu.py)

# per-sample lengths of the ragged batches: one query, a wave plus one, a key tile, and a last 128-query block of two queries
RAGGED_LENS = (1, 33, 64, 130)


def attention_ref(q, k, v, heads, scale, blocked=None):
    """One sample: q [lq, D], k / v [lk, D], blocked [lq, lk] bool or None -> softmax(scale q k^T) v per head, float64 [lq, D]."""
    q, k, v = q.double(), k.double(), v.double()
    lq, d = q.shape
    hd = d // heads
    out = torch.empty(lq, d, dtype=torch.float64)
    for h in range(heads):
        c = slice(h * hd, (h + 1) * hd)
        s = scale * (q[:, c] @ k[:, c].T)
        if blocked is not None:
            s = torch.where(blocked, torch.full_like(s, float("-inf")), s)
        e = torch.exp(s - s.max(dim=1, keepdim=True).values)
        out[:, c] = (e / e.sum(dim=1, keepdim=True)) @ v[:, c]
    return out


def blocked_keys(i, lq, lk, mask_qk=None, kpm=None):
    """The [lq, lk] block table of sample i from mask_qk [lq, >= lk] and kpm [b, >= lk] (either may be None; True = blocked)."""
    if mask_qk is None and kpm is None:
        return None
    blk = torch.zeros(lq, lk, dtype=torch.bool)
    if mask_qk is not None:
        blk |= mask_qk[:lq, :lk]
    if kpm is not None:
        blk |= kpm[i, :lk][None, :]
    return blk


def attention_ref_batch(qs, ks, vs, heads, scale, mask_qk=None, kpm=None):
    """Per sample: qs a list of [lq_i, D] - or one [lq, D] table shared by the batch -, ks / vs lists of [lk_i, D] -> list of
    float64 [lq_i, D]."""
    outs = []
    for i, (k, v) in enumerate(zip(ks, vs)):
        q = qs if torch.is_tensor(qs) else qs[i]
        outs.append(attention_ref(q, k, v, heads, scale, blocked_keys(i, q.shape[0], k.shape[0], mask_qk, kpm)))
    return outs


def layernorm_ref(x, g, b, eps):
    """x [M, D] -> float64 (x - mean) / sqrt(biased variance + eps) * g + b"""
    x = x.double()
    mean = x.sum(dim=1, keepdim=True) / x.shape[1]
    var = ((x - mean) ** 2).sum(dim=1, keepdim=True) / x.shape[1]
    return (x - mean) / torch.sqrt(var + eps) * g.double() + b.double()


def rel_err(got, ref):
    """max |got - ref| over max |ref|, over lists of per-sample tensors or single tensors"""
    if torch.is_tensor(got):
        got, ref = [got], [ref]
    top = max(float(r.abs().max()) for r in ref)
    err = max(float((g.double().cpu() - r).abs().max()) for g, r in zip(got, ref))
    return err / top if top > 0 else err


# ---- input builders (fp32 on the CPU; a test never modifies what it gets)
def qkv(lqs, lks, heads, hd, seed, shared_q=False):
    """-> (qs, ks, vs): lists of [lq_i, D] / [lk_i, D] / [lk_i, D]; shared_q: qs is ONE [lqs, D] table.  q carries a gain of 2 as in
    tests/test_seq_ops_gpu.py: a sharper softmax, which exercises the running-max rescale."""
    g = torch.Generator().manual_seed(seed)
    d = heads * hd
    qs = torch.randn(lqs, d, generator=g) * 2.0 if shared_q else [torch.randn(n, d, generator=g) * 2.0 for n in lqs]
    ks = [torch.randn(n, d, generator=g) for n in lks]
    vs = [torch.randn(n, d, generator=g) for n in lks]
    return qs, ks, vs


def decoder_masks(b, lq, lk, ld_mask, ld_kpm, seed=0):
    """The decoder's two masks, wider than the key list: mask_qk [lq, ld_mask] is causal with the LAST query seeing every key
    (query i is blocked from key j > i + max(0, lk - lq)), kpm [b, ld_kpm] blocks, for sample i >= 1, every key j >= 1 with
    j % 4 == i and the last 3 i keys - never key 0, which so stays open for every query.  The columns from lk on, which no
    launch may read, hold random bits."""
    assert ld_mask >= lk and ld_kpm >= lk
    g = torch.Generator().manual_seed(1000 + seed)
    mask = torch.rand(lq, ld_mask, generator=g) < 0.5
    mask[:, :lk] = torch.triu(torch.ones(lq, lk, dtype=torch.bool), 1 + max(0, lk - lq))
    kpm = torch.rand(b, ld_kpm, generator=g) < 0.5
    kpm[:, :lk] = False
    for i in range(1, b):
        kpm[i, max(1, lk - 3 * i):lk] = True
        kpm[i, i:lk:4] = True
    return mask, kpm


def every_query_has_an_open_key(lq, lks, mask_qk=None, kpm=None):
    """attention over no key at all is outside the kernels' contract: no case may rely on it"""
    for i, lk in enumerate(lks):
        if lk < 1:
            return False
        blk = blocked_keys(i, lq, lk, mask_qk, kpm)
        if blk is not None and not bool((~blk).any(dim=1).all()):
            return False
    return True


def layernorm_inputs(m, d, in_rows_mod, seed=0):
    """x [in_rows_mod or m, d] = randn * 3 + 1 (tests/test_seq_ops_gpu.py), gamma, beta"""
    g = torch.Generator().manual_seed(d + 7 * m + seed)
    x = torch.randn(in_rows_mod or m, d, generator=g) * 3 + 1
    return x, torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)


# ---- the cases: the inputs of each family and their references, built once and shared by every test that asks for them
HEADS = 2  # head 1 is the one whose base pointer can go wrong
PACKED_HD, PACKED_LQ, PACKED_LK = (32, 48, 64, 96), (1, 32, 33, 128, 129), (1, 32, 33, 64, 65, 130)
SMALL_HD, SMALL_LQ, SMALL_LK = (32, 46, 96, 128), (1, 26), (1, 63, 64, 65, 1024)
SMALL_B = 3  # sample i loses its last 3 i keys to kpm
NAR_HEADS, NAR_HD, NAR_LK = (2, 8), (32, 46, 64, 96), (1, 3, 4, 5, 8, 9, 13)
LN_D, LN_M, LN_MOD = (4, 192, 368, 1024), (1, 5, 9), (0, 3)


def nar_lqs(hd):
    """around the queries of one block: 64 lanes x 2 queries at head dim 32, x 1 above"""
    return (128, 129) if hd == 32 else (64, 65)


class Case:
    """qs / ks / vs (attention_ref_batch's arguments), heads, scale, the optional masks, and ref: the float64 outputs"""

    def __init__(self, qs, ks, vs, heads, scale=None, mask_qk=None, kpm=None):
        self.qs, self.ks, self.vs, self.heads, self.mask_qk, self.kpm = qs, ks, vs, heads, mask_qk, kpm
        self.hd = ks[0].shape[1] // heads
        self.scale = self.hd**-0.5 if scale is None else scale
        self.lks = [int(k.shape[0]) for k in ks]
        self.lq = int(qs.shape[0]) if torch.is_tensor(qs) else max(int(q.shape[0]) for q in qs)
        self.ref = attention_ref_batch(qs, ks, vs, heads, self.scale, mask_qk, kpm)


@functools.lru_cache(maxsize=None)
def packed_case(hd, lq, lk):
    """two samples of lq queries and lk keys"""
    return Case(*qkv([lq] * 2, [lk] * 2, HEADS, hd, seed=7 * lq + 1000 * lk + hd), HEADS)


@functools.lru_cache(maxsize=None)
def ragged_self_case(hd, lens=RAGGED_LENS):
    """self attention: sample i has lens[i] queries and as many keys"""
    return Case(*qkv(list(lens), list(lens), HEADS, hd, seed=11 + hd), HEADS)


@functools.lru_cache(maxsize=None)
def ragged_cross_case(hd, lq, lens=RAGGED_LENS):
    """cross attention: lq queries per sample, lens[i] keys"""
    return Case(*qkv([lq] * len(lens), list(lens), HEADS, hd, seed=13 + hd + lq), HEADS)


@functools.lru_cache(maxsize=None)
def decoder_case(hd, lq, lk, spare=2):
    """the decoder's self attention: one query table for the batch, masks of leading dimension lk + spare"""
    mask, kpm = decoder_masks(SMALL_B, lq, lk, lk + spare, lk + spare, seed=lk + lq)
    return Case(*qkv(lq, [lk] * SMALL_B, HEADS, hd, seed=17 + hd + 3 * lq + lk, shared_q=True), HEADS, mask_qk=mask, kpm=kpm)


@functools.lru_cache(maxsize=None)
def nar_case(heads, hd, lq, lks):
    """one query table, ragged keys"""
    return Case(*qkv(lq, list(lks), heads, hd, seed=19 + 100 * heads + hd + lq, shared_q=True), heads)


def all_cases():
    """every attention case of the GPU tests, by name"""
    for hd in PACKED_HD:
        for lq in PACKED_LQ:
            for lk in PACKED_LK:
                yield f"packed hd{hd} lq{lq} lk{lk}", packed_case(hd, lq, lk)
    for hd in PACKED_HD + (46,):
        yield f"ragged self hd{hd}", ragged_self_case(hd)
        yield f"ragged cross hd{hd}", ragged_cross_case(hd, 33)
    for hd in SMALL_HD:
        for lq in SMALL_LQ:
            for lk in SMALL_LK:
                yield f"decoder hd{hd} lq{lq} lk{lk}", decoder_case(hd, lq, lk)
    for heads in NAR_HEADS:
        for hd in NAR_HD:
            for lq in nar_lqs(hd):
                yield f"nar h{heads} hd{hd} lq{lq}", nar_case(heads, hd, lq, NAR_LK)
