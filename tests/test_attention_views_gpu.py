"""Single launches of the attention kernels and of LayerNorm in the forms the models launch them (ymk_op_attention_view,
ymk_op_layernorm_view), which ymk_op_attention / ymk_op_nar_cross_attention / ymk_op_layernorm pin: operands that are columns
of one wider buffer (the PARSeq encoder's [B, L, 3D] q|k|v, RT-DETR's [B, T, 2D] q|k, the decoders' [.., 2D] k|v), an output
written into columns of a wider buffer, batch strides longer than the rows used, ragged batches through offset / length tables,
one query table for the whole batch, masks wider than the key list, and caller-supplied max|x| records.

Every attention case asserts: (a) no NaN and no sentinel inside the output view - every spare column and row of the operand
buffers holds NaN, so a load outside a view that reaches a stored value shows; (b) the error against the float64 reference
(tests/attn_ref.py, itself checked against torch on the CPU) relative to max|ref| is below the project's 2e-5; (c) the result is
bit-identical to the same data passed contiguously through ymk_op_attention / ymk_op_nar_cross_attention, whole or sample by
sample - a leading dimension or a table moves addresses, not arithmetic; (d) every word of the output buffer outside the rows
and columns of the view still holds the sentinel."""
import functools

import pytest
import torch

from tests import attn_ref
from tests.attn_ref import HEADS, TOL
from tests.conv_ref import is_sentinel, options

pytestmark = pytest.mark.gpu

F16 = {"conv_split": 16}  # with three records: both products of the flash kernel on fp16 planes (k_flash_attn_f16)
NONE3 = (None, None, None)
ORDERS = (None, (2, 0, 3, 1))  # the samples one after the other, and a table whose offsets do not increase


def _check(name, outs, obuf, written, ref, want, tol=TOL):
    """assertions (a) - (d) of one launch; want: the per-sample results of the contiguous launch (CPU), or None"""
    got = [o.cpu() for o in outs]
    sent = is_sentinel(obuf).cpu()
    assert not bool(sent[written].any()), f"{name}: (a) a word of the output view was not written"
    assert not any(bool(torch.isnan(g).any()) for g in got), f"{name}: (a) NaN - a word outside an operand's view reached a stored value"
    err = attn_ref.rel_err(got, ref)
    print(f"{name}: err {err:.2e}")
    assert err < tol, f"{name}: (b) {err:.3e} >= {tol:.1e}"
    if want is not None:
        assert all(torch.equal(g, w) for g, w in zip(got, want)), f"{name}: (c) not the bits of the contiguous launch"
    assert bool(sent[~written].all()), f"{name}: (d) a store landed outside the output view"
    return err


def _true_records(case, dev):
    """one record per operand, holding its true maximum - what ymk_op_attention measures for itself"""
    from tests import hipops

    qs = [case.qs] if torch.is_tensor(case.qs) else case.qs
    return tuple(hipops.amax_record(max(float(t.abs().max()) for t in ts), dev) for ts in (qs, case.ks, case.vs))


@functools.lru_cache(maxsize=None)
def _contiguous(case, f16, dev, use_small=False):
    """the case through ymk_op_attention, contiguous: the whole batch where the lengths agree, else sample by sample - with
    f16 the records of the whole batch on every sample, hence through the view entry's uniform form (ymk_op_attention would
    measure each sample's own maxima).  -> per-sample CPU tensors"""
    from tests import hipops

    shared = torch.is_tensor(case.qs)
    qs = [case.qs] * len(case.ks) if shared else case.qs
    uniform = len({k.shape[0] for k in case.ks}) == 1 and len({q.shape[0] for q in qs}) == 1
    with options(F16 if f16 else {}):
        if uniform:
            mask = case.mask_qk[:, :case.lks[0]] if case.mask_qk is not None else None
            kpm = case.kpm[:, :case.lks[0]] if case.kpm is not None else None
            out = hipops.attention(torch.stack(qs).to(dev), torch.stack(case.ks).to(dev), torch.stack(case.vs).to(dev), case.heads,
                                   scale=case.scale, mask_qk=mask, key_padding_mask=kpm, use_small=use_small)
            return [o.cpu() for o in out]
        if not f16:
            return [hipops.attention(q[None].to(dev), k[None].to(dev), v[None].to(dev), case.heads, scale=case.scale, use_small=use_small)[0].cpu()
                    for q, k, v in zip(qs, case.ks, case.vs)]
        recs = _true_records(case, dev)
        return [hipops.attention_view("small" if use_small else "flash", [q], [k], [v], case.heads, dev, scale=case.scale, rowgap=0,
                                      amax=recs)[0][0].cpu() for q, k, v in zip(qs, case.ks, case.vs)]


# ---- packed operands: the three layouts of the launch sites, exact and fp16-split flash kernel
@pytest.mark.parametrize("mode", ["exact", "f16"])
@pytest.mark.parametrize("hd", attn_ref.PACKED_HD)
@pytest.mark.parametrize("pack", ["qkv", "qk", "kv"])
def test_packed_operands(dev, pack, hd, mode):
    """q, k, v as columns of one [B, L, 3D] buffer (PARSeq encoder), q | k packed with v apart (RT-DETR), q apart with k | v packed
    (the decoders' memkv) - at the models' leading dimensions (colgap 0) and with four NaN columns after every operand (colgap
    4: beside head 1 of the <64, 48> instantiation lies NaN, not the next operand) -, the output in columns 8 .. 8 + D of a buffer
    of D + 20, a NaN row after every sample; lq x lk across the edges of a wave's 32 and a block's 128 queries, a 32-key
    sub-tile and a 64-key tile.  Records (f16): one per operand, its true maximum - the bits of ymk_op_attention under the option."""
    from tests import hipops

    f16 = mode == "f16"
    d = HEADS * hd
    worst = 0.0
    for colgap in (0, 4):
        for lq in attn_ref.PACKED_LQ:
            for lk in attn_ref.PACKED_LK:
                case = attn_ref.packed_case(hd, lq, lk)
                want = _contiguous(case, f16, dev)
                with options(F16 if f16 else {}):
                    outs, obuf, written = hipops.attention_view("flash", case.qs, case.ks, case.vs, HEADS, dev, pack=pack, colgap=colgap,
                                                                o_view=(8, d + 20), amax=_true_records(case, dev) if f16 else NONE3)
                worst = max(worst, _check(f"{pack}+{colgap} {mode} hd{hd} lq{lq} lk{lk}", outs, obuf, written, case.ref, want))
    print(f"packed {pack} {mode} hd{hd}: worst err {worst:.2e}")


def test_fp16_split_kernel_is_what_the_f16_cases_run(dev):
    """the bit comparisons of the f16 cases are between two runs of k_flash_attn_f16, not two of the exact kernel"""
    case = attn_ref.packed_case(64, 129, 130)
    assert not all(torch.equal(a, b) for a, b in zip(_contiguous(case, True, dev), _contiguous(case, False, dev)))


# ---- ragged batches
RAGGED = [("flash", "exact"), ("flash", "f16"), ("small", "exact")]


@pytest.mark.parametrize("kernel,mode", RAGGED, ids=[f"{k}-{m}" for k, m in RAGGED])
@pytest.mark.parametrize("hd", attn_ref.PACKED_HD + (46,))
def test_ragged_self_attention(dev, kernel, mode, hd):
    """Four samples of 1, 33, 64 and 130 tokens in one [rows, 3D] buffer, two NaN rows between them, qoff = koff: the grid is sized
    for 130 queries, so the short samples' second blocks leave at once, and waves 1 - 3 of the last block of the 130-token
    sample hold no query but stage its tiles.  Head dim 46 enters flash_attention and must reach the small kernel with the tables."""
    from tests import hipops

    f16 = mode == "f16"
    case = attn_ref.ragged_self_case(hd)
    want = _contiguous(case, f16, dev, use_small=kernel == "small")
    for order in ORDERS:
        with options(F16 if f16 else {}):
            outs, obuf, written = hipops.attention_view(kernel, case.qs, case.ks, case.vs, HEADS, dev, pack="qkv", rowgap=2, q_tab=True,
                                                        k_tab=True, order=order, o_view=(4, HEADS * hd + 8),
                                                        amax=_true_records(case, dev) if f16 else NONE3)
        _check(f"ragged self {kernel} {mode} hd{hd} order {order}", outs, obuf, written, case.ref, want)


@pytest.mark.parametrize("kernel,mode", RAGGED, ids=[f"{k}-{m}" for k, m in RAGGED])
@pytest.mark.parametrize("hd", attn_ref.PACKED_HD + (46,))
def test_ragged_cross_attention(dev, kernel, mode, hd):
    """33 queries per sample at one batch stride, ragged keys only - k | v packed as in memkv, found through (koff, klen), in
    increasing and in mixed order"""
    from tests import hipops

    f16 = mode == "f16"
    case = attn_ref.ragged_cross_case(hd, 33)
    want = _contiguous(case, f16, dev, use_small=kernel == "small")
    for order in ORDERS:
        with options(F16 if f16 else {}):
            outs, obuf, written = hipops.attention_view(kernel, case.qs, case.ks, case.vs, HEADS, dev, pack="kv", rowgap=2, k_tab=True,
                                                        order=order, o_view=(4, HEADS * hd + 8),
                                                        amax=_true_records(case, dev) if f16 else NONE3)
        _check(f"ragged cross {kernel} {mode} hd{hd} order {order}", outs, obuf, written, case.ref, want)


# ---- the small kernel as the decoder calls it
@pytest.mark.parametrize("lq", attn_ref.SMALL_LQ)
@pytest.mark.parametrize("hd", attn_ref.SMALL_HD)
def test_small_kernel_as_the_decoder_calls_it(dev, hd, lq):
    """bsq = 0 (one query table for three samples), k | v packed in one [B, NS, 2D] buffer of which lk < NS rows are keys,
    mask_qk and kpm of leading dimension NS with random bits past lk.  Head dims 32, 96 and 128 load keys as 16-byte words, 46
    (rows only 8-byte aligned) one float at a time."""
    from tests import hipops

    for lk in attn_ref.SMALL_LK:
        case = attn_ref.decoder_case(hd, lq, lk)
        want = _contiguous(case, False, dev, use_small=True)
        outs, obuf, written = hipops.attention_view("small", case.qs, case.ks, case.vs, HEADS, dev, pack="kv", rowgap=2,
                                                    o_view=(3, HEADS * hd + 5), mask_qk=case.mask_qk, kpm=case.kpm)
        _check(f"decoder hd{hd} lq{lq} lk{lk}", outs, obuf, written, case.ref, want)


@pytest.mark.parametrize("lq", attn_ref.SMALL_LQ)
def test_small_kernel_scalar_loads_at_a_head_dim_of_four_floats(dev, lq):
    """hd % 4 == 0 but ldk % 4 != 0 (one spare column after k and after v: ld = 2D + 2): the key loads fall back to single floats,
    whose sum runs in another order than the 16-byte form's - so (c) compares with the same leading dimension sample by sample
    (B = 1, no spare rows, no output view), and the contiguous launch is held to the float64 bound only."""
    from tests import hipops

    hd = 32
    for lk in attn_ref.SMALL_LK:
        case = attn_ref.decoder_case(hd, lq, lk)
        one = [hipops.attention_view("small", case.qs, [k], [v], HEADS, dev, pack="kv", colgap=1, rowgap=0, mask_qk=case.mask_qk,
                                     kpm=case.kpm[i:i + 1])[0][0].cpu() for i, (k, v) in enumerate(zip(case.ks, case.vs))]
        outs, obuf, written = hipops.attention_view("small", case.qs, case.ks, case.vs, HEADS, dev, pack="kv", colgap=1, rowgap=2,
                                                    o_view=(3, HEADS * hd + 5), mask_qk=case.mask_qk, kpm=case.kpm)
        _check(f"decoder scalar hd{hd} lq{lq} lk{lk}", outs, obuf, written, case.ref, one)
        assert attn_ref.rel_err(_contiguous(case, False, dev, use_small=True), case.ref) < TOL


# ---- records
def _scaled_case(hd, which, r):
    """packed_case(hd, 129, 130) with operand `which` ("k" / "v") divided by r"""
    base = attn_ref.packed_case(hd, 129, 130)
    ks = [k / r for k in base.ks] if which == "k" else base.ks
    vs = [v / r for v in base.vs] if which == "v" else base.vs
    return attn_ref.Case(base.qs, ks, vs, HEADS)


@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("which", ["v", "k"])
def test_one_record_shared_by_q_k_and_v(dev, which, hd):
    """The encoder's form: q, k and v are columns of one buffer whose producer left ONE record, so an operand r times smaller
    than the largest is cut into planes at a scale log2 r bits too coarse - that product's 2^-21 grows by r, and so does the
    bound: 2e-5 r for r = 1, 8, 64.
    Measured (MI355X, lq 129, lk 130; relative to max|ref|), r = 1 / 8 / 64:
      v / r, hd 32: 2.46e-07 / 2.46e-07 / 2.46e-07      v / r, hd 64: 3.33e-07 / 3.33e-07 / 3.33e-07
      k / r, hd 32: 2.46e-07 / 3.68e-07 / 4.18e-07      k / r, hd 64: 3.33e-07 / 3.35e-07 / 3.76e-07
    - each equal to the error with a record per operand: the planes are floating-point halves, so a scale 2^6 too small moves
    exponents, not mantissas, and nothing is lost until the low plane meets fp16's subnormals (an operand 2^17 below its record).
    The bound above is the fixed-point worst case and far from reached."""
    from tests import hipops

    for r in (1, 8, 64):
        case = _scaled_case(hd, which, r)
        top = max(float(t.abs().max()) for ts in (case.qs, case.ks, case.vs) for t in ts)
        rec = hipops.amax_record(top, dev)
        with options(F16):
            outs, obuf, written = hipops.attention_view("flash", case.qs, case.ks, case.vs, HEADS, dev, pack="qkv", o_view=(8, HEADS * hd + 20),
                                                        amax=(rec, rec, rec))
            own = hipops.attention_view("flash", case.qs, case.ks, case.vs, HEADS, dev, pack="qkv", amax=_true_records(case, dev))[0]
        err = _check(f"shared record, {which} / {r}, hd{hd}", outs, obuf, written, case.ref, None, tol=TOL * r)
        print(f"shared record, {which} / {r}, hd{hd}: {err:.2e} (a record per operand: {attn_ref.rel_err([o.cpu() for o in own], case.ref):.2e})")


def test_caller_records_of_the_true_maxima_give_the_bits_of_the_measured_ones(dev):
    """the same for the three layouts at the models' leading dimensions is part of test_packed_operands; here: contiguous operands
    (the view entry and ymk_op_attention are then the same launch but for who fills the records), and records that hold the
    maxima in another of their 32 lines"""
    from tests import hipops

    for hd in attn_ref.PACKED_HD:
        case = attn_ref.packed_case(hd, 129, 130)
        recs = _true_records(case, dev)
        moved = tuple(torch.roll(rec, 32 * (5 + i)) for i, rec in enumerate(recs))
        with options(F16):
            for amax in (recs, moved):
                outs, obuf, written = hipops.attention_view("flash", case.qs, case.ks, case.vs, HEADS, dev, rowgap=0, amax=amax)
                _check(f"true records hd{hd}", outs, obuf, written, case.ref, _contiguous(case, True, dev))


def test_zero_v_with_a_zero_record_gives_zero(dev):
    from tests import hipops

    for hd in attn_ref.PACKED_HD:
        base = attn_ref.packed_case(hd, 33, 65)
        zeros = [torch.zeros_like(v) for v in base.vs]
        rq, rk, _ = _true_records(base, dev)
        with options(F16):
            outs, obuf, written = hipops.attention_view("flash", base.qs, base.ks, zeros, HEADS, dev, pack="qkv", o_view=(8, HEADS * hd + 20),
                                                        amax=(rq, rk, hipops.amax_record(0.0, dev)))
        for o in outs:
            assert bool((o.view(torch.int32) == 0).all()), "exactly +0, not NaN and not -0"
        assert bool(is_sentinel(obuf).cpu()[~written].all())


@pytest.mark.parametrize("hd", attn_ref.PACKED_HD)
def test_without_a_record_or_with_a_scale_above_one_the_exact_kernel_runs(dev, hd):
    from tests import hipops

    case = attn_ref.packed_case(hd, 129, 130)
    recs = _true_records(case, dev)
    exact = _contiguous(case, False, dev)
    assert not all(torch.equal(a, b) for a, b in zip(exact, _contiguous(case, True, dev))), "the two kernels differ in bits"
    with options(F16):
        for i in range(3):
            amax = tuple(None if j == i else rec for j, rec in enumerate(recs))
            outs, obuf, written = hipops.attention_view("flash", case.qs, case.ks, case.vs, HEADS, dev, pack="qkv", o_view=(8, HEADS * hd + 20),
                                                        amax=amax)
            _check(f"record {i} missing, hd{hd}", outs, obuf, written, case.ref, exact)
        loud = attn_ref.Case([q / 16 for q in case.qs], case.ks, case.vs, HEADS, scale=16 * case.scale)  # the same logits, scale > 1
        assert loud.scale > 1
        outs, obuf, written = hipops.attention_view("flash", loud.qs, loud.ks, loud.vs, HEADS, dev, scale=loud.scale, pack="qkv",
                                                    o_view=(8, HEADS * hd + 20), amax=_true_records(loud, dev))
    want = hipops.attention(torch.stack(loud.qs).to(dev), torch.stack(loud.ks).to(dev), torch.stack(loud.vs).to(dev), HEADS, scale=loud.scale)
    _check(f"scale {loud.scale:.2f}, hd{hd}", outs, obuf, written, loud.ref, [o.cpu() for o in want])


# ---- the cross attention of the non-autoregressive pass
@pytest.mark.parametrize("hd", attn_ref.NAR_HD)
@pytest.mark.parametrize("heads", attn_ref.NAR_HEADS)
def test_nar_cross_attention_views(dev, heads, hd):
    """One query table, seven samples of 1 .. 13 keys (around the 8- / 4-key tile and the 4-key softmax step) in one memkv
    [rows, 2D] buffer with a NaN row between them, the output in columns 4 .. 4 + D of a buffer of D + 12; lq on both sides of
    a block's queries.  And the uniform form: two samples at one batch stride longer than the keys used."""
    from tests import hipops

    d = heads * hd
    for lq in attn_ref.nar_lqs(hd):
        case = attn_ref.nar_case(heads, hd, lq, attn_ref.NAR_LK)
        want = [o.cpu() for o in hipops.nar_cross_attention(case.qs, case.ks, case.vs, heads, dev)]
        for order in (None, (3, 6, 0, 5, 1, 4, 2)):
            outs, obuf, written = hipops.attention_view("nar", case.qs, case.ks, case.vs, heads, dev, pack="kv", k_tab=True, order=order,
                                                        o_view=(4, d + 12))
            _check(f"nar h{heads} hd{hd} lq{lq} order {order}", outs, obuf, written, case.ref, want)
        for lk in (5, 13):
            two = attn_ref.nar_case(heads, hd, lq, (lk, lk))
            want = [o.cpu() for o in hipops.nar_cross_attention(two.qs, two.ks, two.vs, heads, dev)]
            outs, obuf, written = hipops.attention_view("nar", two.qs, two.ks, two.vs, heads, dev, pack="kv", rowgap=3, o_view=(4, d + 12))
            _check(f"nar uniform h{heads} hd{hd} lq{lq} lk{lk}", outs, obuf, written, two.ref, want)


# ---- LayerNorm
@pytest.mark.parametrize("mod", attn_ref.LN_MOD)
@pytest.mark.parametrize("m", attn_ref.LN_M)
@pytest.mark.parametrize("d", attn_ref.LN_D)
def test_layernorm_views(dev, d, m, mod):
    """ldx != D and ldy != D (the input at columns 4 .. of rows of D + 12 with NaN around it, the output at columns 8 .. of rows
    of D + 20), and in_rows_mod = 3: a three-row table broadcast over the M output rows.  Against float64 at the 2e-5 of
    tests/test_seq_ops_gpu.py on its randn * 3 + 1 data, bit for bit against ymk_op_layernorm on the contiguous copy, and with the
    sentinel in every word outside the output view."""
    from tests import hipops

    x, g, b = attn_ref.layernorm_inputs(m, d, mod)
    rows = x[torch.arange(m) % mod] if mod else x
    for eps in (1e-5, 1e-6):
        ref = attn_ref.layernorm_ref(rows, g, b, eps)
        y, ybuf = hipops.layernorm_view(x.to(dev), g, b, eps, m, x_view=(4, d + 12), y_view=(8, d + 20), in_rows_mod=mod)
        err = float((y.double().cpu() - ref).abs().max())
        print(f"layernorm D{d} M{m} mod{mod} eps{eps}: err {err:.2e}")
        assert not bool(torch.isnan(y).any()) and err < TOL
        assert torch.equal(y, hipops.layernorm(rows.to(dev), g, b, eps)), "a leading dimension moves addresses, not arithmetic"
        sent = is_sentinel(ybuf)
        assert bool(sent[:, :8].all()) and bool(sent[:, 8 + d:].all()) and not bool(sent[:, 8:8 + d].any())
        plain, _ = hipops.layernorm_view(rows.to(dev), g, b, eps, m)
        assert torch.equal(plain, y), "the view entry at ld = D is ymk_op_layernorm"
