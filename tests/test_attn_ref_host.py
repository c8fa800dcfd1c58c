"""CPU self-check of the float64 references the single-op attention and LayerNorm tests compare the kernels with
(tests/attn_ref.py): against torch.nn.functional.scaled_dot_product_attention and F.layer_norm in float64, on the very inputs the
GPU tests use - and the promise those inputs make: every query keeps at least one open key."""
import torch
import torch.nn.functional as F

from tests import attn_ref


def _sdpa64(q, k, v, heads, scale, blocked):
    lq, d = q.shape
    hd = d // heads
    qh, kh, vh = (t.double().view(1, -1, heads, hd).transpose(1, 2) for t in (q, k, v))
    allowed = None if blocked is None else ~blocked
    return F.scaled_dot_product_attention(qh, kh, vh, attn_mask=allowed, scale=scale).transpose(1, 2).reshape(lq, d)


def test_attention_reference_agrees_with_torch_on_every_case_of_the_gpu_tests():
    n, worst = 0, 0.0
    for name, case in attn_ref.all_cases():
        assert attn_ref.every_query_has_an_open_key(case.lq, case.lks, case.mask_qk, case.kpm), name
        for i, (k, v, ref) in enumerate(zip(case.ks, case.vs, case.ref)):
            q = case.qs if torch.is_tensor(case.qs) else case.qs[i]
            assert ref.dtype == torch.float64 and ref.shape == q.shape and bool(torch.isfinite(ref).all()), name
            blk = attn_ref.blocked_keys(i, q.shape[0], k.shape[0], case.mask_qk, case.kpm)
            err = attn_ref.rel_err(_sdpa64(q, k, v, case.heads, case.scale, blk), ref)
            worst = max(worst, err)
            assert err < 1e-12, (name, i, err)
        n += 1
    print(f"{n} cases, worst disagreement with torch {worst:.1e}")
    assert n == 4 * 5 * 6 + 2 * 5 + 4 * 2 * 5 + 2 * 4 * 2


def test_masks_are_wider_than_the_keys_and_block_something():
    """the decoder's masks carry columns past lk (which the reference must ignore), block keys where there are keys to block,
    and differ between the samples"""
    for lk in attn_ref.SMALL_LK:
        case = attn_ref.decoder_case(32, 26, lk)
        assert case.mask_qk.shape == (26, lk + 2) and case.kpm.shape == (attn_ref.SMALL_B, lk + 2)
        assert not bool(case.kpm[0, :lk].any())
        if lk >= 63:
            assert int(case.kpm[2, :lk].sum()) > lk // 4 and int(case.kpm[1, :lk].sum()) >= lk // 4 and not bool(case.kpm[:, 0].any())
            assert bool(case.mask_qk[:, :lk].any()) and not bool(case.mask_qk[-1, :lk].any())
            assert not torch.equal(case.kpm[1, :lk], case.kpm[2, :lk])
            flipped = attn_ref.attention_ref_batch(case.qs, case.ks, case.vs, case.heads, case.scale, case.mask_qk, torch.zeros_like(case.kpm))
            assert attn_ref.rel_err(flipped[2], case.ref[2]) > 1e-3, "kpm changes the answer"


def test_an_all_blocked_query_is_detected():
    mask, kpm = attn_ref.decoder_masks(2, 3, 5, 7, 7)
    assert attn_ref.every_query_has_an_open_key(3, [5, 5], mask, kpm)
    kpm[1, :5] = True
    assert not attn_ref.every_query_has_an_open_key(3, [5, 5], mask, kpm)
    assert not attn_ref.every_query_has_an_open_key(3, [5, 0])


def test_layernorm_reference_agrees_with_torch():
    for d in attn_ref.LN_D:
        for m in attn_ref.LN_M:
            for mod in attn_ref.LN_MOD:
                x, g, b = attn_ref.layernorm_inputs(m, d, mod)
                assert x.shape == (mod or m, d)
                for eps in (1e-5, 1e-6):
                    want = F.layer_norm(x.double(), (d,), g.double(), b.double(), eps)
                    assert float((attn_ref.layernorm_ref(x, g, b, eps) - want).abs().max()) < 1e-12
