"""The RT-DETRv2 decoder's token kernels one at a time (yomitoku_amd/csrc/ymk_det.hip, ymk_elem.hip), each against a plain
float64 restatement on the CPU computed from the fp32 inputs the kernel received: query selection (k_topk_tokens), the query
gather (k_gather_queries), box refinement (k_refine_boxes), the masking of invalid-anchor tokens (k_mask_rows), multi-scale
deformable sampling (k_deform_sample), and the PResNet-vd shortcut pool / FPN up-sampling (k_avgpool2, k_nearest2).

Token rows are level-major across the images: row(b, t) = B * off[l] + b * h[l] * w[l] + (t - off[l]).  Every test gives each
image its own data, so a kernel that reads another image's rows fails."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

L640 = ((80, 80), (40, 40), (20, 20))
L960 = ((120, 120), (60, 60), (30, 30))
LODD = ((13, 7), (7, 4), (4, 2))


def _off(levels):
    hw = [h * w for h, w in levels]
    return hw, [0, hw[0], hw[0] + hw[1]], sum(hw)


def _rows(levels, B, b):
    """row of every token 0 .. ntok-1 of image b (level-major layout)."""
    hw, off, _ = _off(levels)
    return np.concatenate([B * off[l] + b * hw[l] + np.arange(hw[l]) for l in range(3)])


# ---------------------------------------------------------------------------------------------------------------- top-k
PATTERNS = ("normal", "equal", "masked_block", "ulp", "negative", "inf", "signed_zero")


def _scores(kind, n, k, rng):
    """the max-over-classes score of each of n tokens (float32) for one image."""
    if kind == "normal":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "equal":
        return np.full(n, 0.25, np.float32)
    if kind == "masked_block":  # the zeroed memory of invalid anchors: one LayerNorm(0) score shared by a block straddling the cut
        z = min(300, n // 2)
        above = max(0, min(k - z // 2, n - z))
        s = -rng.random(n).astype(np.float32)  # below the block
        perm = rng.permutation(n)
        s[perm[:above]] = 1.0 + rng.random(above).astype(np.float32)
        s[perm[above:above + z]] = 0.5
        return s
    if kind == "ulp":  # pairs of equal values, neighbouring pairs one ulp apart
        base = np.array(1.0, np.float32).view(np.uint32)
        return (base + (rng.permutation(n) // 2).astype(np.uint32)).view(np.float32)
    if kind == "negative":  # all negative, many ties (multiples of 1/8)
        return (-np.round(np.abs(rng.standard_normal(n)) * 8) / 8 - 0.125).astype(np.float32)
    if kind == "inf":
        s = rng.standard_normal(n).astype(np.float32)
        perm = rng.permutation(n)
        npos = max(1, k // 2)
        s[perm[:npos]] = np.inf
        s[perm[npos:npos + n // 4]] = -np.inf
        return s
    if kind == "signed_zero":  # a -0.0 / +0.0 tie across the cut, the -0.0 tokens having the lower ids
        p = k // 3
        z = min(n - p, k + 2)
        s = -(1.0 + rng.random(n)).astype(np.float32)
        perm = rng.permutation(n)
        s[perm[:p]] = 1.0 + rng.random(p).astype(np.float32)
        zeros = np.sort(perm[p:p + z])
        s[zeros[: z // 2]] = -0.0
        s[zeros[z // 2:]] = 0.0
        return s
    raise ValueError(kind)


def _logits_with_max(s, nc, rng):
    """[n, nc] float32 logits whose maximum over classes is exactly s (the other classes strictly below it)."""
    n = s.shape[0]
    lg = np.empty((n, nc), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        other = (s.astype(np.float64)[:, None] - 1.0 - np.abs(rng.standard_normal((n, nc)))).astype(np.float32)
    fin = np.isfinite(s)
    lg[fin] = other[fin]
    lg[s == np.inf] = rng.standard_normal((int((s == np.inf).sum()), nc)).astype(np.float32)
    lg[s == -np.inf] = -np.inf
    lg[np.arange(n), rng.integers(0, nc, n)] = s
    return lg


TOPK_CASES = [  # levels, B, K, nc
    (L640, 2, 300, 1),
    (L640, 2, 300, 6),
    (L640, 2, 300, 17),
    (L960, 1, 1500, 6),
    (L960, 1, 1500, 17),
    (LODD, 3, 1, 1),
    (LODD, 3, 37, 6),
    (LODD, 3, 37, 17),
    (LODD, 3, "N", 6),
]


@pytest.mark.parametrize("levels,B,K,nc", TOPK_CASES)
def test_topk_tokens_rank_order_is_exact(dev, levels, B, K, nc):
    """Expected: np.lexsort((token_id, -value)) of the float64 max over classes - descending value, lowest id among equal
    values (-0.0 equal to +0.0) - the first K, exactly.  Every score pattern is the pattern of image 0 once, the other images
    taking the next patterns, so a mix-up of the level-major rows of two images cannot pass."""
    from tests import hipops

    _, _, ntok = _off(levels)
    K = ntok if K == "N" else K
    rng = np.random.default_rng(1000 + ntok + K + nc)
    for start in range(len(PATTERNS)):
        logits = np.empty((B * ntok, nc), np.float32)
        want = []
        for b in range(B):
            lg = _logits_with_max(_scores(PATTERNS[(start + b) % len(PATTERNS)], ntok, K, rng), nc, rng)
            logits[_rows(levels, B, b)] = lg
            m = lg.astype(np.float64).max(axis=1)
            want.append(np.lexsort((np.arange(ntok), -m))[:K])
        got = hipops.topk_tokens(torch.from_numpy(logits).to(dev), B, levels, K).cpu().numpy()
        for b in range(B):
            bad = np.flatnonzero(got[b] != want[b])
            print(f"{PATTERNS[(start + b) % len(PATTERNS)]:>12} image {b}: {bad.size} of {K} ranks differ")
            assert bad.size == 0, (PATTERNS[(start + b) % len(PATTERNS)], b, bad[:5], got[b][bad[:5]], want[b][bad[:5]])


# ---------------------------------------------------------------------------------------------------------------- gather
def test_gather_queries_copies_rows_and_sigmoids_boxes(dev):
    """content is the selected token's row of the encoder output, bit for bit; ref = sigmoid(bbox + anchor) within 1e-7 of
    float64: the kernel's fp32 sum, expf (1 ulp) and reciprocal each move a result in (0, 1) by at most 2^-24-ish, three of
    them 9e-8 at the worst point.  An anchor of +inf (an invalid anchor that got selected) gives exactly 1.0."""
    from tests import hipops

    levels, B, K, D = LODD, 3, 37, 256
    _, _, ntok = _off(levels)
    g = torch.Generator().manual_seed(21)
    om = torch.randn(B * ntok, D, generator=g)
    bbox = torch.randn(B * ntok, 4, generator=g) * 3
    anchors = torch.randn(ntok, 4, generator=g) * 2
    inv = torch.randperm(ntok, generator=g)[: ntok // 3]
    anchors[inv] = float("inf")
    idx = torch.stack([torch.randperm(ntok, generator=g)[:K] for _ in range(B)]).int()
    idx[:, 0] = inv[:B].int()  # every image selects an invalid anchor
    content, ref = hipops.gather_queries(om.to(dev), bbox.to(dev), anchors.to(dev), idx.to(dev), levels)
    content, ref = content.cpu(), ref.cpu()
    rows = torch.from_numpy(np.stack([_rows(levels, B, b) for b in range(B)]))
    src_rows = torch.gather(rows, 1, idx.long())
    assert torch.equal(content, om[src_rows])
    want = torch.sigmoid(bbox.double()[src_rows] + anchors.double()[idx.long()])
    err = (ref.double() - want).abs().max().item()
    print(f"gather: max|ref - fp64| = {err:.2e}")
    assert err < 1e-7
    is_inf = torch.isinf(anchors[idx.long()])
    assert is_inf.any() and bool((ref[is_inf] == 1.0).all())


# ---------------------------------------------------------------------------------------------------------------- refine
def _inverse_sigmoid(x, eps=1e-5):  # rtdetrv2_decoder.inverse_sigmoid
    x = x.clip(min=0.0, max=1.0)
    return torch.log(x.clip(min=eps) / (1 - x).clip(min=eps))


def test_refine_boxes_matches_inverse_sigmoid_clip(dev):
    """sigmoid(delta + inverse_sigmoid(ref)) with the 1e-5 clip, over ref in {0, 1e-6, 0.5, 1-1e-6, 1, -0.1, 1.1} and delta in
    [-100, 100] (with a dense band around -11.5, where the clip decides the answer for ref = 1), n = 1 200 003: past the 4096-block
    grid cap, so the grid-stride loop runs.  Tolerance 1e-6 absolute: the fp32 logf is good to about 1 ulp of |log| <= 11.52
    (9.5e-7), the quotient and 1 - x add 2^-24 each, the sum delta + log rounds by 2^-24 |z| where sigmoid'(z) |z| < 0.23, and the
    derivative of the outer sigmoid is at most 1/4; expf and the reciprocal add 2^-23 - about 4e-7 in all."""
    from tests import hipops

    n = 1_200_003
    g = torch.Generator().manual_seed(5)
    refs = torch.tensor([0.0, 1e-6, 0.5, 1 - 1e-6, 1.0, -0.1, 1.1], dtype=torch.float32)
    ref = refs[torch.randint(0, len(refs), (n,), generator=g)]
    delta = torch.rand(n, generator=g) * 200 - 100
    band = torch.rand(n, generator=g) < 0.3
    delta[band] = -11.5 + (torch.rand(int(band.sum()), generator=g) - 0.5) * 0.2
    delta[:7], ref[:7] = -11.5, refs  # the exact point, once per reference value
    out = hipops.refine_boxes(delta.to(dev), ref.to(dev)).cpu()
    want = torch.sigmoid(delta.double() + _inverse_sigmoid(ref.double()))
    err = (out.double() - want).abs()
    print(f"refine: max|out - fp64| = {err.max().item():.2e}")
    assert err.max().item() < 1e-6


# ---------------------------------------------------------------------------------------------------------------- mask
def test_mask_rows_zeroes_invalid_tokens_of_every_image(dev):
    """out[row(b, t)] = valid[t] * in[row(b, t)], exactly, for three images over odd level grids."""
    from tests import hipops

    levels, B, D = LODD, 3, 256
    _, _, ntok = _off(levels)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B * ntok, D, generator=g)
    valid = (torch.rand(ntok, generator=g) < 0.6).float()
    out = hipops.mask_rows(x.to(dev), valid.to(dev), B, levels).cpu()
    want = torch.empty_like(x)
    for b in range(B):
        r = torch.from_numpy(_rows(levels, B, b))
        want[r] = x[r] * valid[:, None]
    assert torch.equal(out, want)
    assert 0 < int(valid.sum()) < ntok


# ---------------------------------------------------------------------------------------------------------------- deformable sampling
def _deform_reference(offs, attw, ref, value, levels, B, K):
    """deformable_attention_core_func_v2(method="default") in float64, with the sampling locations of
    MSDeformableAttention.forward for 4-d reference points: loc = ref[:2] + off * (1/4) * ref[2:] * 0.5.
    value [B, ntok, 8, 32] (token order within each image); offs [B*K, 8, 12, 2]; attw [B*K, 8, 12]; ref [B*K, 4]."""
    hw, off, _ = _off(levels)
    offs = offs.double().reshape(B, K, 8, 12, 2)
    w = torch.softmax(attw.double().reshape(B, K, 8, 12), dim=-1)
    r = ref.double().reshape(B, K, 1, 1, 4)
    loc = r[..., :2] + offs * 0.25 * r[..., 2:] * 0.5
    grid = (2 * loc - 1).permute(0, 2, 1, 3, 4).reshape(B * 8, K, 12, 2)
    v = value.double()
    samples = []
    for l, (h, wd) in enumerate(levels):
        vl = v[:, off[l]:off[l] + hw[l]].permute(0, 2, 3, 1).reshape(B * 8, 32, h, wd)
        samples.append(F.grid_sample(vl, grid[:, :, 4 * l:4 * l + 4], mode="bilinear", padding_mode="zeros", align_corners=False))
    s = torch.cat(samples, dim=-1)  # [B*8, 32, K, 12]
    aw = w.permute(0, 2, 1, 3).reshape(B * 8, 1, K, 12)
    return (s * aw).sum(-1).reshape(B, 8 * 32, K).permute(0, 2, 1).reshape(B * K, 256)


def _deform_inputs(levels, B, K, g):
    """offsets, logits and reference boxes with the rows the product really produces among random ones."""
    M = B * K
    ref = torch.rand(M, 4, generator=g) * 0.9 + 0.05
    offs = torch.randn(M, 8, 12, 2, generator=g) * 2
    attw = torch.randn(M, 8, 12, generator=g) * 2
    for b in range(B):
        q = b * K
        ref[q] = 1.0                                                   # a selected invalid anchor: sigmoid(inf) = 1
        if K > 1:
            ref[q + 1, :2] = 0.0                                       # (0, 0, w, h)
        if K > 2:
            ref[q + 2] = torch.tensor([0.5, 0.5, 1.0, 1.0])            # offsets +-4 land exactly on the -0.5 / W - 0.5 borders
            offs[q + 2] = torch.tensor([4.0, -4.0])[torch.randint(0, 2, (8, 12, 2), generator=g)]
        if K > 3:                                                      # pixel centres: loc = off / 8 = (p + 0.5) / W
            ref[q + 3] = torch.tensor([0.0, 0.0, 1.0, 1.0])
            for p in range(12):
                h, w = levels[p // 4]
                offs[q + 3, :, p, 0] = 8 * (torch.randint(0, w, (8,), generator=g) + 0.5) / w
                offs[q + 3, :, p, 1] = 8 * (torch.randint(0, h, (8,), generator=g) + 0.5) / h
        if K > 4:                                                      # far outside: |ix| up to about 1e4 pixels
            ref[q + 4] = torch.tensor([0.5, 0.5, 1.0, 1.0])
            offs[q + 4] = (torch.rand(8, 12, 2, generator=g) * 2 - 1) * 8e4 / 80
        if K > 5:
            attw[q + 5] = torch.tensor([80.0, -80.0])[torch.randint(0, 2, (8, 12), generator=g)]  # softmax stability
        if K > 6:
            attw[q + 6] = 80.0 + torch.randn(8, 12, generator=g) * 1e-3
    return offs, attw, ref


DEFORM_CASES = [  # levels, B, K, layer (column offset / 256 of the value buffer)
    (L640, 1, 300, 0),
    (L640, 3, 300, 5),
    (L640, 3, 7, 0),
    (L640, 1, 7, 5),
    (L960, 1, 300, 5),
    (L960, 3, 7, 0),
    (LODD, 3, 300, 0),
    (LODD, 1, 7, 5),
    (LODD, 3, 7, 5),
]


@pytest.mark.parametrize("levels,B,K,layer", DEFORM_CASES)
def test_deform_sample_matches_grid_sample(dev, levels, B, K, layer):
    """F.grid_sample(bilinear, zeros, align_corners=False) of every head / level / point, soft-max weighted, in float64.
    Tolerance 1e-4 max|value|: the fp32 sample coordinate ix = ((2 loc - 1 + 1) W - 1) / 2 carries a few roundings of 2^-24 times
    max(|ix|, W) <= 1.3e4 px wherever a tap is in range - < 4e-5 px at the grids here, out-of-range taps being zero either way -
    and bilinear sampling moves by at most 2 max|value| per pixel (the soft-max weights sum to one: 8e-5 max|value|); the fp32
    weights and the sum of 12 points add 2^-20 max|value|.  Also: the output is bit-identical on repeat, and new values for
    the other images leave an image's output bit-identical.  The value buffer is [rows][6 * 256] as in the model, its other
    layers NaN: a read outside the layer's 256 columns poisons the result."""
    from tests import hipops

    _, _, ntok = _off(levels)
    g = torch.Generator().manual_seed(31 + ntok + B * 7 + K)
    offs, attw, ref = _deform_inputs(levels, B, K, g)
    value = torch.randn(B, ntok, 256, generator=g)
    value[:, :, 128:] *= 3.0  # heads differ in scale
    rows = torch.from_numpy(np.stack([_rows(levels, B, b) for b in range(B)]))

    def upload(v):
        buf = torch.full((B * ntok, 6 * 256), float("nan"))
        for b in range(B):
            buf[rows[b], layer * 256:(layer + 1) * 256] = v[b]
        return buf.to(dev)

    buf = upload(value)
    d_offs, d_attw, d_ref = offs.to(dev), attw.to(dev), ref.to(dev)
    out = hipops.deform_sample(d_offs, d_attw, d_ref, buf, layer * 256, B, levels, K).cpu()
    want = _deform_reference(offs, attw, ref, value.reshape(B, ntok, 8, 32), levels, B, K)
    scale = value.abs().max().item()
    err = (out.double() - want).abs().max().item() / scale
    print(f"deform {levels[0]} B={B} K={K} layer {layer}: max|out - fp64| / max|value| = {err:.2e}")
    assert err < 1e-4
    again = hipops.deform_sample(d_offs, d_attw, d_ref, buf, layer * 256, B, levels, K).cpu()
    assert torch.equal(out, again), "bit-identical on repeat"
    if B == 3:
        other = value.clone()
        other[0] = torch.randn(ntok, 256, generator=g)
        other[2] = torch.randn(ntok, 256, generator=g) * 5
        out2 = hipops.deform_sample(d_offs, d_attw, d_ref, upload(other), layer * 256, B, levels, K).cpu()
        assert torch.equal(out2[K:2 * K], out[K:2 * K]), "image 1 must not see images 0 and 2"
        assert not torch.equal(out2[:K], out[:K])


# ---------------------------------------------------------------------------------------------------------------- pool / up-sample
POOL_SHAPES = [(2, 4, 1, 1), (2, 64, 8, 6), (2, 64, 7, 9), (2, 260, 11, 4), (2, 4, 1, 10), (2, 260, 5, 1), (2, 64, 40, 41)]


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_avgpool2x2_ceil_and_nearest2x(dev, shape):
    """AvgPool2d(2, 2, 0, ceil_mode=True) (the divisor counts only the taps inside: 4, 2 or 1) within 1e-6 max|x| - at most three
    fp32 additions of terms <= max|x| and an exact division by a power of two, 3 * 2^-24 * 4 / 4 = 1.8e-7 - and nearest x2
    exactly, over even / odd / 1-pixel sizes."""
    from tests import hipops

    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g)
    x[1] += 4.0  # the images differ
    y = hipops.avgpool2x2_ceil(x.to(dev)).cpu()
    want = F.avg_pool2d(x.double(), 2, 2, 0, ceil_mode=True)
    assert y.shape == want.shape
    err = (y.double() - want).abs().max().item() / x.abs().max().item()
    print(f"avgpool {shape}: {err:.2e}")
    assert err < 1e-6
    up = hipops.upsample_nearest2x(x.to(dev)).cpu()
    assert torch.equal(up, F.interpolate(x, scale_factor=2, mode="nearest"))
