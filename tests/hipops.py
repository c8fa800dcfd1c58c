"""Thin Python entry points to single HIP operators of libymk_hip.so (NHWC fp32 on device).

They exist so the parity tests can exercise exactly the kernels the models use, one at a time.
Inputs/outputs here are NCHW torch tensors on a HIP device; the layout change is done with torch.
"""

from __future__ import annotations

import torch

from yomitoku_amd import _lib

ACT = {"none": 0, "relu": 1, "silu": 2, "sigmoid": 3, "gelu": 4}


def _nhwc(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 3, 1, 2).contiguous()


def conv2d(x, weight, scale=None, bias=None, residual=None, stride=1, padding=0, dilation=1, act="none"):
    """y = act(scale * conv(x, weight) + bias + residual); x NCHW on device, weight OIHW (any device)."""
    lib = _lib.load()
    assert x.is_cuda
    n, c, h, w = x.shape
    cout, cin, kh, kw = weight.shape
    assert cin == c
    tap4 = c <= 4
    xh = _nhwc(x.float())
    if tap4 and c < 4:
        xh = torch.cat([xh, xh.new_zeros(n, h, w, 4 - c)], dim=-1).contiguous()
    cpad = xh.shape[-1]
    if not tap4 and cpad % 4:
        raise ValueError("channels must be a multiple of 4")
    oh = (h + 2 * padding - dilation * (kh - 1) - 1) // stride + 1
    ow = (w + 2 * padding - dilation * (kw - 1) - 1) // stride + 1
    y = torch.empty((n, oh, ow, cout), dtype=torch.float32, device=x.device)
    wh = weight.detach().float().cpu().contiguous()
    sh = scale.detach().float().cpu().contiguous() if scale is not None else None
    bh = bias.detach().float().cpu().contiguous() if bias is not None else None
    rh = _nhwc(residual.float()) if residual is not None else None
    with torch.cuda.device(x.device):
        _lib.check(
            lib.ymk_op_conv2d(
                xh.data_ptr(), n, h, w, cpad, wh.data_ptr(), cout, cin, kh, kw, _lib.ptr(sh), _lib.ptr(bh),
                _lib.ptr(rh), stride, padding, dilation, ACT[act], 1 if tap4 else 0, y.data_ptr(),
                _lib.current_stream_ptr(),
            ),
            "ymk_op_conv2d",
        )
    return _nchw(y)


SENTINEL = 0x7FA5A5A5  # what conv2d_view pre-fills its output buffer with: a NaN bit pattern no kernel produces
AMAX_REC_WORDS = 1024  # a max|x| record: 32 lines of 32 words, the value in word 0 of each line (csrc/ymk_common.h)


def amax_record(value, device):
    """A caller-filled max|x| record holding `value` (as absmax_record leaves it: word 0, the rest zero)."""
    rec = torch.zeros(AMAX_REC_WORDS, dtype=torch.int32)
    rec[0] = torch.tensor(abs(float(value)), dtype=torch.float32).view(torch.int32)
    return rec.to(device)


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def _into_view(t_nhwc, view):
    """t [..., c] -> (whole NaN-filled buffer [..., ld] with t at channels c0 .., the view's first-channel address)."""
    c0, ld = view
    c = t_nhwc.shape[-1]
    assert 0 <= c0 and c0 + c <= ld
    buf = torch.full(t_nhwc.shape[:-1] + (ld,), float("nan"), dtype=torch.float32, device=t_nhwc.device)
    buf[..., c0:c0 + c] = t_nhwc
    return buf, buf.data_ptr() + 4 * c0


def conv2d_view(x, weight, scale=None, bias=None, residual=None, stride=1, padding=0, dilation=1, act="none", res_post=False,
                in_view=None, out_view=None, res_view=None, row_group=None, group_open=None, amax_in=None, record=False):
    """ymk_op_conv2d_view: conv2d with leading dimensions, a rectangular stride, the residual on either side of the activation,
    a row predicate and records.  x NCHW on the device, weight OIHW; stride an int or (vertical, horizontal).
    *_view = (first channel, leading dimension) of the tensor inside a wider NHWC buffer allocated here (default: contiguous):
    inputs and residuals get NaN outside the view, the output SENTINEL everywhere.  residual: NCHW like the output, or a [cout]
    vector = one row broadcast to every pixel (res_ld 0).  row_group [M] / group_open [groups]: int32 on the device.
    -> (y NCHW: the output view, the whole output buffer [n, oh, ow, out_ld], the output's record as int32 [1024] or None)."""
    lib = _lib.load()
    assert x.is_cuda
    n, c, h, w = x.shape
    cout, cin, kh, kw = weight.shape
    assert cin == c
    tap4 = c <= 4
    xh = _nhwc(x.float())
    wh = weight.detach().float().cpu().contiguous()
    if tap4 and c < 4:  # the 4-channel stem form: the image and the weights zero padded to four channels
        xh = torch.cat([xh, xh.new_zeros(n, h, w, 4 - c)], dim=-1).contiguous()
        wh = torch.cat([wh, wh.new_zeros(cout, 4 - c, kh, kw)], dim=1).contiguous()
    cpad = xh.shape[-1]
    sh_, sw_ = _pair(stride)
    oh = (h + 2 * padding - dilation * (kh - 1) - 1) // sh_ + 1
    ow = (w + 2 * padding - dilation * (kw - 1) - 1) // sw_ + 1
    xbuf, xptr = _into_view(xh, in_view or (0, cpad))
    oc0, out_ld = out_view or (0, cout)
    assert 0 <= oc0 and oc0 + cout <= out_ld
    ybuf = torch.empty((n, oh, ow, out_ld), dtype=torch.float32, device=x.device)
    ybuf.view(torch.int32).fill_(SENTINEL)
    sh = scale.detach().float().cpu().contiguous() if scale is not None else None
    bh = bias.detach().float().cpu().contiguous() if bias is not None else None
    rbuf, rptr, res_ld = None, None, 0
    if residual is not None and residual.dim() == 1:
        assert residual.numel() == cout
        rbuf, rptr = _into_view(residual.float().to(x.device).reshape(1, cout), res_view or (0, cout))
    elif residual is not None:
        assert tuple(residual.shape) == (n, cout, oh, ow)
        rbuf, rptr = _into_view(_nhwc(residual.float().to(x.device)), res_view or (0, cout))
        res_ld = rbuf.shape[-1]
    rg, go = _i32(row_group, x.device), _i32(group_open, x.device)
    if rg is not None:
        assert rg.numel() == n * oh * ow and 0 <= int(rg.min()) and int(rg.max()) < go.numel()  # the kernel trusts its indices
    rec = torch.zeros(AMAX_REC_WORDS, dtype=torch.int32, device=x.device) if record else None
    if amax_in is not None:
        assert amax_in.is_cuda and amax_in.dtype == torch.int32 and amax_in.numel() == AMAX_REC_WORDS
    with torch.cuda.device(x.device):
        _lib.check(
            lib.ymk_op_conv2d_view(xptr, n, h, w, cpad, xbuf.shape[-1], wh.data_ptr(), cout, kh, kw, 1 if tap4 else 0, _lib.ptr(sh),
                                   _lib.ptr(bh), rptr, res_ld, 1 if res_post else 0, sh_, sw_, padding, dilation, ACT[act],
                                   _lib.ptr(rg), _lib.ptr(go), _lib.ptr(amax_in), _lib.ptr(rec), ybuf.data_ptr() + 4 * oc0, out_ld,
                                   _lib.current_stream_ptr()),
            "ymk_op_conv2d_view",
        )
    return _nchw(ybuf[..., oc0:oc0 + cout]), ybuf, rec


def conv_planes_pair(x, w1, w2, p1=None, p2=None, amax_in=None):
    """ymk_op_conv_planes_pair: y = conv2(conv1(x)) under the fp16-split form, the intermediate as fp16 planes where the pair
    qualifies.  x NCHW on the device; w1 / w2 OIHW; p1 / p2: dicts of stride, padding, dilation (ints), act, scale, bias,
    residual (NCHW).  -> (y NCHW, the raw intermediate [n, h1, w1, cout1] fp32 words on the device - planes or values -, its
    record int32 [1024], planes_taken, pl_a, pl_b)."""
    import ctypes

    lib = _lib.load()
    assert x.is_cuda
    n, c, h, w = x.shape
    xh = _nhwc(x.float())
    keep, args, dims = [], [], []
    hh, ww = h, w
    for wt, p in ((w1, p1 or {}), (w2, p2 or {})):
        cout, _, kh, kw = wt.shape
        st, pad, dil = int(p.get("stride", 1)), int(p.get("padding", 0)), int(p.get("dilation", 1))
        hh = (hh + 2 * pad - dil * (kh - 1) - 1) // st + 1
        ww = (ww + 2 * pad - dil * (kw - 1) - 1) // st + 1
        host = [wt.detach().float().cpu().contiguous()]
        host += [p[k].detach().float().cpu().contiguous() if p.get(k) is not None else None for k in ("scale", "bias")]
        res = _nhwc(p["residual"].float().to(x.device)) if p.get("residual") is not None else None
        if res is not None:
            assert tuple(res.shape) == (n, hh, ww, cout)
        keep += host + [res]
        args += [host[0].data_ptr(), cout, kh, kw, st, pad, dil, ACT[p.get("act", "none")], _lib.ptr(host[1]), _lib.ptr(host[2]), _lib.ptr(res)]
        dims.append((n, hh, ww, cout))
    assert w1.shape[1] == c and w2.shape[1] == w1.shape[0]
    mid = torch.empty(dims[0], dtype=torch.float32, device=x.device)
    mid.view(torch.int32).fill_(SENTINEL)
    y = torch.empty(dims[1], dtype=torch.float32, device=x.device)
    rec = torch.zeros(AMAX_REC_WORDS, dtype=torch.int32, device=x.device)
    if amax_in is not None:
        assert amax_in.is_cuda and amax_in.dtype == torch.int32 and amax_in.numel() == AMAX_REC_WORDS
    taken, pl_a, pl_b = ctypes.c_int(-1), ctypes.c_float(), ctypes.c_float()
    with torch.cuda.device(x.device):
        _lib.check(lib.ymk_op_conv_planes_pair(xh.data_ptr(), n, h, w, c, _lib.ptr(amax_in), *args, mid.data_ptr(), rec.data_ptr(),
                                               y.data_ptr(), ctypes.byref(taken), ctypes.byref(pl_a), ctypes.byref(pl_b),
                                               _lib.current_stream_ptr()), "ymk_op_conv_planes_pair")
    return _nchw(y), mid, rec, int(taken.value), float(pl_a.value), float(pl_b.value)


def conv1x1_astat(x, weight, scale=None, bias=None, residual=None, act="none", reps=1, ln=None):
    """The A-stationary kernel at any row count (ymk_op_conv1x1_astat): x [M, C] on the device, weight [Cout, C] -> (y [M, Cout],
    ms of the last of `reps` launches).  ln = (gamma [C], beta [C], eps): LayerNorm folded into the operand load."""
    import ctypes

    lib = _lib.load()
    assert x.is_cuda and x.dim() == 2
    m, c = x.shape
    cout = weight.shape[0]
    xh = x.float().contiguous()
    wh = weight.detach().float().cpu().contiguous()
    sh = scale.detach().float().cpu().contiguous() if scale is not None else None
    bh = bias.detach().float().cpu().contiguous() if bias is not None else None
    rh = residual.float().contiguous() if residual is not None else None
    gh = ln[0].detach().float().cpu().contiguous() if ln is not None else None
    beh = ln[1].detach().float().cpu().contiguous() if ln is not None else None
    y = torch.empty((m, cout), dtype=torch.float32, device=x.device)
    ms = ctypes.c_float()
    with torch.cuda.device(x.device):
        _lib.check(lib.ymk_op_conv1x1_astat(xh.data_ptr(), m, c, wh.data_ptr(), cout, _lib.ptr(sh), _lib.ptr(bh), _lib.ptr(rh), ACT[act],
                                            _lib.ptr(gh), _lib.ptr(beh), float(ln[2]) if ln is not None else 0.0,
                                            y.data_ptr(), reps, ctypes.byref(ms), _lib.current_stream_ptr()), "ymk_op_conv1x1_astat")
    return y, float(ms.value)


def vit_mlp(x, gamma, beta, eps, w1, b1, w2, b2, reps=1):
    """ymk_op_vit_mlp: x [M, D] on the device -> (x + fc2(gelu(fc1(layer_norm(x)))) [M, D], ms of the last launch)."""
    import ctypes

    lib = _lib.load()
    m, d = x.shape
    f = w1.shape[0]
    xh = x.float().contiguous()
    host = [t.detach().float().cpu().contiguous() for t in (gamma, beta, w1, b1, w2, b2)]
    y = torch.empty_like(xh)
    ms = ctypes.c_float()
    with torch.cuda.device(x.device):
        _lib.check(lib.ymk_op_vit_mlp(xh.data_ptr(), m, d, f, host[0].data_ptr(), host[1].data_ptr(), float(eps), host[2].data_ptr(),
                                      host[3].data_ptr(), host[4].data_ptr(), host[5].data_ptr(), y.data_ptr(), reps, ctypes.byref(ms),
                                      _lib.current_stream_ptr()), "ymk_op_vit_mlp")
    return y, float(ms.value)


def maxpool3x3s2(x):
    lib = _lib.load()
    n, c, h, w = x.shape
    xh = _nhwc(x.float())
    y = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(
            lib.ymk_op_maxpool3x3s2(xh.data_ptr(), n, h, w, c, y.data_ptr(), _lib.current_stream_ptr()),
            "ymk_op_maxpool3x3s2",
        )
    return _nchw(y)


def upsample_bilinear(x, size, add=None):
    lib = _lib.load()
    n, c, h, w = x.shape
    oh, ow = size
    xh = _nhwc(x.float())
    ah = _nhwc(add.float()) if add is not None else None
    y = torch.empty((n, oh, ow, c), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(
            lib.ymk_op_upsample_bilinear(
                xh.data_ptr(), n, h, w, c, oh, ow, _lib.ptr(ah), y.data_ptr(), _lib.current_stream_ptr()
            ),
            "ymk_op_upsample_bilinear",
        )
    return _nchw(y)


def layernorm(x, weight, bias, eps):
    lib = _lib.load()
    d = x.shape[-1]
    xs = x.float().contiguous()
    y = torch.empty_like(xs)
    g = weight.float().to(x.device).contiguous()
    b = bias.float().to(x.device).contiguous()
    with torch.cuda.device(x.device):
        _lib.check(
            lib.ymk_op_layernorm(xs.data_ptr(), xs.numel() // d, d, g.data_ptr(), b.data_ptr(), float(eps), y.data_ptr(),
                                 _lib.current_stream_ptr()),
            "ymk_op_layernorm",
        )
    return y


def attention(q, k, v, heads, scale=None, mask_qk=None, key_padding_mask=None, use_small=False):
    """q [B, Lq, D], k/v [B, Lk, D] on device -> [B, Lq, D]; masks are bool tensors (True = blocked)."""
    lib = _lib.load()
    b, lq, d = q.shape
    lk = k.shape[1]
    hd = d // heads
    scale = hd**-0.5 if scale is None else scale
    qs, ks, vs = q.float().contiguous(), k.float().contiguous(), v.float().contiguous()
    o = torch.empty_like(qs)
    m = mask_qk.to(device=q.device, dtype=torch.uint8).contiguous() if mask_qk is not None else None
    kp = key_padding_mask.to(device=q.device, dtype=torch.uint8).contiguous() if key_padding_mask is not None else None
    with torch.cuda.device(q.device):
        _lib.check(
            lib.ymk_op_attention(qs.data_ptr(), ks.data_ptr(), vs.data_ptr(), o.data_ptr(), b, heads, lq, lk, hd,
                                 float(scale), _lib.ptr(m), _lib.ptr(kp), 1 if use_small else 0,
                                 _lib.current_stream_ptr()),
            "ymk_op_attention",
        )
    return o


def layernorm_view(x, weight, bias, eps, m, x_view=None, y_view=None, in_rows_mod=0):
    """ymk_op_layernorm_view: x [in_rows_mod or m, D] on the device -> (y [m, D]: the output view, the whole output buffer
    [m, ldy]).  *_view = (first column, leading dimension) inside a wider buffer allocated here: NaN beside the input view,
    SENTINEL in every word of the output buffer.  in_rows_mod > 0: output row r reads input row r % in_rows_mod."""
    lib = _lib.load()
    assert x.is_cuda and x.dim() == 2
    rows_in, d = x.shape
    assert rows_in == (in_rows_mod or m)
    xbuf, xptr = _into_view(x.float(), x_view or (0, d))
    yc0, ldy = y_view or (0, d)
    assert 0 <= yc0 and yc0 + d <= ldy
    for c0, ld in ((x_view or (0, d)), (yc0, ldy)):  # the kernel moves 16-byte words
        assert c0 % 4 == 0 and ld % 4 == 0 and d % 4 == 0 and d <= 1024
    ybuf = torch.empty((m, ldy), dtype=torch.float32, device=x.device)
    ybuf.view(torch.int32).fill_(SENTINEL)
    g = weight.float().to(x.device).contiguous()
    b = bias.float().to(x.device).contiguous()
    with torch.cuda.device(x.device):
        _lib.check(lib.ymk_op_layernorm_view(xptr, xbuf.shape[-1], in_rows_mod, m, d, g.data_ptr(), b.data_ptr(), float(eps),
                                             ybuf.data_ptr() + 4 * yc0, ldy, _lib.current_stream_ptr()), "ymk_op_layernorm_view")
    return ybuf[:, yc0:yc0 + d].clone(), ybuf


def nar_cross_attention(q, ks, vs, heads, device, scale=None):
    """ymk_op_nar_cross_attention on contiguous operands: q [lq, D] shared by the batch, ks / vs lists of per-sample [lk_i, D]
    laid end to end and found through the (koff, klen) tables -> list of [lq, D] device tensors."""
    lib = _lib.load()
    b, (lq, d) = len(ks), q.shape
    hd = d // heads
    lens = [int(k.shape[0]) for k in ks]
    assert heads <= 8 and hd <= 96 and min(lens) >= 1
    qd = q.float().to(device).contiguous()
    kd, vd = (torch.cat([t.float() for t in ts]).to(device).contiguous() for ts in (ks, vs))
    off = [sum(lens[:i]) for i in range(b)]
    koff, klen = (torch.tensor(t, dtype=torch.int32, device=device) for t in (off, lens))
    o = torch.empty((b, lq, d), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.check(lib.ymk_op_nar_cross_attention(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), b, heads, lq, max(lens), hd,
                                                  float(hd**-0.5 if scale is None else scale), koff.data_ptr(), klen.data_ptr(),
                                                  _lib.current_stream_ptr()), "ymk_op_nar_cross_attention")
    return list(o)


ATTN_KERNELS = {"flash": 0, "small": 1, "nar": 2}
# which operands share one buffer: the PARSeq encoder's [.., 3D] rows, RT-DETR's [.., 2D] q|k with its own v, the decoders'
# q with the [.., 2D] k|v of memkv / skv, and three buffers
ATTN_PACKS = {"qkv": ("A", "A", "A"), "qk": ("A", "A", "V"), "kv": ("Q", "A", "A"), "sep": ("Q", "K", "V")}


def _row_layout(caps, rowgap, table, order=None):
    """Row offsets of the samples of a buffer holding caps[i] rows of sample i, `rowgap` spare rows after each (and before the
    first, with tables): the uniform form - equal caps, one batch stride - or, with tables, the samples in `order`.
    -> (offsets, rows of the buffer)"""
    b = len(caps)
    if not table:
        assert len(set(caps)) == 1, "the uniform form has one length"
        return [i * (caps[0] + rowgap) for i in range(b)], b * (caps[0] + rowgap)
    off, r = [0] * b, rowgap
    for i in (order if order is not None else range(b)):
        off[i] = r
        r += caps[i] + rowgap
    return off, r


def attention_view(kernel, qs, ks, vs, heads, device, scale=None, pack="sep", colgap=0, rowgap=1, q_tab=False, k_tab=False, order=None,
                   o_view=None, mask_qk=None, kpm=None, amax=(None, None, None)):
    """ymk_op_attention_view: one launch of flash_attention / small_attention / nar_cross_attention ("flash" / "small" / "nar")
    with the strides, tables, masks and records a model passes.  qs: a list of per-sample [lq_i, D] tensors, or ONE [lq, D]
    table for the whole batch (bsq = 0; always so for "nar"); ks / vs: lists of [lk_i, D] (CPU or device, fp32).
    pack (ATTN_PACKS) puts operands side by side in one buffer, `colgap` spare columns after each; samples follow each other
    with `rowgap` spare rows - at one batch stride, or with q_tab / k_tab at the rows of int32 offset / length tables (samples
    placed in `order`; lengths may then differ).  Operands that share a buffer share its rows: a sample gets max(lq_i, lk_i) of
    them.  o_view = (first column, leading dimension) of the output, whose rows follow the queries'.  mask_qk [lq, ld_mask] /
    kpm [b, ld_kpm]: bool, True = blocked.  amax: the max|x| records of q, k, v (amax_record; None = absent).
    Every spare word of an operand buffer is NaN, every word of the output buffer SENTINEL before the launch.
    -> (outs: per-sample [lq_i, D] device tensors, the whole output buffer [rows, ldo], written: bool [rows, ldo] on the CPU,
    True where the launch has to store)."""
    lib = _lib.load()
    kid = ATTN_KERNELS[kernel]
    b = len(ks)
    shared_q = torch.is_tensor(qs)
    assert shared_q or kernel != "nar"
    d = ks[0].shape[1]
    hd = d // heads
    assert hd * heads == d and len(vs) == b and (shared_q or len(qs) == b)
    lks = [int(k.shape[0]) for k in ks]
    lqs = [int(qs.shape[0])] * b if shared_q else [int(q.shape[0]) for q in qs]
    assert all(v.shape == k.shape for k, v in zip(ks, vs)) and min(lks) >= 1 and min(lqs) >= 1
    scale = hd**-0.5 if scale is None else float(scale)
    names = ATTN_PACKS[pack]
    share = names[0] == names[1]
    assert not (share and shared_q) and (not share or q_tab == k_tab) and not (shared_q and q_tab)
    assert (q_tab or len(set(lqs)) == 1) and (k_tab or len(set(lks)) == 1), "lengths differ only under tables"
    # what the kernels trust
    if kernel == "nar":
        assert heads <= 8 and hd <= 96
    if kernel == "small" or (kernel == "flash" and hd not in (32, 48, 64, 96)):
        assert max(lks) <= 1024 and hd <= 128
    if kernel != "small":
        assert mask_qk is None and kpm is None
    assert not ((q_tab or k_tab) and (mask_qk is not None or kpm is not None)), "ragged batches come without masks"

    # columns: operand j of a buffer at j * (D + colgap)
    col, ld = {}, {}
    for op, name in zip("qkv", names):
        col[op] = ld.get(name, 0)
        ld[name] = col[op] + d + colgap
    # rows: the key side (k, v) and the query side (q, o) - one and the same where q and k share a buffer
    kcaps = [max(a, c) for a, c in zip(lqs, lks)] if share else lks
    koff, krows = _row_layout(kcaps, rowgap, k_tab, order)
    if share:
        qoff, qrows = koff, krows
    elif shared_q:
        qoff, qrows = [0] * b, lqs[0]
    else:
        qoff, qrows = _row_layout(lqs, rowgap, q_tab, order)
    ooff, orows = _row_layout(lqs, rowgap, False) if shared_q else (qoff, qrows)
    bufs = {name: torch.full((qrows if name == "Q" else krows, ld[name]), float("nan"), dtype=torch.float32) for name in set(names)}
    for i in range(b):
        if not shared_q:
            bufs[names[0]][qoff[i]:qoff[i] + lqs[i], col["q"]:col["q"] + d] = qs[i].float().cpu()
        bufs[names[1]][koff[i]:koff[i] + lks[i], col["k"]:col["k"] + d] = ks[i].float().cpu()
        bufs[names[2]][koff[i]:koff[i] + lks[i], col["v"]:col["v"] + d] = vs[i].float().cpu()
    if shared_q:
        bufs["Q"][:, col["q"]:col["q"] + d] = qs.float().cpu()
    bufs = {name: t.to(device) for name, t in bufs.items()}
    oc0, ldo = o_view or (0, d)
    assert 0 <= oc0 and oc0 + d <= ldo
    obuf = torch.empty((orows, ldo), dtype=torch.float32, device=device)
    obuf.view(torch.int32).fill_(SENTINEL)
    written = torch.zeros(orows, ldo, dtype=torch.bool)
    for i in range(b):
        written[ooff[i]:ooff[i] + lqs[i], oc0:oc0 + d] = True
    lds = [ld[names[0]], ld[names[1]], ld[names[2]], ldo]
    if kernel == "flash":
        assert all(v % 4 == 0 for v in lds + [col["q"], col["k"], col["v"], oc0]), "flash attention moves 16-byte words"
    # the tables, in range
    tabs = [None] * 4
    if q_tab:
        tabs[0], tabs[1] = (torch.tensor(t, dtype=torch.int32, device=device) for t in (qoff, lqs))
        assert all(0 <= o and o + n <= qrows and n >= 1 for o, n in zip(qoff, lqs))
    if k_tab:
        tabs[2], tabs[3] = (torch.tensor(t, dtype=torch.int32, device=device) for t in (koff, lks))
        assert all(0 <= o and o + n <= krows and n >= 1 for o, n in zip(koff, lks))
    stride = lambda off: (off[1] - off[0]) if b > 1 else 0  # noqa: E731 - rows between samples (uniform form)
    bsq = 0 if (shared_q or q_tab) else stride(qoff) * lds[0]
    bsk, bsv = (0, 0) if k_tab else (stride(koff) * lds[1], stride(koff) * lds[2])
    bso = 0 if q_tab else stride(ooff) * ldo
    m = mask_qk.to(device=device, dtype=torch.uint8).contiguous() if mask_qk is not None else None
    kp = kpm.to(device=device, dtype=torch.uint8).contiguous() if kpm is not None else None
    if m is not None:
        assert m.dim() == 2 and m.shape[0] >= lqs[0] and m.shape[1] >= lks[0]
    if kp is not None:
        assert kp.dim() == 2 and kp.shape[0] >= b and kp.shape[1] >= lks[0]
    for rec in amax:
        assert rec is None or (rec.is_cuda and rec.dtype == torch.int32 and rec.numel() == AMAX_REC_WORDS)
    ptr = lambda op, name: bufs[name].data_ptr() + 4 * col[op]  # noqa: E731
    with torch.cuda.device(device):
        _lib.check(
            lib.ymk_op_attention_view(kid, ptr("q", names[0]), ptr("k", names[1]), ptr("v", names[2]), obuf.data_ptr() + 4 * oc0, b, heads,
                                      max(lqs), max(lks), hd, scale, lds[0], lds[1], lds[2], ldo, bsq, bsk, bsv, bso,
                                      _lib.ptr(m), m.shape[1] if m is not None else 0, _lib.ptr(kp), kp.shape[1] if kp is not None else 0,
                                      _lib.ptr(tabs[0]), _lib.ptr(tabs[1]), _lib.ptr(tabs[2]), _lib.ptr(tabs[3]),
                                      _lib.ptr(amax[0]), _lib.ptr(amax[1]), _lib.ptr(amax[2]), _lib.current_stream_ptr()),
            "ymk_op_attention_view",
        )
    outs = [obuf[ooff[i]:ooff[i] + lqs[i], oc0:oc0 + d].clone() for i in range(b)]
    return outs, obuf, written


# ---- the RT-DETRv2 decoder's token kernels: rows are level-major across the images (include/ymk.h, ymk_op_topk_tokens)
def _level_hw(levels):
    """levels ((h0, w0), (h1, w1), (h2, w2)) -> the HOST int array {h0, w0, h1, w1, h2, w2} of the ABI."""
    import ctypes

    flat = [int(v) for hw in levels for v in hw]
    assert len(flat) == 6
    return (ctypes.c_int * 6)(*flat)


def topk_tokens(logits, b, levels, k):
    """logits [b * ntok, nc] (device, level-major rows) -> idx [b, k] int32: per image the k best tokens in rank order."""
    lib = _lib.load()
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2
    lg = logits.contiguous()
    idx = torch.empty((b, k), dtype=torch.int32, device=logits.device)
    with torch.cuda.device(logits.device):
        _lib.check(lib.ymk_op_topk_tokens(lg.data_ptr(), b, _level_hw(levels), lg.shape[1], k, idx.data_ptr(),
                                          _lib.current_stream_ptr()), "ymk_op_topk_tokens")
    return idx


def gather_queries(om, bbox, anchors, idx, levels):
    """om [rows, d], bbox [rows, 4], anchors [ntok, 4], idx [b, k] int32 (device) -> (content [b, k, d], ref [b, k, 4])."""
    lib = _lib.load()
    b, k = idx.shape
    d = om.shape[1]
    om, bbox, anchors, idx = (t.contiguous() for t in (om, bbox, anchors, idx))
    content = torch.empty((b, k, d), dtype=torch.float32, device=om.device)
    ref = torch.empty((b, k, 4), dtype=torch.float32, device=om.device)
    with torch.cuda.device(om.device):
        _lib.check(lib.ymk_op_gather_queries(om.data_ptr(), bbox.data_ptr(), anchors.data_ptr(), idx.data_ptr(), b, _level_hw(levels), k, d,
                                             content.data_ptr(), ref.data_ptr(), _lib.current_stream_ptr()), "ymk_op_gather_queries")
    return content, ref


def refine_boxes(delta, ref):
    """sigmoid(delta + inverse_sigmoid(ref)), elementwise over same-shaped device tensors."""
    lib = _lib.load()
    delta, ref = delta.float().contiguous(), ref.float().contiguous()
    assert delta.shape == ref.shape
    out = torch.empty_like(delta)
    with torch.cuda.device(delta.device):
        _lib.check(lib.ymk_op_refine_boxes(delta.data_ptr(), ref.data_ptr(), out.data_ptr(), delta.numel(), _lib.current_stream_ptr()),
                   "ymk_op_refine_boxes")
    return out


def mask_rows(x, valid, b, levels):
    """x [b * ntok, d] (level-major rows), valid [ntok] (device) -> valid[token] * x[row]."""
    lib = _lib.load()
    x, valid = x.float().contiguous(), valid.float().contiguous()
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(lib.ymk_op_mask_rows(x.data_ptr(), valid.data_ptr(), b, _level_hw(levels), x.shape[1], out.data_ptr(),
                                        _lib.current_stream_ptr()), "ymk_op_mask_rows")
    return out


def deform_sample(offs, attw, ref, value_buf, col, b, levels, k):
    """offs [b*k, 8, 12, 2], attw [b*k, 8, 12], ref [b*k, 4]; the value rows are columns col .. col+255 of value_buf
    [b * ntok, ldv] (all on the device) -> [b*k, 256]."""
    lib = _lib.load()
    offs, attw, ref = (t.float().contiguous() for t in (offs, attw, ref))
    assert value_buf.is_contiguous() and value_buf.dtype == torch.float32 and 0 <= col and col + 256 <= value_buf.shape[1]
    out = torch.empty((b * k, 256), dtype=torch.float32, device=offs.device)
    with torch.cuda.device(offs.device):
        _lib.check(lib.ymk_op_deform_sample(offs.data_ptr(), attw.data_ptr(), ref.data_ptr(), value_buf.data_ptr() + 4 * col,
                                            value_buf.shape[1], b, _level_hw(levels), k, out.data_ptr(), _lib.current_stream_ptr()),
                   "ymk_op_deform_sample")
    return out


def avgpool2x2_ceil(x):
    """AvgPool2d(2, 2, 0, ceil_mode=True) of an NCHW device tensor (C a multiple of 4)."""
    lib = _lib.load()
    n, c, h, w = x.shape
    xh = _nhwc(x.float())
    y = torch.empty((n, (h + 1) // 2, (w + 1) // 2, c), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.ymk_op_avgpool2x2_ceil(xh.data_ptr(), n, h, w, c, y.data_ptr(), _lib.current_stream_ptr()), "ymk_op_avgpool2x2_ceil")
    return _nchw(y)


def upsample_nearest2x(x):
    """Nearest x2 up-sampling of an NCHW device tensor (C a multiple of 4)."""
    lib = _lib.load()
    n, c, h, w = x.shape
    xh = _nhwc(x.float())
    y = torch.empty((n, 2 * h, 2 * w, c), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.ymk_op_upsample_nearest2x(xh.data_ptr(), n, h, w, c, y.data_ptr(), _lib.current_stream_ptr()),
                   "ymk_op_upsample_nearest2x")
    return _nchw(y)


# ---- the DBNet++ head
def deconv2x2(x, weight, scale=None, bias=None, act="none"):
    """act(ConvTranspose2d(cin, cout, 2, 2)(x) * scale + bias) through the convolution path's scattering epilogue; x NCHW on the
    device, weight [cin, cout, 2, 2] (any device)."""
    lib = _lib.load()
    n, cin, h, w = x.shape
    cout = weight.shape[1]
    assert weight.shape == (cin, cout, 2, 2)
    xh = _nhwc(x.float())
    wh = weight.detach().float().cpu().contiguous()
    sh = scale.detach().float().cpu().contiguous() if scale is not None else None
    bh = bias.detach().float().cpu().contiguous() if bias is not None else None
    y = torch.empty((n, 2 * h, 2 * w, cout), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.ymk_op_deconv2x2(xh.data_ptr(), n, h, w, cin, wh.data_ptr(), cout, _lib.ptr(sh), _lib.ptr(bh), ACT[act],
                                        y.data_ptr(), _lib.current_stream_ptr()), "ymk_op_deconv2x2")
    return _nchw(y)


def deconv2x2_to1_sigmoid(x, weight, bias):
    """sigmoid(ConvTranspose2d(64, 1, 2, 2)(x) + bias): x NCHW (C = 64) on the device, weight [64, 1, 2, 2] -> [n, 1, 2h, 2w]."""
    lib = _lib.load()
    n, c, h, w = x.shape
    xh = _nhwc(x.float())
    wh = weight.detach().float().cpu().reshape(c, 4).contiguous()
    y = torch.empty((n, 1, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.ymk_op_deconv2x2_to1_sigmoid(xh.data_ptr(), n, h, w, wh.data_ptr(), float(bias), y.data_ptr(),
                                                    _lib.current_stream_ptr()), "ymk_op_deconv2x2_to1_sigmoid")
    return y


def dbnet_asf(ax, fuse, w1, w2, sp33, sp11, watt):
    """ScaleChannelSpatialAttention(ax) applied per scale to fuse (ScaleFeatureSelection): ax [n, 64, h, w], fuse [n, 256, h, w]
    NCHW on the device; w1 [cmid, 64], w2 [64, cmid], sp33 [3, 3], sp11 float, watt [4, 64] (any device) -> [n, 256, h, w]."""
    lib = _lib.load()
    n, c, h, w = ax.shape
    cmid = w1.shape[0]
    axh, fh = _nhwc(ax.float()), _nhwc(fuse.float())
    host = [t.detach().float().cpu().contiguous() for t in (w1, w2, sp33, watt)]
    y = torch.empty((n, h, w, 256), dtype=torch.float32, device=ax.device)
    with torch.cuda.device(ax.device):
        _lib.check(lib.ymk_op_dbnet_asf(axh.data_ptr(), fh.data_ptr(), n, h, w, host[0].data_ptr(), host[1].data_ptr(), cmid,
                                        host[2].data_ptr(), float(sp11), host[3].data_ptr(), y.data_ptr(), _lib.current_stream_ptr()),
                   "ymk_op_dbnet_asf")
    return _nchw(y)


# ---- the PARSeq greedy decode (include/ymk.h: "single operators of the PARSeq greedy decode")
DEC_STEP_WEIGHTS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                    "cross_attn.in_proj_weight", "cross_attn.in_proj_bias", "cross_attn.out_proj.weight", "cross_attn.out_proj.bias",
                    "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias")
DEC_STEP_NORMS = ("norm_q", "norm_c", "norm1", "norm2", "decoder.norm")


def _i32(t, device):
    return None if t is None else t.to(device=device, dtype=torch.int32).contiguous()


def parseq_dec_step(w, heads, qsa, tok, skv, memkv, out, step, L, mem_off=None, mem_len=None, prev_not_done=None, gid=None,
                    gopen=None, ng=1):
    """One launch of the fused decoder step, IN PLACE on skv [B, NS, 2D] and out [B, D] (device, fp32).  w: host fp32 tensors
    under the names DEC_STEP_WEIGHTS, "<norm>.weight" / "<norm>.bias" for DEC_STEP_NORMS, "emb" [ntok, D], "pos_queries" [NS, D];
    qsa [NS, D] host.  tok [B, NS] int32, memkv [rows, 2D], the optional tables int32, all on the device."""
    import ctypes

    lib = _lib.load()
    B, NS, D2 = skv.shape
    D = D2 // 2
    F = w["linear1.weight"].shape[0]
    ntok = w["emb"].shape[0]
    dev = skv.device
    for t in (tok, skv, memkv, out):
        assert t.is_cuda and t.is_contiguous()
    assert tok.dtype == torch.int32 and tok.shape == (B, NS) and out.shape == (B, D) and memkv.shape[1] == 2 * D
    assert w["pos_queries"].shape == (NS, D) and qsa.shape == (NS, D) and w["emb"].shape[1] == D
    # the kernel trusts its indices: check what it will dereference
    if 0 <= step < NS:
        assert 0 <= int(tok[:, step].min()) and int(tok[:, step].max()) < ntok
    if mem_off is not None:
        assert mem_off.dtype == mem_len.dtype == torch.int32 and mem_off.shape == mem_len.shape == (B,)
        assert int(mem_len.min()) >= 1 and int(mem_len.max()) <= L and int(mem_off.min()) >= 0
        assert int((mem_off + mem_len).max()) <= memkv.shape[0]
    else:
        assert memkv.shape[0] >= B * L
    if gid is not None:
        assert gid.dtype == gopen.dtype == torch.int32 and gid.shape == (B,) and gopen.shape == (NS, ng)
        assert 0 <= int(gid.min()) and int(gid.max()) < ng
    host = [w[n].detach().float().cpu().contiguous() for n in DEC_STEP_WEIGHTS]
    norms = [w[f"{n}.{k}"].detach().float().cpu().contiguous() for n in DEC_STEP_NORMS for k in ("weight", "bias")]
    ln = (ctypes.c_void_p * 10)(*[t.data_ptr() for t in norms])
    emb, posq, qs = (t.detach().float().cpu().contiguous() for t in (w["emb"], w["pos_queries"], qsa))
    with torch.cuda.device(dev):
        _lib.check(lib.ymk_op_parseq_dec_step(D, heads, F, *[t.data_ptr() for t in host], ln, emb.data_ptr(), ntok, posq.data_ptr(),
                                              qs.data_ptr(), tok.data_ptr(), skv.data_ptr(), memkv.data_ptr(), _lib.ptr(mem_off),
                                              _lib.ptr(mem_len), _lib.ptr(prev_not_done), _lib.ptr(gid), _lib.ptr(gopen), ng, step, B, L,
                                              NS, out.data_ptr(), _lib.current_stream_ptr()), "ymk_op_parseq_dec_step")


def greedy_step(logits, C, step, num_steps, tok, raw, state, not_done, eos_id=0, rep=(1, 8, 8, 3), prev_not_done=None, gid=None,
                gopen=None, ng=1, partials=0):
    """One launch of k_greedy_step (flag form), IN PLACE on tok / raw [B, ld_tok], state [B, 4], not_done [1], gopen [num_steps,
    ng] (int32, device).  logits [B, ld_b] fp32: C logits per row, or - partials - C (max, column bits) pairs.
    rep = (rep_on, period_max, min_run_p1, min_repeats)."""
    lib = _lib.load()
    B, ld_tok = tok.shape
    for t in (logits, tok, raw, state, not_done):
        assert t.is_cuda and t.is_contiguous()
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.shape[0] == B and logits.shape[1] >= C * (2 if partials else 1)
    assert tok.dtype == raw.dtype == state.dtype == not_done.dtype == torch.int32
    assert raw.shape == tok.shape and state.shape == (B, 4) and 0 <= step < num_steps <= ld_tok
    if gid is not None:
        assert gid.dtype == gopen.dtype == torch.int32 and gid.shape == (B,) and gopen.shape[1] == ng and gopen.shape[0] >= num_steps
        assert 0 <= int(gid.min()) and int(gid.max()) < ng
    with torch.cuda.device(tok.device):
        _lib.check(lib.ymk_op_greedy_step(logits.data_ptr(), logits.shape[1], C, step, num_steps, tok.data_ptr(), raw.data_ptr(), ld_tok,
                                          state.data_ptr(), eos_id, rep[0], rep[1], rep[2], rep[3], not_done.data_ptr(),
                                          _lib.ptr(prev_not_done), _lib.ptr(gid), _lib.ptr(gopen), ng, partials, B,
                                          _lib.current_stream_ptr()), "ymk_op_greedy_step")


def refine_prep(raw, S, bos_id, eos_id, gid=None, gsteps=None):
    """raw [B, ld_tok] int32 (device) -> (tok2 [B, ld_tok] int32, kpm [B, ld_tok] uint8), both pre-filled with the sentinel 77."""
    lib = _lib.load()
    B, ld_tok = raw.shape
    assert raw.is_cuda and raw.is_contiguous() and raw.dtype == torch.int32 and 1 <= S <= ld_tok
    if gid is not None:
        assert gid.dtype == gsteps.dtype == torch.int32 and gid.shape == (B,) and 0 <= int(gid.min()) and int(gid.max()) < gsteps.numel()
    tok2 = torch.full((B, ld_tok), 77, dtype=torch.int32, device=raw.device)
    kpm = torch.full((B, ld_tok), 77, dtype=torch.uint8, device=raw.device)
    with torch.cuda.device(raw.device):
        _lib.check(lib.ymk_op_refine_prep(raw.data_ptr(), ld_tok, S, bos_id, eos_id, tok2.data_ptr(), kpm.data_ptr(), B, _lib.ptr(gid),
                                          _lib.ptr(gsteps), _lib.current_stream_ptr()), "ymk_op_refine_prep")
    return tok2, kpm


def rep_cut(logits, S, state, eos_id):
    """IN PLACE on logits [B, rows, C] fp32 (device, rows >= S); state [B, 4] int32."""
    lib = _lib.load()
    B, rows, C = logits.shape
    assert logits.is_cuda and logits.is_contiguous() and logits.dtype == torch.float32 and 0 <= S <= rows
    assert state.dtype == torch.int32 and state.shape == (B, 4) and state.is_contiguous() and 0 <= eos_id < C
    with torch.cuda.device(logits.device):
        _lib.check(lib.ymk_op_rep_cut(logits.data_ptr(), rows * C, C, S, state.data_ptr(), eos_id, B, _lib.current_stream_ptr()),
                   "ymk_op_rep_cut")


def row_argmax(logits):
    """logits [rows, C] fp32 (device) -> int32 [rows]."""
    lib = _lib.load()
    assert logits.is_cuda and logits.is_contiguous() and logits.dtype == torch.float32 and logits.dim() == 2
    out = torch.full((logits.shape[0],), -7, dtype=torch.int32, device=logits.device)
    with torch.cuda.device(logits.device):
        _lib.check(lib.ymk_op_row_argmax(logits.data_ptr(), logits.shape[0], logits.shape[1], out.data_ptr(), _lib.current_stream_ptr()),
                   "ymk_op_row_argmax")
    return out


def token_stats(logits):
    """ymk_parseq_token_stats: logits [rows, C] fp32 (device) -> (ids int32 [rows], probs fp32 [rows])."""
    lib = _lib.load()
    assert logits.is_cuda and logits.is_contiguous() and logits.dtype == torch.float32 and logits.dim() == 2
    ids = torch.full((logits.shape[0],), -7, dtype=torch.int32, device=logits.device)
    probs = torch.full((logits.shape[0],), -7.0, dtype=torch.float32, device=logits.device)
    with torch.cuda.device(logits.device):
        _lib.check(lib.ymk_parseq_token_stats(logits.data_ptr(), logits.shape[0], logits.shape[1], ids.data_ptr(), probs.data_ptr(),
                                              _lib.current_stream_ptr()), "ymk_parseq_token_stats")
    return ids, probs


def ctx_embed_ln(tok, pos0, npos, emb, posq, g, b, eps, out):
    """IN PLACE on out [B, out_rows, D] (device): rows pos0 .. pos0 + npos - 1 of every sample.  tok [B, ld_tok] int32."""
    lib = _lib.load()
    B, out_rows, D = out.shape
    for t in (tok, emb, posq, g, b, out):
        assert t.is_cuda and t.is_contiguous()
    assert tok.dtype == torch.int32 and tok.shape[0] == B and emb.shape[1] == D and posq.shape[1] == D and g.numel() == b.numel() == D
    if npos > 0 and D <= 1024:  # the kernel trusts its indices
        assert 0 <= pos0 and pos0 + npos <= min(tok.shape[1], out_rows) and pos0 + npos - 1 <= posq.shape[0]
        used = tok[:, pos0:pos0 + npos]
        assert 0 <= int(used.min()) and int(used.max()) < emb.shape[0]
    with torch.cuda.device(out.device):
        _lib.check(lib.ymk_op_ctx_embed_ln(tok.data_ptr(), tok.shape[1], pos0, npos, emb.data_ptr(), posq.data_ptr(), g.data_ptr(),
                                           b.data_ptr(), float(eps), out.data_ptr(), out_rows, D, B, _lib.current_stream_ptr()),
                   "ymk_op_ctx_embed_ln")


def init_decode(B, ld_tok, bos_id, pad_id, device):
    """-> (tok [B, ld_tok], state [B, 4]) int32, both pre-filled with the sentinel 77."""
    lib = _lib.load()
    tok = torch.full((B, ld_tok), 77, dtype=torch.int32, device=device)
    state = torch.full((B, 4), 77, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(lib.ymk_op_init_decode(tok.data_ptr(), ld_tok, state.data_ptr(), bos_id, pad_id, B, _lib.current_stream_ptr()),
                   "ymk_op_init_decode")
    return tok, state


def tile_rows(src, B):
    """src [rows, D] fp32 (device) -> [B, rows, D]."""
    lib = _lib.load()
    assert src.is_cuda and src.is_contiguous() and src.dtype == torch.float32 and src.dim() == 2
    rows, D = src.shape
    dst = torch.full((B, rows, D), -7.0, dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(lib.ymk_op_tile_rows(src.data_ptr(), rows, D, dst.data_ptr(), B, _lib.current_stream_ptr()), "ymk_op_tile_rows")
    return dst


def add_pos_embed(x, pos, full_gw):
    """x [B, gh, gw, D] fp32 (device), pos [full_gh * full_gw, D] -> x + pos[r * full_gw + c] (a copy; the op works in place)."""
    lib = _lib.load()
    B, gh, gw, D = x.shape
    assert x.is_cuda and x.dtype == torch.float32 and pos.is_cuda and pos.is_contiguous() and pos.dtype == torch.float32
    assert gw <= full_gw and pos.shape[1] == D and pos.shape[0] >= (gh - 1) * full_gw + gw
    y = x.contiguous().clone()
    with torch.cuda.device(x.device):
        _lib.check(lib.ymk_op_add_pos_embed(y.data_ptr(), pos.data_ptr(), B, gh, gw, full_gw, D, _lib.current_stream_ptr()),
                   "ymk_op_add_pos_embed")
    return y


# ---- the NHWC glue kernels and the max|x| passes in the forms the models launch them (include/ymk.h: "*_view", ymk_op_absmax ..)
GLUE_VIEW_OPS = {  # kind -> (entry, output size of an h x w input)
    "maxpool": ("ymk_op_maxpool3x3s2_view", lambda h, w: ((h - 1) // 2 + 1, (w - 1) // 2 + 1)),
    "avgpool": ("ymk_op_avgpool2x2_ceil_view", lambda h, w: ((h + 1) // 2, (w + 1) // 2)),
    "nearest": ("ymk_op_upsample_nearest2x_view", lambda h, w: (2 * h, 2 * w)),
}


def _glue_in(t_nhwc, view, unchecked):
    """_into_view; `unchecked`: a view the entry has to refuse (c0 + c > ld, ld % 4, c0 % 4) is declared as it stands, inside a
    NaN buffer wide enough that a launch that went through anyway would stay inside it."""
    if not unchecked:
        return _into_view(t_nhwc, view)
    c0, ld = view
    wide = (max(ld, c0 + t_nhwc.shape[-1]) + 7) // 4 * 4
    buf = torch.full(t_nhwc.shape[:-1] + (wide,), float("nan"), dtype=torch.float32, device=t_nhwc.device)
    buf[..., c0:c0 + t_nhwc.shape[-1]] = t_nhwc
    return buf, buf.data_ptr() + 4 * c0


def _glue_out(shape, c, view, device, unchecked, into=None):
    """-> (the whole output buffer [.., ld], every word SENTINEL - or `into`, a buffer of an earlier launch -, the view's address)"""
    c0, ld = view
    if not unchecked:
        assert 0 <= c0 and c0 + c <= ld
    wide = ld if not unchecked else (max(ld, c0 + c) + 7) // 4 * 4
    if into is not None:
        assert tuple(into.shape) == tuple(shape) + (wide,) and into.is_contiguous()
        return into, into.data_ptr() + 4 * c0
    buf = torch.empty(tuple(shape) + (wide,), dtype=torch.float32, device=device)
    buf.view(torch.int32).fill_(SENTINEL)
    return buf, buf.data_ptr() + 4 * c0


def _glue_call(lib, name, unchecked, *args):
    status = getattr(lib, name)(*args, _lib.current_stream_ptr())
    if not unchecked:
        _lib.check(status, name)
        return None
    msg = lib.ymk_last_error() if status != 0 else None
    return None if status == 0 else (msg.decode("utf-8", "replace") if msg else str(status))


def pool_view(kind, x, in_view=None, out_view=None, unchecked=False):
    """ymk_op_maxpool3x3s2_view / ymk_op_avgpool2x2_ceil_view / ymk_op_upsample_nearest2x_view (kind "maxpool" / "avgpool" /
    "nearest"): x NCHW on the device.  *_view = (first channel, leading dimension) inside a wider NHWC buffer allocated here
    (default: contiguous): NaN beside the input view, SENTINEL in every word of the output buffer.
    -> (y NCHW: the output view, the whole output buffer [n, oh, ow, out_ld]); unchecked: (the entry's error message or None,
    the whole output buffer) for views the entry has to refuse."""
    lib = _lib.load()
    assert x.is_cuda
    n, c, h, w = x.shape
    name, size = GLUE_VIEW_OPS[kind]
    oh, ow = size(h, w)
    xbuf, xptr = _glue_in(_nhwc(x.float()), in_view or (0, c), unchecked)
    oc0, out_ld = out_view or (0, c)
    ybuf, yptr = _glue_out((n, oh, ow), c, (oc0, out_ld), x.device, unchecked)
    with torch.cuda.device(x.device):
        err = _glue_call(lib, name, unchecked, xptr, n, h, w, c, (in_view or (0, c))[1], yptr, out_ld)
    if unchecked:
        return err, ybuf
    return _nchw(ybuf[..., oc0:oc0 + c]), ybuf


def upsample_bilinear_view(x, size, add=None, in_view=None, out_view=None, add_view=None, into=None, unchecked=False):
    """ymk_op_upsample_bilinear_view: x NCHW on the device -> size = (oh, ow), `add` NCHW of the output's shape or None; views as
    pool_view (NaN beside x and add).  into: the whole output buffer of an earlier launch, to write another slice of it.
    -> (y NCHW: the output view, the whole output buffer); unchecked: (error message or None, the whole output buffer)."""
    lib = _lib.load()
    assert x.is_cuda
    n, c, h, w = x.shape
    oh, ow = size
    xbuf, xptr = _glue_in(_nhwc(x.float()), in_view or (0, c), unchecked)
    abuf, aptr, add_ld = None, None, 0
    if add is not None:
        assert tuple(add.shape) == (n, c, oh, ow)
        abuf, aptr = _glue_in(_nhwc(add.float().to(x.device)), add_view or (0, c), unchecked)
        add_ld = (add_view or (0, c))[1]
    oc0, out_ld = out_view or (0, c)
    ybuf, yptr = _glue_out((n, max(oh, 0), max(ow, 0)), c, (oc0, out_ld), x.device, unchecked, into)
    with torch.cuda.device(x.device):
        err = _glue_call(lib, "ymk_op_upsample_bilinear_view", unchecked, xptr, n, h, w, c, (in_view or (0, c))[1], oh, ow, aptr, add_ld,
                         yptr, out_ld)
    if unchecked:
        return err, ybuf
    return _nchw(ybuf[..., oc0:oc0 + c]), ybuf


def nchw3_to_nhwc4(x, unchecked=False, offset=0):
    """ymk_op_nchw3_to_nhwc4: x [n, 3, h, w] fp32 on the device -> y [n, h, w, 4] (NHWC as the kernel leaves it, SENTINEL before
    the launch).  unchecked: (error message or None, y), the output pointer `offset` floats into its buffer."""
    lib = _lib.load()
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.shape[1] == 3
    n, _, h, w = x.shape
    y = torch.empty((n, h, w, 4 + (4 if unchecked else 0)), dtype=torch.float32, device=x.device)
    y.view(torch.int32).fill_(SENTINEL)
    with torch.cuda.device(x.device):
        err = _glue_call(lib, "ymk_op_nchw3_to_nhwc4", unchecked, x.data_ptr(), n, h, w, y.data_ptr() + 4 * offset)
    return (err, y) if unchecked else y


def add_bcast(a, b, unchecked=False, offset=0, d=None):
    """ymk_op_add_bcast: a [m, d], b [rows_mod, d] fp32 on the device -> out [m, d] = a[r] + b[r % rows_mod] (SENTINEL before the
    launch).  unchecked: (error message or None, out), the row length declared as `d`, the output `offset` floats in."""
    lib = _lib.load()
    assert a.is_cuda and b.is_cuda and a.dtype == b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous()
    m, da = a.shape
    assert b.shape[1] == da
    out = torch.empty((m, da + (8 if unchecked else 0)), dtype=torch.float32, device=a.device)
    out.view(torch.int32).fill_(SENTINEL)
    with torch.cuda.device(a.device):
        err = _glue_call(lib, "ymk_op_add_bcast", unchecked, a.data_ptr(), b.data_ptr(), b.shape[0], m, da if d is None else d,
                         out.data_ptr() + 4 * offset)
    return (err, out) if unchecked else out


def absmax(buf, pixels, c, view, slot, nxt, unchecked=False):
    """ymk_op_absmax: one launch of k_absmax over `pixels` pixels of c floats at view = (first channel, leading dimension) of the
    flat fp32 device buffer `buf`, IN PLACE on the records slot / nxt (int32 [1024], device).  unchecked: -> error message or None."""
    lib = _lib.load()
    c0, ld = view
    assert buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous()
    assert unchecked or (0 <= c0 and c0 + c <= ld and (pixels - 1) * ld + c0 + c <= buf.numel())
    for rec in (slot, nxt):
        assert rec.is_cuda and rec.dtype == torch.int32 and rec.numel() == AMAX_REC_WORDS and rec.is_contiguous()
    with torch.cuda.device(buf.device):
        return _glue_call(lib, "ymk_op_absmax", unchecked, buf.data_ptr() + 4 * c0, pixels, c, ld, slot.data_ptr(), nxt.data_ptr())


def amax_merge(dst, src):
    """ymk_op_amax_merge IN PLACE on dst: records int32 [1024] on the device, or None (= a null record)."""
    lib = _lib.load()
    for rec in (dst, src):
        assert rec is None or (rec.is_cuda and rec.dtype == torch.int32 and rec.numel() == AMAX_REC_WORDS and rec.is_contiguous())
    dev = (dst if dst is not None else src).device
    with torch.cuda.device(dev):
        _glue_call(lib, "ymk_op_amax_merge", False, _lib.ptr(dst), _lib.ptr(src))


# ---- the page / text-line pre-processing kernels (csrc/ymk_image.hip) through their own entries, on guarded buffers
IMAGE_GUARD = 256  # words (fp32 outputs) or bytes (uint8 outputs) behind every output, pre-filled like the output itself
SCRATCH_FILL = 0xA5


def _guarded(shape, dtype, device):
    """A view of `shape` at the front of a buffer IMAGE_GUARD elements longer; every fp32 word SENTINEL, every byte SCRATCH_FILL."""
    n = 1
    for v in shape:
        n *= int(v)
    buf = torch.empty(n + IMAGE_GUARD, dtype=dtype, device=device)
    if dtype == torch.float32:
        buf.view(torch.int32).fill_(SENTINEL)
    else:
        buf.fill_(SCRATCH_FILL)
    return buf[:n].view(*shape)


def guard_tail(view):
    """The IMAGE_GUARD elements behind a `_guarded` view."""
    return view._base.view(-1)[view.numel():]


def untouched(t):
    """True when every element still holds what `_guarded` put there."""
    if t.dtype == torch.float32:
        return bool((t.contiguous().view(torch.int32) == SENTINEL).all().item())
    return bool((t == SCRATCH_FILL).all().item())


def det_preprocess(page_u8_dev, oh, ow, unchecked=False):
    """ymk_det_preprocess at any output size: page uint8 [h, w, 3] BGR on the device -> y fp32 [3, oh, ow], a `_guarded` view.
    unchecked: -> (the entry's error message or None, y) for sizes the entry has to refuse."""
    lib = _lib.load()
    assert page_u8_dev.is_cuda and page_u8_dev.dtype == torch.uint8 and page_u8_dev.is_contiguous() and page_u8_dev.shape[2] == 3
    h, w = page_u8_dev.shape[:2]
    y = _guarded((3, oh, ow), torch.float32, page_u8_dev.device)
    with torch.cuda.device(page_u8_dev.device):
        err = _glue_call(lib, "ymk_det_preprocess", unchecked, page_u8_dev.data_ptr(), h, w, oh, ow, y.data_ptr())
    return (err, y) if unchecked else y


def halve(page_u8_dev, unchecked=False):
    """ymk_halve_u8c3: uint8 [h, w, 3] on the device -> [round-half-even(h / 2), round-half-even(w / 2), 3], a `_guarded` view.
    unchecked: -> (error message or None, y)."""
    lib = _lib.load()
    assert page_u8_dev.is_cuda and page_u8_dev.dtype == torch.uint8 and page_u8_dev.is_contiguous() and page_u8_dev.shape[2] == 3
    h, w = page_u8_dev.shape[:2]
    dh, dw = int(round(h * 0.5)), int(round(w * 0.5))
    y = _guarded((dh, dw, 3), torch.uint8, page_u8_dev.device)
    with torch.cuda.device(page_u8_dev.device):
        err = _glue_call(lib, "ymk_halve_u8c3", unchecked, page_u8_dev.data_ptr(), h, w, y.data_ptr(), dh, dw)
    return (err, y) if unchecked else y


def crop_batch(levels, descs, out_h, batch_w, slots=None, flip=False):
    """ymk_crop_batch_levels: levels = the page and its pyramid levels (uint8 [h, w, 3] BGR device tensors, None for a level
    not built); descs = a numpy record array of imaging.CropDesc (rows of a plan's `table`, fields edited at will).  warp_off
    is laid out as imaging.build_crop_batch does (each crop's bytes start on a multiple of 16); slot = `slots` (a permutation;
    default 0 .. n - 1); flip: one value or one per crop.
    -> (out fp32 [n, 3, out_h, batch_w], scratch uint8 [bytes + IMAGE_GUARD], warp_off int64 [n]); out is a `_guarded` view,
    the scratch held SCRATCH_FILL in every byte before the launch."""
    import ctypes

    import numpy as np

    from yomitoku_amd import imaging

    lib = _lib.load()
    assert ctypes.sizeof(imaging.CropDesc) == lib.ymk_crop_desc_size() and descs.dtype == imaging._CROP_DTYPE
    arr = np.array(descs, copy=True)
    n = len(arr)
    arr["slot"] = np.arange(n) if slots is None else np.asarray(slots)
    assert sorted(arr["slot"].tolist()) == list(range(n))
    arr["flip"] = np.asarray(flip, dtype=np.int32)
    sizes = (arr["ww"].astype(np.int64) * arr["wh"] * 3 + 15) & ~15
    ends = np.cumsum(sizes)
    arr["warp_off"] = ends - sizes
    dev = levels[0].device
    for k in np.unique(arr["level"]).tolist():
        assert k < len(levels) and levels[k] is not None
    for d in arr:  # the kernels trust the descriptor: keep every box inside its level
        lh, lw = levels[int(d["level"])].shape[:2]
        assert 0 <= d["bx"] and 0 <= d["by"] and d["bx"] + d["bw"] <= lw and d["by"] + d["bh"] <= lh and d["nw"] <= batch_w and d["nh"] <= out_h
    scratch = torch.full((int(ends[-1]) + IMAGE_GUARD,), SCRATCH_FILL, dtype=torch.uint8, device=dev)
    out = _guarded((n, 3, out_h, batch_w), torch.float32, dev)
    descs_dev = torch.from_numpy(arr.view(np.uint8).copy()).to(dev)
    nl = len(levels)
    ptrs = (ctypes.c_void_p * nl)(*[(t.data_ptr() if t is not None else None) for t in levels])
    hs = (ctypes.c_int * nl)(*[(t.shape[0] if t is not None else 0) for t in levels])
    ws = (ctypes.c_int * nl)(*[(t.shape[1] if t is not None else 0) for t in levels])
    with torch.cuda.device(dev):
        _glue_call(lib, "ymk_crop_batch_levels", False, ptrs, hs, ws, nl, descs_dev.data_ptr(), n, max(1, int(arr["ww"].max())),
                   max(1, int(arr["wh"].max())), scratch.data_ptr(), out.data_ptr(), batch_w, out_h)
        torch.cuda.synchronize()
    return out, scratch, (ends - sizes).astype(np.int64)
