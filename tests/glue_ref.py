"""Plain float64 (or exact index / bit) restatements of the memory-bound NHWC kernels between the convolutions
(yomitoku_amd/csrc/ymk_elem.hip, k_add_bcast of ymk_det.hip) and of the max|x| records, for tests/test_glue_views_gpu.py.
tests/test_glue_ref_host.py checks every one against torch's own operators on the CPU.  Tensors are NCHW, as the tests hold them."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from tests.hipops import AMAX_REC_WORDS

AMAX_LINES = 32
AMAX_LINE_WORDS = AMAX_REC_WORDS // AMAX_LINES


def maxpool3x3s2(x, dtype=torch.float64):
    """MaxPool2d(3, 2, 1): the window clipped to the image (a -inf border).  A maximum rounds nothing, so the result is exact in
    float64 and in the input's own fp32 alike (dtype: what the largest case uses to stay small)."""
    return F.max_pool2d(x.to(dtype), 3, 2, 1)


def avgpool2x2_ceil(x):
    """AvgPool2d(2, 2, 0, ceil_mode=True) in float64: the divisor counts the taps inside the image."""
    n, c, h, w = x.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    acc = torch.zeros(n, c, oh, ow, dtype=torch.float64)
    cnt = torch.zeros(oh, ow, dtype=torch.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            part = x[:, :, dy::2, dx::2].double()
            acc[:, :, :part.shape[2], :part.shape[3]] += part
            cnt[:part.shape[2], :part.shape[3]] += 1
    return acc / cnt


def nearest2x(x):
    """out[.., oy, ox] = x[.., oy // 2, ox // 2]: index arithmetic, the values untouched."""
    n, c, h, w = x.shape
    oy, ox = torch.arange(2 * h) // 2, torch.arange(2 * w) // 2
    return x[:, :, oy][:, :, :, ox]


def nchw3_to_nhwc4(x):
    """x [n, 3, h, w] -> [n, h, w, 4], the fourth channel +0.0."""
    n, c, h, w = x.shape
    assert c == 3
    out = torch.zeros(n, h, w, 4, dtype=x.dtype)
    out[..., :3] = x.permute(0, 2, 3, 1)
    return out


def add_bcast(a, b):
    """a [m, d] + b[r % rows_mod] in float64; the kernel's single fp32 addition is this sum rounded once (.float())."""
    rows = torch.arange(a.shape[0]) % b.shape[0]
    return a.double() + b.double()[rows]


def bilinear_axis(n_in, n_out):
    """The source rows and weights of one axis exactly as k_bilinear documents them, in fp32:
    s = (float)n_in / (float)n_out; f = max(((float)o + 0.5f) * s - 0.5f, 0); i0 = (int)f; i1 = i0 + (i0 < n_in - 1);
    l = f - i0; hgh = 1.f - l - every operation rounded to fp32 on its own (no fused multiply-add).
    -> (i0, i1 int64 [n_out], hgh, l float64 [n_out] holding the fp32 values)"""
    f32 = np.float32
    s = f32(n_in) / f32(n_out)
    o = np.arange(n_out).astype(f32)
    f = ((o + f32(0.5)) * s).astype(f32) - f32(0.5)
    f = np.maximum(f.astype(f32), f32(0))
    i0 = f.astype(np.int32)
    i1 = i0 + (i0 < n_in - 1)
    l = (f - i0.astype(f32)).astype(f32)
    hgh = (f32(1) - l).astype(f32)
    assert f.dtype == f32 and l.dtype == f32 and hgh.dtype == f32
    return (torch.from_numpy(i0.astype(np.int64)), torch.from_numpy(i1.astype(np.int64)),
            torch.from_numpy(hgh.astype(np.float64)), torch.from_numpy(l.astype(np.float64)))


def bilinear(x, size, add=None):
    """F.interpolate(x, size, mode="bilinear", align_corners=False) (+ add): the fp32 source coordinates of bilinear_axis, the
    interpolation itself in float64 with those weights: hy (hx a + lx b) + ly (hx c + lx d)."""
    oh, ow = size
    y0, y1, hy, ly = bilinear_axis(x.shape[2], oh)
    x0, x1, hx, lx = bilinear_axis(x.shape[3], ow)
    xd = x.double()
    top, bot = xd[:, :, y0], xd[:, :, y1]
    hy, ly = hy.view(1, 1, oh, 1), ly.view(1, 1, oh, 1)
    out = hy * (hx * top[..., x0] + lx * top[..., x1]) + ly * (hx * bot[..., x0] + lx * bot[..., x1])
    return out if add is None else out + add.double()


def record_value(rec):
    """The number a max|x| record holds: the maximum over word 0 of its 32 lines (fp32 bit patterns of non-negative values
    order as unsigned integers) -> float."""
    words = rec.detach().cpu().to(torch.int32).reshape(AMAX_LINES, AMAX_LINE_WORDS)[:, 0].to(torch.int64) & 0xFFFFFFFF
    top = int(words.max())
    return float(np.array([top], dtype=np.uint32).view(np.float32)[0])
