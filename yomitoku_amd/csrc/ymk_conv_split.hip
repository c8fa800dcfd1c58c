// Implicit-GEMM convolution with SPLIT operands and fp32 accumulation (gfx950), the alternative to the exact fp32-MFMA
// kernel of ymk_conv.hip for the same layers (models/dbnet_plus.py:33-38,56-127; rtdetr_backbone.py;
// parseq_transformer.py): same GEMM view, same gathers, same epilogue.
//
// Why: v_mfma_f32_32x32x2_f32 runs at the fp32 VECTOR rate (157 TFLOP/s); the 16-bit MFMAs are 16 x faster.  An fp32 value
// splits exactly into short pieces (round-to-nearest at every cut, remainders exact in fp32), so a product is a sum of
// short x short products, each exact in fp32:
//   bf16, 3 planes, 6 MFMAs  x_h y_h + (x_h y_m + x_m y_h) + (x_m y_m + x_h y_l + x_l y_h)   dropped terms <= 2^-23 |xy|
//   bf16, 2 planes, 3 MFMAs  x_h y_h + (x_h y_l + x_l y_h)                                   dropped terms <= 2^-15 |xy|
//   fp16, 2 planes, 3 MFMAs  the same three terms on 11-bit pieces                           dropped terms <= 2^-21 |xy|
// The fp16 form - pieces, scales, error analysis - is ymk_f16_planes.h, shared with every other fp16-split kernel: 22 of the 24
// significand bits in the same 3 MFMAs that two bf16 planes need (16 bits), i.e. fp32-grade products at 16 / 3 = 5.3 x the
// fp32 matrix rate.  What fp16 lacks is range, so the operands are scaled by powers of two (exact): the activations by ONE
// scale per launch that puts max|x| of the input view into [2^14, 2^15) - a pass over the input (k_absmax) ahead of the
// convolution, or the record its producer left, read by the kernel from device memory, no host round trip -, the weights per
// output channel at panel-build time (row maximum into [2^14, 2^15); the inverse goes into the epilogue's per-channel scale).
// Accumulation is fp32 inside the MFMA (not an fmaf chain in k order: results agree with the fp32 kernel to rounding, not
// bit for bit).
//
// Data path: activations stay fp32 in HBM; a thread splits the 4 floats it stages into NS x 4 halves on the way to LDS
// (v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32).  Weights are split once per (panel, format) at ymk_model_finalize (SplitCtx::prebuild;
// SplitCtx::panels is the counted fallback for a pair first asked for inside a forward) into panels
// [Cout^128][K tiles][NS][32], so a K tile's B rows are copied to LDS verbatim.  LDS row = NS x 64 B + 16 B pad
// (conflict-free ds_read_b128: row stride 36 or 52 dwords = 4 x odd), one ds_read_b128 per (32-row tile, plane, 16-k
// step) feeds v_mfma_f32_32x32x16_{bf16,f16}: lane l holds row l & 31, k = 8 (l >> 5) .. + 7 of the step, for A and B alike.
#include <algorithm>
#include <atomic>
#include <iterator>
#include <string>
#include <type_traits>
#include <unordered_map>

#include "ymk_conv_kernel.h"
#include "ymk_entry.h"
#include "ymk_vit_mlp.h"

namespace ymk {

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

// FMT 0: bf16 pieces, 1: fp16 pieces of the scaled operand
template <int FMT> struct Half;
template <> struct Half<0> { typedef bf16x8_t v8; };
template <> struct Half<1> { typedef f16x8 v8; };

template <int FMT>
__device__ __forceinline__ f32x16 mfma16(const typename Half<FMT>::v8 a, const typename Half<FMT>::v8 b, const f32x16 c) {
  if constexpr (FMT == 0) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// 4 floats -> NS planes of 4 halves (8 B each): bf16 pieces, or the two fp16 planes of the values times sa (ymk_f16_planes.h)
template <int FMT, int NS>
__device__ __forceinline__ void split4(const f32x4 v, float sa, uint2* planes) {
  f32x2 a = {v.x, v.y}, b = {v.z, v.w};
  if constexpr (FMT == 1) {
    static_assert(NS == 2, "fp16 operands have two planes");
    f16_split4(a * sa, b * sa, planes[0], planes[1]);
    return;
  }
#pragma unroll
  for (int pl = 0; pl < NS; ++pl) {
    const bf16x2_t pa = __builtin_convertvector(a, bf16x2_t), pb = __builtin_convertvector(b, bf16x2_t);
    planes[pl].x = __builtin_bit_cast(unsigned, pa);
    planes[pl].y = __builtin_bit_cast(unsigned, pb);
    if (pl + 1 < NS) {
      a -= __builtin_convertvector(pa, f32x2);  // exact: the remainder of a round-to-nearest cut fits fp32
      b -= __builtin_convertvector(pb, f32x2);
    }
  }
}

// blocks of this shape a CU's 160 KB of LDS holds (at most 2 are asked for) -> minimum waves per SIMD for the register allocator
template <int BM, int BN, int WM, int WN, int NS>
constexpr int split_waves_per_simd() {
  constexpr int lds = 2 * (BM + BN) * (NS * 64 + 16);
  constexpr int blocks = 2 * lds <= 160 * 1024 ? 2 : 1;
  return blocks * 64 * WM * WN / 256;
}

// The register-staged kernel: BM x BN tile, WM x WN waves, NS planes of format FMT.  A stage is one 32-k tile in one of two
// LDS buffers; the global loads of tile st + 1 are issued ahead of the MFMAs of tile st and held in registers (one set), then
// split and written to the other buffer behind them - one barrier per K tile.
// OPL (fp16 form): the epilogue writes fp16 planes (epilogue_tile<.., PL>, Tensor::planes).
template <int BM, int BN, int WM, int WN, int NS, int FMT, bool OPL = false>
__global__ __launch_bounds__(64 * WM * WN, (split_waves_per_simd<BM, BN, WM, WN, NS>())) void conv_igemm_split(ConvK p, const uint4* __restrict__ wsplit) {
  typedef typename Half<FMT>::v8 h8;
  constexpr int NT = 64 * WM * WN;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int ROWB = NS * 64 + 16;           // bytes of an LDS row: NS planes of 32 halves + pad (row stride = 4 x odd dwords)
  constexpr int STAGE_B = (BM + BN) * ROWB;    // bytes of one stage
  constexpr int RPP = NT / 8;                  // A rows staged per pass (8 threads x 16 B of fp32 per 32-k row)
  constexpr int APASS = BM / RPP;
  static_assert(BM % RPP == 0, "tile rows must divide by the staging pass");
  constexpr int PPR = NS * 4;                  // 16 B pieces of a B row per 32-k tile
  constexpr int BPASS = (BN * PPR + NT - 1) / NT;
  constexpr int LDC = BN + 4;
  constexpr int ECAP = 2 * STAGE_B / 4 / LDC;  // rows of the fp32 output tile the two stages can hold
  constexpr int EROWS = ECAP >= BM ? BM : (ECAP >= BM / 2 ? BM / 2 : BM / 4);  // rows per epilogue pass: divides BM
  static_assert(EROWS >= WTM && EROWS % WTM == 0 && EROWS <= ECAP, "an epilogue pass must hold whole wave tiles");
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE_B];

  const int t = threadIdx.x;
  float sa = 1.f, inv_sa = 1.f;
  if (FMT == 1) {
    const float2 sc = f16_plane_scales((unsigned)__builtin_amdgcn_readfirstlane((int)amax_read(p.amax, t)));  // wave-uniform: scalar registers
    sa = sc.x;
    inv_sa = sc.y;
  }
  int tile;
  {
    const int nblk = gridDim.x, bid = blockIdx.x;
    const int xcd = bid & 7, idx = bid >> 3, q = nblk >> 3, r = nblk & 7;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int tile_m = tile / p.ntiles_n, tile_n = tile - tile_m * p.ntiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  if (!tile_needed<BM, NT>(p, m0, t)) return;

  const int colq = t & 7, rowb = t >> 3;
  int pixb[APASS], ih0[APASS], iw0[APASS];
  const bool pointwise = (p.fast & 1) && p.KH == 1 && p.KW == 1 && p.stride == 1 && p.stride_w == 1 && p.pad == 0;
#pragma unroll
  for (int i = 0; i < APASS; ++i) {
    const int m = m0 + rowb + RPP * i;
    if (m < p.M && pointwise) {
      pixb[i] = m;
      ih0[i] = 0;
      iw0[i] = 0;
    } else if (m < p.M) {
      const int ohw = p.OH * p.OW;
      const int n = m / ohw, rem = m - n * ohw;
      const int oh = rem / p.OW, ow = rem - oh * p.OW;
      pixb[i] = n * p.H * p.W;
      ih0[i] = oh * p.stride - p.pad;
      iw0[i] = ow * p.stride_w - p.pad;
    } else {
      pixb[i] = 0;
      ih0[i] = -(1 << 20);
      iw0[i] = 0;
    }
  }
  const int ktiles = p.Kpad >> 5;
  // B pieces of this thread: piece q = t + NT * j of the tile's BN x PPR, row-major
  const uint4* wsrc[BPASS];
  int boff[BPASS];  // byte offset inside the B half of a stage, or -1 past the tile
#pragma unroll
  for (int j = 0; j < BPASS; ++j) {
    const int q = t + NT * j;
    const int row = q / PPR, piece = q - row * PPR;
    const bool ok = q < BN * PPR;
    wsrc[j] = wsplit + ((size_t)(n0 + (ok ? row : 0)) * ktiles) * PPR + piece;
    boff[j] = ok ? row * ROWB + piece * 16 : -1;
  }

  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0, p.in_bytes, 0x00020000);
  f32x4 ra[APASS];
  uint4 rb[1][BPASS];  // (the [1] is for the compiler: as a flat array the three-plane kernels come out with another register allocation)
  int cur_kh = 0, cur_kw = 0, cur_cc = 0;
  unsigned voff[APASS];
#pragma unroll
  for (int i = 0; i < APASS; ++i) voff[i] = OOB_OFFSET;

  // K tile st -> the staging registers; the tap cursor walks K tile by K tile
  auto load_stage = [&](int st) {
    if (FMT == 1 ? (cur_cc == 0 || p.KH * p.KW > 1) : cur_cc == 0) {  // wave-uniform: a new filter tap (fp16 panels: every K tile of a k x k layer)
      const int dh = cur_kh * p.dil, dw = cur_kw * p.dil;
#pragma unroll
      for (int i = 0; i < APASS; ++i) {
        const int ih = ih0[i] + dh, iw = iw0[i] + dw;
        const bool ok = (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
        const unsigned off = ((unsigned)(pixb[i] + ih * p.W + iw) * (unsigned)p.in_ld + (unsigned)(colq * 4)) * 4u;
        voff[i] = ok ? off : OOB_OFFSET;
      }
    }
    const bool chan_ok = cur_cc * 32 + colq * 4 < p.C;
    const int soff = cur_cc * 128;
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(chan_ok ? voff[i] : OOB_OFFSET), soff, 0);
      ra[i] = __builtin_bit_cast(f32x4, v);
    }
    if (FMT == 1) {  // channel-major panels: the taps of one channel slice back to back
      if (++cur_kw == p.KW) {
        cur_kw = 0;
        if (++cur_kh == p.KH) {
          cur_kh = 0;
          ++cur_cc;
        }
      }
    } else if (++cur_cc == p.ctiles) {
      cur_cc = 0;
      if (++cur_kw == p.KW) {
        cur_kw = 0;
        ++cur_kh;
      }
    }
#pragma unroll
    for (int j = 0; j < BPASS; ++j) rb[0][j] = wsrc[j][(size_t)st * PPR];
  };

  auto store_stage = [&](int buf) {
    char* As = lds + buf * STAGE_B;
    char* Bs = As + BM * ROWB;
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
      uint2 pl[NS];
      split4<FMT, NS>(ra[i], sa, pl);
      char* row = As + (rowb + RPP * i) * ROWB + colq * 8;
#pragma unroll
      for (int q = 0; q < NS; ++q) *reinterpret_cast<uint2*>(row + q * 64) = pl[q];
    }
#pragma unroll
    for (int j = 0; j < BPASS; ++j)
      if (boff[j] >= 0) *reinterpret_cast<uint4*>(Bs + boff[j]) = rb[0][j];
  };

  const int wv = t >> 6, lane = t & 63;
  const int wm = wv / WN, wn = wv - wm * WN;
  const int li = lane & 31, lh = lane >> 5;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  // product terms, smallest first: (A plane, B plane)
  constexpr int NTERM = NS == 3 ? 6 : 3;
  constexpr int TA[6] = {NS - 1, 0, 1, 1, 0, 0};
  constexpr int TB[6] = {0, NS - 1, 1, 0, 1, 0};
  constexpr int T0 = NS == 3 ? 0 : 3;

  auto compute = [&](int buf) {
    const char* As = lds + buf * STAGE_B + (wm * WTM + li) * ROWB + lh * 16;
    const char* Bs = lds + buf * STAGE_B + BM * ROWB + (wn * WTN + li) * ROWB + lh * 16;
#pragma unroll
    for (int s = 0; s < 2; ++s) {  // two 16-k steps per 32-k tile
      h8 fa[TM][NS], fb[TN][NS];
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int q = 0; q < NS; ++q) fa[a][q] = *reinterpret_cast<const h8*>(As + a * 32 * ROWB + q * 64 + s * 32);
#pragma unroll
      for (int b = 0; b < TN; ++b)
#pragma unroll
        for (int q = 0; q < NS; ++q) fb[b][q] = *reinterpret_cast<const h8*>(Bs + b * 32 * ROWB + q * 64 + s * 32);
      // term-major: consecutive MFMAs go to different accumulators whenever a wave owns more than one 32 x 32 tile
#pragma unroll
      for (int tm = 0; tm < NTERM; ++tm)
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
          for (int b = 0; b < TN; ++b)
            acc[a][b] = mfma16<FMT>(fa[a][TA[T0 + tm]], fb[b][TB[T0 + tm]], acc[a][b]);
    }
  };

  load_stage(0);
  store_stage(0);
  __syncthreads();
  for (int st = 0; st < ktiles; ++st) {
    const int buf = st & 1;
    if (st + 1 < ktiles) load_stage(st + 1);
    compute(buf);
    if (st + 1 < ktiles) store_stage(buf ^ 1);
    __syncthreads();
  }

  float* Cs = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int e0 = 0; e0 < BM; e0 += EROWS) {
    if (e0 > 0) __syncthreads();
    if (wm * WTM >= e0 && wm * WTM < e0 + EROWS) {
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = wm * WTM - e0 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            Cs[row * LDC + wn * WTN + b * 32 + li] = FMT == 1 ? acc[a][b][r] * inv_sa : acc[a][b][r];
          }
    }
    __syncthreads();
    epilogue_tile<EROWS, BN, NT, false, 4, OPL>(p, Cs, m0 + e0, n0, t);
  }
}

// ---- fp32 panel [rows][kpad] -> split panel [rows][kpad / 32][NS][32] halves (once per panel and format)
template <int NS>
__global__ void k_split_panel(const float* __restrict__ w, unsigned short* __restrict__ out, size_t n_elems, int kpad) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_elems) return;
  const size_t row = i / kpad;
  const int k = (int)(i - row * kpad), kt = k >> 5, kk = k & 31;
  float r = w[i];
#pragma unroll
  for (int pl = 0; pl < NS; ++pl) {
    const __bf16 h = (__bf16)r;
    out[((row * (kpad >> 5) + kt) * NS + pl) * 32 + kk] = __builtin_bit_cast(unsigned short, h);
    r -= (float)h;
  }
}

// fp16 form: one block per panel row.  The row is scaled by the power of two that puts its largest |w| into [2^14, 2^15);
// scale_out[row] = (BatchNorm scale of the channel, or 1) / that power - what the epilogue multiplies the accumulators by.
// K ORDER of the fp16 panels: CHANNEL-major - K tile (channel slice cc, tap) sits at cc * taps + tap, where the fp32 panel has
// it at tap * ctiles + cc.  The kernels then walk the taps of one 32-channel slice back to back: the nine shifted windows of
// a 3 x 3 layer overlap in all but one pixel column / row, and with only 128 bytes per pixel live they stay in L1 / L2, where
// the tap-major order streams the whole Cin x 4 B of every pixel past between two visits (section 9 item 3 of round 3).
// perm = 1 (1 x 1 panels only; the fused ViT MLP, ymk_vit_mlp.hip): inside every 32-wide K tile, source position k goes to the
// slot whose MFMA k index reads it as "accumulator register order": slot 16 s + 8 lh + j holds k = 16 s + 8 (j >> 2) + 4 lh +
// (j & 3) - the order in which a lane of the TRANSPOSED first product holds the hidden units of its row.
__global__ void k_split_panel_f16(const float* __restrict__ w, unsigned short* __restrict__ out, int kpad, const float* __restrict__ scale,
                                  int cout, float* __restrict__ scale_out, int taps, int ctiles, int perm) {
  __shared__ unsigned red[4];
  const int row = blockIdx.x, t = threadIdx.x;
  const float* wr = w + (size_t)row * kpad;
  unsigned m = 0;
  for (int k = t; k < kpad; k += 256) m = max(m, __float_as_uint(fabsf(wr[k])));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
  if ((t & 63) == 0) red[t >> 6] = m;
  __syncthreads();
  m = max(max(red[0], red[1]), max(red[2], red[3]));
  const float2 sc = f16_plane_scales(m);
  for (int k = t; k < kpad; k += 256) {
    const int kt_src = k >> 5;
    int kk = k & 31;
    const int tap = kt_src / ctiles, cc = kt_src - tap * ctiles;
    const int kt = cc * taps + tap;
    if (perm) {  // source k = 16 s + 8 q + 4 lh + e  ->  slot 16 s + 8 lh + 4 q + e
      const int rem = kk & 15;
      kk = (kk & 16) | (((rem >> 2) & 1) << 3) | ((rem >> 3) << 2) | (rem & 3);
    }
    _Float16 h, l;
    f16_split1(wr[k], sc.x, h, l);
    unsigned short* o = out + (((size_t)row * (kpad >> 5) + kt) * 2) * 32 + kk;
    o[0] = __builtin_bit_cast(unsigned short, h);
    o[32] = __builtin_bit_cast(unsigned short, l);
  }
  if (t == 0 && row < cout) scale_out[row] = (scale ? scale[row] : 1.f) * sc.y;
}

// ---- max|x| over an NHWC view (pixels x c floats, pixel stride ld; c, ld multiples of 4) -> atomicMax of the fp32 bit
// patterns into word 0 of the record `slot` (zero before the launch; the other lines of these records stay zero); the
// launch also clears word 0 of `next`, the record the following launch will use
__global__ __launch_bounds__(256) void k_absmax(const float* __restrict__ in, size_t items, int c4, int ld, unsigned* __restrict__ slot,
                                                unsigned* __restrict__ next) {
  __shared__ unsigned red[4];
  const int t = threadIdx.x;
  if (blockIdx.x == 0 && t == 0) *next = 0u;
  unsigned m = 0;
  const size_t stride = (size_t)gridDim.x * 256;
  auto fold = [&](const float4 v) {
    m = max(max(m, __float_as_uint(fabsf(v.x))), max(__float_as_uint(fabsf(v.y)), max(__float_as_uint(fabsf(v.z)), __float_as_uint(fabsf(v.w)))));
  };
  size_t i = (size_t)blockIdx.x * 256 + t;
  if (ld == c4 * 4) {  // contiguous view
    const float4* p = reinterpret_cast<const float4*>(in);
    for (; i + 3 * stride < items; i += 4 * stride) {  // four loads in flight per thread
      const float4 a = p[i], b = p[i + stride], c = p[i + 2 * stride], d = p[i + 3 * stride];
      fold(a);
      fold(b);
      fold(c);
      fold(d);
    }
    for (; i < items; i += stride) fold(p[i]);
  } else {
    for (; i < items; i += stride) {
      const size_t pix = i / (unsigned)c4;
      const int q = (int)(i - pix * (unsigned)c4);
      fold(*reinterpret_cast<const float4*>(in + pix * ld + q * 4));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
  if ((t & 63) == 0) red[t >> 6] = m;
  __syncthreads();
  if (t == 0) atomicMax(slot, max(max(red[0], red[1]), max(red[2], red[3])));
}

void absmax_launch(hipStream_t s, const float* x, size_t pixels, int c, int ld, unsigned* slot, unsigned* next) {
  const size_t items = pixels * (size_t)(c / 4);
  const int blocks = (int)std::min<size_t>(1024, (items + 1023) / 1024);
  hipLaunchKernelGGL(k_absmax, dim3(blocks), dim3(256), 0, s, x, items, c / 4, ld, slot, next);
}
void absmax_record(hipStream_t s, const float* x, size_t n, unsigned* rec) {
  absmax_launch(s, x, n / 4, 4, 4, rec, rec + AMAX_LINE_WORDS);  // (clears a word nobody reads)
  YMK_HIP(hipGetLastError());
}

// ---- self-check of the producers' records (ymk_debug_option("amax_check", 1); tests/test_conv_split_gpu.py): a launch whose
// input came with a record ALSO makes the pass, and a one-wave kernel compares the two: counters[0] = launches checked,
// [1] = records BELOW the true max|x| (a stale or incomplete record: the fp16 planes may overflow - a bug), [2] = records more
// than 2^8 above it (a derived bound so loose that it costs low-plane bits), [3] = the largest record / truth ratio as a power of two
static std::atomic<int> g_amax_check{0};
static unsigned long long* g_amax_counters = nullptr;  // device, 4 words
__global__ void k_amax_verify(const unsigned* __restrict__ rec, const unsigned* __restrict__ truth, unsigned long long* __restrict__ counters) {
  const unsigned got = amax_read(rec, threadIdx.x), want = amax_read(truth, threadIdx.x);
  if (threadIdx.x != 0) return;
  atomicAdd(&counters[0], 1ull);
  if (got < want) atomicAdd(&counters[1], 1ull);
  const int slack = (int)(got >> 23) - (int)(want >> 23);  // exponent distance
  if (want != 0u && slack > 8) atomicAdd(&counters[2], 1ull);
  if (want != 0u && slack > 0) atomicMax(&counters[3], (unsigned long long)slack);
}
void amax_check_counters(long long* out4) {
  for (int i = 0; i < 4; ++i) out4[i] = 0;
  if (!g_amax_counters) return;
  YMK_HIP(hipDeviceSynchronize());
  YMK_HIP(hipMemcpy(out4, g_amax_counters, 4 * sizeof(long long), hipMemcpyDeviceToHost));
}

// cache key of the fc2 panel of the fused ViT MLP: fp16 planes with the accumulator-order K permutation (never a "conv_split" code)
constexpr int SPLIT_F16X2_PERM = 17;

// ---- per-model state
class SplitCtx {
 public:
  struct Panels {
    void* planes = nullptr;
    float* scale = nullptr;  // fp16 form only: the epilogue's per-channel scale with the row's power of two taken back out
  };
  ~SplitCtx() {
    for (void* q : allocs_) dev_free(q);
    if (moved_) (void)hipEventDestroy(moved_);
  }
  // split copy of panel w for `code`.  Built at ymk_model_finalize for the precision the model runs (prebuild below); a pair
  // that is first asked for inside a forward - the process-wide precision switched after finalize, a single-operator call -
  // is built here on stream s, counted ("lazy_panel_builds"), and waited for
  const Panels& panels(hipStream_t s, const ConvW& w, int code) {
    const Key key{w.w, code};
    auto it = cache_.find(key);
    if (it != cache_.end()) return it->second;
    note_lazy_panel_build();
    const Panels pn = build(s, w, code);
    // on the stream of the forward that asked first: wait for it here, so that a later forward of this model on ANOTHER
    // stream (a second lane, a caller that changed streams) can never read a panel that is still being written
    forward_sync(s);
    return cache_.emplace(key, pn).first->second;
  }
  // every (panel, code) pair a forward of the owning model can ask for, and the max|x| words, on stream s (ymk_model_finalize:
  // the null stream, followed by a device synchronisation) - so that a forward never allocates, never builds, never waits
  void prebuild(hipStream_t s, const std::vector<ConvW>& convs, const std::vector<ConvW>& perm, int code) {
    if (code != 2 && code != 3 && code != SPLIT_F16X2) return;
    for (const ConvW& w : convs)
      if (w.mode == 0 && cache_.find(Key{w.w, code}) == cache_.end()) cache_.emplace(Key{w.w, code}, build(s, w, code));
    if (code == SPLIT_F16X2)
      for (const ConvW& w : perm)
        if (w.mode == 0 && cache_.find(Key{w.w, SPLIT_F16X2_PERM}) == cache_.end())
          cache_.emplace(Key{w.w, SPLIT_F16X2_PERM}, build(s, w, SPLIT_F16X2_PERM));
    ensure_slots(s);
  }
  // max|x| of the input view of launch k, on stream s; returns the device word the convolution kernel reads
  const unsigned* absmax(hipStream_t s, const ConvK& k) {
    ensure_slots(s);
    // the two words alternate along ONE stream (each launch clears the other word for its successor); when the context
    // moves to another stream, that stream waits for the old one first
    if (have_stream_ && s != stream_) {  // an event in the old stream's order, the new stream behind it: the host does not wait
      YMK_HIP(hipEventRecord(moved_, stream_));
      YMK_HIP(hipStreamWaitEvent(s, moved_, 0));
    }
    stream_ = s;
    have_stream_ = true;
    const size_t pixels = (size_t)(k.in_bytes / 4 - k.C) / k.in_ld + 1;
    unsigned* cur = slots_ + parity_ * AMAX_REC_WORDS;
    absmax_launch(s, k.in, pixels, k.C, k.in_ld, cur, slots_ + (parity_ ^ 1) * AMAX_REC_WORDS);
    parity_ ^= 1;
    return cur;
  }

 private:
  struct Key {
    const float* w;
    int code;
    bool operator==(const Key& o) const { return w == o.w && code == o.code; }
  };
  struct KeyHash {
    size_t operator()(const Key& k) const { return std::hash<const void*>()(k.w) * 31 + (size_t)k.code; }
  };
  void* alloc(size_t bytes) {
    void* q = dev_malloc(bytes);
    allocs_.push_back(q);
    return q;
  }
  Panels build(hipStream_t s, const ConvW& w, int code) {
    const int ns = code == 3 ? 3 : 2;
    const size_t rows = (size_t)((w.cout + 255) / 256 * 256), real = (size_t)((w.cout + 127) / 128 * 128), n = real * w.kpad;
    Panels pn;
    pn.planes = alloc(rows * w.kpad * ns * 2);  // rows padded to 256: the 256-wide tile reads whole tiles
    YMK_HIP(hipMemsetAsync(pn.planes, 0, rows * w.kpad * ns * 2, s));
    if (code == SPLIT_F16X2 || code == SPLIT_F16X2_PERM) {
      pn.scale = reinterpret_cast<float*>(alloc(real * sizeof(float)));
      hipLaunchKernelGGL(k_split_panel_f16, dim3((unsigned)real), dim3(256), 0, s, w.w, reinterpret_cast<unsigned short*>(pn.planes), w.kpad,
                         w.scale, w.cout, pn.scale, w.kh * w.kw, w.ctiles, code == SPLIT_F16X2_PERM ? 1 : 0);
    } else {
      const int blocks = (int)((n + 255) / 256);
      if (ns == 2) hipLaunchKernelGGL(k_split_panel<2>, dim3(blocks), dim3(256), 0, s, w.w, reinterpret_cast<unsigned short*>(pn.planes), n, w.kpad);
      else hipLaunchKernelGGL(k_split_panel<3>, dim3(blocks), dim3(256), 0, s, w.w, reinterpret_cast<unsigned short*>(pn.planes), n, w.kpad);
    }
    YMK_HIP(hipGetLastError());
    return pn;
  }
  // the two max|x| words of launches whose input came without a record
  void ensure_slots(hipStream_t s) {
    if (slots_) return;
    slots_ = reinterpret_cast<unsigned*>(alloc(2 * AMAX_REC_WORDS * sizeof(unsigned)));
    YMK_HIP(hipEventCreateWithFlags(&moved_, hipEventDisableTiming));
    if (debug_hazard_null_memset()) {
      // the round-5 form, reachable only through YMK_DEBUG_HAZARD_NULL_MEMSET (tools/stress_call.py): the fill goes to the NULL
      // stream, which the callers' non-blocking streams do not order with - it can land after the first k_absmax has written
      // the word, and the model's first split launch then scales its operands for max|x| = 0
      YMK_HIP(hipMemset(slots_, 0, 2 * AMAX_REC_WORDS * sizeof(unsigned)));
      return;
    }
    // ON stream s, ahead of the first k_absmax that will use the words
    YMK_HIP(hipMemsetAsync(slots_, 0, 2 * AMAX_REC_WORDS * sizeof(unsigned), s));
  }
  std::unordered_map<Key, Panels, KeyHash> cache_;
  std::vector<void*> allocs_;
  unsigned* slots_ = nullptr;
  int parity_ = 0;
  hipStream_t stream_ = nullptr;
  bool have_stream_ = false;
  hipEvent_t moved_ = nullptr;
};

SplitCtx* SplitCtxOwner::get() {
  if (!p_) p_ = new SplitCtx();
  return p_;
}
SplitCtxOwner::~SplitCtxOwner() { delete p_; }

void Model::prebuild_split() {
  if (debug_lazy_split()) return;
  SplitCtx* ctx = split_ctx.get();
  int code;
  {
    ConvSplitScope scope(conv_split(), ctx, SPLIT_MODEL_DEFAULT);
    code = conv_effective_split();
  }
  ctx->prebuild(nullptr, pool.convs(), pool.perm_convs(), code);
  const int enc = (int)param("conv_split_encoder", -1);  // the recogniser's evaluation switch: a second precision for the ViT blocks
  if (enc > 0 && enc != code) ctx->prebuild(nullptr, pool.convs(), pool.perm_convs(), enc);
  YMK_HIP(hipStreamSynchronize(nullptr));
}

// amax_check mode: the launch's record against a pass over its input (counters above).  Level 2 also waits for the answer
// and names the launch whose record lies below the truth on stderr (a debugging aid: it serialises the stream).
static void amax_verify(hipStream_t s, const ConvK& k, SplitCtx* ctx) {
  if (!g_amax_counters) {
    YMK_HIP(hipMalloc((void**)&g_amax_counters, 4 * sizeof(unsigned long long)));
    YMK_HIP(hipMemset(g_amax_counters, 0, 4 * sizeof(unsigned long long)));
  }
  const unsigned* truth = ctx->absmax(s, k);
  hipLaunchKernelGGL(k_amax_verify, dim3(1), dim3(64), 0, s, k.amax, truth, g_amax_counters);
  if (g_amax_check.load(std::memory_order_relaxed) >= 2) {
    unsigned got[AMAX_REC_WORDS], want[AMAX_REC_WORDS];
    YMK_HIP(hipStreamSynchronize(s));
    YMK_HIP(hipMemcpy(got, k.amax, sizeof(got), hipMemcpyDeviceToHost));
    YMK_HIP(hipMemcpy(want, truth, sizeof(want), hipMemcpyDeviceToHost));
    unsigned g = 0, w = 0;
    for (int i = 0; i < AMAX_LINES; ++i) {
      g = std::max(g, got[i * AMAX_LINE_WORDS]);
      w = std::max(w, want[i * AMAX_LINE_WORDS]);
    }
    if (g < w) {
      float gf, wf;
      std::memcpy(&gf, &g, 4);
      std::memcpy(&wf, &w, 4);
      std::fprintf(stderr, "amax_check: record BELOW the truth: %g < %g  M=%d C=%d ld=%d Cout=%d k=%dx%d stride=%d H=%d W=%d act=%d res=%d rec=%p in=%p\n", gf, wf,
                   k.M, k.C, k.in_ld, k.Cout, k.KH, k.KW, k.stride, k.H, k.W, k.act, k.res ? 1 : 0, (const void*)k.amax, (const void*)k.in);
    }
  }
}

template <int FMT, int BM, int BN, int WM, int WN, int NS, bool OPL = false>
static void launch_split(hipStream_t s, ConvK& k, const void* wsplit, SplitCtx* ctx) {
  const int mt = (k.M + BM - 1) / BM, nt = (k.Cout + BN - 1) / BN;
  k.ntiles_n = nt;
  auto* e = conv_prof_open(s, k, BM, BN, mt * nt, (FMT ? 160 : 10 * NS));
  if (FMT == 1 && k.amax == nullptr) {
    k.amax = ctx->absmax(s, k);  // no record from the producer: a pass over the input (inside the timed span)
  } else if (FMT == 1 && g_amax_check.load(std::memory_order_relaxed)) {
    amax_verify(s, k, ctx);
  }
  hipLaunchKernelGGL((conv_igemm_split<BM, BN, WM, WN, NS, FMT, OPL>), dim3(mt * nt), dim3(64 * WM * WN), 0, s, k,
                     reinterpret_cast<const uint4*>(wsplit));
  if (e) YMK_HIP(hipEventRecord(e->second, s));
}

// ymk_debug_option("conv_split_tile", v): 0 = every launch by the rule (route_f16; the bf16 forms run the register-staged kernel);
// the others force one of the product kernels, for tests that reach or compare them - any other value is refused (SPLIT_TILES):
//   1 = the register-staged kernel, narrow tile (128 x 64)
//   3 = the register-staged kernel, the format's own wide tile (256 x 128 for three bf16 planes, else 128 x 128 x 16 waves: the
//       measured best per format, profiles/r03_conv_sweep_bf16_split*.txt)
//   fp16 form only (the bf16 forms run as 3): 21 = the LDS-DMA kernel, 30 = the A-stationary kernel for every launch it can run
static constexpr int SPLIT_TILES[] = {0, 1, 3, 21, 30};
static std::atomic<int> g_split_tile{0};
// ... or, for the calling thread only, a ConvSplitTileScope (single-operator entry points: the process-wide word would
// reroute forwards that other threads have in flight)
static thread_local int t_split_tile = 0;
static int split_tile_now() { return t_split_tile != 0 ? t_split_tile : g_split_tile.load(std::memory_order_relaxed); }
ConvSplitTileScope::ConvSplitTileScope(int tile) : prev_(t_split_tile) { t_split_tile = tile; }
ConvSplitTileScope::~ConvSplitTileScope() { t_split_tile = prev_; }
// ymk_debug_option("astat", v): 1 (default) = the short-K pointwise layers the A-stationary kernel measured ahead on take it;
// 0 = none does (the round-4 routing, what the tests compare it with); "conv_split_tile" 30 forces it for every launch it can run
static std::atomic<int> g_astat{1};
// ymk_debug_option("act_planes", v): 1 (default) = the tensor between a bottleneck's 1 x 1 reduction and its 3 x 3 convolution
// lives in HBM as the two fp16 planes the 3 x 3 multiplies with (written by the reduction's epilogue under a bound, read by
// LDS-DMA without any conversion: ymk_conv_dma.hip APL) wherever conv_planes_pair_ok allows; 0 = fp32 activations everywhere
static std::atomic<int> g_act_planes{1};
// ymk_debug_option("rowmax_tile", v): the kernel of a row-max launch (the greedy loop's vocabulary head) where 128 x 128 tiles fill
// the chip: 0 = the A-stationary kernel, one column block per block, where it runs (K <= 192: ymk_conv_astat.hip astat_rowmax),
// else the 128 x 64 x 8-wave tile; 6 = 128 x 64 always (the route of a head with K > 192, and what the A-stationary head is compared
// with bit for bit) - the same (max, column) pairs per 64-column sub-tile from each (ymk_conv_kernel.h, EPI_ROWMAX).
// profiles/r06_rowmax_head_tiles.md: 35.2 us per step at 1234 rows on 128 x 64, 28.2 on (0)
static std::atomic<int> g_rowmax_tile{0};
// launch counters since the process started (ymk_stat; tests assert that a route was really taken).  "rowmax_wide_launches"
// keeps its name from when the head also ran on wide tiles of the staged kernel: it counts the head's A-stationary launches
// (128-column blocks), the only form wider than the 128 x 64 tile that is left
static std::atomic<long long> g_n_astat{0}, g_n_ln_fused{0}, g_n_planes_read{0}, g_n_planes_written{0}, g_n_rowmax_wide{0}, g_n_mlp_fused{0};
bool conv_split_stat(const std::string& key, long long* value) {
  if (key == "astat_launches") *value = g_n_astat.load();
  else if (key == "ln_fused_launches") *value = g_n_ln_fused.load();
  else if (key == "planes_read_launches") *value = g_n_planes_read.load();
  else if (key == "planes_written_launches") *value = g_n_planes_written.load();
  else if (key == "rowmax_wide_launches") *value = g_n_rowmax_wide.load();
  else if (key == "mlp_fused_launches") *value = g_n_mlp_fused.load();
  else return false;
  return true;
}
bool conv_split_debug_option(const std::string& key, int value) {
  if (key == "conv_split_tile") {
    const bool known_tile = std::find(std::begin(SPLIT_TILES), std::end(SPLIT_TILES), value) != std::end(SPLIT_TILES);
    std::string accepted;
    for (int v : SPLIT_TILES) accepted += " " + std::to_string(v);
    YMK_CHECK(known_tile, "conv_split_tile " + std::to_string(value) + " is no selector; accepted:" + accepted);
    g_split_tile = value;
  }
  else if (key == "amax_check") g_amax_check = value;
  else if (key == "astat") g_astat = value;
  else if (key == "act_planes") g_act_planes = value;
  else if (key == "rowmax_tile") {
    YMK_CHECK(value == 0 || value == 6, "rowmax_tile " + std::to_string(value) + " is no selector; accepted: 0 6");
    g_rowmax_tile = value;
  }
  else return false;
  return true;
}

// the tile shapes of the register-staged kernel, for every format (FMT 0: NS bf16 planes, 1: two fp16 planes)
template <int FMT, int NS>
static void dispatch_staged(hipStream_t s, ConvK& k, const void* ws, bool narrow, SplitCtx* ctx) {
  if constexpr (FMT == 1) {
    if (k.out_planes) {
      if (narrow) launch_split<1, 128, 64, 4, 2, 2, true>(s, k, ws, ctx);
      else launch_split<1, 128, 128, 4, 4, 2, true>(s, k, ws, ctx);
      return;
    }
  }
  if (narrow) launch_split<FMT, 128, 64, 4, 2, NS>(s, k, ws, ctx);
  else if constexpr (FMT == 0 && NS == 3) launch_split<0, 256, 128, 4, 4, 3>(s, k, ws, ctx);
  else launch_split<FMT, 128, 128, 4, 4, NS>(s, k, ws, ctx);
}

// ---- which kernel an fp16-split launch runs on: ONE rule, asked by conv2d_split for the launch itself and by
// conv_planes_pair_ok (ymk_conv.hip) for a producer / consumer pair before either is launched
//   none: not a launch that fills the chip (>= 256 tiles of 128 x 128, or - few - of 128 x 64): the exact fp32 paths keep it
//   astat (ymk_conv_astat.hip): pointwise layers with K <= 192 and more than 64 output channels - the ViT blocks' qkv / proj /
//     fc1 and the final vocabulary head (K = 192), the ResNet expands 64 -> 256 / 128 -> 512 with their residual: A rows are
//     fetched and cut into planes once per 128 rows instead of once per tile (profiles/r05_conv_astat_timing.jsonl: qkv 371 us
//     against 514, 64 -> 256 + residual 403 against 475, the 124 634 x 7119 head 1.76 ms against 3.22).  At K = 256 the A
//     planes leave registers for 64-column blocks only, and the per-layer table of the serial pass
//     (profiles/r05_conv_two_roof_by_layer*.md) has that form BEHIND the register-staged kernel wherever a residual is read
//     (256 -> 1024 + residual 2.67 ms against 2.27): K = 256 stays where it was.  A launch with a LayerNorm to fuse has no
//     other kernel to go to: taken there or refused.  It neither reads nor writes planes.
//   dma (ymk_conv_dma.hip; 128-row tiles, two or three blocks per CU) where it measured ahead of the register-staged kernel
//     (profiles/r04_conv_sweep_f16_lds_dma.txt): every k x k layer (+2..17 %), long-K 1 x 1 reductions (+3..7 %) and the
//     64-column 1 x 1 layers (+1..6 %)
//   staged (conv_igemm_split): the rest - wide 1 x 1 layers with K > 256 (the ViT fc2, the 512 -> 128 reductions)
enum SplitRoute : int { ROUTE_NONE = 0, ROUTE_ASTAT = 1, ROUTE_DMA = 2, ROUTE_STAGED = 3 };
struct RouteQuery {
  long M;
  int cout, kpad, taps;
  bool rowmax, row_group, astat_can, ln, planes_io;
};
static SplitRoute route_f16(const RouteQuery& q, bool& narrow) {
  const long mt128 = (q.M + 127) / 128;
  const long blocks128 = mt128 * ((q.cout + 127) / 128), blocks64 = mt128 * ((q.cout + 63) / 64);
  // ---- the forcing options (tests reach and compare the product kernels with them), each turned into one flag here.  With
  // none set, `rule`, `astat_rule` and `head_astat` are true, the two `force_` flags false, and what follows is the rule above:
  // the astat and dma conditions below choose a kernel BY THE RULE only under their flag, so "conv_split_tile" 1 and 3, which
  // set no other flag, leave every launch on the staged kernel
  const int force = split_tile_now();
  const bool rule = force == 0;
  const bool force_narrow = force == 1, force_dma = force == 21;
  const bool astat_rule = rule && g_astat.load(std::memory_order_relaxed) != 0;           // "astat" 0
  const bool head_astat = astat_rule && g_rowmax_tile.load(std::memory_order_relaxed) == 0;  // "rowmax_tile" 6
  const bool astat_able = q.astat_can && !q.planes_io;
  if (force == 30) {  // the A-stationary kernel at any size it can run; else the staged kernel, where 128 x 128 tiles fill the chip
    narrow = q.cout <= 64 || q.rowmax;
    if (astat_able && !q.rowmax) return ROUTE_ASTAT;
    return q.ln || blocks128 < 256 ? ROUTE_NONE : ROUTE_STAGED;
  }

  // none
  if (blocks128 < 256 && blocks64 < 256) return ROUTE_NONE;
  const bool few = blocks128 < 256;
  narrow = q.cout <= 64 || q.rowmax || few || force_narrow;
  // astat
  if (q.ln) return astat_able ? ROUTE_ASTAT : ROUTE_NONE;
  if (astat_able && (q.rowmax ? head_astat : astat_rule) && q.cout > 64 && !few && q.kpad <= 192) return ROUTE_ASTAT;
  // dma (a row-max or row-predicated launch stays staged, and so does a few-row launch of more than 64 columns)
  const bool dma_shape = q.taps > 1 || (q.kpad >= 1024 && q.cout <= 512) || q.cout <= 64;
  const bool dma_runs = !q.rowmax && !q.row_group;
  if (dma_runs && (force_dma || (rule && dma_shape && (!few || q.cout <= 64)))) return ROUTE_DMA;
  return ROUTE_STAGED;
}

int conv_split_route_with_planes(long M, int cout, int kpad, int taps, bool* auto_tile) {
  bool narrow = false;
  *auto_tile = split_tile_now() == 0 && g_act_planes.load(std::memory_order_relaxed) != 0;
  return (int)route_f16(RouteQuery{M, cout, kpad, taps, false, false, false, false, true}, narrow);
}

bool conv2d_split(hipStream_t s, ConvK& k, const ConvW& w, int code, SplitCtx* ctx) {
  if (w.mode != 0 || ctx == nullptr || (code != 2 && code != 3 && code != SPLIT_F16X2)) return false;  // 4-channel stems keep the fp32 kernel
  const bool planes_io = k.in_planes != 0 || k.out_planes != 0;
  if ((k.ln_g != nullptr || planes_io) && code != SPLIT_F16X2) return false;  // fused LayerNorm / planes in HBM: fp16 form only
  const bool rowmax = k.epi == EPI_ROWMAX;  // (max, column) per 64-column tile: the 128 x 64 tile
  const size_t w_bytes_f16 = (size_t)((w.cout + 255) / 256 * 256) * w.kpad * 2 * 2;
  bool narrow = false;
  SplitRoute route = ROUTE_STAGED;
  if (code == SPLIT_F16X2) {
    route = route_f16(RouteQuery{k.M, w.cout, k.Kpad, k.KH * k.KW, rowmax, has_row_predicate(k), conv2d_f16_astat_can(k, w_bytes_f16),
                                 k.ln_g != nullptr, planes_io}, narrow);
  } else {  // bf16 evaluation forms: the register-staged kernel, for launches that fill the chip
    const long mt128 = (k.M + 127) / 128;
    const long blocks128 = mt128 * ((w.cout + 127) / 128), blocks64 = mt128 * ((w.cout + 63) / 64);
    if (blocks128 < 256 && blocks64 < 256) return false;
    narrow = w.cout <= 64 || split_tile_now() == 1 || rowmax || blocks128 < 256;
  }
  if (route == ROUTE_NONE) return false;
  YMK_CHECK(!k.in_planes || route == ROUTE_DMA, "a tensor stored as fp16 planes reached a kernel that cannot read it");
  YMK_CHECK(!k.out_planes || route == ROUTE_DMA || route == ROUTE_STAGED, "fp16 planes asked of a kernel that cannot write them");
  const SplitCtx::Panels& pn = ctx->panels(s, w, code);
  if (k.in_planes) ++g_n_planes_read;
  if (k.out_planes) ++g_n_planes_written;
  if (route == ROUTE_ASTAT) {
    k.scale = pn.scale;
    const int bn = conv2d_f16_astat_columns(k);
    auto* e = conv_prof_open(s, k, 128, bn, ((k.M + 127) / 128) * ((k.Cout + bn - 1) / bn), 162);
    if (k.amax == nullptr) k.amax = ctx->absmax(s, k);
    else if (g_amax_check.load(std::memory_order_relaxed) && k.ln_g == nullptr) amax_verify(s, k, ctx);
    const bool taken = conv2d_f16_astat(s, k, pn.planes, w_bytes_f16);
    if (e) YMK_HIP(hipEventRecord(e->second, s));
    YMK_HIP(hipGetLastError());
    YMK_CHECK(taken, "conv_f16_astat refused a launch it had accepted");
    ++g_n_astat;
    if (rowmax) ++g_n_rowmax_wide;
    if (k.ln_g != nullptr) ++g_n_ln_fused;
    return true;
  }
  if (route == ROUTE_DMA) {
    k.scale = pn.scale;
    const bool nar = w.cout <= 64;
    k.ntiles_n = (k.Cout + (nar ? 64 : 128) - 1) / (nar ? 64 : 128);
    auto* e = conv_prof_open(s, k, 128, nar ? 64 : 128, ((k.M + 127) / 128) * k.ntiles_n, 161);
    YMK_CHECK(!k.in_planes || k.amax != nullptr, "a tensor of fp16 planes without the record that holds its scale");
    if (k.amax == nullptr) k.amax = ctx->absmax(s, k);
    else if (g_amax_check.load(std::memory_order_relaxed) && !k.in_planes) amax_verify(s, k, ctx);
    const bool taken = conv2d_f16_dma(s, k, pn.planes, w_bytes_f16, nar);
    if (e) YMK_HIP(hipEventRecord(e->second, s));
    YMK_HIP(hipGetLastError());
    YMK_CHECK(taken, "conv_f16_dma refused a launch");
    return true;
  }
  if (code == SPLIT_F16X2) {
    k.scale = pn.scale;
    dispatch_staged<1, 2>(s, k, pn.planes, narrow, ctx);
  } else if (code == 2) {
    dispatch_staged<0, 2>(s, k, pn.planes, narrow, ctx);
  } else {
    dispatch_staged<0, 3>(s, k, pn.planes, narrow, ctx);
  }
  YMK_HIP(hipGetLastError());
  return true;
}

// ---- the fused ViT MLP (ymk_vit_mlp.hip): planes of fc1 (standard) and fc2 (permuted), the bounds, the launch
bool vit_mlp_split_launch(hipStream_t s, SplitCtx* ctx, float* x, int M, int ld, const float* ln_g, const float* ln_b, float ln_eps,
                          float ln_bound, const ConvW& fc1, const ConvW& fc2) {
  const int D = fc1.cin, F = fc1.cout;
  if (ctx == nullptr || fc1.mode != 0 || fc2.mode != 0 || fc1.kh * fc1.kw != 1 || fc2.kh * fc2.kw != 1) return false;
  if (fc2.cin != F || fc2.cout != D || fc1.kpad != D || fc2.kpad != F || fc1.scale != nullptr || fc2.scale != nullptr) return false;
  if (fc1.bias == nullptr || fc2.bias == nullptr || D != 192 || F != 768) return false;
  if ((M + 127) / 128 < 256) return false;  // one block per CU: fewer blocks than CUs leave the layer to the GEMM kernels
  const SplitCtx::Panels& p1 = ctx->panels(s, fc1, SPLIT_F16X2);
  const SplitCtx::Panels& p2 = ctx->panels(s, fc2, SPLIT_F16X2_PERM);
  MlpK k{};
  k.x = x;
  k.out = x;
  k.M = M;
  k.ld = ld;
  k.ln_g = ln_g;
  k.ln_b = ln_b;
  k.ln_eps = ln_eps;
  k.ln_bound = ln_bound;
  k.w1 = reinterpret_cast<const uint4*>(p1.planes);
  k.w1_bytes = (unsigned)((size_t)((F + 255) / 256 * 256) * fc1.kpad * 4);
  k.s1 = p1.scale;
  k.b1 = fc1.bias;
  k.w2 = reinterpret_cast<const uint4*>(p2.planes);
  k.w2_bytes = (unsigned)((size_t)((D + 255) / 256 * 256) * fc2.kpad * 4);
  k.s2 = p2.scale;
  k.b2 = fc2.bias;
  k.g_bound = fc1.pl_a * ln_bound + fc1.pl_b;  // |GELU(v)| <= |v| <= pl_a max|LayerNorm output| + pl_b
  char desc[160];
  // (the by-layer tools parse this line: the fused layer shows as M x D -> D with a residual on a 128 x D tile, ksplit 163)
  snprintf(desc, sizeof desc, "M=%7d Cin=%4d Cout=%4d k=1x1 s=1 d=1 res=1 tile=128x%d ksplit=163 grid=%d", M, D, D, D, (M + 127) / 128);
  // algorithmic work of the fused layer: both products; bytes: the rows in and out, the residual read, the two weight matrices
  auto* e = conv_prof_open_raw(s, desc, 4.0 * (double)M * D * F, 4.0 * (3.0 * (double)M * D + 2.0 * (double)D * F), 3.0);
  const bool taken = vit_mlp_f16_launch(s, k, D, F);
  if (e) YMK_HIP(hipEventRecord(e->second, s));
  YMK_HIP(hipGetLastError());
  if (taken) ++g_n_mlp_fused;
  return taken;
}

}  // namespace ymk
