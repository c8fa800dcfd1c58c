// Cross attention of PARSeq's non-autoregressive pass (decode_ar = 0, models/parseq.py:253-262): every sample of the
// batch asks the SAME Lq x D queries (W_q(norm1(pos_queries + the <bos> self-attention row)), weights only) of its own
// encoder memory K|V.
//
// One block per (sample, 64 * QPT queries); wave h of the block owns head h, a lane owns QPT queries of that head: its
// query rows (pre-scaled) and its output rows live in registers for the whole kernel.  The block walks the sample's keys
// in tiles of 8 rows (4 at head dim 96); a tile holds the FULL K|V rows (all heads) in LDS, fetched from HBM once, coalesced, by all
// waves together and one tile ahead of the arithmetic (registers -> LDS after the barrier).  Inside a wave every lane
// reads the same LDS address (its head's slice of key k): a broadcast, free of bank conflicts, and because a lane owns
// whole queries the online softmax needs no cross-lane step at all - running max, sum and the rescale are lane-local,
// fp32 throughout.  QPT = 2 at head dim 32 (two FMAs per LDS operand, 101 queries in one block), 1 above (the
// accumulators of one query already fill the register budget of a 512-thread block; the K|V rows are then read once per
// 64 queries).
#include "ymk_common.h"
#include "ymk_seq.h"

namespace ymk {

constexpr int NAR_KC = 4;  // keys per softmax step (scores, rescale, P V): what a lane holds in registers at a time

struct NarAttnP {
  const float *q, *k, *v;
  float* o;
  int ldq, ldk, ldv, ldo;
  long bsk, bsv, bso;
  int Lq, Lk, H, hd;
  float scale;
  const int *koff, *klen;  // ragged keys/values: sample b reads klen[b] rows from row koff[b] (null = strided, Lk)
};

// HDP: head dim as laid out in LDS / registers (a multiple of 16 >= hd); QPT: queries per lane; TK: keys per LDS tile
template <int HDP, int QPT, int TK>
__global__ __launch_bounds__(512) void k_nar_cross_attn(NarAttnP p) {
  extern __shared__ float4 nar_lds4[];
  float* lds = reinterpret_cast<float*>(nar_lds4);
  constexpr int NCOL = (HDP + 31) / 32;  // K|V columns a thread stages: 2 D = 2 H hd columns over 64 H threads
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int h = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x;
  const int hd = p.hd, D = p.H * hd;
  const int RS = p.H * HDP;   // LDS row stride (floats): head h of a row at h * HDP, columns hd..HDP-1 stay zero
  float* Ks = lds;            // [TK][RS]
  float* Vs = lds + TK * RS;  // [TK][RS]

  const float* kb = p.k + (size_t)b * p.bsk;
  const float* vb = p.v + (size_t)b * p.bsv;
  int Lk = p.Lk;
  if (p.koff) {
    kb = p.k + (size_t)p.koff[b] * p.ldk;
    vb = p.v + (size_t)p.koff[b] * p.ldv;
    Lk = p.klen[b];
  }

  // queries of this lane, scaled; rows past Lq compute on zeros and store nothing
  float qr[QPT][HDP];
  int qi[QPT];
#pragma unroll
  for (int j = 0; j < QPT; ++j) {
    qi[j] = blockIdx.y * (64 * QPT) + lane + 64 * j;
    const float* src = p.q + (size_t)(qi[j] < p.Lq ? qi[j] : 0) * p.ldq + h * hd;
#pragma unroll
    for (int d = 0; d < HDP; ++d) qr[j][d] = (qi[j] < p.Lq && d < hd) ? src[d] * p.scale : 0.f;
  }
  float acc[QPT][HDP];
  float mx[QPT], sum[QPT];
#pragma unroll
  for (int j = 0; j < QPT; ++j) {
    mx[j] = -INFINITY;
    sum[j] = 0.f;
#pragma unroll
    for (int d = 0; d < HDP; ++d) acc[j][d] = 0.f;
  }

  for (int i = tid; i < 2 * TK * RS; i += nthr) lds[i] = 0.f;  // the pad columns are never written again

  // staging: a thread owns columns c = tid + i * 64 H of the [K row | V row] pair (2 D floats) in every row of a tile
  const float* gsrc[NCOL];  // column c of key row 0 (K or V side)
  int gld[NCOL], loff[NCOL];
#pragma unroll
  for (int i = 0; i < NCOL; ++i) {
    const int c = tid + i * nthr;
    const bool on = c < 2 * D, isk = c < D;
    const int cc = isk ? c : c - D;
    const int hh = cc / hd, d = cc - hh * hd;
    gsrc[i] = on ? (isk ? kb + cc : vb + cc) : nullptr;
    gld[i] = isk ? p.ldk : p.ldv;
    loff[i] = (isk ? 0 : TK * RS) + hh * HDP + d;
  }
  float stage[NCOL][TK];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NCOL; ++i)
#pragma unroll
      for (int r = 0; r < TK; ++r) stage[i][r] = (gsrc[i] != nullptr && k0 + r < Lk) ? gsrc[i][(size_t)(k0 + r) * gld[i]] : 0.f;
  };
  auto commit = [&]() {
#pragma unroll
    for (int i = 0; i < NCOL; ++i)
      if (gsrc[i] != nullptr) {
#pragma unroll
        for (int r = 0; r < TK; ++r) lds[loff[i] + r * RS] = stage[i][r];
      }
  };

  fetch(0);
  __syncthreads();  // the zero fill is done
  for (int k0 = 0; k0 < Lk; k0 += TK) {
    commit();
    __syncthreads();
    if (k0 + TK < Lk) fetch(k0 + TK);  // in flight during the arithmetic below
    const int kn = min(TK, Lk - k0);   // block-uniform
#pragma unroll 1
    for (int kc = 0; kc < kn; kc += NAR_KC) {
      const float* kt = Ks + kc * RS + h * HDP;
      const float* vt = Vs + kc * RS + h * HDP;
      float sc[QPT][NAR_KC];
#pragma unroll
      for (int kk = 0; kk < NAR_KC; ++kk) {
        const float4* kr = reinterpret_cast<const float4*>(kt + kk * RS);
        float a[QPT];
#pragma unroll
        for (int j = 0; j < QPT; ++j) a[j] = 0.f;
#pragma unroll
        for (int d4 = 0; d4 < HDP / 4; ++d4) {
          const float4 kv = kr[d4];
#pragma unroll
          for (int j = 0; j < QPT; ++j) {
            a[j] = fmaf(qr[j][4 * d4 + 0], kv.x, a[j]);
            a[j] = fmaf(qr[j][4 * d4 + 1], kv.y, a[j]);
            a[j] = fmaf(qr[j][4 * d4 + 2], kv.z, a[j]);
            a[j] = fmaf(qr[j][4 * d4 + 3], kv.w, a[j]);
          }
        }
#pragma unroll
        for (int j = 0; j < QPT; ++j) sc[j][kk] = kc + kk < kn ? a[j] : -INFINITY;  // rows past the sample's last key
      }
#pragma unroll
      for (int j = 0; j < QPT; ++j) {
        float m = mx[j];
#pragma unroll
        for (int kk = 0; kk < NAR_KC; ++kk) m = fmaxf(m, sc[j][kk]);
        const float alpha = __expf(mx[j] - m);  // first step: exp(-inf) = 0 on zero accumulators (a step holds >= 1 key: m is finite)
        mx[j] = m;
        float ps = 0.f;
#pragma unroll
        for (int kk = 0; kk < NAR_KC; ++kk) {
          sc[j][kk] = __expf(sc[j][kk] - m);
          ps += sc[j][kk];
        }
        sum[j] = sum[j] * alpha + ps;
#pragma unroll
        for (int d = 0; d < HDP; ++d) acc[j][d] *= alpha;
      }
#pragma unroll
      for (int kk = 0; kk < NAR_KC; ++kk) {
        const float4* vr = reinterpret_cast<const float4*>(vt + kk * RS);
#pragma unroll
        for (int d4 = 0; d4 < HDP / 4; ++d4) {
          const float4 vv = vr[d4];
#pragma unroll
          for (int j = 0; j < QPT; ++j) {
            acc[j][4 * d4 + 0] = fmaf(sc[j][kk], vv.x, acc[j][4 * d4 + 0]);
            acc[j][4 * d4 + 1] = fmaf(sc[j][kk], vv.y, acc[j][4 * d4 + 1]);
            acc[j][4 * d4 + 2] = fmaf(sc[j][kk], vv.z, acc[j][4 * d4 + 2]);
            acc[j][4 * d4 + 3] = fmaf(sc[j][kk], vv.w, acc[j][4 * d4 + 3]);
          }
        }
      }
    }
    __syncthreads();  // every wave is done with the tile before the next one lands on it
  }

  float* ob = p.o + (size_t)b * p.bso;
#pragma unroll
  for (int j = 0; j < QPT; ++j) {
    if (qi[j] >= p.Lq) continue;
    const float inv = sum[j] > 0.f ? 1.f / sum[j] : 0.f;
    float* orow = ob + (size_t)qi[j] * p.ldo + h * hd;
#pragma unroll
    for (int d = 0; d < HDP; ++d)
      if (d < hd) orow[d] = acc[j][d] * inv;
  }
}

template <int HDP, int QPT, int TK>
static void launch_nar(hipStream_t s, const NarAttnP& p, int B) {
  static_assert(TK % NAR_KC == 0, "a tile is a whole number of softmax steps");
  const size_t lds = (size_t)2 * TK * p.H * HDP * sizeof(float);  // <= 2 * 8 * 8 * 64 * 4 = 32 KB
  hipLaunchKernelGGL((k_nar_cross_attn<HDP, QPT, TK>), dim3(B, (p.Lq + 64 * QPT - 1) / (64 * QPT)), dim3(64 * p.H), lds, s, p);
  YMK_HIP(hipGetLastError());
}

void nar_cross_attention(hipStream_t s, const float* q, const float* k, const float* v, float* o, int B, int H, int Lq, int Lk,
                         int hd, int ldq, int ldk, int ldv, int ldo, long bsk, long bsv, long bso, float scale, const SeqTab* tab) {
  if (B == 0 || Lq == 0) return;
  YMK_CHECK(Lk > 0, "nar cross attention: no keys");
  YMK_CHECK(H >= 1 && H <= 8 && hd >= 1 && hd <= 96, "nar cross attention: 1..8 heads of at most 96 channels");
  YMK_CHECK(ldq >= H * hd && ldk >= H * hd && ldv >= H * hd && ldo >= H * hd, "nar cross attention: rows shorter than heads x head dim");
  NarAttnP p{q, k, v, o, ldq, ldk, ldv, ldo, bsk, bsv, bso, Lq, Lk, H, hd, scale, tab ? tab->koff : nullptr, tab ? tab->klen : nullptr};
  YMK_CHECK((p.koff == nullptr) == (p.klen == nullptr), "nar cross attention: offset and length tables come in pairs");
  if (hd <= 32) launch_nar<32, 2, 8>(s, p, B);
  else if (hd <= 48) launch_nar<48, 1, 8>(s, p, B);
  else if (hd <= 64) launch_nar<64, 1, 8>(s, p, B);
  else launch_nar<96, 1, 4>(s, p, B);
}

}  // namespace ymk
