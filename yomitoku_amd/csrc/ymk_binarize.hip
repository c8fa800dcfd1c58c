// Thresholded pages: a grey-valued page of a wave turned into the packed rows the Group 4 coder takes (include/ymk.h,
// "Binariser"; yomitoku_amd/ccitt.py; DESIGN.md, "Thresholded pages").  tests/binarize_ref.py is the definition; every stage
// equals it bit for bit.  The page table is the Group 4 encoder's (ymk_ccitt.hip); ymk_g4_encode_pages runs behind these
// launches unchanged.
//
//   k_bin_test_hist      per page: is B == G == R everywhere (one channel: always)?  - an OR into the page's flag, as
//                        k_g4_test_pack does - and, where the caller wants it, the page's 256-bin histogram: per block in LDS
//                        (eight copies a lane picks by its number, so that a page of paper white does not queue a whole wave on
//                        one counter), flushed with one integer atomic per non-empty bin and block.
//   k_bin_otsu           one block per page, thread t = threshold t: inclusive prefix sums of hist and i hist as int64 in LDS,
//                        sigma in double exactly as the definition orders it, arg-max with the smallest t on ties.
//   k_bin_otsu_pack      p <= t*, a ballot per 64 pixels of a row, into the packed rows.
//   k_bin_row_scan       adaptive, pass 1: P[y][x] = sum of the row's pixels up to x.  One wave per row, 64 pixels a step:
//                        a shuffle scan and a carry.  At most 255 * 16383: no wrap.
//   k_bin_col_scan       pass 2, in place: A[y][x] = sum of P down to row y.  A block owns 64 columns; its 16 waves take a
//                        sixteenth of the rows each, sum it, exchange the sums through LDS and walk their rows again adding.
//   k_bin_adaptive_pack  the window's sum from four corners of A, the comparison in 64 bits, the ballot.
//
// The summed-area table A is uint32 and WRAPS: 255 h w passes 2^32 beyond 16.8 M pixels, and the API takes 268 M.  The wrapping
// form is exact all the same: a window's sum is A11 - A01 - A10 + A00 modulo 2^32, and its true value is at most 255 * 2047^2
// < 2^31 (r <= 16383 / 16), so the residue IS the value.  Half the bytes of an int64 table, on a stage that is all memory traffic.

#include "ymk_pages.h"

#include "../../include/ymk.h"

namespace ymk {

constexpr int BZ_REC = YMK_G4_PAGE_WORDS;
constexpr int BZ_MAX_SIDE = 16383;

struct BzLimits {
  long long packed_words, sat_words;
};

// A page's record, read and checked against the buffers' sizes, as g4_page of ymk_ccitt.hip does: a kernel takes a page whose
// record fails the check for what it touches as absent.
struct BzPage {
  const unsigned char* src;
  int h, w, ch, row_words;
  long long packed_at, sat_at;
  bool ok, pack_ok, sat_ok;
};
__device__ __forceinline__ BzPage bz_page(const int* blob, int p, const BzLimits& lim) {
  const int* r = blob + (size_t)p * BZ_REC;
  BzPage g;
  g.src = reinterpret_cast<const unsigned char*>((unsigned long long)page_word64(r, 0));
  g.h = r[2], g.w = r[3], g.ch = r[4];
  g.packed_at = page_word64(r, 6), g.sat_at = page_word64(r, 14);
  g.ok = g.h >= 1 && g.w >= 1 && g.h <= BZ_MAX_SIDE && g.w <= BZ_MAX_SIDE && g.src != nullptr && (g.ch == 1 || g.ch == 3);
  g.row_words = g.ok ? (g.w + 31) >> 5 : 0;
  g.pack_ok = g.ok && g.packed_at >= 0 && g.packed_at + (long long)g.h * g.row_words <= lim.packed_words;
  g.sat_ok = g.ok && g.sat_at >= 0 && g.sat_at + (long long)g.h * g.w <= lim.sat_words;
  return g;
}

// ------------------------------------------------------------------------------------------------ test and histogram
constexpr int TH_THREADS = 256, TH_COPIES = 8, TH_STRIDE = 257;  // 257: the copies of one bin lie in different LDS banks
// flags[p] |= 1 where page p has a pixel with B != G or G != R; -1 for a record that is no page.  flags and hist are zero
// before the launch.  hist: uint32 [n_pages][256] of the page's first channel, or null.
__global__ __launch_bounds__(TH_THREADS) void k_bin_test_hist(const int* __restrict__ blob, int* __restrict__ flags,
                                                              unsigned* __restrict__ hist) {
  __shared__ unsigned lh[TH_COPIES * TH_STRIDE];
  const int p = blockIdx.y, t = threadIdx.x;
  const BzPage g = bz_page(blob, p, BzLimits{0, 0});
  if (!g.ok) {  // the whole block
    if (blockIdx.x == 0 && t == 0) atomicOr(flags + p, -1);
    return;
  }
  const bool count = hist != nullptr;  // uniform in the launch
  if (count) {
    for (int i = t; i < TH_COPIES * TH_STRIDE; i += TH_THREADS) lh[i] = 0u;
    __syncthreads();
  }
  const long long n = (long long)g.h * g.w;
  unsigned* mine = lh + (t & (TH_COPIES - 1)) * TH_STRIDE;
  unsigned bad = 0;
  for (long long i = (long long)blockIdx.x * TH_THREADS + t; i < n; i += (long long)gridDim.x * TH_THREADS) {
    const unsigned char* px = g.src + (size_t)i * g.ch;
    const unsigned v = px[0];
    if (g.ch == 3) {
      const unsigned gg = px[1], rr = px[2];
      bad |= (v ^ gg) | (gg ^ rr);
    }
    if (count) atomicAdd(mine + v, 1u);
  }
  if (count) {
    __syncthreads();
    unsigned s = 0;
#pragma unroll
    for (int c = 0; c < TH_COPIES; ++c) s += lh[c * TH_STRIDE + t];  // TH_THREADS == 256: thread t owns bin t
    if (s) atomicAdd(hist + (size_t)p * 256 + t, s);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o);
  if ((t & 63) == 0 && bad) atomicOr(flags + p, 1);
}

// ------------------------------------------------------------------------------------------------ Otsu's threshold
constexpr int OT_THREADS = 256;
// thresholds[p] = the smallest t in 0..254 with both classes non-empty whose sigma(t) = double(d) * double(d) / double(w0 w1),
// d = m1 w0 - m0 w1, is the largest; 0 where no t has both classes (a uniform page, an absent one).  Three IEEE operations in
// that order: the pragma keeps the compiler from fusing, the build has no fast-math to let it reassociate.
__global__ __launch_bounds__(OT_THREADS) void k_bin_otsu(const unsigned* __restrict__ hist, int* __restrict__ thresholds) {
#pragma clang fp contract(off)
  __shared__ long long cw[OT_THREADS], cm[OT_THREADS];
  __shared__ double best[OT_THREADS];
  __shared__ int best_t[OT_THREADS];
  const int p = blockIdx.x, t = threadIdx.x;
  const long long hv = (long long)hist[(size_t)p * 256 + t];
  cw[t] = hv;
  cm[t] = hv * t;
  __syncthreads();
  for (int o = 1; o < OT_THREADS; o <<= 1) {  // inclusive scans of the counts and of the first moments
    const long long aw = t >= o ? cw[t - o] : 0ll, am = t >= o ? cm[t - o] : 0ll;
    __syncthreads();
    cw[t] += aw;
    cm[t] += am;
    __syncthreads();
  }
  const long long w0 = cw[t], m0 = cm[t], w1 = cw[OT_THREADS - 1] - w0, m1 = cm[OT_THREADS - 1] - m0;
  double sigma = -1.0;  // below every sigma of a threshold that counts
  if (t < 255 && w0 > 0 && w1 > 0) {
    const long long d = m1 * w0 - m0 * w1;
    const double dd = (double)d;
    const double sq = dd * dd;
    sigma = sq / (double)(w0 * w1);
  }
  best[t] = sigma;
  best_t[t] = t;
  __syncthreads();
  for (int o = OT_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) {
      const double a = best[t], b = best[t + o];
      if (b > a || (b == a && best_t[t + o] < best_t[t])) {
        best[t] = b;
        best_t[t] = best_t[t + o];
      }
    }
    __syncthreads();
  }
  if (t == 0) thresholds[p] = best[0] >= 0.0 ? best_t[0] : 0;
}

// ------------------------------------------------------------------------------------------------ pack
constexpr int PK_THREADS = 256;
// the two words of a wave's ballot over 64 pixels of row y, from column 64 c on, into the packed row
__device__ __forceinline__ void bz_store_ballot(unsigned* __restrict__ packed, const BzPage& g, int y, int c, int lane, bool black) {
  const unsigned long long m = __ballot(black);
  unsigned* row = packed + g.packed_at + (long long)y * g.row_words;
  if (lane == 0) row[2 * c] = __brev((unsigned)m);
  if (lane == 1 && 2 * c + 1 < g.row_words) row[2 * c + 1] = __brev((unsigned)(m >> 32));
}

__global__ __launch_bounds__(PK_THREADS) void k_bin_otsu_pack(const int* __restrict__ blob, BzLimits lim, const int* __restrict__ thresholds,
                                                              unsigned* __restrict__ packed) {
  const int p = blockIdx.y;
  const BzPage g = bz_page(blob, p, lim);
  if (!g.pack_ok) return;  // the whole block
  const unsigned thr = (unsigned)thresholds[p];
  const int lane = threadIdx.x & 63, chunks = (g.w + 63) >> 6;
  const long long units = (long long)g.h * chunks, waves = (long long)gridDim.x * (PK_THREADS / 64);
  for (long long u = (long long)blockIdx.x * (PK_THREADS / 64) + (threadIdx.x >> 6); u < units; u += waves) {  // uniform in a wave
    const int y = (int)(u / chunks), c = (int)(u - (long long)y * chunks), x = c * 64 + lane;
    const bool black = x < g.w && (unsigned)g.src[((size_t)y * g.w + x) * g.ch] <= thr;
    bz_store_ballot(packed, g, y, c, lane, black);
  }
}

// ------------------------------------------------------------------------------------------------ adaptive: the table
constexpr int RS_THREADS = 256;
__global__ __launch_bounds__(RS_THREADS) void k_bin_row_scan(const int* __restrict__ blob, BzLimits lim, unsigned* __restrict__ sat) {
  const int p = blockIdx.y;
  const BzPage g = bz_page(blob, p, lim);
  if (!g.sat_ok) return;  // the whole block
  const int lane = threadIdx.x & 63, chunks = (g.w + 63) >> 6;
  const int waves = (int)gridDim.x * (RS_THREADS / 64);
  for (int y = (int)blockIdx.x * (RS_THREADS / 64) + (threadIdx.x >> 6); y < g.h; y += waves) {  // uniform in a wave
    unsigned* row = sat + g.sat_at + (long long)y * g.w;
    const unsigned char* src = g.src + (size_t)y * g.w * g.ch;
    unsigned carry = 0;
    for (int c = 0; c < chunks; ++c) {
      const int x = c * 64 + lane;
      unsigned v = x < g.w ? (unsigned)src[(size_t)x * g.ch] : 0u;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(v, o);
        if (lane >= o) v += up;
      }
      v += carry;
      if (x < g.w) row[x] = v;
      carry = __shfl(v, 63);
    }
  }
}

constexpr int CS_WAVES = 16, CS_THREADS = CS_WAVES * 64;
__global__ __launch_bounds__(CS_THREADS) void k_bin_col_scan(const int* __restrict__ blob, BzLimits lim, unsigned* __restrict__ sat) {
  __shared__ unsigned tot[CS_WAVES][64];
  const int p = blockIdx.y;
  const BzPage g = bz_page(blob, p, lim);
  if (!g.sat_ok || (int)blockIdx.x * 64 >= g.w) return;  // the whole block
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, x = (int)blockIdx.x * 64 + lane;
  const int seg = (g.h + CS_WAVES - 1) / CS_WAVES, y0 = min(wv * seg, g.h), y1 = min(y0 + seg, g.h);
  unsigned* col = sat + g.sat_at + x;
  unsigned s = 0;
  if (x < g.w)
    for (int y = y0; y < y1; ++y) s += col[(long long)y * g.w];
  tot[wv][lane] = s;
  __syncthreads();
  unsigned run = 0;
  for (int k = 0; k < wv; ++k) run += tot[k][lane];
  if (x < g.w)
    for (int y = y0; y < y1; ++y) {
      run += col[(long long)y * g.w];  // wraps beyond 2^32: see the head of the file
      col[(long long)y * g.w] = run;
    }
}

// black iff p n 20 <= S 17, n and S the pixel count and the sum of the window rows [y - r, y + r] x columns [x - r, x + r]
// clipped to the page, r = max(1, max(h, w) / 16)
__global__ __launch_bounds__(PK_THREADS) void k_bin_adaptive_pack(const int* __restrict__ blob, BzLimits lim, const unsigned* __restrict__ sat,
                                                                  unsigned* __restrict__ packed) {
  const int p = blockIdx.y;
  const BzPage g = bz_page(blob, p, lim);
  if (!g.pack_ok || !g.sat_ok) return;  // the whole block
  const unsigned* a = sat + g.sat_at;
  const int r = max(1, max(g.h, g.w) / 16);
  const int lane = threadIdx.x & 63, chunks = (g.w + 63) >> 6;
  const long long units = (long long)g.h * chunks, waves = (long long)gridDim.x * (PK_THREADS / 64);
  for (long long u = (long long)blockIdx.x * (PK_THREADS / 64) + (threadIdx.x >> 6); u < units; u += waves) {  // uniform in a wave
    const int y = (int)(u / chunks), c = (int)(u - (long long)y * chunks), x = c * 64 + lane;
    bool black = false;
    if (x < g.w) {
      const int ya = max(y - r, 0) - 1, yb = min(y + r, g.h - 1), xa = max(x - r, 0) - 1, xb = min(x + r, g.w - 1);  // ya, xa: -1 = none
      const unsigned a11 = a[(long long)yb * g.w + xb];
      const unsigned a01 = ya >= 0 ? a[(long long)ya * g.w + xb] : 0u;
      const unsigned a10 = xa >= 0 ? a[(long long)yb * g.w + xa] : 0u;
      const unsigned a00 = ya >= 0 && xa >= 0 ? a[(long long)ya * g.w + xa] : 0u;
      const unsigned sum = a11 - a01 - a10 + a00;  // modulo 2^32, and below 2^31: exact
      const unsigned long long n = (unsigned long long)(yb - ya) * (unsigned long long)(xb - xa);
      const unsigned long long v = g.src[((size_t)y * g.w + x) * g.ch];
      black = v * n * 20ull <= (unsigned long long)sum * 17ull;
    }
    bz_store_ballot(packed, g, y, c, lane, black);
  }
}

static void bz_check_table(const int* blob_dev, int64_t blob_words, int n_pages) {
  check_page_table(blob_dev, blob_words, n_pages, BZ_REC, 3, 4096, "0..4096 pages", "page table: n records");
}
// a pixel per thread and step, sixteen steps where the largest page has that many; 512 blocks per page at the most
static unsigned bz_pixel_blocks(int64_t max_pixels) {
  const int64_t per_block = (int64_t)PK_THREADS * 16;
  return (unsigned)std::min<int64_t>(std::max<int64_t>((max_pixels + per_block - 1) / per_block, 1), 512);
}

}  // namespace ymk

extern "C" {

int ymk_bin_scratch_bytes(const int* h, const int* w, int n_pages, int64_t* sizes2_out) {
  YMK_API_BEGIN
  YMK_CHECK(n_pages >= 0 && n_pages <= 4096 && sizes2_out && (n_pages == 0 || (h && w)), "bad argument");
  int64_t cells = 0;
  for (int k = 0; k < n_pages; ++k) {
    YMK_CHECK(h[k] >= 1 && w[k] >= 1 && h[k] <= ymk::BZ_MAX_SIDE && w[k] <= ymk::BZ_MAX_SIDE, "a page has 1..16383 pixels on a side");
    cells += (int64_t)h[k] * w[k];
  }
  sizes2_out[0] = (int64_t)n_pages * 256 * 4;
  sizes2_out[1] = ((cells + 1) & ~1LL) * 4;
  YMK_API_END
}

int ymk_bin_test_hist(const int* blob_dev, int64_t blob_words, int n_pages, int64_t max_pixels, int* flags_dev, uint32_t* hist_dev,
                      void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(max_pixels >= 0 && max_pixels <= 16383LL * 16383LL, "bad argument");
  if (n_pages == 0) return 0;
  ymk::bz_check_table(blob_dev, blob_words, n_pages);
  YMK_CHECK(flags_dev && ((uintptr_t)flags_dev & 3) == 0, "null or misaligned flags");
  YMK_CHECK(((uintptr_t)hist_dev & 3) == 0, "misaligned histograms");
  const hipStream_t s = (hipStream_t)stream;
  YMK_HIP(hipMemsetAsync(flags_dev, 0, (size_t)n_pages * sizeof(int), s));
  if (hist_dev) YMK_HIP(hipMemsetAsync(hist_dev, 0, (size_t)n_pages * 256 * sizeof(uint32_t), s));
  hipLaunchKernelGGL(ymk::k_bin_test_hist, dim3(ymk::bz_pixel_blocks(max_pixels), (unsigned)n_pages), dim3(ymk::TH_THREADS), 0, s,
                     blob_dev, flags_dev, (unsigned*)hist_dev);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}

int ymk_bin_otsu(int n_pages, const uint32_t* hist_dev, int* thresholds_dev, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(n_pages >= 0 && n_pages <= 4096, "0..4096 pages");
  if (n_pages == 0) return 0;
  YMK_CHECK(hist_dev && ((uintptr_t)hist_dev & 3) == 0 && thresholds_dev && ((uintptr_t)thresholds_dev & 3) == 0,
            "null or misaligned histograms / thresholds");
  hipLaunchKernelGGL(ymk::k_bin_otsu, dim3((unsigned)n_pages), dim3(ymk::OT_THREADS), 0, (hipStream_t)stream, (const unsigned*)hist_dev,
                     thresholds_dev);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}

int ymk_bin_otsu_pack(const int* blob_dev, int64_t blob_words, int n_pages, int64_t max_pixels, const int* thresholds_dev,
                      uint32_t* packed_dev, int64_t packed_bytes, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(max_pixels >= 0 && max_pixels <= 16383LL * 16383LL && packed_bytes >= 0, "bad argument");
  if (n_pages == 0) return 0;
  ymk::bz_check_table(blob_dev, blob_words, n_pages);
  YMK_CHECK(thresholds_dev && ((uintptr_t)thresholds_dev & 3) == 0, "null or misaligned thresholds");
  ymk::check_aligned8(packed_dev, "packed rows: 8-byte aligned");
  const ymk::BzLimits lim{packed_bytes / 4, 0};
  hipLaunchKernelGGL(ymk::k_bin_otsu_pack, dim3(ymk::bz_pixel_blocks(max_pixels), (unsigned)n_pages), dim3(ymk::PK_THREADS), 0,
                     (hipStream_t)stream, blob_dev, lim, thresholds_dev, (unsigned*)packed_dev);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}

int ymk_bin_adaptive_pack(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, uint32_t* sat_dev, int64_t sat_bytes,
                          uint32_t* packed_dev, int64_t packed_bytes, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(max_h >= 1 && max_w >= 1 && max_h <= ymk::BZ_MAX_SIDE && max_w <= ymk::BZ_MAX_SIDE && sat_bytes >= 0 && packed_bytes >= 0,
            "bad argument");
  if (n_pages == 0) return 0;
  ymk::bz_check_table(blob_dev, blob_words, n_pages);
  ymk::check_aligned8(sat_dev, "summed-area tables: 8-byte aligned");
  ymk::check_aligned8(packed_dev, "packed rows: 8-byte aligned");
  const ymk::BzLimits lim{packed_bytes / 4, sat_bytes / 4};
  const hipStream_t s = (hipStream_t)stream;
  const unsigned rows_x = (unsigned)((max_h + ymk::RS_THREADS / 64 - 1) / (ymk::RS_THREADS / 64));  // a wave per row
  hipLaunchKernelGGL(ymk::k_bin_row_scan, dim3(rows_x, (unsigned)n_pages), dim3(ymk::RS_THREADS), 0, s, blob_dev, lim, (unsigned*)sat_dev);
  YMK_HIP(hipGetLastError());
  hipLaunchKernelGGL(ymk::k_bin_col_scan, dim3((unsigned)((max_w + 63) / 64), (unsigned)n_pages), dim3(ymk::CS_THREADS), 0, s, blob_dev, lim,
                     (unsigned*)sat_dev);
  YMK_HIP(hipGetLastError());
  hipLaunchKernelGGL(ymk::k_bin_adaptive_pack, dim3(ymk::bz_pixel_blocks((int64_t)max_h * max_w), (unsigned)n_pages), dim3(ymk::PK_THREADS), 0, s,
                     blob_dev, lim, (const unsigned*)sat_dev, (unsigned*)packed_dev);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}
}
