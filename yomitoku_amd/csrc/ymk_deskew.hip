// Page skew: the pages of a wave estimated and turned upright on the device (include/ymk.h, "Page skew"; yomitoku_amd/deskew.py;
// DESIGN.md, "Page skew").  tests/deskew_ref.py is the definition; every stage equals it bit for bit - all of it is integer
// arithmetic, and integer additions commute, so no order of the atomics below can change a result.
//
//   k_dsk_luma      Y = (29 B + 150 G + 77 R + 128) >> 8 of every three-channel page into its plane: four pixels a thread, three
//                   32-bit loads and one 32-bit store where the page is 4-byte aligned.  A one-channel page is its own plane.
//   k_dsk_planes    one thread per page: the binariser's record of the page's plane (one channel, the plane's address), so that
//                   ymk_bin_adaptive_pack - unchanged - writes the ink of the plane as packed rows; zeros for a record that is no page.
//   k_dsk_scores    the hot path.  One block per (page, angle, axis), the profile of that axis in LDS (uint32 [DK_BINS], 63 KiB).
//                   A thread takes packed 32-pixel words and skips the zero ones - most of a document.  ROW profile: along a row
//                   the bin y c + x s changes only every 2^14 / |s| >= 11 pixels at the default angles, so an atomic per ink
//                   pixel would queue a wave's lanes on one address; the word is cut at its bin boundaries instead (one division
//                   per piece) and adds one popcount per (word, bin).  COLUMN profile: consecutive pixels fall into consecutive
//                   bins, one atomic per set bit.  Then sum_b (P[b + 1] - P[b])^2 in 64 bits, a shuffle reduction per wave, the
//                   waves' sums through LDS, one 64-bit atomic per block into S[page][angle] (zeroed before the launch).
//   k_dsk_choose    one wave per page: arg-max with the tie rule (smallest |k|, then the negative k), dead band, 9 / 8 margin.
//   k_dsk_rotate    reads the page's k from the choice words - the host never waits for the decision - and writes the turned page
//                   (k = 0: a copy) four bytes a thread: one 32-bit store, 32-bit loads for the copy.  The four taps of the
//                   bilinear blend are byte loads - their address has no alignment - and 255 outside the page.
//
// Bins.  m(n) = ceil((n - 1) s_max / 2^14), s_max the largest |s| of the table.  Row bins: (y c + x s + (m(w) << 14)) >> 14 lies in
// 0 .. h + 2 m(w) - 1 for 0 < c <= 2^14; column bins in 0 .. w + 2 m(h) - 1.  A page is estimated when both counts are at most
// DK_BINS = 16128: at the default 5 degrees (s_max = 1428) every page up to 13700 x 13700, at 401 angles of 0.1 degree (20
// degrees) up to 9500 x 9500.  A larger page scores 0 everywhere, k = 0, flag 0: it is copied, not failed.
// No overflow: |y c|, |x s| <= 16382 * 2^14 < 2^28 and m << 14 <= 2^28: below 2^30.  The rotation: see k_dsk_rotate.

#include "ymk_pages.h"

#include "../../include/ymk.h"

namespace ymk {

constexpr int DK_REC = YMK_DSK_PAGE_WORDS;
static_assert(DK_REC == YMK_G4_PAGE_WORDS, "k_dsk_planes writes records the binariser reads");
constexpr int DK_MAX_SIDE = 16383, DK_SHIFT = 14, DK_ONE = 1 << DK_SHIFT;
constexpr int DK_BINS = 16128;  // 63 KiB of uint32: under the 64 KiB a block may declare
constexpr int DK_MAX_ANGLES = 401;
constexpr int DK_CHOICE = YMK_DSK_CHOICE_WORDS;

struct DkLimits {
  long long packed_words, sat_words, luma_bytes;
};

__host__ __device__ __forceinline__ int dk_margin(int n, int s_max) {
  return (int)(((long long)(n - 1) * s_max + DK_ONE - 1) >> DK_SHIFT);
}
__host__ __device__ __forceinline__ bool dk_fits(int h, int w, int s_max) {
  return h + 2 * dk_margin(w, s_max) <= DK_BINS && w + 2 * dk_margin(h, s_max) <= DK_BINS;
}

// A page's record, read and checked against the buffers' sizes as bz_page of ymk_binarize.hip does: a kernel takes a page whose
// record fails the check for what it touches as absent.
struct DkPage {
  const unsigned char* src;
  unsigned char* dst;
  int h, w, ch, row_words;
  long long packed_at, luma_at, sat_at;
  bool ok, plane_ok, est_ok, dst_ok;
};
__device__ __forceinline__ DkPage dk_page(const int* blob, int p, const DkLimits& lim) {
  const int* r = blob + (size_t)p * DK_REC;
  DkPage g;
  g.src = reinterpret_cast<const unsigned char*>((unsigned long long)page_word64(r, 0));
  g.dst = reinterpret_cast<unsigned char*>((unsigned long long)page_word64(r, 11));
  g.h = r[2], g.w = r[3], g.ch = r[4];
  g.packed_at = page_word64(r, 6), g.luma_at = page_word64(r, 8), g.sat_at = page_word64(r, 14);
  g.ok = g.h >= 1 && g.w >= 1 && g.h <= DK_MAX_SIDE && g.w <= DK_MAX_SIDE && g.src != nullptr && (g.ch == 1 || g.ch == 3);
  g.row_words = g.ok ? (g.w + 31) >> 5 : 0;
  // the plane: the page itself, or h w bytes of luma_dev at a multiple of 4
  g.plane_ok = g.ok && (g.ch == 1 || (g.luma_at >= 0 && (g.luma_at & 3) == 0 && g.luma_at + (long long)g.h * g.w <= lim.luma_bytes));
  g.est_ok = g.plane_ok && g.packed_at >= 0 && g.packed_at + (long long)g.h * g.row_words <= lim.packed_words && g.sat_at >= 0 &&
             g.sat_at + (long long)g.h * g.w <= lim.sat_words;
  g.dst_ok = g.ok && g.dst != nullptr && ((unsigned long long)g.dst & 3) == 0 && g.dst != g.src;
  return g;
}

// ------------------------------------------------------------------------------------------------ luminance
constexpr int LM_THREADS = 256;
__device__ __forceinline__ unsigned dk_luma(unsigned b, unsigned g, unsigned r) { return (29u * b + 150u * g + 77u * r + 128u) >> 8; }

__global__ __launch_bounds__(LM_THREADS) void k_dsk_luma(const int* __restrict__ blob, DkLimits lim, unsigned char* __restrict__ luma) {
  const int p = blockIdx.y;
  const DkPage g = dk_page(blob, p, lim);
  if (!g.plane_ok || g.ch != 3) return;  // the whole block
  unsigned char* out = luma + g.luma_at;
  const long long n = (long long)g.h * g.w, groups = (n + 3) >> 2;
  const bool aligned = ((unsigned long long)g.src & 3) == 0 && ((unsigned long long)luma & 3) == 0;
  for (long long q = (long long)blockIdx.x * LM_THREADS + threadIdx.x; q < groups; q += (long long)gridDim.x * LM_THREADS) {
    const long long i0 = q << 2;
    if (aligned && i0 + 4 <= n) {
      const unsigned* s3 = reinterpret_cast<const unsigned*>(g.src + i0 * 3);  // 12 bytes: B G R B | G R B G | R B G R
      const unsigned a = s3[0], b = s3[1], c = s3[2];
      const unsigned y0 = dk_luma(a & 255u, (a >> 8) & 255u, (a >> 16) & 255u);
      const unsigned y1 = dk_luma(a >> 24, b & 255u, (b >> 8) & 255u);
      const unsigned y2 = dk_luma((b >> 16) & 255u, b >> 24, c & 255u);
      const unsigned y3 = dk_luma((c >> 8) & 255u, (c >> 16) & 255u, c >> 24);
      *reinterpret_cast<unsigned*>(out + i0) = y0 | (y1 << 8) | (y2 << 16) | (y3 << 24);
    } else {
      for (long long i = i0; i < min(i0 + 4, n); ++i) out[i] = (unsigned char)dk_luma(g.src[i * 3], g.src[i * 3 + 1], g.src[i * 3 + 2]);
    }
  }
}

// the binariser's table of the planes: record p = page p's h, w, one channel, the plane's address, the packed rows' and the
// table's places; zeros - no page - for a record that is none
__global__ void k_dsk_planes(const int* __restrict__ blob, DkLimits lim, int n_pages, const unsigned char* __restrict__ luma,
                             int* __restrict__ planes) {
  const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (p >= n_pages) return;
  const DkPage g = dk_page(blob, p, lim);
  const int* r = blob + (size_t)p * DK_REC;
  int* o = planes + (size_t)p * DK_REC;
  for (int k = 0; k < DK_REC; ++k) o[k] = 0;
  if (!g.est_ok) return;
  const unsigned long long at = (unsigned long long)(g.ch == 1 ? g.src : luma + g.luma_at);
  o[0] = (int)(unsigned)at, o[1] = (int)(unsigned)(at >> 32);
  o[2] = g.h, o[3] = g.w, o[4] = 1;
  o[6] = r[6], o[7] = r[7], o[14] = r[14], o[15] = r[15];
}

// ------------------------------------------------------------------------------------------------ scores
constexpr int SC_THREADS = 512;
__global__ __launch_bounds__(SC_THREADS) void k_dsk_scores(const int* __restrict__ blob, DkLimits lim, const unsigned* __restrict__ packed,
                                                           const int* __restrict__ table, int n_angles, int s_max,
                                                           unsigned long long* __restrict__ scores) {
  __shared__ unsigned prof[DK_BINS];
  __shared__ unsigned long long part[SC_THREADS / 64];
  const int p = blockIdx.y, a = (int)blockIdx.x >> 1, axis = (int)blockIdx.x & 1, t = threadIdx.x;
  const DkPage g = dk_page(blob, p, lim);
  if (!g.est_ok || a >= n_angles || !dk_fits(g.h, g.w, s_max)) return;  // the whole block: S stays 0
  const int s = table[2 * a], c = table[2 * a + 1];
  if (c <= 0 || c > DK_ONE || s > s_max || s < -s_max) return;  // no entry of a table this launch's bins were sized for
  const int mr = dk_margin(g.w, s_max), mq = dk_margin(g.h, s_max);
  const int nb = axis ? g.w + 2 * mq : g.h + 2 * mr;
  for (int i = t; i < nb; i += SC_THREADS) prof[i] = 0u;
  __syncthreads();
  const unsigned* rows = packed + g.packed_at;
  const int n_words = g.h * g.row_words;  // at most 16383 * 512
  for (int i = t; i < n_words; i += SC_THREADS) {
    unsigned wd = rows[i];
    if (!wd) continue;
    const int y = i / g.row_words, x0 = (i - y * g.row_words) << 5;
    if (axis == 0) {
      // pixel x0 + j is bit 31 - j; wd is kept shifted so that the next pixel is bit 31.  v: the next pixel's y c + x s + offset
      int v = y * c + x0 * s + (mr << DK_SHIFT), left = 32;
      while (wd) {
        const int b = v >> DK_SHIFT;
        int n = 32;  // how many pixels from here on share bin b
        if (s > 0) n = (((b + 1) << DK_SHIFT) - v + s - 1) / s;
        if (s < 0) n = (v - (b << DK_SHIFT)) / (-s) + 1;
        n = min(n, left);
        const unsigned head = n >= 32 ? 0xffffffffu : ~(0xffffffffu >> n);
        const unsigned cnt = (unsigned)__popc(wd & head);
        if (cnt && (unsigned)b < (unsigned)nb) atomicAdd(prof + b, cnt);
        wd = n >= 32 ? 0u : wd << n;
        v += n * s;
        left -= n;
      }
    } else {
      const int base = x0 * c - y * s + (mq << DK_SHIFT);
      while (wd) {
        const int j = __clz((int)wd);
        wd &= ~(0x80000000u >> j);
        const int b = (base + j * c) >> DK_SHIFT;
        if ((unsigned)b < (unsigned)nb) atomicAdd(prof + b, 1u);
      }
    }
  }
  __syncthreads();
  unsigned long long acc = 0;
  for (int b = t; b <= nb; b += SC_THREADS) {  // P[b] - P[b - 1] for b = 0 .. nb, the bins below 0 and from nb on being empty
    const long long d = (long long)(b < nb ? prof[b] : 0u) - (long long)(b > 0 ? prof[b - 1] : 0u);
    acc += (unsigned long long)(d * d);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((t & 63) == 0) part[t >> 6] = acc;
  __syncthreads();
  if (t == 0) {
    unsigned long long total = 0;
    for (int k = 0; k < SC_THREADS / 64; ++k) total += part[k];
    atomicAdd(scores + (size_t)p * n_angles + a, total);  // the other axis's block adds the other half
  }
}

// ------------------------------------------------------------------------------------------------ choice
__device__ __forceinline__ bool dk_better(unsigned long long s1, int k1, unsigned long long s2, int k2) {
  const int a1 = k1 < 0 ? -k1 : k1, a2 = k2 < 0 ? -k2 : k2;
  return s1 > s2 || (s1 == s2 && (a1 < a2 || (a1 == a2 && k1 < k2)));
}
// choice[p]: word 0 k (0: leave the page as it is), word 1 the flag - 1 estimated, 0 a page too large for the profile, -1 no page -,
// words 2-3 the largest S (uint64), 4-5 S_0, 6-7 zero
__global__ __launch_bounds__(64) void k_dsk_choose(const int* __restrict__ blob, DkLimits lim, const unsigned long long* __restrict__ scores,
                                                   int n_angles, int s_max, int dead, int* __restrict__ choice) {
  const int p = blockIdx.x, lane = threadIdx.x, K = n_angles >> 1;
  const DkPage g = dk_page(blob, p, lim);
  unsigned long long best = 0;
  int bk = 1 << 20;  // loses every tie
  for (int a = lane; a < n_angles; a += 64) {
    const unsigned long long sv = scores[(size_t)p * n_angles + a];
    if (dk_better(sv, a - K, best, bk)) best = sv, bk = a - K;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long so = __shfl_xor(best, o);
    const int ko = __shfl_xor(bk, o);
    if (dk_better(so, ko, best, bk)) best = so, bk = ko;
  }
  if (lane == 0) {
    const unsigned long long zero = scores[(size_t)p * n_angles + K];
    int k = bk;
    if ((k < 0 ? -k : k) < dead || 8ull * best < 9ull * zero) k = 0;  // S < 2^48: no wrap
    int* o = choice + (size_t)p * DK_CHOICE;
    o[0] = k;
    o[1] = !g.est_ok ? -1 : dk_fits(g.h, g.w, s_max) ? 1 : 0;
    o[2] = (int)(unsigned)best, o[3] = (int)(unsigned)(best >> 32);
    o[4] = (int)(unsigned)zero, o[5] = (int)(unsigned)(zero >> 32);
    o[6] = o[7] = 0;
  }
}

// ------------------------------------------------------------------------------------------------ rotation
constexpr int RT_THREADS = 256;
// u = 2 X - (w - 1), v = 2 Y - (h - 1); SX = c u + s v + ((w - 1) << 14), SY = -s u + c v + ((h - 1) << 14): |c u|, |s v| <=
// 2^14 * 16382 < 2^28 and (w - 1) << 14 < 2^28, so |SX|, |SY| < 3 * 2^28: 32 bits hold them.  The blend is at most
// 2^16 * 255 + 2^15 < 2^24.
__global__ __launch_bounds__(RT_THREADS) void k_dsk_rotate(const int* __restrict__ blob, const int* __restrict__ table, int n_angles,
                                                           const int* __restrict__ choice) {
  const int p = blockIdx.y, K = n_angles >> 1;
  const DkPage g = dk_page(blob, p, DkLimits{0, 0, 0});
  if (!g.dst_ok) return;  // the whole block
  int k = choice[(size_t)p * DK_CHOICE];
  if (k < -K || k > K) k = 0;
  const int s = table[2 * (k + K)], c = table[2 * (k + K) + 1];
  const long long n = (long long)g.h * g.w * g.ch, groups = (n + 3) >> 2;
  const bool src_aligned = ((unsigned long long)g.src & 3) == 0;
  const int h = g.h, w = g.w, ch = g.ch;
  for (long long q = (long long)blockIdx.x * RT_THREADS + threadIdx.x; q < groups; q += (long long)gridDim.x * RT_THREADS) {
    const long long i0 = q << 2;
    const int count = (int)min(4ll, n - i0);
    unsigned word = 0;
    if (k == 0) {
      if (src_aligned && count == 4) word = *reinterpret_cast<const unsigned*>(g.src + i0);
      else
        for (int j = 0; j < count; ++j) word |= (unsigned)g.src[i0 + j] << (8 * j);
    } else {
      const long long px = ch == 3 ? i0 / 3 : i0;
      int chn = (int)(i0 - px * ch), Y = (int)(px / w), X = (int)(px - (long long)Y * w);
      int w00 = 0, w10 = 0, w01 = 0, w11 = 0;
      long long a00 = -1, a10 = -1, a01 = -1, a11 = -1;  // byte offsets of the taps' channel 0; -1: outside, paper
      for (int j = 0; j < count; ++j) {
        if (j == 0 || chn == 0) {
          const int u = 2 * X - (w - 1), v = 2 * Y - (h - 1);
          const int sx = c * u + s * v + ((w - 1) << DK_SHIFT), sy = -s * u + c * v + ((h - 1) << DK_SHIFT);
          const int x0 = sx >> 15, fx = (sx >> 7) & 255, y0 = sy >> 15, fy = (sy >> 7) & 255;
          w00 = (256 - fx) * (256 - fy), w10 = fx * (256 - fy), w01 = (256 - fx) * fy, w11 = fx * fy;
          const bool xa = x0 >= 0 && x0 < w, xb = x0 + 1 >= 0 && x0 + 1 < w, ya = y0 >= 0 && y0 < h, yb = y0 + 1 >= 0 && y0 + 1 < h;
          const long long at = ((long long)y0 * w + x0) * ch;
          a00 = xa && ya ? at : -1;
          a10 = xb && ya ? at + ch : -1;
          a01 = xa && yb ? at + (long long)w * ch : -1;
          a11 = xb && yb ? at + (long long)w * ch + ch : -1;
        }
        const unsigned p00 = a00 >= 0 ? g.src[a00 + chn] : 255u, p10 = a10 >= 0 ? g.src[a10 + chn] : 255u;
        const unsigned p01 = a01 >= 0 ? g.src[a01 + chn] : 255u, p11 = a11 >= 0 ? g.src[a11 + chn] : 255u;
        word |= (((unsigned)w00 * p00 + (unsigned)w10 * p10 + (unsigned)w01 * p01 + (unsigned)w11 * p11 + 32768u) >> 16) << (8 * j);
        if (++chn == ch) {
          chn = 0;
          if (++X == w) X = 0, ++Y;
        }
      }
    }
    if (count == 4) *reinterpret_cast<unsigned*>(g.dst + i0) = word;
    else
      for (int j = 0; j < count; ++j) g.dst[i0 + j] = (unsigned char)(word >> (8 * j));
  }
}

// ------------------------------------------------------------------------------------------------ host
static void dk_check_table(const int* blob_dev, int64_t blob_words, int n_pages) {
  check_page_table(blob_dev, blob_words, n_pages, DK_REC, 3, 4096, "0..4096 pages", "page table: n records");
}
static void dk_check_angles(int n_angles, int s_max) {
  YMK_CHECK(n_angles >= 1 && n_angles <= DK_MAX_ANGLES && (n_angles & 1) == 1, "1..401 angles, an odd number");
  YMK_CHECK(s_max >= 0 && s_max < DK_ONE, "s_max in 0 .. 2^14 - 1");
}
static DkLimits dk_limits(int64_t packed_bytes, int64_t sat_bytes, int64_t luma_bytes) {
  YMK_CHECK(packed_bytes >= 0 && sat_bytes >= 0 && luma_bytes >= 0, "negative size");
  return DkLimits{packed_bytes / 4, sat_bytes / 4, luma_bytes};
}
// four bytes per thread and step, sixteen steps where the largest page has that many; 1024 blocks per page at the most
static unsigned dk_byte_blocks(int64_t bytes, int threads) {
  const int64_t per_block = (int64_t)threads * 4 * 16;
  return (unsigned)std::min<int64_t>(std::max<int64_t>((bytes + per_block - 1) / per_block, 1), 1024);
}

}  // namespace ymk

extern "C" {

int ymk_dsk_page_words(void) { return ymk::DK_REC; }

int ymk_dsk_check_angles(const int* table_host, int n_angles, int* s_max_out) {
  YMK_API_BEGIN
  YMK_CHECK(table_host && s_max_out, "bad argument");
  YMK_CHECK(n_angles >= 1 && n_angles <= ymk::DK_MAX_ANGLES && (n_angles & 1) == 1, "1..401 angles, an odd number");
  const int K = n_angles / 2;
  int s_max = 0;
  for (int a = 0; a < n_angles; ++a) {
    const int s = table_host[2 * a], c = table_host[2 * a + 1], sm = table_host[2 * (n_angles - 1 - a)], cm = table_host[2 * (n_angles - 1 - a) + 1];
    YMK_CHECK(c > 0 && c <= ymk::DK_ONE && s > -ymk::DK_ONE && s < ymk::DK_ONE, "an angle of the table: 0 < c <= 2^14, |s| < 2^14");
    YMK_CHECK(s == -sm && c == cm, "the table is symmetric about its middle");
    const long long norm = (long long)s * s + (long long)c * c, one = (long long)ymk::DK_ONE * ymk::DK_ONE;
    YMK_CHECK(norm >= one - 4 * ymk::DK_ONE && norm <= one + 4 * ymk::DK_ONE, "s^2 + c^2 = 2^28 to rounding");
    s_max = std::max(s_max, s < 0 ? -s : s);
  }
  YMK_CHECK(table_host[2 * K] == 0 && table_host[2 * K + 1] == ymk::DK_ONE, "the middle angle is 0");
  *s_max_out = s_max;
  YMK_API_END
}

int ymk_dsk_scratch_bytes(const int* h, const int* w, const int* ch, int n_pages, int n_angles, int s_max, int64_t* sizes5_out, int* fits_out) {
  YMK_API_BEGIN
  YMK_CHECK(n_pages >= 0 && n_pages <= 4096 && sizes5_out && (n_pages == 0 || (h && w && ch)), "bad argument");
  ymk::dk_check_angles(n_angles, s_max);
  int64_t luma = 0, cells = 0, words = 0;
  for (int k = 0; k < n_pages; ++k) {
    YMK_CHECK(h[k] >= 1 && w[k] >= 1 && h[k] <= ymk::DK_MAX_SIDE && w[k] <= ymk::DK_MAX_SIDE, "a page has 1..16383 pixels on a side");
    YMK_CHECK(ch[k] == 1 || ch[k] == 3, "a page has one or three channels");
    const int64_t px = (int64_t)h[k] * w[k];
    if (ch[k] == 3) luma += (px + 15) & ~15LL;
    cells += px;
    words += (int64_t)h[k] * ((w[k] + 31) >> 5);
    if (fits_out) fits_out[k] = ymk::dk_fits(h[k], w[k], s_max) ? 1 : 0;
  }
  sizes5_out[0] = luma;
  sizes5_out[1] = ((cells + 1) & ~1LL) * 4;
  sizes5_out[2] = ((words + 1) & ~1LL) * 4;
  sizes5_out[3] = (int64_t)n_pages * n_angles * 8;
  sizes5_out[4] = (int64_t)n_pages * ymk::DK_CHOICE * 4;
  YMK_API_END
}

int ymk_dsk_luma(const int* blob_dev, int64_t blob_words, int n_pages, int64_t max_pixels, unsigned char* luma_dev, int64_t luma_bytes,
                 int64_t packed_bytes, int64_t sat_bytes, int* planes_dev, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(max_pixels >= 0 && max_pixels <= 16383LL * 16383LL, "bad argument");
  if (n_pages == 0) return 0;
  ymk::dk_check_table(blob_dev, blob_words, n_pages);
  YMK_CHECK(luma_bytes == 0 || (luma_dev && ((uintptr_t)luma_dev & 7) == 0), "planes: 8-byte aligned");
  YMK_CHECK(planes_dev && ((uintptr_t)planes_dev & 3) == 0, "null or misaligned table of the planes");
  const ymk::DkLimits lim = ymk::dk_limits(packed_bytes, sat_bytes, luma_bytes);
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ymk::k_dsk_luma, dim3(ymk::dk_byte_blocks(max_pixels, ymk::LM_THREADS), (unsigned)n_pages), dim3(ymk::LM_THREADS), 0, s,
                     blob_dev, lim, luma_dev);
  YMK_HIP(hipGetLastError());
  hipLaunchKernelGGL(ymk::k_dsk_planes, dim3((unsigned)((n_pages + 63) / 64)), dim3(64), 0, s, blob_dev, lim, n_pages,
                     (const unsigned char*)luma_dev, planes_dev);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}

int ymk_dsk_scores(const int* blob_dev, int64_t blob_words, int n_pages, const uint32_t* packed_dev, int64_t packed_bytes, int64_t sat_bytes,
                   int64_t luma_bytes, const int* table_dev, int n_angles, int s_max, uint64_t* scores_dev, void* stream) {
  YMK_API_BEGIN
  ymk::dk_check_angles(n_angles, s_max);
  if (n_pages == 0) return 0;
  ymk::dk_check_table(blob_dev, blob_words, n_pages);
  ymk::check_aligned8(packed_dev, "packed rows: 8-byte aligned");
  ymk::check_aligned8(scores_dev, "scores: 8-byte aligned");
  YMK_CHECK(table_dev && ((uintptr_t)table_dev & 3) == 0, "null or misaligned angle table");
  const ymk::DkLimits lim = ymk::dk_limits(packed_bytes, sat_bytes, luma_bytes);
  const hipStream_t s = (hipStream_t)stream;
  YMK_HIP(hipMemsetAsync(scores_dev, 0, (size_t)n_pages * n_angles * sizeof(uint64_t), s));
  hipLaunchKernelGGL(ymk::k_dsk_scores, dim3(2u * (unsigned)n_angles, (unsigned)n_pages), dim3(ymk::SC_THREADS), 0, s, blob_dev, lim,
                     (const unsigned*)packed_dev, table_dev, n_angles, s_max, (unsigned long long*)scores_dev);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}

int ymk_dsk_choose(const int* blob_dev, int64_t blob_words, int n_pages, int64_t packed_bytes, int64_t sat_bytes, int64_t luma_bytes,
                   const uint64_t* scores_dev, int n_angles, int s_max, int dead, int* choice_dev, void* stream) {
  YMK_API_BEGIN
  ymk::dk_check_angles(n_angles, s_max);
  YMK_CHECK(dead >= 0, "bad argument");
  if (n_pages == 0) return 0;
  ymk::dk_check_table(blob_dev, blob_words, n_pages);
  ymk::check_aligned8(scores_dev, "scores: 8-byte aligned");
  ymk::check_aligned8(choice_dev, "choice words: 8-byte aligned");
  const ymk::DkLimits lim = ymk::dk_limits(packed_bytes, sat_bytes, luma_bytes);
  hipLaunchKernelGGL(ymk::k_dsk_choose, dim3((unsigned)n_pages), dim3(64), 0, (hipStream_t)stream, blob_dev, lim,
                     (const unsigned long long*)scores_dev, n_angles, s_max, dead, choice_dev);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}

int ymk_dsk_rotate(const int* blob_dev, int64_t blob_words, int n_pages, int64_t max_bytes, const int* table_dev, int n_angles,
                   const int* choice_dev, void* stream) {
  YMK_API_BEGIN
  ymk::dk_check_angles(n_angles, 0);
  YMK_CHECK(max_bytes >= 0 && max_bytes <= 3LL * 16383LL * 16383LL, "bad argument");
  if (n_pages == 0) return 0;
  ymk::dk_check_table(blob_dev, blob_words, n_pages);
  YMK_CHECK(table_dev && ((uintptr_t)table_dev & 3) == 0, "null or misaligned angle table");
  YMK_CHECK(choice_dev && ((uintptr_t)choice_dev & 3) == 0, "null or misaligned choice words");
  hipLaunchKernelGGL(ymk::k_dsk_rotate, dim3(ymk::dk_byte_blocks(max_bytes, ymk::RT_THREADS), (unsigned)n_pages), dim3(ymk::RT_THREADS), 0,
                     (hipStream_t)stream, blob_dev, table_dev, n_angles, choice_dev);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}

int ymk_dsk_pages(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, unsigned char* luma_dev, int64_t luma_bytes,
                  uint32_t* sat_dev, int64_t sat_bytes, uint32_t* packed_dev, int64_t packed_bytes, int* planes_dev, const int* table_dev,
                  int n_angles, int s_max, int dead, uint64_t* scores_dev, int* choice_dev, int rotate, void* stream) {
  if (ymk_dsk_luma(blob_dev, blob_words, n_pages, (int64_t)max_h * max_w, luma_dev, luma_bytes, packed_bytes, sat_bytes, planes_dev,
                            stream) != 0) return 1;
  if (n_pages > 0)
    if (ymk_bin_adaptive_pack(planes_dev, (int64_t)n_pages * ymk::DK_REC, n_pages, max_h, max_w, sat_dev, sat_bytes, packed_dev,
                                       packed_bytes, stream) != 0) return 1;
  if (ymk_dsk_scores(blob_dev, blob_words, n_pages, packed_dev, packed_bytes, sat_bytes, luma_bytes, table_dev, n_angles, s_max,
                              scores_dev, stream) != 0) return 1;
  if (ymk_dsk_choose(blob_dev, blob_words, n_pages, packed_bytes, sat_bytes, luma_bytes, scores_dev, n_angles, s_max, dead,
                              choice_dev, stream) != 0) return 1;
  if (rotate)
    if (ymk_dsk_rotate(blob_dev, blob_words, n_pages, 3LL * max_h * max_w, table_dev, n_angles, choice_dev, stream) != 0) return 1;
  return 0;
}
}
