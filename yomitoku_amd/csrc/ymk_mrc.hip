// Layered pages: the pages of a wave separated into an ink mask and two low-resolution pictures - the ink's colour and the paper
// with the ink lifted out of it (include/ymk.h, "Layered pages"; yomitoku_amd/mrc.py; DESIGN.md, "Layered pages").
// tests/mrc_ref.py is the definition; every stage equals it bit for bit - all of it is integer arithmetic on sums that no order
// of addition can change.
//
//   k_mrc_cells   the hot path: level 0 of BOTH layers from one pass over the page.  One wave per 64 x 16 pixel tile - cells are
//                 powers of two up to 16, so a tile holds whole cells of both layers.  Lanes 0..17 read the packed ink of rows
//                 y0 - 1 .. y0 + 16 (four words: the tile's two and a halo word either side, zero outside the page), put the
//                 tile's 64 bits and their horizontal dilation into LDS; a row's 3 x 3 dilation is the OR of three of those.
//                 A lane owns one column: per row three byte loads (B G R; a wave reads 192 consecutive bytes), the column sums
//                 of both layers in registers - (S0 | S1 << 16, S2 | N << 16): S <= 16 * 255, N <= 16 -, and on the last row of a
//                 cell log2(d) xor shuffles add the d columns of the cell: S <= 256 * 255 < 2^16, N <= 256.  The first lane of a
//                 cell writes its word: three values, the known byte.  No atomics, no block barrier after the mask.
//   k_mrc_pull    one launch per level: a thread per parent cell of a layer of a page averages its known children.
//   k_mrc_flags   one thread per page: 1 where the top cell of both layers is known, 0 where not, -1 for a record that is none.
//   k_mrc_push    a thread per level-0 cell of a layer of a page whose flag is 1: the cell's value, or that of its first known
//                 ancestor, into the layer image.
//
// A page's pyramids: the foreground's levels 0 .. L one behind the other, then the background's; level l + 1 has ceil(H_l / 2) x
// ceil(W_l / 2) words, the last 1 x 1.  At most 15 levels (16383 = 2^14 - 1), at most 4/3 H0 W0 + 15 words.

#include "ymk_pages.h"

#include "../../include/ymk.h"

namespace ymk {

constexpr int MR_REC = YMK_MRC_PAGE_WORDS;
static_assert(MR_REC == YMK_DSK_PAGE_WORDS && MR_REC == YMK_G4_PAGE_WORDS, "ymk_dsk_luma and the binariser read these records");
constexpr int MR_MAX_SIDE = 16383, MR_MAX_LEVELS = 15;
constexpr int MR_TILE_W = 64, MR_TILE_H = 16;

struct MrLimits {
  long long packed_words, pyr_words, layers_bytes;
};

__host__ __device__ __forceinline__ bool mr_cell_ok(int d) { return d == 1 || d == 2 || d == 4 || d == 8 || d == 16; }
__host__ __device__ __forceinline__ int mr_log2(int d) { return d == 1 ? 0 : d == 2 ? 1 : d == 4 ? 2 : d == 8 ? 3 : 4; }
// the words of the pyramid on an H0 x W0 level 0
__host__ __device__ __forceinline__ long long mr_pyramid_words(int H0, int W0) {
  long long total = 0;
  for (int H = H0, W = W0;; H = (H + 1) >> 1, W = (W + 1) >> 1) {
    total += (long long)H * W;
    if (H == 1 && W == 1) return total;
  }
}

// One layer of a page: log2 of its cell, level 0's size, where its pyramid and its image are.
struct MrLayer {
  int shift, H0, W0;
  long long pyr_at, img_at;
};
// A page's record, read and checked against the buffers' sizes: a kernel takes a page whose record fails the check as absent.
struct MrPage {
  const unsigned char* src;
  int h, w, ch, row_words;
  long long packed_at;
  MrLayer fg, bg;
  bool ok;
};
__device__ __forceinline__ MrPage mr_page(const int* blob, int p, int bg_cell, int fg_cell, const MrLimits& lim) {
  const int* r = blob + (size_t)p * MR_REC;
  MrPage g;
  g.src = reinterpret_cast<const unsigned char*>((unsigned long long)page_word64(r, 0));
  g.h = r[2], g.w = r[3], g.ch = r[4];
  g.packed_at = page_word64(r, 6);
  g.ok = g.h >= 1 && g.w >= 1 && g.h <= MR_MAX_SIDE && g.w <= MR_MAX_SIDE && g.src != nullptr && (g.ch == 1 || g.ch == 3);
  g.row_words = g.ok ? (g.w + 31) >> 5 : 0;
  g.fg.shift = mr_log2(fg_cell), g.bg.shift = mr_log2(bg_cell);
  g.fg.H0 = g.fg.W0 = g.bg.H0 = g.bg.W0 = 0;
  g.fg.pyr_at = g.bg.pyr_at = g.fg.img_at = g.bg.img_at = 0;
  if (!g.ok) return g;
  g.fg.H0 = (g.h + fg_cell - 1) >> g.fg.shift, g.fg.W0 = (g.w + fg_cell - 1) >> g.fg.shift;
  g.bg.H0 = (g.h + bg_cell - 1) >> g.bg.shift, g.bg.W0 = (g.w + bg_cell - 1) >> g.bg.shift;
  const long long fg_words = mr_pyramid_words(g.fg.H0, g.fg.W0), bg_words = mr_pyramid_words(g.bg.H0, g.bg.W0);
  const long long fg_bytes = (long long)g.fg.H0 * g.fg.W0 * g.ch, bg_bytes = (long long)g.bg.H0 * g.bg.W0 * g.ch;
  g.fg.pyr_at = (long long)r[5], g.bg.pyr_at = g.fg.pyr_at + fg_words;
  g.fg.img_at = page_word64(r, 11), g.bg.img_at = g.fg.img_at + ((fg_bytes + 15) & ~15LL);
  g.ok = g.packed_at >= 0 && g.packed_at + (long long)g.h * g.row_words <= lim.packed_words && g.fg.pyr_at >= 0 &&
         g.bg.pyr_at + bg_words <= lim.pyr_words && g.fg.img_at >= 0 && (g.fg.img_at & 15) == 0 && g.bg.img_at + bg_bytes <= lim.layers_bytes;
  return g;
}

// ------------------------------------------------------------------------------------------------ cells
__device__ __forceinline__ unsigned mr_mean(unsigned s, unsigned n) { return (2u * s + n) / (2u * n); }
// a cell's word from its sums: byte k the value of channel k, byte 3 whether any pixel was selected
__device__ __forceinline__ unsigned mr_cell_word(unsigned a, unsigned b, int ch) {
  const unsigned n = b >> 16;
  if (!n) return 0u;
  unsigned word = mr_mean(a & 0xffffu, n) | (1u << 24);
  if (ch == 3) word |= (mr_mean(a >> 16, n) << 8) | (mr_mean(b & 0xffffu, n) << 16);
  return word;
}

__global__ __launch_bounds__(64) void k_mrc_cells(const int* __restrict__ blob, MrLimits lim, int bg_cell, int fg_cell,
                                                  const unsigned* __restrict__ packed, unsigned* __restrict__ pyr) {
  __shared__ unsigned long long s_ink[MR_TILE_H + 2], s_wide[MR_TILE_H + 2];  // rows y0 - 1 .. y0 + 16: the ink, and it dilated along the row
  const int p = blockIdx.z, lane = threadIdx.x;
  const MrPage g = mr_page(blob, p, bg_cell, fg_cell, lim);
  const int x0 = (int)blockIdx.x * MR_TILE_W, y0 = (int)blockIdx.y * MR_TILE_H;
  if (!g.ok || x0 >= g.w || y0 >= g.h) return;  // the whole block
  if (lane < MR_TILE_H + 2) {
    const int y = y0 - 1 + lane, wx = x0 >> 5;
    unsigned w4[4] = {0u, 0u, 0u, 0u};  // words wx - 1 .. wx + 2 of the row; zero outside the page
    if (y >= 0 && y < g.h) {
      const unsigned* row = packed + g.packed_at + (long long)y * g.row_words;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (wx - 1 + k >= 0 && wx - 1 + k < g.row_words) w4[k] = row[wx - 1 + k];
    }
    const unsigned long long v = ((unsigned long long)w4[1] << 32) | w4[2];  // pixel x0 + j in bit 63 - j
    s_ink[lane] = v;
    s_wide[lane] = v | (v >> 1) | (v << 1) | ((unsigned long long)(w4[0] & 1u) << 63) | (unsigned long long)(w4[3] >> 31);
  }
  __syncthreads();
  const int x = x0 + lane, ch = g.ch;
  const bool col = x < g.w;
  unsigned fa = 0, fb = 0, ba = 0, bb = 0;  // the column's sums of the two layers: S0 | S1 << 16, S2 | N << 16
#pragma unroll
  for (int r = 0; r < MR_TILE_H; ++r) {
    const int y = y0 + r;
    if (col && y < g.h) {
      const bool ink = (s_ink[r + 1] >> (63 - lane)) & 1ull;
      const bool near = ((s_wide[r] | s_wide[r + 1] | s_wide[r + 2]) >> (63 - lane)) & 1ull;
      if (ink || !near) {
        const unsigned char* px = g.src + ((long long)y * g.w + x) * ch;
        unsigned a = px[0], b = 1u << 16;
        if (ch == 3) a |= (unsigned)px[1] << 16, b |= px[2];
        if (ink) fa += a, fb += b;
        else ba += a, bb += b;
      }
    }
    // the last row of a cell (wave-uniform): add the cell's columns, write its word, start the next
    if (((r + 1) & (fg_cell - 1)) == 0) {
      for (int o = 1; o < fg_cell; o <<= 1) fa += __shfl_xor(fa, o), fb += __shfl_xor(fb, o);
      const int cy = y >> g.fg.shift, cx = x >> g.fg.shift;
      if ((lane & (fg_cell - 1)) == 0 && cy < g.fg.H0 && cx < g.fg.W0) pyr[g.fg.pyr_at + (long long)cy * g.fg.W0 + cx] = mr_cell_word(fa, fb, ch);
      fa = fb = 0;
    }
    if (((r + 1) & (bg_cell - 1)) == 0) {
      for (int o = 1; o < bg_cell; o <<= 1) ba += __shfl_xor(ba, o), bb += __shfl_xor(bb, o);
      const int cy = y >> g.bg.shift, cx = x >> g.bg.shift;
      if ((lane & (bg_cell - 1)) == 0 && cy < g.bg.H0 && cx < g.bg.W0) pyr[g.bg.pyr_at + (long long)cy * g.bg.W0 + cx] = mr_cell_word(ba, bb, ch);
      ba = bb = 0;
    }
  }
}

// ------------------------------------------------------------------------------------------------ pull
constexpr int PL_THREADS = 256;
// level `level` (>= 1) of both layers of every page from the level below; a layer that has no such level is skipped
__global__ __launch_bounds__(PL_THREADS) void k_mrc_pull(const int* __restrict__ blob, MrLimits lim, int bg_cell, int fg_cell, int level,
                                                         unsigned* __restrict__ pyr) {
  const int p = blockIdx.z;
  const MrPage g = mr_page(blob, p, bg_cell, fg_cell, lim);
  if (!g.ok) return;
  const MrLayer& a = blockIdx.y ? g.bg : g.fg;
  int H = a.H0, W = a.W0;
  long long at = a.pyr_at;  // of the level below
  for (int l = 1; l < level; ++l) {
    if (H == 1 && W == 1) return;
    at += (long long)H * W, H = (H + 1) >> 1, W = (W + 1) >> 1;
  }
  if (H == 1 && W == 1) return;  // the level below is the top
  const int PH = (H + 1) >> 1, PW = (W + 1) >> 1;
  const unsigned* below = pyr + at;
  unsigned* out = pyr + at + (long long)H * W;
  const int cells = PH * PW;  // at most 8192 * 8192
  for (int i = (int)(blockIdx.x * PL_THREADS + threadIdx.x); i < cells; i += (int)(gridDim.x * PL_THREADS)) {
    const int cy = i / PW, cx = i - cy * PW;
    unsigned s0 = 0, s1 = 0, s2 = 0, k = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int yy = 2 * cy + (j >> 1), xx = 2 * cx + (j & 1);
      if (yy < H && xx < W) {
        const unsigned v = below[(long long)yy * W + xx];
        if (v >> 24) s0 += v & 255u, s1 += (v >> 8) & 255u, s2 += (v >> 16) & 255u, ++k;
      }
    }
    out[i] = k ? mr_mean(s0, k) | (mr_mean(s1, k) << 8) | (mr_mean(s2, k) << 16) | (1u << 24) : 0u;
  }
}

// ------------------------------------------------------------------------------------------------ flags and push
__global__ void k_mrc_flags(const int* __restrict__ blob, MrLimits lim, int bg_cell, int fg_cell, int n_pages, const unsigned* __restrict__ pyr,
                            int* __restrict__ flags) {
  const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (p >= n_pages) return;
  const MrPage g = mr_page(blob, p, bg_cell, fg_cell, lim);
  if (!g.ok) {
    flags[p] = -1;
    return;
  }
  const unsigned top_fg = pyr[g.fg.pyr_at + mr_pyramid_words(g.fg.H0, g.fg.W0) - 1];
  const unsigned top_bg = pyr[g.bg.pyr_at + mr_pyramid_words(g.bg.H0, g.bg.W0) - 1];
  flags[p] = (top_fg >> 24) && (top_bg >> 24) ? 1 : 0;
}

constexpr int PS_THREADS = 256;
__global__ __launch_bounds__(PS_THREADS) void k_mrc_push(const int* __restrict__ blob, MrLimits lim, int bg_cell, int fg_cell,
                                                         const unsigned* __restrict__ pyr, const int* __restrict__ flags,
                                                         unsigned char* __restrict__ layers) {
  const int p = blockIdx.z;
  if (flags[p] != 1) return;  // no layers: nothing is written
  const MrPage g = mr_page(blob, p, bg_cell, fg_cell, lim);
  if (!g.ok) return;
  const MrLayer& a = blockIdx.y ? g.bg : g.fg;
  const unsigned* base = pyr + a.pyr_at;
  unsigned char* out = layers + a.img_at;
  const int cells = a.H0 * a.W0, ch = g.ch;
  for (int i = (int)(blockIdx.x * PS_THREADS + threadIdx.x); i < cells; i += (int)(gridDim.x * PS_THREADS)) {
    int cy = i / a.W0, cx = i - cy * a.W0, H = a.H0, W = a.W0;
    const unsigned* lvl = base;
    unsigned v = lvl[i];
    while (!(v >> 24) && !(H == 1 && W == 1)) {  // the top is known where the flag is 1
      lvl += (long long)H * W, H = (H + 1) >> 1, W = (W + 1) >> 1, cy >>= 1, cx >>= 1;
      v = lvl[(long long)cy * W + cx];
    }
    if (ch == 1) out[i] = (unsigned char)v;
    else out[3ll * i] = (unsigned char)v, out[3ll * i + 1] = (unsigned char)(v >> 8), out[3ll * i + 2] = (unsigned char)(v >> 16);
  }
}

// ------------------------------------------------------------------------------------------------ host
struct MrCall {
  MrLimits lim;
  int max_H0, max_W0;  // of the finer layer at the largest page: what the grids are sized by
};
static MrCall mr_check(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, int bg_cell, int fg_cell, int64_t packed_bytes,
                       const void* pyr_dev, int64_t pyr_bytes, int64_t layers_bytes) {
  check_page_table(blob_dev, blob_words, n_pages, MR_REC, 3, 4096, "0..4096 pages", "page table: n records");  // no caller comes with 0
  YMK_CHECK(mr_cell_ok(bg_cell) && mr_cell_ok(fg_cell), "a cell is 1, 2, 4, 8 or 16");
  YMK_CHECK(max_h >= 1 && max_w >= 1 && max_h <= MR_MAX_SIDE && max_w <= MR_MAX_SIDE, "a page has 1..16383 pixels on a side");
  YMK_CHECK(pyr_dev && ((uintptr_t)pyr_dev & 7) == 0, "pyramids: 8-byte aligned");
  YMK_CHECK(packed_bytes >= 0 && pyr_bytes >= 0 && layers_bytes >= 0, "negative size");
  const int d = std::min(bg_cell, fg_cell);
  return MrCall{MrLimits{packed_bytes / 4, pyr_bytes / 4, layers_bytes}, (max_h + d - 1) / d, (max_w + d - 1) / d};
}
static unsigned mr_cell_blocks(int64_t cells, int threads) {
  return (unsigned)std::min<int64_t>(std::max<int64_t>((cells + threads - 1) / threads, 1), 4096);
}

}  // namespace ymk

extern "C" {

int ymk_mrc_page_words(void) { return ymk::MR_REC; }

int ymk_mrc_scratch_bytes(const int* h, const int* w, const int* ch, int n_pages, int bg_cell, int fg_cell, int64_t* sizes6_out, int64_t* places_out) {
  YMK_API_BEGIN
  YMK_CHECK(n_pages >= 0 && n_pages <= 4096 && sizes6_out && (n_pages == 0 || (h && w && ch)), "bad argument");
  YMK_CHECK(ymk::mr_cell_ok(bg_cell) && ymk::mr_cell_ok(fg_cell), "a cell is 1, 2, 4, 8 or 16");
  int64_t luma = 0, cells = 0, words = 0, pyr = 0, layers = 0;
  for (int k = 0; k < n_pages; ++k) {
    YMK_CHECK(h[k] >= 1 && w[k] >= 1 && h[k] <= ymk::MR_MAX_SIDE && w[k] <= ymk::MR_MAX_SIDE, "a page has 1..16383 pixels on a side");
    YMK_CHECK(ch[k] == 1 || ch[k] == 3, "a page has one or three channels");
    const int64_t px = (int64_t)h[k] * w[k];
    if (ch[k] == 3) luma += (px + 15) & ~15LL;
    cells += px;
    words += (int64_t)h[k] * ((w[k] + 31) >> 5);
    const int fH = (h[k] + fg_cell - 1) / fg_cell, fW = (w[k] + fg_cell - 1) / fg_cell;
    const int bH = (h[k] + bg_cell - 1) / bg_cell, bW = (w[k] + bg_cell - 1) / bg_cell;
    const int64_t fg_at = layers, bg_at = fg_at + (((int64_t)fH * fW * ch[k] + 15) & ~15LL);
    if (places_out) places_out[3 * k] = pyr, places_out[3 * k + 1] = fg_at, places_out[3 * k + 2] = bg_at;
    pyr += ymk::mr_pyramid_words(fH, fW) + ymk::mr_pyramid_words(bH, bW);
    layers = bg_at + (((int64_t)bH * bW * ch[k] + 15) & ~15LL);
    YMK_CHECK(pyr < (1LL << 31), "the pyramids of a call have fewer than 2^31 words");
  }
  sizes6_out[0] = luma;
  sizes6_out[1] = ((cells + 1) & ~1LL) * 4;
  sizes6_out[2] = ((words + 1) & ~1LL) * 4;
  sizes6_out[3] = ((pyr + 1) & ~1LL) * 4;
  sizes6_out[4] = layers;
  sizes6_out[5] = (((int64_t)n_pages + 1) & ~1LL) * 4;
  YMK_API_END
}

int ymk_mrc_cells(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, int bg_cell, int fg_cell, const uint32_t* packed_dev,
                  int64_t packed_bytes, uint32_t* pyr_dev, int64_t pyr_bytes, int64_t layers_bytes, void* stream) {
  YMK_API_BEGIN
  if (n_pages == 0) return 0;
  const ymk::MrCall c = ymk::mr_check(blob_dev, blob_words, n_pages, max_h, max_w, bg_cell, fg_cell, packed_bytes, pyr_dev, pyr_bytes, layers_bytes);
  YMK_CHECK(packed_dev && ((uintptr_t)packed_dev & 7) == 0, "packed rows: 8-byte aligned");
  const dim3 grid((unsigned)((max_w + ymk::MR_TILE_W - 1) / ymk::MR_TILE_W), (unsigned)((max_h + ymk::MR_TILE_H - 1) / ymk::MR_TILE_H), (unsigned)n_pages);
  hipLaunchKernelGGL(ymk::k_mrc_cells, grid, dim3(64), 0, (hipStream_t)stream, blob_dev, c.lim, bg_cell, fg_cell, (const unsigned*)packed_dev,
                     (unsigned*)pyr_dev);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}

int ymk_mrc_pull(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, int bg_cell, int fg_cell, int64_t packed_bytes,
                 uint32_t* pyr_dev, int64_t pyr_bytes, int64_t layers_bytes, void* stream) {
  YMK_API_BEGIN
  if (n_pages == 0) return 0;
  const ymk::MrCall c = ymk::mr_check(blob_dev, blob_words, n_pages, max_h, max_w, bg_cell, fg_cell, packed_bytes, pyr_dev, pyr_bytes, layers_bytes);
  int H = c.max_H0, W = c.max_W0;
  for (int level = 1; level < ymk::MR_MAX_LEVELS && !(H == 1 && W == 1); ++level) {
    H = (H + 1) >> 1, W = (W + 1) >> 1;
    hipLaunchKernelGGL(ymk::k_mrc_pull, dim3(ymk::mr_cell_blocks((int64_t)H * W, ymk::PL_THREADS), 2u, (unsigned)n_pages), dim3(ymk::PL_THREADS), 0,
                       (hipStream_t)stream, blob_dev, c.lim, bg_cell, fg_cell, level, (unsigned*)pyr_dev);
    YMK_HIP(hipGetLastError());
  }
  YMK_API_END
}

int ymk_mrc_push(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, int bg_cell, int fg_cell, int64_t packed_bytes,
                 const uint32_t* pyr_dev, int64_t pyr_bytes, unsigned char* layers_dev, int64_t layers_bytes, int* flags_dev, void* stream) {
  YMK_API_BEGIN
  if (n_pages == 0) return 0;
  const ymk::MrCall c = ymk::mr_check(blob_dev, blob_words, n_pages, max_h, max_w, bg_cell, fg_cell, packed_bytes, pyr_dev, pyr_bytes, layers_bytes);
  YMK_CHECK(layers_bytes == 0 || (layers_dev && ((uintptr_t)layers_dev & 15) == 0), "layers: 16-byte aligned");
  YMK_CHECK(flags_dev && ((uintptr_t)flags_dev & 3) == 0, "null or misaligned flags");
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ymk::k_mrc_flags, dim3((unsigned)((n_pages + 63) / 64)), dim3(64), 0, s, blob_dev, c.lim, bg_cell, fg_cell, n_pages,
                     (const unsigned*)pyr_dev, flags_dev);
  YMK_HIP(hipGetLastError());
  hipLaunchKernelGGL(ymk::k_mrc_push, dim3(ymk::mr_cell_blocks((int64_t)c.max_H0 * c.max_W0, ymk::PS_THREADS), 2u, (unsigned)n_pages),
                     dim3(ymk::PS_THREADS), 0, s, blob_dev, c.lim, bg_cell, fg_cell, (const unsigned*)pyr_dev, (const int*)flags_dev, layers_dev);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}

int ymk_mrc_pages(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, int bg_cell, int fg_cell, unsigned char* luma_dev,
                  int64_t luma_bytes, uint32_t* sat_dev, int64_t sat_bytes, uint32_t* packed_dev, int64_t packed_bytes, int* planes_dev,
                  uint32_t* pyr_dev, int64_t pyr_bytes, unsigned char* layers_dev, int64_t layers_bytes, int* flags_dev, void* stream) {
  if (n_pages == 0) return 0;
  if (planes_dev) {  // the ink from the pages; without, packed_dev holds the caller's
    if (ymk_dsk_luma(blob_dev, blob_words, n_pages, (int64_t)max_h * max_w, luma_dev, luma_bytes, packed_bytes, sat_bytes, planes_dev, stream) != 0)
      return 1;
    if (ymk_bin_adaptive_pack(planes_dev, (int64_t)n_pages * ymk::MR_REC, n_pages, max_h, max_w, sat_dev, sat_bytes, packed_dev, packed_bytes,
                              stream) != 0)
      return 1;
  }
  if (ymk_mrc_cells(blob_dev, blob_words, n_pages, max_h, max_w, bg_cell, fg_cell, packed_dev, packed_bytes, pyr_dev, pyr_bytes, layers_bytes,
                    stream) != 0) return 1;
  if (ymk_mrc_pull(blob_dev, blob_words, n_pages, max_h, max_w, bg_cell, fg_cell, packed_bytes, pyr_dev, pyr_bytes, layers_bytes, stream) != 0)
    return 1;
  return ymk_mrc_push(blob_dev, blob_words, n_pages, max_h, max_w, bg_cell, fg_cell, packed_bytes, pyr_dev, pyr_bytes, layers_dev, layers_bytes,
                      flags_dev, stream);
}
}
