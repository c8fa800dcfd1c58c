// Despeckled pages: connected-component labelling of the packed rows of the Group 4 encoder, and the removal of every component
// below a size (include/ymk.h, "Despeckled pages"; yomitoku_amd/despeckle.py; DESIGN.md, "Despeckled pages").
// tests/despeckle_ref.py is the definition; the bits and the four counts equal it exactly: a component's area is a sum of ones,
// which no order of addition changes.
//
// One pass per colour - black under 8-connectivity, then, on its result, white under 4 -, four launches each.  A page's pixel
// (y, x) has the index i = y w + x < 2^28 and two words of scratch, label[i] and area[i].
//
//   k_cc_label   one block per 64 x 16 pixel tile: union-find over the tile's pixels of the colour in LDS (a pixel is united with
//                the run above it - by the first pixel at which the two runs overlap -, under 8-connectivity with the upper diagonals
//                where the upper neighbour is not of the colour), then label[i] = the page index of the pixel's tile-local root
//                (-1: not of the colour), area[i] = 0.
//   k_cc_merge   one thread per pixel of a tile's first row or first column: united with its neighbours across the seam.
//   k_cc_areas   one thread per pixel: its root; label[i] = root; area[root] += 1 - one add per run of lanes with one root, and none
//                once the area has reached n: area[root] is the component's size where that is below n, and at least n otherwise.
//   k_cc_apply   one thread per pixel, a wave per two packed words: the pixel flips where area[label[i]] < n; the ballot is the
//                words' change, its population and that of the flipped roots go to the page's counters.
//
// Termination.  A label slot only ever receives a value that is not larger than the slot's index, and the label of a pixel that
// is no root is smaller than its index:
//   - k_cc_label starts a pixel at the first pixel of its run along the row and stores the tile root's index, the smallest of
//     the tile's component (row-major order in the tile is the page's order);
//   - unite() stores with atomicMin(&label[a], b) where b < a;
//   - k_cc_areas stores find(i) <= i.
// So cc_find, which steps from x to label[x] only while label[x] < x, strictly descends and ends after at most x steps whatever
// other threads do meanwhile; and every round of unite() that does not end it replaces its larger root a by a value below a,
// while b never grows: a + b falls by at least one per round.  No loop waits for another thread's progress; a value read late is
// an older parent, still a smaller index in what will be the same component once every unite() has returned.  There is no
// barrier across blocks: the launch boundaries are the barriers.
//
// Determinism.  Which pixel a component's root is may depend on timing between k_cc_merge's threads; its area, and with it
// every output bit and every count, does not.

#include "ymk_common.h"

#include <algorithm>

#include "../../include/ymk.h"

namespace ymk {

constexpr int CC_REC = YMK_G4_PAGE_WORDS;
constexpr int CC_MAX_SIDE = 16383;
constexpr int CC_TILE_W = YMK_CC_TILE_W, CC_TILE_H = YMK_CC_TILE_H, CC_TILE = CC_TILE_W * CC_TILE_H;
constexpr int CC_THREADS = 256;
static_assert(CC_TILE_W == 64 && CC_TILE % CC_THREADS == 0, "a tile's row is one 64-bit word of LDS");

struct CcLimits {
  long long packed_words, label_words;
  int max_h, max_w;  // what the call's grids are sized by
};

__device__ __forceinline__ long long cc_word64(const int* r, int k) {
  return (long long)(((unsigned long long)(unsigned)r[k + 1] << 32) | (unsigned long long)(unsigned)r[k]);
}

// A page's record (the Group 4 page table: h, w, words 6-7 the packed rows, words 14-15 the place of its h w labels and areas),
// read and checked against the buffers' sizes and the call's max_h, max_w: every kernel takes a page whose record fails as absent.
struct CcPage {
  int h, w, row_words;
  long long packed_at, label_at;
  bool ok;
};
__device__ __forceinline__ CcPage cc_page(const int* blob, int p, const CcLimits& lim) {
  const int* r = blob + (size_t)p * CC_REC;
  CcPage g;
  g.h = r[2], g.w = r[3];
  g.packed_at = cc_word64(r, 6), g.label_at = cc_word64(r, 14);
  g.ok = g.h >= 1 && g.w >= 1 && g.h <= lim.max_h && g.w <= lim.max_w;  // a larger page the grids would cover in part only
  g.row_words = g.ok ? (g.w + 31) >> 5 : 0;
  g.ok = g.ok && g.packed_at >= 0 && g.packed_at + (long long)g.h * g.row_words <= lim.packed_words && g.label_at >= 0 &&
         g.label_at + (long long)g.h * g.w <= lim.label_words;
  return g;
}

// whether pixel (y, x) is of the pass's colour (invert: 0 black, ~0 white); false outside the page
__device__ __forceinline__ bool cc_is(const unsigned* rows, const CcPage& g, unsigned invert, int y, int x) {
  if (y < 0 || x < 0 || y >= g.h || x >= g.w) return false;
  return ((rows[(long long)y * g.row_words + (x >> 5)] ^ invert) >> (31 - (x & 31))) & 1u;
}

// ------------------------------------------------------------------------------------------------ union-find
// L: labels, in LDS or in global memory.  Slots of pixels of the colour only; see "Termination" above.
template <bool GLOBAL>
__device__ __forceinline__ int cc_load(const int* L, int x) {
  if (GLOBAL) return __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return *reinterpret_cast<const volatile int*>(L + x);
}
template <bool GLOBAL>
__device__ __forceinline__ int cc_find(const int* L, int x) {
  int parent = cc_load<GLOBAL>(L, x);
  while (parent < x && parent >= 0) {  // strictly down
    x = parent;
    parent = cc_load<GLOBAL>(L, x);
  }
  return x;
}
template <bool GLOBAL>
__device__ __forceinline__ void cc_unite(int* L, int a, int b) {
  for (;;) {
    a = cc_find<GLOBAL>(L, a), b = cc_find<GLOBAL>(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicMin(L + a, b);  // b < a
    if (old >= a) return;                 // a was a root, and now hangs below b
    a = old;                              // a hung below old < a already: old's tree and b's are still to unite
  }
}

// ------------------------------------------------------------------------------------------------ label
__global__ __launch_bounds__(CC_THREADS) void k_cc_label(const int* __restrict__ blob, CcLimits lim, unsigned invert, int eight,
                                                         const unsigned* __restrict__ packed, int* __restrict__ labels, int* __restrict__ areas) {
  __shared__ unsigned long long s_row[CC_TILE_H + 1];  // s_row[r + 1]: row y0 + r of the tile, pixel x0 + c in bit 63 - c; s_row[0] = 0
  __shared__ int s_lab[CC_TILE];
  const CcPage g = cc_page(blob, blockIdx.z, lim);
  const int x0 = (int)blockIdx.x * CC_TILE_W, y0 = (int)blockIdx.y * CC_TILE_H, tid = threadIdx.x;
  if (!g.ok || x0 >= g.w || y0 >= g.h) return;  // the whole block
  if (tid <= CC_TILE_H) {
    const int y = y0 + tid - 1, wx = x0 >> 5;
    unsigned long long v = 0;
    if (tid >= 1 && y < g.h) {
      const unsigned* row = packed + g.packed_at + (long long)y * g.row_words;
      const unsigned hi = row[wx] ^ invert, lo = wx + 1 < g.row_words ? row[wx + 1] ^ invert : 0u;
      v = ((unsigned long long)hi << 32) | lo;
      const int cols = min(g.w - x0, CC_TILE_W);  // 1..64: the pad bits are no pixels
      v &= cols == 64 ? ~0ull : ~(~0ull >> cols);
    }
    s_row[tid] = v;
  }
  __syncthreads();
  // a pixel starts below the first pixel of its run along the row (<= its own index): the row's neighbours are united already
  for (int t = tid; t < CC_TILE; t += CC_THREADS) {
    const int c = t & 63;
    const unsigned long long here = s_row[(t >> 6) + 1];
    int v = -1;
    if ((here >> (63 - c)) & 1ull) {
      const unsigned long long gaps = c ? ~here >> (64 - c) : 0ull;  // bit j: pixel c - 1 - j is not of the colour
      v = t - (gaps ? __ffsll((long long)gaps) - 1 : c);
    }
    s_lab[t] = v;
  }
  __syncthreads();
  for (int t = tid; t < CC_TILE; t += CC_THREADS) {
    const int r = t >> 6, c = t & 63;
    const unsigned long long here = s_row[r + 1], above = s_row[r];
    if (!((here >> (63 - c)) & 1ull)) continue;
    const bool left = c > 0 && ((here >> (64 - c)) & 1ull);
    const bool up = (above >> (63 - c)) & 1ull, up_left = c > 0 && ((above >> (64 - c)) & 1ull);
    if (up) {
      // where the left neighbour and the one above it are of the colour too, that pair has united the two runs
      if (!(left && up_left)) cc_unite<false>(s_lab, t, t - 64);
    } else if (eight) {
      // with `up` both diagonals hang on it along the row above; with `left` the upper left one is left's upper neighbour
      if (!left && c > 0 && ((above >> (64 - c)) & 1ull)) cc_unite<false>(s_lab, t, t - 65);
      if (c < 63 && ((above >> (62 - c)) & 1ull)) cc_unite<false>(s_lab, t, t - 63);
    }
  }
  __syncthreads();
  int* lab = labels + g.label_at;
  int* area = areas + g.label_at;
  for (int t = tid; t < CC_TILE; t += CC_THREADS) {
    const int y = y0 + (t >> 6), x = x0 + (t & 63);
    if (y >= g.h || x >= g.w) continue;
    int v = -1;
    if (s_lab[t] >= 0) {
      const int root = cc_find<false>(s_lab, t);
      v = (y0 + (root >> 6)) * g.w + x0 + (root & 63);
    }
    lab[y * g.w + x] = v;
    area[y * g.w + x] = 0;
  }
}

// ------------------------------------------------------------------------------------------------ merge
// Seam pixels of a page: those of the rows y = 16, 32, ... (first) and those of the columns x = 64, 128, ...
__global__ __launch_bounds__(CC_THREADS) void k_cc_merge(const int* __restrict__ blob, CcLimits lim, unsigned invert, int eight,
                                                         const unsigned* __restrict__ packed, int* __restrict__ labels) {
  const CcPage g = cc_page(blob, blockIdx.z, lim);
  if (!g.ok) return;
  const unsigned* rows = packed + g.packed_at;
  int* lab = labels + g.label_at;
  const int seam_rows = (g.h - 1) / CC_TILE_H, seam_cols = (g.w - 1) / CC_TILE_W;
  const long long across = (long long)seam_rows * g.w, total = across + (long long)seam_cols * g.h;
  for (long long e = (long long)blockIdx.x * CC_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * CC_THREADS) {
    if (e < across) {  // above: (y - 1, x - 1 .. x + 1)
      const int y = ((int)(e / g.w) + 1) * CC_TILE_H, x = (int)(e % g.w);
      if (!cc_is(rows, g, invert, y, x)) continue;
      const int i = y * g.w + x;
      if (cc_is(rows, g, invert, y - 1, x)) {
        // inside a tile's width: where the left neighbour and the one above it are of the colour too, that pair unites the runs
        if ((x % CC_TILE_W) == 0 || !(cc_is(rows, g, invert, y, x - 1) && cc_is(rows, g, invert, y - 1, x - 1))) cc_unite<true>(lab, i, i - g.w);
      } else if (eight) {
        if (cc_is(rows, g, invert, y - 1, x - 1)) cc_unite<true>(lab, i, i - g.w - 1);
        if (cc_is(rows, g, invert, y - 1, x + 1)) cc_unite<true>(lab, i, i - g.w + 1);
      }
    } else {  // to the left: (y - 1 .. y + 1, x - 1)
      const long long f = e - across;
      const int x = ((int)(f / g.h) + 1) * CC_TILE_W, y = (int)(f % g.h);
      if (!cc_is(rows, g, invert, y, x)) continue;
      const int i = y * g.w + x;
      if (cc_is(rows, g, invert, y, x - 1)) {
        // inside a tile's height: where the upper neighbour and the one left of it are of the colour too, that pair does it
        if ((y % CC_TILE_H) == 0 || !(cc_is(rows, g, invert, y - 1, x) && cc_is(rows, g, invert, y - 1, x - 1))) cc_unite<true>(lab, i, i - 1);
      } else if (eight) {
        if (cc_is(rows, g, invert, y - 1, x - 1)) cc_unite<true>(lab, i, i - g.w - 1);
        if (cc_is(rows, g, invert, y + 1, x - 1)) cc_unite<true>(lab, i, i + g.w - 1);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ areas and apply
// Both: thread t of a page is bit t & 31 (from the left) of packed word t >> 5 - a wave is two words.  No lane of a page that
// is one leaves before its wave's ballots: a lane behind the page's last word, or in a row's pad, is a pixel of no colour.
__device__ __forceinline__ bool cc_pixel(const CcPage& g, long long t, int& y, int& x) {
  const long long word = t >> 5;
  if (word >= (long long)g.h * g.row_words) return false;
  y = (int)(word / g.row_words), x = (int)(word % g.row_words) * 32 + (int)(t & 31);
  return x < g.w;
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_areas(const int* __restrict__ blob, CcLimits lim, unsigned invert, int n,
                                                         const unsigned* __restrict__ packed, int* __restrict__ labels, int* __restrict__ areas) {
  const CcPage g = cc_page(blob, blockIdx.z, lim);
  const long long t = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (!g.ok) return;  // the whole grid row of the page; otherwise every lane stays for the ballot
  int y = 0, x = 0;
  const bool mine = cc_pixel(g, t, y, x) && cc_is(packed + g.packed_at, g, invert, y, x);
  int* lab = labels + g.label_at;
  int root = -1;
  if (mine) {
    const int i = y * g.w + x;
    root = cc_find<true>(lab, i);
    __hip_atomic_store(lab + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // <= i
  }
  // a run of lanes with one root adds once: its first lane, the run's length
  const int lane = threadIdx.x & 63;
  const int before = __shfl_up(root, 1);
  const bool head = lane == 0 || before != root;
  const unsigned long long heads = __ballot(head);
  if (mine && head) {
    const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
    const int len = rest ? __ffsll((long long)rest) : 64 - lane;
    // an area that has reached n is large whatever else is added: the page's background costs a load, not an atomic on one word
    int* slot = areas + g.label_at + root;
    if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < n) atomicAdd(slot, len);
  }
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_apply(const int* __restrict__ blob, CcLimits lim, unsigned invert, int n,
                                                         unsigned* __restrict__ packed, const int* __restrict__ labels,
                                                         const int* __restrict__ areas, int* __restrict__ counts) {
  const CcPage g = cc_page(blob, blockIdx.z, lim);
  const long long t = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (!g.ok) return;
  unsigned* rows = packed + g.packed_at;
  int y = 0, x = 0;
  const bool mine = cc_pixel(g, t, y, x) && cc_is(rows, g, invert, y, x);
  bool flip = false, root = false;
  if (mine) {
    const int i = y * g.w + x, r = labels[g.label_at + i];
    if (r >= 0 && r <= i) {  // what k_cc_areas left: the root
      flip = areas[g.label_at + r] < n;
      root = flip && r == i;
    }
  }
  const unsigned long long flips = __ballot(flip), roots = __ballot(root);
  if (!flips) return;  // the wave
  const int lane = threadIdx.x & 63;
  if ((lane & 31) == 0) {
    const unsigned half = lane ? (unsigned)(flips >> 32) : (unsigned)flips;  // lane b of the half is bit 31 - b of the word
    if (half) rows[t >> 5] ^= __brev(half);
  }
  if (lane == 0) {
    int* c = counts + 4 * (int)blockIdx.z + (invert ? 2 : 0);
    if (roots) atomicAdd(c, __popcll(roots));
    atomicAdd(c + 1, __popcll(flips));
  }
}

// ------------------------------------------------------------------------------------------------ host
static unsigned cc_blocks(long long threads, long long most) {
  return (unsigned)std::min<long long>(std::max<long long>((threads + CC_THREADS - 1) / CC_THREADS, 1), most);
}

// One colour's launches on `s`; stages: bit k = launch k (label, merge, areas, apply) - all four but for the timing tool.
static void cc_pass(hipStream_t s, const int* blob, int n_pages, int max_h, int max_w, const CcLimits& lim, unsigned invert, int eight, int n,
                    uint32_t* packed, int* labels, int* areas, int* counts, int stages = 15) {
  const unsigned pages = (unsigned)n_pages;
  const dim3 tiles((unsigned)((max_w + CC_TILE_W - 1) / CC_TILE_W), (unsigned)((max_h + CC_TILE_H - 1) / CC_TILE_H), pages);
  if (stages & 1) {
    hipLaunchKernelGGL(k_cc_label, tiles, dim3(CC_THREADS), 0, s, blob, lim, invert, eight, (const unsigned*)packed, labels, areas);
    YMK_HIP(hipGetLastError());
  }
  const long long seams = (long long)((max_h - 1) / CC_TILE_H) * max_w + (long long)((max_w - 1) / CC_TILE_W) * max_h;
  if ((stages & 2) && seams > 0) {
    hipLaunchKernelGGL(k_cc_merge, dim3(cc_blocks(seams, 65535), 1u, pages), dim3(CC_THREADS), 0, s, blob, lim, invert, eight,
                       (const unsigned*)packed, labels);
    YMK_HIP(hipGetLastError());
  }
  const long long bits = (long long)max_h * ((max_w + 31) >> 5) * 32;  // below 2^28 + 2^19: fewer than 2^21 blocks
  const dim3 words(cc_blocks(bits, 1LL << 22), 1u, pages);
  if (stages & 4) {
    hipLaunchKernelGGL(k_cc_areas, words, dim3(CC_THREADS), 0, s, blob, lim, invert, n, (const unsigned*)packed, labels, areas);
    YMK_HIP(hipGetLastError());
  }
  if (stages & 8) {
    hipLaunchKernelGGL(k_cc_apply, words, dim3(CC_THREADS), 0, s, blob, lim, invert, n, (unsigned*)packed, (const int*)labels, (const int*)areas,
                       counts);
    YMK_HIP(hipGetLastError());
  }
}

struct CcCall {
  hipStream_t s;
  CcLimits lim;
};
static CcCall cc_check(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, const uint32_t* packed_dev, int64_t packed_bytes,
                       const int* labels_dev, int64_t labels_bytes, const int* areas_dev, int64_t areas_bytes, int n_black, int n_white,
                       const int* counts_dev, void* stream) {
  YMK_CHECK(n_pages >= 1 && n_pages <= 4096, "0..4096 pages");
  YMK_CHECK(blob_dev && ((uintptr_t)blob_dev & 3) == 0 && blob_words >= (int64_t)n_pages * CC_REC, "page table: n records");
  YMK_CHECK(max_h >= 1 && max_w >= 1 && max_h <= CC_MAX_SIDE && max_w <= CC_MAX_SIDE, "a page has 1..16383 pixels on a side");
  YMK_CHECK(packed_dev && ((uintptr_t)packed_dev & 3) == 0 && packed_bytes >= 0, "packed rows: null, misaligned or a negative size");
  YMK_CHECK(labels_dev && areas_dev && (((uintptr_t)labels_dev | (uintptr_t)areas_dev) & 3) == 0, "null or misaligned labels or areas");
  YMK_CHECK(labels_bytes >= 0 && areas_bytes >= 0, "negative size");
  YMK_CHECK(n_black >= 0 && n_black <= 65535 && n_white >= 0 && n_white <= 65535, "n is 0..65535");
  YMK_CHECK(counts_dev && ((uintptr_t)counts_dev & 3) == 0, "null or misaligned counts");
  return CcCall{(hipStream_t)stream, CcLimits{packed_bytes / 4, std::min(labels_bytes, areas_bytes) / 4, max_h, max_w}};
}

}  // namespace ymk

extern "C" {

int ymk_cc_tile_w(void) { return ymk::CC_TILE_W; }
int ymk_cc_tile_h(void) { return ymk::CC_TILE_H; }

int ymk_cc_scratch_bytes(const int* h, const int* w, int n_pages, int64_t* sizes2_out) {
  try {
    YMK_CHECK(n_pages >= 0 && n_pages <= 4096 && sizes2_out && (n_pages == 0 || (h && w)), "bad argument");
    int64_t pixels = 0;
    for (int k = 0; k < n_pages; ++k) {
      YMK_CHECK(h[k] >= 1 && w[k] >= 1 && h[k] <= ymk::CC_MAX_SIDE && w[k] <= ymk::CC_MAX_SIDE, "a page has 1..16383 pixels on a side");
      pixels += (int64_t)h[k] * w[k];
    }
    sizes2_out[0] = sizes2_out[1] = ((pixels + 1) & ~1LL) * 4;
    return 0;
  } catch (const std::exception& e) {
    ymk::set_error(e.what());
    return 1;
  }
}

int ymk_cc_despeckle_pages(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, uint32_t* packed_dev, int64_t packed_bytes,
                           int* labels_dev, int64_t labels_bytes, int* areas_dev, int64_t areas_bytes, int n_black, int n_white, int* counts_dev,
                           void* stream) {
  try {
    if (n_pages == 0) return 0;
    const ymk::CcCall c = ymk::cc_check(blob_dev, blob_words, n_pages, max_h, max_w, packed_dev, packed_bytes, labels_dev, labels_bytes, areas_dev,
                                        areas_bytes, n_black, n_white, counts_dev, stream);
    YMK_HIP(hipMemsetAsync(counts_dev, 0, (size_t)n_pages * 4 * sizeof(int), c.s));
    if (n_black > 0) ymk::cc_pass(c.s, blob_dev, n_pages, max_h, max_w, c.lim, 0u, 1, n_black, packed_dev, labels_dev, areas_dev, counts_dev);
    if (n_white > 0) ymk::cc_pass(c.s, blob_dev, n_pages, max_h, max_w, c.lim, ~0u, 0, n_white, packed_dev, labels_dev, areas_dev, counts_dev);
    return 0;
  } catch (const std::exception& e) {
    ymk::set_error(e.what());
    return 1;
  }
}

int ymk_cc_stage(int stage, int white, const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, uint32_t* packed_dev,
                 int64_t packed_bytes, int* labels_dev, int64_t labels_bytes, int* areas_dev, int64_t areas_bytes, int n, int* counts_dev,
                 void* stream) {
  try {
    if (n_pages == 0) return 0;
    YMK_CHECK(stage >= 0 && stage <= 3, "a stage is 0 (label), 1 (merge), 2 (areas) or 3 (apply)");
    const ymk::CcCall c = ymk::cc_check(blob_dev, blob_words, n_pages, max_h, max_w, packed_dev, packed_bytes, labels_dev, labels_bytes, areas_dev,
                                        areas_bytes, n, n, counts_dev, stream);
    ymk::cc_pass(c.s, blob_dev, n_pages, max_h, max_w, c.lim, white ? ~0u : 0u, white ? 0 : 1, n, packed_dev, labels_dev, areas_dev, counts_dev,
                 1 << stage);
    return 0;
  } catch (const std::exception& e) {
    ymk::set_error(e.what());
    return 1;
  }
}
}
