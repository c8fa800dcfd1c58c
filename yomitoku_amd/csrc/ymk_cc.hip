// Despeckled pages: connected-component labelling of the packed rows of the Group 4 encoder, and the removal of every component
// below a size (include/ymk.h, "Despeckled pages"; yomitoku_amd/despeckle.py; DESIGN.md, "Despeckled pages").
// tests/despeckle_ref.py is the definition; the bits and the four counts equal it exactly: a component's area is a sum of ones,
// which no order of addition changes.
//
// One pass per colour - black under 8-connectivity, then, on its result, white under 4 -, four launches each.  A page's pixel
// (y, x) has the index i = y w + x < 2^28 and two words of scratch, label[i] and area[i] (8 bytes a pixel; the blob pass of
// ymk_cc_filter_pages, below, has three more: 20 bytes a pixel).
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
// The root.  Every parent link goes from a larger index to a smaller one, so a tree's root is below every other pixel of the
// tree; once every unite() of a pass has returned a component is one tree; so after k_cc_merge a component's root is the smallest
// index of the component, whatever the timing - which pixels stand between a pixel and its root is what may differ from run to
// run, and k_cc_areas / k_cc_boxes store the root itself.  Row-major order makes the root's row the component's first row.
//
// Determinism.  A component's root is its smallest index, and its area is a sum of ones: every output bit and every count is
// independent of timing.
//
// Filtered ink (ymk_cc_filter_pages; tests/ink_filter_ref.py is the definition): behind the two passes a third, the blob pass,
// over the black components under 8-connectivity again - k_cc_label and k_cc_merge as they are, then
//
//   k_cc_boxes   one block per tile: a pixel stands for the pixel its label names where that is one of this tile - its tile's
//                root, which k_cc_label left and k_cc_merge did not touch: it only stores into roots' slots -, else for itself;
//                area and extents per such pixel in LDS, a run of lanes along a tile's row at a time (a wave is one row of the
//                tile, so a run never spans two rows); then one find, one add of the true area - not stopped at any n - and at
//                most three atomicMax into the root's words per pixel that stands for any; label[i] = that root.
//   k_cc_blob_apply  one thread per pixel: the pixel is cleared where its root's box has bh >= side, bw >= side and
//                256 area >= fill bh bw (64 bits); the ballot is the words' change, the two counts go to the page's counters.
//
// A pixel then has five words of scratch, 20 bytes: label, area, and three box words in boxes_dev, plane k of a page at
// 3 label_at + k h w.  The box words only ever grow, by atomicMax, from the 0 that k_cc_label stores at every pixel that is its
// tile's root (a component's root is one of them): plane 0 max(w - x) = w - x_min, plane 1 max(x + 1) = x_max + 1, plane 2
// max(y + 1) = y_max + 1; y_min is the root's row (above).  A maximum and a sum do not depend on the order of their terms, and
// the load that spares an atomicMax can only read a value that is at most the final one: skipped or not, the final word is the
// same.  Both kernels are straight-line code behind cc_find, which ends as argued above: what k_cc_boxes stores into the label slot
// of pixel i is find(rep) <= rep <= i, rep the pixel that i stands for - a pixel of i's own component, because a label only ever
// names one -, so the store keeps the invariant like k_cc_areas' does, and a find of another block that passes through the slot
// meanwhile reads an older parent or the root.  The barriers are __syncthreads inside a block, reached by all of its threads or
// by none.  Still no loop waits for another thread's progress.
//
#include "ymk_pages.h"

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
  g.packed_at = page_word64(r, 6), g.label_at = page_word64(r, 14);
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
                                                         const unsigned* __restrict__ packed, int* __restrict__ labels, int* __restrict__ areas,
                                                         int* __restrict__ boxes) {
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
    if (boxes && v == y * g.w + x) {  // the blob pass: a tile's root may be its component's
      int* b = boxes + 3 * g.label_at + v;
      const long long plane = (long long)g.h * g.w;
      b[0] = b[plane] = b[2 * plane] = 0;
    }
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
                                                         const int* __restrict__ areas, int* __restrict__ counts, int per_page) {
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
    int* c = counts + per_page * (int)blockIdx.z + (invert ? 2 : 0);  // per_page: 4, or the filter's 6
    if (roots) atomicAdd(c, __popcll(roots));
    atomicAdd(c + 1, __popcll(flips));
  }
}

// ------------------------------------------------------------------------------------------------ boxes and blob apply
// The blob pass (black, 8-connected).  A root's box words: see the file's header; `plane` = h w.
__device__ __forceinline__ void cc_raise(int* slot, int v) {
  // a word that has reached v stays at least v: a page-sized component costs a load, not an atomic on one word
  if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) atomicMax(slot, v);
}

// One block per tile, as k_cc_label.  What that launch left and k_cc_merge kept: the label of a pixel that is not its tile's root
// is its tile's root, a pixel of this tile; k_cc_merge has only ever stored into the slots of roots.  So a pixel stands for
// rep = label[i] where that lies in this tile and for itself otherwise (a tile's root, hung below a pixel elsewhere or below
// nothing) - either way a pixel of its own component, in this tile, and not larger than i.  The tile's pixels are summed per rep
// in LDS - per run of one rep along a tile row first -, and each rep that stands for any pixel takes its sums to its component's
// root once: a frame or a grid costs the root's words an atomic per tile it crosses, not one per run of every row.
__global__ __launch_bounds__(CC_THREADS) void k_cc_boxes(const int* __restrict__ blob, CcLimits lim, const unsigned* __restrict__ packed,
                                                         int* __restrict__ labels, int* __restrict__ areas, int* __restrict__ boxes) {
  __shared__ int s_area[CC_TILE], s_left[CC_TILE], s_right[CC_TILE], s_low[CC_TILE], s_root[CC_TILE];
  constexpr int PER = CC_TILE / CC_THREADS;
  const CcPage g = cc_page(blob, blockIdx.z, lim);
  const int x0 = (int)blockIdx.x * CC_TILE_W, y0 = (int)blockIdx.y * CC_TILE_H, tid = threadIdx.x;
  if (!g.ok || x0 >= g.w || y0 >= g.h) return;  // the whole block
  int* lab = labels + g.label_at;
  int rep[PER];  // the tile-local place (row * 64 + column) of what the pixel stands for; -1: no pixel of the colour
  bool any = false;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int t = tid + k * CC_THREADS, y = y0 + (t >> 6), x = x0 + (t & 63);
    rep[k] = -1;
    if (cc_is(packed + g.packed_at, g, 0u, y, x)) {
      const int i = y * g.w + x, v = lab[i];
      const int ry = v >= 0 ? v / g.w - y0 : -1, rx = v >= 0 ? v % g.w - x0 : -1;
      rep[k] = ry >= 0 && ry < CC_TILE_H && rx >= 0 && rx < CC_TILE_W && v <= i ? ry * CC_TILE_W + rx : t;
      any = true;
    }
  }
  if (!__syncthreads_or(any)) return;  // paper
  for (int t = tid; t < CC_TILE; t += CC_THREADS) s_area[t] = s_left[t] = s_right[t] = s_low[t] = 0;
  __syncthreads();
  const int lane = tid & 63;
#pragma unroll
  for (int k = 0; k < PER; ++k) {  // a wave's 64 lanes are one row of the tile
    const int t = tid + k * CC_THREADS, y = y0 + (t >> 6), x = x0 + lane;
    const int before = __shfl_up(rep[k], 1);
    const bool head = lane == 0 || before != rep[k];
    const unsigned long long heads = __ballot(head);
    if (rep[k] >= 0 && head) {
      const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
      const int len = rest ? __ffsll((long long)rest) : 64 - lane;  // the run is columns x .. x + len - 1 of row y
      atomicAdd(&s_area[rep[k]], len);
      atomicMax(&s_left[rep[k]], g.w - x);
      atomicMax(&s_right[rep[k]], x + len);
      atomicMax(&s_low[rep[k]], y + 1);
    }
  }
  __syncthreads();
  const long long plane = (long long)g.h * g.w;
  for (int t = tid; t < CC_TILE; t += CC_THREADS) {
    if (s_area[t] == 0) continue;
    const int root = cc_find<true>(lab, (y0 + (t >> 6)) * g.w + x0 + (t & 63));
    s_root[t] = root;
    atomicAdd(areas + g.label_at + root, s_area[t]);
    int* b = boxes + 3 * g.label_at + root;
    cc_raise(b, s_left[t]);
    cc_raise(b + plane, s_right[t]);
    cc_raise(b + 2 * plane, s_low[t]);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (rep[k] < 0) continue;
    const int t = tid + k * CC_THREADS;
    __hip_atomic_store(lab + (y0 + (t >> 6)) * g.w + x0 + (t & 63), s_root[rep[k]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // <= rep <= i
  }
}

// Thread t of a page is bit t & 31 of packed word t >> 5, as in k_cc_apply; the two counts are summed over the block first.
__global__ __launch_bounds__(CC_THREADS) void k_cc_blob_apply(const int* __restrict__ blob, CcLimits lim, int side, int fill,
                                                              unsigned* __restrict__ packed, const int* __restrict__ labels,
                                                              const int* __restrict__ areas, const int* __restrict__ boxes,
                                                              int* __restrict__ counts, int per_page) {
  __shared__ int s_count[2];
  const CcPage g = cc_page(blob, blockIdx.z, lim);
  const long long t = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (!g.ok) return;  // the whole grid row of the page
  if (threadIdx.x < 2) s_count[threadIdx.x] = 0;
  __syncthreads();
  unsigned* rows = packed + g.packed_at;
  int y = 0, x = 0;
  const bool mine = cc_pixel(g, t, y, x) && cc_is(rows, g, 0u, y, x);
  bool flip = false, root = false;
  if (mine) {
    const int i = y * g.w + x, r = labels[g.label_at + i];
    if (r >= 0 && r <= i) {  // what k_cc_boxes left: the root
      const long long plane = (long long)g.h * g.w;
      const int* b = boxes + 3 * g.label_at + r;
      const int bw = b[0] + b[plane] - g.w;         // (x_max + 1) - x_min
      const int bh = b[2 * plane] - r / g.w;        // (y_max + 1) - y_min: the root's row is the first
      flip = bh >= side && bw >= side && 256LL * areas[g.label_at + r] >= (long long)fill * bh * bw;
      root = flip && r == i;
    }
  }
  const unsigned long long flips = __ballot(flip), roots = __ballot(root);
  const int lane = threadIdx.x & 63;
  if (flips && (lane & 31) == 0) {
    const unsigned half = lane ? (unsigned)(flips >> 32) : (unsigned)flips;  // lane b of the half is bit 31 - b of the word
    if (half) rows[t >> 5] ^= __brev(half);
  }
  if (flips && lane == 0) {
    if (roots) atomicAdd(&s_count[0], __popcll(roots));
    atomicAdd(&s_count[1], __popcll(flips));
  }
  __syncthreads();
  if (threadIdx.x < 2 && s_count[threadIdx.x]) atomicAdd(counts + per_page * (int)blockIdx.z + 4 + threadIdx.x, s_count[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------ host
static unsigned cc_blocks(long long threads, long long most) {
  return (unsigned)std::min<long long>(std::max<long long>((threads + CC_THREADS - 1) / CC_THREADS, 1), most);
}

// One colour's launches on `s`; stages: bit k = launch k (label, merge, areas, apply) - all four but for the timing tool.
static void cc_pass(hipStream_t s, const int* blob, int n_pages, int max_h, int max_w, const CcLimits& lim, unsigned invert, int eight, int n,
                    uint32_t* packed, int* labels, int* areas, int* counts, int stages = 15, int per_page = 4, int* boxes = nullptr, int side = 0,
                    int fill = 0) {
  const unsigned pages = (unsigned)n_pages;
  const dim3 tiles((unsigned)((max_w + CC_TILE_W - 1) / CC_TILE_W), (unsigned)((max_h + CC_TILE_H - 1) / CC_TILE_H), pages);
  if (stages & 1) {
    hipLaunchKernelGGL(k_cc_label, tiles, dim3(CC_THREADS), 0, s, blob, lim, invert, eight, (const unsigned*)packed, labels, areas, boxes);
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
  if (boxes) {  // the blob pass: the third and fourth launch are its own
    if (stages & 4) {
      hipLaunchKernelGGL(k_cc_boxes, tiles, dim3(CC_THREADS), 0, s, blob, lim, (const unsigned*)packed, labels, areas, boxes);
      YMK_HIP(hipGetLastError());
    }
    if (stages & 8) {
      hipLaunchKernelGGL(k_cc_blob_apply, words, dim3(CC_THREADS), 0, s, blob, lim, side, fill, (unsigned*)packed, (const int*)labels,
                         (const int*)areas, (const int*)boxes, counts, per_page);
      YMK_HIP(hipGetLastError());
    }
    return;
  }
  if (stages & 4) {
    hipLaunchKernelGGL(k_cc_areas, words, dim3(CC_THREADS), 0, s, blob, lim, invert, n, (const unsigned*)packed, labels, areas);
    YMK_HIP(hipGetLastError());
  }
  if (stages & 8) {
    hipLaunchKernelGGL(k_cc_apply, words, dim3(CC_THREADS), 0, s, blob, lim, invert, n, (unsigned*)packed, (const int*)labels, (const int*)areas,
                       counts, per_page);
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
  check_page_table(blob_dev, blob_words, n_pages, CC_REC, 3, 4096, "0..4096 pages", "page table: n records");  // no caller comes with 0
  YMK_CHECK(max_h >= 1 && max_w >= 1 && max_h <= CC_MAX_SIDE && max_w <= CC_MAX_SIDE, "a page has 1..16383 pixels on a side");
  YMK_CHECK(packed_dev && ((uintptr_t)packed_dev & 3) == 0 && packed_bytes >= 0, "packed rows: null, misaligned or a negative size");
  YMK_CHECK(labels_dev && areas_dev && (((uintptr_t)labels_dev | (uintptr_t)areas_dev) & 3) == 0, "null or misaligned labels or areas");
  YMK_CHECK(labels_bytes >= 0 && areas_bytes >= 0, "negative size");
  YMK_CHECK(n_black >= 0 && n_black <= 65535 && n_white >= 0 && n_white <= 65535, "n is 0..65535");
  YMK_CHECK(counts_dev && ((uintptr_t)counts_dev & 3) == 0, "null or misaligned counts");
  return CcCall{(hipStream_t)stream, CcLimits{packed_bytes / 4, std::min(labels_bytes, areas_bytes) / 4, max_h, max_w}};
}

// What the filter's entries check beyond cc_check: the blob rule's two numbers, and - side > 0 - the box words, three a pixel, which
// then bound a page's place like the labels and the areas do.
static void cc_check_blobs(CcCall& c, int side, int fill, const int* boxes_dev, int64_t boxes_bytes) {
  YMK_CHECK(side == 0 || (side >= 2 && side <= CC_MAX_SIDE), "side is 0 or 2..16383");
  if (side == 0) return;
  YMK_CHECK(fill >= 1 && fill <= 256, "fill is 1..256, in 256ths of the box");
  YMK_CHECK(boxes_dev && ((uintptr_t)boxes_dev & 3) == 0 && boxes_bytes >= 0, "boxes: null, misaligned or a negative size");
  c.lim.label_words = std::min<long long>(c.lim.label_words, boxes_bytes / 12);
}

}  // namespace ymk

extern "C" {

int ymk_cc_tile_w(void) { return ymk::CC_TILE_W; }
int ymk_cc_tile_h(void) { return ymk::CC_TILE_H; }

int ymk_cc_scratch_bytes(const int* h, const int* w, int n_pages, int64_t* sizes2_out) {
  YMK_API_BEGIN
  YMK_CHECK(n_pages >= 0 && n_pages <= 4096 && sizes2_out && (n_pages == 0 || (h && w)), "bad argument");
  int64_t pixels = 0;
  for (int k = 0; k < n_pages; ++k) {
    YMK_CHECK(h[k] >= 1 && w[k] >= 1 && h[k] <= ymk::CC_MAX_SIDE && w[k] <= ymk::CC_MAX_SIDE, "a page has 1..16383 pixels on a side");
    pixels += (int64_t)h[k] * w[k];
  }
  sizes2_out[0] = sizes2_out[1] = ((pixels + 1) & ~1LL) * 4;
  YMK_API_END
}

int ymk_cc_despeckle_pages(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, uint32_t* packed_dev, int64_t packed_bytes,
                           int* labels_dev, int64_t labels_bytes, int* areas_dev, int64_t areas_bytes, int n_black, int n_white, int* counts_dev,
                           void* stream) {
  YMK_API_BEGIN
  if (n_pages == 0) return 0;
  const ymk::CcCall c = ymk::cc_check(blob_dev, blob_words, n_pages, max_h, max_w, packed_dev, packed_bytes, labels_dev, labels_bytes, areas_dev,
                                      areas_bytes, n_black, n_white, counts_dev, stream);
  YMK_HIP(hipMemsetAsync(counts_dev, 0, (size_t)n_pages * 4 * sizeof(int), c.s));
  if (n_black > 0) ymk::cc_pass(c.s, blob_dev, n_pages, max_h, max_w, c.lim, 0u, 1, n_black, packed_dev, labels_dev, areas_dev, counts_dev);
  if (n_white > 0) ymk::cc_pass(c.s, blob_dev, n_pages, max_h, max_w, c.lim, ~0u, 0, n_white, packed_dev, labels_dev, areas_dev, counts_dev);
  YMK_API_END
}

int ymk_cc_filter_scratch_bytes(const int* h, const int* w, int n_pages, int64_t* sizes3_out) {
  if (ymk_cc_scratch_bytes(h, w, n_pages, sizes3_out) != 0) return 1;  // sizes3_out is checked there
  sizes3_out[2] = 3 * sizes3_out[0];
  return 0;
}

int ymk_cc_filter_pages(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, uint32_t* packed_dev, int64_t packed_bytes,
                        int* labels_dev, int64_t labels_bytes, int* areas_dev, int64_t areas_bytes, int* boxes_dev, int64_t boxes_bytes, int n_black,
                        int n_white, int side, int fill, int* counts_dev, void* stream) {
  YMK_API_BEGIN
  if (n_pages == 0) return 0;
  ymk::CcCall c = ymk::cc_check(blob_dev, blob_words, n_pages, max_h, max_w, packed_dev, packed_bytes, labels_dev, labels_bytes, areas_dev,
                                areas_bytes, n_black, n_white, counts_dev, stream);
  ymk::cc_check_blobs(c, side, fill, boxes_dev, boxes_bytes);
  YMK_HIP(hipMemsetAsync(counts_dev, 0, (size_t)n_pages * 6 * sizeof(int), c.s));
  if (n_black > 0) ymk::cc_pass(c.s, blob_dev, n_pages, max_h, max_w, c.lim, 0u, 1, n_black, packed_dev, labels_dev, areas_dev, counts_dev, 15, 6);
  if (n_white > 0) ymk::cc_pass(c.s, blob_dev, n_pages, max_h, max_w, c.lim, ~0u, 0, n_white, packed_dev, labels_dev, areas_dev, counts_dev, 15, 6);
  if (side > 0)
    ymk::cc_pass(c.s, blob_dev, n_pages, max_h, max_w, c.lim, 0u, 1, 0, packed_dev, labels_dev, areas_dev, counts_dev, 15, 6, boxes_dev, side, fill);
  YMK_API_END
}

int ymk_cc_filter_stage(int stage, const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, uint32_t* packed_dev,
                        int64_t packed_bytes, int* labels_dev, int64_t labels_bytes, int* areas_dev, int64_t areas_bytes, int* boxes_dev,
                        int64_t boxes_bytes, int side, int fill, int* counts_dev, void* stream) {
  YMK_API_BEGIN
  if (n_pages == 0) return 0;
  YMK_CHECK(stage >= 0 && stage <= 3, "a stage is 0 (label), 1 (merge), 2 (boxes) or 3 (apply)");
  YMK_CHECK(side >= 2, "the blob pass needs a side");
  ymk::CcCall c = ymk::cc_check(blob_dev, blob_words, n_pages, max_h, max_w, packed_dev, packed_bytes, labels_dev, labels_bytes, areas_dev,
                                areas_bytes, 0, 0, counts_dev, stream);
  ymk::cc_check_blobs(c, side, fill, boxes_dev, boxes_bytes);
  ymk::cc_pass(c.s, blob_dev, n_pages, max_h, max_w, c.lim, 0u, 1, 0, packed_dev, labels_dev, areas_dev, counts_dev, 1 << stage, 6, boxes_dev, side,
               fill);
  YMK_API_END
}

int ymk_cc_stage(int stage, int white, const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, uint32_t* packed_dev,
                 int64_t packed_bytes, int* labels_dev, int64_t labels_bytes, int* areas_dev, int64_t areas_bytes, int n, int* counts_dev,
                 void* stream) {
  YMK_API_BEGIN
  if (n_pages == 0) return 0;
  YMK_CHECK(stage >= 0 && stage <= 3, "a stage is 0 (label), 1 (merge), 2 (areas) or 3 (apply)");
  const ymk::CcCall c = ymk::cc_check(blob_dev, blob_words, n_pages, max_h, max_w, packed_dev, packed_bytes, labels_dev, labels_bytes, areas_dev,
                                      areas_bytes, n, n, counts_dev, stream);
  ymk::cc_pass(c.s, blob_dev, n_pages, max_h, max_w, c.lim, white ? ~0u : 0u, white ? 0 : 1, n, packed_dev, labels_dev, areas_dev, counts_dev,
               1 << stage);
  YMK_API_END
}
}
