// Overlay rasteriser for visualize=True: an ordered list of primitives drawn onto a uint8 [h][w][3] canvas resident in HBM.
//
//   k_draw_overlay     one block per TILE x TILE canvas tile.  The host bins the commands by bounding box into per-tile lists
//                      (CSR: tile_offsets[tiles + 1], tile_cmds[] = command indices, ascending).  A block walks ITS list through
//                      LDS in chunks of CHUNK records; every thread owns PX horizontally adjacent pixels of the tile, keeps them
//                      in registers over the whole list and stores them once.  A tile with an empty list returns before it has
//                      read or written a canvas byte.  No atomics, no allocation, no host wait: tiles are disjoint, and inside a
//                      tile the commands are applied in list (= command) order, so the result equals drawing the commands one
//                      after the other over the whole canvas.
//   k_heatmap_blend    det_visualizer(vis_heatmap=True) (utils/visualizer.py:81-91 of the reference) in integers: the
//                      probability map quantised to uint8, a fixed-point bilinear sample, a 256-entry jet table, a 50 % blend.
//
//   The layer ("Overlay rasteriser", "Layer"): next to its PX canvas pixels a thread keeps a LAYER for the same pixels,
//   a colour and a coverage packed into one register per pixel.  A record with YMK_OVERLAY_TO_LAYER in word 0 paints the layer
//   instead of the canvas; YMK_OVERLAY_FLUSH composites the layer over the canvas ONCE and clears it.  overlay_apply is the one
//   per-record loop of both draw kernels.
//
// Every coverage test is exact integer arithmetic ("Overlay rasteriser"): coordinates lie in [-16383, 16383], so
// squared lengths stay below 2^32 and the products compared stay below 2^63; the factor 4 of `4 c <= T` is moved to the right
// as an integer division (c integer: 4 c <= T  <=>  c <= T / 4 for T >= 0).
#include "ymk_common.h"

#include "../../include/ymk.h"

namespace ymk {

constexpr int OV_TILE = 32;                              // tile edge (ymk_overlay_tile)
constexpr int OV_PX = 4;                                 // pixels per thread, adjacent in x
constexpr int OV_THREADS = OV_TILE * OV_TILE / OV_PX;    // 256
constexpr int OV_CHUNK = 64;                             // command records staged in LDS at a time
constexpr int OV_WORDS = YMK_OVERLAY_CMD_WORDS;          // int32 words per record
static_assert(OV_WORDS == 16, "the staging loop moves a record as four int4");
static_assert(OV_PX == 4, "a thread's layer is four packed registers");
static_assert(OV_CHUNK * OV_WORDS / 4 == OV_THREADS, "one int4 per thread stages a chunk");

__device__ __forceinline__ int blend_u8(int dst, int colour, int a) { return (colour * a + dst * (255 - a) + 127) / 255; }

// coverage (0..255; 0 = not covered) of command `c` of kind `kind` (word 0 without its flag) at pixel (px, py)
__device__ __forceinline__ int overlay_alpha(int kind, const int* __restrict__ c, int px, int py,
                                             const unsigned char* __restrict__ atlas, long long atlas_bytes) {
  if (kind == YMK_OVERLAY_SEG) {
    // coordinates lie in [-16383, 16383] and pixels in [0, 16383): differences fit 32 bits, every product is widened to 64
    const int x0 = c[5], y0 = c[6], x1 = c[7], y1 = c[8], t = c[9];
    const int dx = x1 - x0, dy = y1 - y0, qx = px - x0, qy = py - y0;
    const long long l2 = (long long)dx * dx + (long long)dy * dy, u = (long long)qx * dx + (long long)qy * dy, t2 = (long long)t * t;
    bool in;
    if (l2 == 0 || u <= 0) {
      in = (long long)qx * qx + (long long)qy * qy <= t2 / 4;
    } else if (u >= l2) {
      const int ex = px - x1, ey = py - y1;
      in = (long long)ex * ex + (long long)ey * ey <= t2 / 4;
    } else {
      const long long cr = (long long)qx * dy - (long long)qy * dx;  // |cr| < 2^32: cr * cr < 2^63 (|q|, |d| <= 32766 sqrt 2)
      in = cr * cr <= (t2 * l2) / 4;
    }
    return in ? c[4] : 0;
  }
  if (kind == YMK_OVERLAY_BOX) {
    const bool outer = px >= c[5] && px <= c[7] && py >= c[6] && py <= c[8];
    const bool inner = c[9] <= c[11] && c[10] <= c[12] && px >= c[9] && px <= c[11] && py >= c[10] && py <= c[12];
    return outer && !inner ? c[4] : 0;
  }
  if (kind == YMK_OVERLAY_GLYPH) {
    const int gx = px - c[5], gy = py - c[6];
    if (gx < 0 || gy < 0 || gx >= c[7] || gy >= c[8]) return 0;
    const long long at = (long long)c[9] + (long long)gy * c[10] + gx;
    return at >= 0 && at < atlas_bytes ? (int)atlas[at] : 0;  // a record that points outside the atlas draws nothing
  }
  if (kind == YMK_OVERLAY_RBOX) {
    const int x1 = c[5], y1 = c[6], x2 = c[7], y2 = c[8];
    if (px < x1 || px > x2 || py < y1 || py > y2) return 0;
    const int r = max(min(min(c[9], (x2 - x1) / 2), (y2 - y1) / 2), 0);
    const int ex = px - min(max(px, x1 + r), x2 - r), ey = py - min(max(py, y1 + r), y2 - r);  // |ex|, |ey| <= r <= 16383
    return ex * ex + ey * ey <= r * r ? c[4] : 0;
  }
  return 0;
}

// the layer of one pixel in one register: colour channel ch in bits 8 ch .. 8 ch + 7, coverage in bits 24 .. 31
__device__ __forceinline__ unsigned layer_pack(int c0, int c1, int c2, int cov) {
  return (unsigned)(c0 & 255) | (unsigned)(c1 & 255) << 8 | (unsigned)(c2 & 255) << 16 | (unsigned)(cov & 255) << 24;
}

// Records s_cmd[0 .. count) applied in order to the thread's PX canvas pixels and to their layer.  Every branch on a record's
// word is wave-uniform (the record is an LDS broadcast); only the coverage of a pixel diverges.
__device__ __forceinline__ void overlay_apply(const int* __restrict__ s_cmd, int count, int (&pix)[OV_PX][3], unsigned (&layer)[OV_PX],
                                              int px0, int py, const unsigned char* __restrict__ atlas, long long atlas_bytes) {
  for (int i = 0; i < count; ++i) {
    // the same address in every lane: an LDS broadcast.  The words are moved to scalar registers, so whatever depends on the
    // record alone (a segment's direction and squared length, a rounded box's radius) is computed once per wave
    int c[13];
#pragma unroll
    for (int j = 0; j < 13; ++j) c[j] = __builtin_amdgcn_readfirstlane(s_cmd[i * OV_WORDS + j]);
    const int word0 = c[0];
    if (word0 & ~(YMK_OVERLAY_KIND_MASK | YMK_OVERLAY_TO_LAYER)) continue;  // -1 (an empty glyph) and any other stray bit
    const int kind = word0 & YMK_OVERLAY_KIND_MASK;
    const bool to_layer = (word0 & YMK_OVERLAY_TO_LAYER) != 0;
    if (kind == YMK_OVERLAY_FLUSH) {
      if (to_layer || py < c[6] || py > c[8]) continue;
      const int alpha = c[4];
      const bool keep255 = c[9] != 0;
#pragma unroll
      for (int k = 0; k < OV_PX; ++k) {
        if (px0 + k < c[5] || px0 + k > c[7]) continue;
        const unsigned l = layer[k];
        layer[k] = 0;
        const int cov = (int)(l >> 24);
        if (cov == 0) continue;
        const int e = (cov * alpha + 127) / 255;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int colour = (int)(l >> (8 * ch)) & 255;
          if (!(keep255 && colour == 255)) pix[k][ch] = blend_u8(pix[k][ch], colour, e);
        }
      }
      continue;
    }
    const int cb = c[1], cg = c[2], cr = c[3];
    if (!to_layer) {
#pragma unroll
      for (int k = 0; k < OV_PX; ++k) {
        const int a = overlay_alpha(kind, c, px0 + k, py, atlas, atlas_bytes);
        if (a > 0) {
          pix[k][0] = blend_u8(pix[k][0], cb, a);
          pix[k][1] = blend_u8(pix[k][1], cg, a);
          pix[k][2] = blend_u8(pix[k][2], cr, a);
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < OV_PX; ++k) {
        const int a = overlay_alpha(kind, c, px0 + k, py, atlas, atlas_bytes);
        if (a > 0) {
          const unsigned l = layer[k];
          const int cov = (int)(l >> 24);
          layer[k] = cov == 0 ? layer_pack(cb, cg, cr, a)
                              : layer_pack(blend_u8((int)(l & 255), cb, a), blend_u8((int)(l >> 8) & 255, cg, a),
                                           blend_u8((int)(l >> 16) & 255, cr, a), blend_u8(cov, 255, a));
        }
      }
    }
  }
}

__global__ __launch_bounds__(OV_THREADS) void k_draw_overlay(unsigned char* __restrict__ canvas, int h, int w,
                                                             const int* __restrict__ cmds, int n,
                                                             const int* __restrict__ tile_offsets,
                                                             const int* __restrict__ tile_cmds, int n_list,
                                                             const unsigned char* __restrict__ atlas, long long atlas_bytes) {
  __shared__ __attribute__((aligned(16))) int s_cmd[OV_CHUNK * OV_WORDS];
  const int tile = blockIdx.y * gridDim.x + blockIdx.x;
  const int begin = max(tile_offsets[tile], 0), end = min(tile_offsets[tile + 1], n_list);
  if (begin >= end) return;  // block-uniform: an empty list leaves the tile alone
  const int px0 = blockIdx.x * OV_TILE + (threadIdx.x % (OV_TILE / OV_PX)) * OV_PX;
  const int py = blockIdx.y * OV_TILE + threadIdx.x / (OV_TILE / OV_PX);
  const bool row_in = py < h;
  unsigned char* row = canvas + ((size_t)(row_in ? py : 0) * w) * 3;
  int pix[OV_PX][3];
  unsigned layer[OV_PX] = {0, 0, 0, 0};  // dropped when the tile ends, flushed or not
#pragma unroll
  for (int k = 0; k < OV_PX; ++k) {
    const bool in = row_in && px0 + k < w;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) pix[k][ch] = in ? (int)row[(size_t)(px0 + k) * 3 + ch] : 0;
  }
  for (int base = begin; base < end; base += OV_CHUNK) {
    const int count = min(OV_CHUNK, end - base);
    __syncthreads();  // the previous chunk has been read by every thread
    {
      const int rec = threadIdx.x / 4, quarter = threadIdx.x % 4;
      if (rec < count) {
        const int id = tile_cmds[base + rec];
        int4 v = make_int4(-1, 0, 0, 0);  // kind -1: a list entry outside [0, n) draws nothing
        if (id >= 0 && id < n) v = reinterpret_cast<const int4*>(cmds + (size_t)id * OV_WORDS)[quarter];
        else if (quarter != 0) v = make_int4(0, 0, 0, 0);
        reinterpret_cast<int4*>(s_cmd + rec * OV_WORDS)[quarter] = v;
      }
    }
    __syncthreads();
    overlay_apply(s_cmd, count, pix, layer, px0, py, atlas, atlas_bytes);
  }
  if (!row_in) return;
#pragma unroll
  for (int k = 0; k < OV_PX; ++k) {
    if (px0 + k < w) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) row[(size_t)(px0 + k) * 3 + ch] = (unsigned char)pix[k][ch];
    }
  }
}

// ---- a wave of canvases in one launch (DocumentAnalyzer.serve(overlays=True)) -------------------------------------------------
//
//   k_overlay_layout       one wavefront per text run: the pen of character i is the run's pen plus the exclusive prefix sum of
//                          the advances before it (horizontal) or plus i steps (vertical); the scan runs OV_SCAN characters at a
//                          time with a carry.  Writes words 5..10 of the run's GLYPH slots, kind -1 into a slot whose character
//                          has no pixels.
//   k_overlay_bounds       every command's inclusive bounding box clipped to ITS canvas, four int16 (1, 1, 0, 0 = covers nothing).
//   k_draw_overlay_pages   one block per tile of ANY canvas of the wave.  No host binning: the block culls its canvas's commands
//                          against its tile OV_THREADS boxes at a time, compacts the hits IN COMMAND ORDER into an LDS ring
//                          (64-bit ballot + popcount prefix) and applies them through the chunk loop of k_draw_overlay.  Culling
//                          by the clipped box is bin_commands' predicate and the order inside a tile is command order, so the
//                          canvas equals what k_draw_overlay draws from the host's lists.
constexpr int OV_SCAN = 64;                // characters per scan step: one per lane of a wavefront
constexpr int OV_RING = 512;               // hit ring: at most OV_CHUNK - 1 pending hits + OV_THREADS new ones
constexpr int OV_COORD = 16383;
static_assert(OV_RING >= OV_CHUNK + OV_THREADS && (OV_RING & (OV_RING - 1)) == 0, "ring holds a pass on top of a partial chunk");
static_assert(OV_THREADS % 64 == 0, "the compaction counts per 64-lane wavefront");

__device__ __forceinline__ int clamp_coord(long long v) {
  return (int)(v < -OV_COORD ? -OV_COORD : (v > OV_COORD ? OV_COORD : v));
}

__global__ __launch_bounds__(OV_SCAN) void k_overlay_layout(int* __restrict__ cmds, int n_cmds, const int* __restrict__ runs,
                                                            int n_runs, const int* __restrict__ codes, int n_codes,
                                                            const int* __restrict__ glyphs, int n_glyphs) {
  const int r = blockIdx.x;
  if (r >= n_runs) return;
  const int* run = runs + (size_t)r * YMK_OVERLAY_RUN_WORDS;
  const long long slot0 = run[0], code0 = run[1], count = run[2];
  const long long pen_x = run[3], pen_y = run[4];
  const bool vertical = run[5] != 0;
  const long long step = run[6];
  // a run that points outside the slot or code arrays is skipped, not trusted (block-uniform)
  if (count <= 0 || slot0 < 0 || code0 < 0 || slot0 + count > n_cmds || code0 + count > n_codes) return;
  const int lane = threadIdx.x;
  long long carry = 0;  // sum of the advances of the characters before this step
  for (long long base = 0; base < count; base += OV_SCAN) {
    const long long i = base + lane;
    const bool live = i < count;
    int off = 0, gw = 0, gh = 0, ox = 0, oy = 0, adv = 0;
    bool known = false;
    if (live) {
      const int id = codes[code0 + i];
      if (id >= 0 && id < n_glyphs) {
        const int* g = glyphs + (size_t)id * YMK_OVERLAY_GLYPH_WORDS;
        off = g[0], gw = g[1], gh = g[2], ox = g[3], oy = g[4], adv = g[5];
        known = true;
      }
    }
    int incl = adv;  // inclusive scan over the wavefront
#pragma unroll
    for (int d = 1; d < OV_SCAN; d <<= 1) {
      const int up = __shfl_up(incl, d, OV_SCAN);
      if (lane >= d) incl += up;
    }
    const int total = __shfl(incl, OV_SCAN - 1, OV_SCAN);
    if (live) {
      int* c = cmds + (size_t)(slot0 + i) * OV_WORDS;
      if (known && gw > 0 && gh > 0) {
        const long long x = vertical ? pen_x : pen_x + carry + (incl - adv);
        const long long y = vertical ? pen_y + i * step : pen_y;
        c[5] = clamp_coord(x + ox);
        c[6] = clamp_coord(y + oy);
        c[7] = gw;
        c[8] = gh;
        c[9] = off;
        c[10] = gw;
      } else {
        c[0] = -1;  // a space, or an id outside the table: a record that draws nothing
#pragma unroll
        for (int k = 5; k <= 10; ++k) c[k] = 0;
      }
    }
    carry += total;
  }
}

// canvas table entry: YMK_OVERLAY_CANVAS_WORDS int64 = byte offset, h, w, first command, command count, first tile
struct OvCanvas {
  long long offset, h, w, first, count, tile0;
};

__device__ __forceinline__ bool canvas_ok(const OvCanvas& cv, long long canvas_bytes, int n_cmds) {
  if (!(cv.h > 0 && cv.w > 0 && cv.h <= OV_COORD && cv.w <= OV_COORD)) return false;
  return cv.offset >= 0 && cv.offset <= canvas_bytes - cv.h * cv.w * 3 && cv.first >= 0 && cv.first <= n_cmds && cv.count >= 0 &&
         cv.count <= n_cmds - cv.first && cv.tile0 >= 0;
}

__global__ __launch_bounds__(256) void k_overlay_bounds(const int* __restrict__ cmds, int n_cmds, short* __restrict__ bounds,
                                                        const long long* __restrict__ table, int n_canvases) {
  const int ci = blockIdx.y;
  if (ci >= n_canvases) return;
  const OvCanvas cv = reinterpret_cast<const OvCanvas*>(table)[ci];
  if (!canvas_ok(cv, 0x7fffffffffffffffLL, n_cmds)) return;
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < cv.count; k += (long long)gridDim.x * blockDim.x) {
    const int* c = cmds + (size_t)(cv.first + k) * OV_WORDS;
    int x0 = 1, y0 = 1, x1 = 0, y1 = 0;
    const int kind = c[0] & ~(YMK_OVERLAY_KIND_MASK | YMK_OVERLAY_TO_LAYER) ? -1 : c[0] & YMK_OVERLAY_KIND_MASK;  // flagged: the bounds of its kind
    if (kind == YMK_OVERLAY_SEG) {
      const int pad = (c[9] + 1) / 2;  // t >= 0: a segment reaches t / 2 from its axis
      x0 = min(c[5], c[7]) - pad, y0 = min(c[6], c[8]) - pad, x1 = max(c[5], c[7]) + pad, y1 = max(c[6], c[8]) + pad;
    } else if (kind == YMK_OVERLAY_BOX || kind == YMK_OVERLAY_RBOX || kind == YMK_OVERLAY_FLUSH) {
      x0 = c[5], y0 = c[6], x1 = c[7], y1 = c[8];
    } else if (kind == YMK_OVERLAY_GLYPH) {
      x0 = c[5], y0 = c[6], x1 = c[5] + c[7] - 1, y1 = c[6] + c[8] - 1;
    }
    x0 = max(x0, 0), y0 = max(y0, 0), x1 = min(x1, (int)cv.w - 1), y1 = min(y1, (int)cv.h - 1);
    if (x0 > x1 || y0 > y1) x0 = 1, y0 = 1, x1 = 0, y1 = 0;
    short* b = bounds + (size_t)(cv.first + k) * 4;
    b[0] = (short)x0, b[1] = (short)y0, b[2] = (short)x1, b[3] = (short)y1;
  }
}

__global__ __launch_bounds__(OV_THREADS) void k_draw_overlay_pages(unsigned char* __restrict__ canvases, long long canvas_bytes,
                                                                   const long long* __restrict__ table, int n_canvases,
                                                                   const int* __restrict__ cmds, int n_cmds,
                                                                   const short* __restrict__ bounds,
                                                                   const unsigned char* __restrict__ atlas, long long atlas_bytes) {
  __shared__ __attribute__((aligned(16))) int s_cmd[OV_CHUNK * OV_WORDS];
  __shared__ int s_hits[OV_RING];
  __shared__ int s_wave[OV_THREADS / 64];
  // the canvas this tile belongs to: the table is a few dozen entries, every thread walks it (uniform, scalar loads)
  const long long tile = blockIdx.x;
  OvCanvas cv;
  int tiles_x = 0;
  bool found = false;
  for (int ci = 0; ci < n_canvases && !found; ++ci) {
    cv = reinterpret_cast<const OvCanvas*>(table)[ci];
    if (!canvas_ok(cv, canvas_bytes, n_cmds)) continue;
    tiles_x = (int)((cv.w + OV_TILE - 1) / OV_TILE);
    const long long tiles = (long long)tiles_x * ((cv.h + OV_TILE - 1) / OV_TILE);
    found = tile >= cv.tile0 && tile - cv.tile0 < tiles;
  }
  if (!found || cv.count == 0) return;  // block-uniform
  const int h = (int)cv.h, w = (int)cv.w;
  const int local = (int)(tile - cv.tile0);
  const int tx0 = (local % tiles_x) * OV_TILE, ty0 = (local / tiles_x) * OV_TILE;
  const int tx1 = tx0 + OV_TILE - 1, ty1 = ty0 + OV_TILE - 1;
  const int px0 = tx0 + (threadIdx.x % (OV_TILE / OV_PX)) * OV_PX;
  const int py = ty0 + threadIdx.x / (OV_TILE / OV_PX);
  const bool row_in = py < h;
  // byte offset of the thread's first pixel in the canvas buffer: recomputed where it is used, not held over the command loop
  auto first_byte = [&]() { return cv.offset + ((long long)(row_in ? py : 0) * w + px0) * 3; };
  const int* ccmds = cmds + (size_t)cv.first * OV_WORDS;
  const short4* cbounds = reinterpret_cast<const short4*>(bounds) + cv.first;
  const int count = (int)cv.count, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int pix[OV_PX][3];
  unsigned layer[OV_PX] = {0, 0, 0, 0};
  bool loaded = false;
  int head = 0, tail = 0;  // ring positions (block-uniform, only ever grow)
  for (int base = 0; base < count; base += OV_THREADS) {
    {
      const int k = base + threadIdx.x;
      bool hit = false;
      if (k < count) {
        const short4 b = cbounds[k];
        hit = b.x <= b.z && b.x <= tx1 && b.z >= tx0 && b.y <= ty1 && b.w >= ty0;
      }
      const unsigned long long mask = __ballot(hit);
      if (lane == 0) s_wave[wv] = __popcll(mask);
      __syncthreads();
      int before = 0, all = 0;
#pragma unroll
      for (int v = 0; v < OV_THREADS / 64; ++v) {
        const int cnt = s_wave[v];
        before += v < wv ? cnt : 0;
        all += cnt;
      }
      if (hit) s_hits[(tail + before + __popcll(mask & ((1ull << lane) - 1ull))) & (OV_RING - 1)] = k;
      tail += all;
      __syncthreads();  // the hits are visible; s_wave may be rewritten by the next pass
    }
    const bool last = base + OV_THREADS >= count;
    while (tail - head >= OV_CHUNK || (last && head < tail)) {
      const int n_chunk = min(OV_CHUNK, tail - head);
      if (!loaded) {  // the first hit of this tile: only now is the canvas read
        loaded = true;
#pragma unroll
        for (int k = 0; k < OV_PX; ++k) {
          const bool in = row_in && px0 + k < w;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) pix[k][ch] = in ? (int)canvases[first_byte() + k * 3 + ch] : 0;
        }
      }
      __syncthreads();  // the previous chunk has been read by every thread
      {
        const int rec = threadIdx.x / 4, quarter = threadIdx.x % 4;
        if (rec < n_chunk) {
          const int id = s_hits[(head + rec) & (OV_RING - 1)];  // in [0, count) by construction
          reinterpret_cast<int4*>(s_cmd + rec * OV_WORDS)[quarter] = reinterpret_cast<const int4*>(ccmds + (size_t)id * OV_WORDS)[quarter];
        }
      }
      __syncthreads();
      overlay_apply(s_cmd, n_chunk, pix, layer, px0, py, atlas, atlas_bytes);
      head += n_chunk;
    }
  }
  if (!loaded || !row_in) return;  // a tile without hits has neither read nor written a canvas byte
#pragma unroll
  for (int k = 0; k < OV_PX; ++k) {
    if (px0 + k < w) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) canvases[first_byte() + k * 3 + ch] = (unsigned char)pix[k][ch];
    }
  }
}

__device__ __forceinline__ int quantise_prob(float p) {
  p = fminf(fmaxf(p, 0.f), 1.f);
  return (int)(unsigned char)(int)(p * 255.f);  // truncation, as ndarray.astype(np.uint8) of a value in [0, 255]
}

// fixed-point source coordinate of destination index d: (first tap, second tap, 10-bit fraction)
__device__ __forceinline__ void heat_taps(int d, int dn, int sn, int& i0, int& i1, int& f) {
  long long X = ((long long)(2 * d + 1) * sn * 1024) / (2LL * dn) - 512;
  const long long hi = (long long)(sn - 1) * 1024;
  X = X < 0 ? 0 : (X > hi ? hi : X);
  i0 = (int)(X >> 10);
  f = (int)(X & 1023);
  i1 = min(i0 + 1, sn - 1);
}

__global__ __launch_bounds__(256) void k_heatmap_blend(unsigned char* __restrict__ canvas, int h, int w,
                                                       const float* __restrict__ prob, int mh, int mw,
                                                       const unsigned char* __restrict__ jet) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= w || y >= h) return;
  int x0, x1, fx, y0, y1, fy;
  heat_taps(x, w, mw, x0, x1, fx);
  heat_taps(y, h, mh, y0, y1, fy);
  const int m00 = quantise_prob(prob[(size_t)y0 * mw + x0]), m01 = quantise_prob(prob[(size_t)y0 * mw + x1]);
  const int m10 = quantise_prob(prob[(size_t)y1 * mw + x0]), m11 = quantise_prob(prob[(size_t)y1 * mw + x1]);
  const int v = (m00 * (1024 - fx) * (1024 - fy) + m01 * fx * (1024 - fy) + m10 * (1024 - fx) * fy + m11 * fx * fy + (1 << 19)) >> 20;
  unsigned char* o = canvas + ((size_t)y * w + x) * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) o[ch] = (unsigned char)(((int)o[ch] + (int)jet[v * 3 + ch] + 1) >> 1);
}

}  // namespace ymk

extern "C" {
int ymk_overlay_tile(void) { return ymk::OV_TILE; }
int ymk_overlay_chunk(void) { return ymk::OV_CHUNK; }

int ymk_draw_overlay(unsigned char* canvas_dev, int h, int w, const int* cmds_dev, int n, const int* tile_offsets_dev,
                     const int* tile_cmds_dev, int n_list, const unsigned char* atlas_dev, int64_t atlas_bytes, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(canvas_dev && h > 0 && w > 0 && h <= 16383 && w <= 16383, "canvas: 1..16383 pixels on a side");
  YMK_CHECK(n >= 0 && n_list >= 0 && atlas_bytes >= 0, "bad argument");
  if (n == 0 || n_list == 0) return 0;
  YMK_CHECK(cmds_dev && tile_offsets_dev && tile_cmds_dev, "null command / list pointer");
  YMK_CHECK(atlas_dev || atlas_bytes == 0, "null atlas with a non-zero size");
  YMK_CHECK(((uintptr_t)cmds_dev & 15) == 0, "command records must be 16-byte aligned");
  const dim3 grid((w + ymk::OV_TILE - 1) / ymk::OV_TILE, (h + ymk::OV_TILE - 1) / ymk::OV_TILE);
  hipLaunchKernelGGL(ymk::k_draw_overlay, grid, dim3(ymk::OV_THREADS), 0, (hipStream_t)stream, canvas_dev, h, w, cmds_dev, n,
                     tile_offsets_dev, tile_cmds_dev, n_list, atlas_dev, (long long)atlas_bytes);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}

int ymk_overlay_cull_pass(void) { return ymk::OV_THREADS; }

int ymk_overlay_layout(int* cmds_dev, int n_cmds, int16_t* bounds_dev, const int* runs_dev, int n_runs, const int* codes_dev,
                       int n_codes, const int* glyphs_dev, int n_glyphs, const int64_t* canvases_dev, int n_canvases, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(n_cmds >= 0 && n_runs >= 0 && n_codes >= 0 && n_glyphs >= 0 && n_canvases >= 0 && n_canvases <= 65535, "bad argument");
  if (n_cmds == 0) return 0;
  YMK_CHECK(cmds_dev && bounds_dev, "null command / bounds pointer");
  YMK_CHECK(((uintptr_t)cmds_dev & 15) == 0 && ((uintptr_t)bounds_dev & 7) == 0 && ((uintptr_t)canvases_dev & 7) == 0,
            "command records must be 16-byte, bounds and the canvas table 8-byte aligned");
  if (n_runs > 0) {
    YMK_CHECK(runs_dev && (codes_dev || n_codes == 0) && (glyphs_dev || n_glyphs == 0), "null run / code / glyph pointer");
    hipLaunchKernelGGL(ymk::k_overlay_layout, dim3(n_runs), dim3(ymk::OV_SCAN), 0, (hipStream_t)stream, cmds_dev, n_cmds, runs_dev,
                       n_runs, codes_dev, n_codes, glyphs_dev, n_glyphs);
    YMK_HIP(hipGetLastError());
  }
  if (n_canvases > 0) {
    YMK_CHECK(canvases_dev, "null canvas table");
    const int gx = std::min(std::max((n_cmds + 255) / 256, 1), 256);
    hipLaunchKernelGGL(ymk::k_overlay_bounds, dim3(gx, n_canvases), dim3(256), 0, (hipStream_t)stream, cmds_dev, n_cmds,
                       (short*)bounds_dev, (const long long*)canvases_dev, n_canvases);
    YMK_HIP(hipGetLastError());
  }
  YMK_API_END
}

int ymk_draw_overlay_pages(unsigned char* canvases_dev, int64_t canvas_bytes, const int64_t* table_dev, int n_canvases,
                           int64_t total_tiles, const int* cmds_dev, int n_cmds, const int16_t* bounds_dev,
                           const unsigned char* atlas_dev, int64_t atlas_bytes, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(canvas_bytes >= 0 && n_canvases >= 0 && total_tiles >= 0 && total_tiles <= 0x7fffffffLL && n_cmds >= 0 &&
                atlas_bytes >= 0, "bad argument");
  if (n_canvases == 0 || total_tiles == 0 || n_cmds == 0) return 0;
  YMK_CHECK(canvases_dev && table_dev && cmds_dev && bounds_dev, "null canvas / table / command / bounds pointer");
  YMK_CHECK(atlas_dev || atlas_bytes == 0, "null atlas with a non-zero size");
  YMK_CHECK(((uintptr_t)cmds_dev & 15) == 0 && ((uintptr_t)bounds_dev & 7) == 0 && ((uintptr_t)table_dev & 7) == 0,
            "command records must be 16-byte, bounds and the canvas table 8-byte aligned");
  hipLaunchKernelGGL(ymk::k_draw_overlay_pages, dim3((unsigned)total_tiles), dim3(ymk::OV_THREADS), 0, (hipStream_t)stream,
                     canvases_dev, (long long)canvas_bytes, (const long long*)table_dev, n_canvases, cmds_dev, n_cmds,
                     (const short*)bounds_dev, atlas_dev, (long long)atlas_bytes);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}

int ymk_heatmap_blend(unsigned char* canvas_dev, int h, int w, const float* prob_dev, int mh, int mw, const unsigned char* jet_dev,
                      void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(canvas_dev && prob_dev && jet_dev, "null pointer");
  YMK_CHECK(h > 0 && w > 0 && h <= 16383 && w <= 16383 && mh > 0 && mw > 0 && mh <= 16383 && mw <= 16383,
            "canvas and map: 1..16383 on a side");
  hipLaunchKernelGGL(ymk::k_heatmap_blend, dim3((w + 255) / 256, h), dim3(256), 0, (hipStream_t)stream, canvas_dev, h, w, prob_dev,
                     mh, mw, jet_dev);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}
}
