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
static_assert(OV_CHUNK * OV_WORDS / 4 == OV_THREADS, "one int4 per thread stages a chunk");

__device__ __forceinline__ int blend_u8(int dst, int colour, int a) { return (colour * a + dst * (255 - a) + 127) / 255; }

// coverage (0..255; 0 = not covered) of command `c` at pixel (px, py)
__device__ __forceinline__ int overlay_alpha(const int* __restrict__ c, int px, int py, const unsigned char* __restrict__ atlas,
                                             long long atlas_bytes) {
  const int kind = c[0];
  if (kind == YMK_OVERLAY_SEG) {
    const long long x0 = c[5], y0 = c[6], x1 = c[7], y1 = c[8], t = c[9];
    const long long dx = x1 - x0, dy = y1 - y0, qx = px - x0, qy = py - y0;
    const long long l2 = dx * dx + dy * dy, u = qx * dx + qy * dy, t2 = t * t;
    bool in;
    if (l2 == 0 || u <= 0) {
      in = qx * qx + qy * qy <= t2 / 4;
    } else if (u >= l2) {
      const long long ex = px - x1, ey = py - y1;
      in = ex * ex + ey * ey <= t2 / 4;
    } else {
      const long long cr = qx * dy - qy * dx;  // |cr| < 2^32: cr * cr < 2^63 (|q|, |d| <= 32766 sqrt 2)
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
  return 0;
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
    for (int i = 0; i < count; ++i) {
      const int* c = s_cmd + i * OV_WORDS;  // the same address in every lane: an LDS broadcast
      const int cb = c[1], cg = c[2], cr = c[3];
#pragma unroll
      for (int k = 0; k < OV_PX; ++k) {
        const int a = overlay_alpha(c, px0 + k, py, atlas, atlas_bytes);
        if (a > 0) {
          pix[k][0] = blend_u8(pix[k][0], cb, a);
          pix[k][1] = blend_u8(pix[k][1], cg, a);
          pix[k][2] = blend_u8(pix[k][2], cr, a);
        }
      }
    }
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
  try {
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
    return 0;
  } catch (const std::exception& e) {
    ymk::set_error(e.what());
    return 1;
  }
}

int ymk_heatmap_blend(unsigned char* canvas_dev, int h, int w, const float* prob_dev, int mh, int mw, const unsigned char* jet_dev,
                      void* stream) {
  try {
    YMK_CHECK(canvas_dev && prob_dev && jet_dev, "null pointer");
    YMK_CHECK(h > 0 && w > 0 && h <= 16383 && w <= 16383 && mh > 0 && mw > 0 && mh <= 16383 && mw <= 16383,
              "canvas and map: 1..16383 on a side");
    hipLaunchKernelGGL(ymk::k_heatmap_blend, dim3((w + 255) / 256, h), dim3(256), 0, (hipStream_t)stream, canvas_dev, h, w, prob_dev,
                       mh, mw, jet_dev);
    YMK_HIP(hipGetLastError());
    return 0;
  } catch (const std::exception& e) {
    ymk::set_error(e.what());
    return 1;
  }
}
}
