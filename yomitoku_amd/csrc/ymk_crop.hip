// Rectangles cut from uint8 pages resident in HBM: the figure crops of DocumentAnalyzer.serve(figures=...) (yomitoku_amd/figures.py),
// which the JPEG encoder then takes as pages of their own.  DESIGN.md, "Figure crops"; tests/figures_ref.py is the definition.
//
//   k_crop_u8   one thread per 16-byte chunk of a crop's destination [ch][cw][C]; 256 threads a block, a 1-D grid over the
//               chunks of all crops of the launch.  A thread finds its record with the first-and-count search k_jpeg_coefficients
//               uses (ymk_jpeg.hip, jpeg_find): a record is first asked, from its first chunk and its size, whether the chunk
//               could be its own, and only then checked in full.  The chunks of a wave mostly belong to one crop: the wave asks
//               for the records of its first and of its last chunk with a wave-uniform index (scalar loads), and only where the
//               two differ does every lane search for itself.
//               A chunk that lies inside one source row and inside the crop is 16 contiguous source bytes at any address `a`:
//                 a % 16 == 0   one 16-byte load;
//                 a %  4 == 0   four dword loads;
//                 otherwise     the five aligned dwords that cover it and a byte-align (v_alignbyte_b32) per output dword -
//                               where those five lie inside [source, source + H W C); a chunk at the very start or end of a page
//                               that is an unaligned view takes byte loads instead: no load leaves the page.
//               It goes out as one 16-byte store.  A chunk that straddles source rows (with cw C < 16: several) gathers its
//               bytes one by one, each from its own row, and is stored the same way; the crop's last chunk, where ch cw C is no
//               multiple of 16, stores its bytes one by one: nothing is written behind the crop.
//
// A record that does not fit is no crop (never trusted): nothing is read or written for it.  Nothing is allocated and nothing
// waited for; no atomics; no thread waits for another.
#include "ymk_common.h"

#include "../../include/ymk.h"

namespace ymk {

constexpr int CR_REC = YMK_CROP_U8_WORDS;
constexpr int CR_THREADS = 256;

struct Crop {
  const unsigned char* src;
  unsigned char* dst;
  int w, c, x0, y0, row_bytes;        // row_bytes = cw * C
  long long src_bytes, bytes, first;  // H W C; ch cw C; word 11
};
// the chunks of a crop of cw x ch pixels of c channels, from words not yet checked (a record that is no crop may answer anything)
__device__ __forceinline__ long long crop_chunks(unsigned cw, unsigned ch, unsigned c) {
  return (long long)(((unsigned long long)cw * ch * c + 15) >> 4);
}
// Record p, checked: a record that does not fit is no crop.
__device__ __forceinline__ bool crop_record(const int* __restrict__ blob, long long total_chunks, int p, Crop& g) {
  const int* r = blob + (size_t)p * CR_REC;
  const unsigned long long src = ((unsigned long long)(unsigned)r[1] << 32) | (unsigned)r[0];
  const unsigned long long dst = ((unsigned long long)(unsigned)r[10] << 32) | (unsigned)r[9];
  const int H = r[2], W = r[3], C = r[4], x0 = r[5], y0 = r[6], cw = r[7], ch = r[8];
  if (src == 0 || dst == 0 || (dst & 15) != 0) return false;
  if (H < 1 || W < 1 || H > 16383 || W > 16383 || (C != 1 && C != 3)) return false;
  if (cw < 1 || ch < 1 || cw > 16383 || ch > 16383 || x0 < 0 || y0 < 0 || x0 > W - cw || y0 > H - ch) return false;
  g.src = reinterpret_cast<const unsigned char*>(src), g.dst = reinterpret_cast<unsigned char*>(dst);
  g.w = W, g.c = C, g.x0 = x0, g.y0 = y0, g.row_bytes = cw * C;
  g.src_bytes = (long long)H * W * C, g.bytes = (long long)ch * cw * C, g.first = r[11];
  return g.first >= 0 && g.first + ((g.bytes + 15) >> 4) <= total_chunks;
}
// The crop whose destination has chunk `idx` of the launch, or -1: the first record that has the index and is a crop.
__device__ __forceinline__ int crop_find(const int* __restrict__ blob, long long total_chunks, int n, long long idx, Crop& g) {
  for (int p = 0; p < n; ++p) {
    const int* r = blob + (size_t)p * CR_REC;
    const long long first = r[11];
    if (idx < first || idx >= first + crop_chunks((unsigned)r[7], (unsigned)r[8], (unsigned)r[4])) continue;
    if (crop_record(blob, total_chunks, p, g)) return p;
  }
  return -1;
}

// byte `d` of the crop's destination: where it lies in the page
__device__ __forceinline__ long long crop_source(const Crop& g, long long d) {
  const long long row = d / g.row_bytes;
  return ((g.y0 + row) * g.w + g.x0) * g.c + (d - row * g.row_bytes);
}

__global__ __launch_bounds__(CR_THREADS) void k_crop_u8(const int* __restrict__ blob, int n, long long total_chunks) {
  const long long idx = (long long)blockIdx.x * CR_THREADS + threadIdx.x;
  // the wave's first and last chunk: the same in all its lanes, so these two searches are scalar work
  const long long lo = (long long)blockIdx.x * CR_THREADS + __builtin_amdgcn_readfirstlane(threadIdx.x & ~63);
  if (lo >= total_chunks) return;
  const long long hi = min(lo + 63, total_chunks - 1);
  Crop g, g_hi;
  int p = crop_find(blob, total_chunks, n, lo, g);
  const int p_hi = crop_find(blob, total_chunks, n, hi, g_hi);
  if (idx >= total_chunks) return;
  if (p != p_hi || p < 0) p = crop_find(blob, total_chunks, n, idx, g);  // more than one crop in the wave: each lane for itself
  if (p < 0) return;
  const long long d0 = (idx - g.first) * 16;  // the chunk's first byte in the destination
  if (d0 < 0 || d0 >= g.bytes) return;       // p was the wave's and this chunk is not of it: records that overlap are no crops
  const int count = (int)min(16LL, g.bytes - d0);
  const long long row = d0 / g.row_bytes;
  const int col = (int)(d0 - row * g.row_bytes);
  const long long s0 = ((g.y0 + row) * g.w + g.x0) * g.c + col;  // the first byte's place in the page
  unsigned v[4];
  if (count == 16 && col + 16 <= g.row_bytes) {
    const unsigned char* a = g.src + s0;
    const unsigned long long addr = reinterpret_cast<unsigned long long>(a);
    const unsigned sh = (unsigned)(addr & 3);
    if ((addr & 15) == 0) {
      const uint4 q = *reinterpret_cast<const uint4*>(a);
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else if (sh == 0) {
      const unsigned* q = reinterpret_cast<const unsigned*>(a);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = q[i];
    } else if (s0 >= (long long)sh && s0 - sh + 20 <= g.src_bytes) {
      const unsigned* q = reinterpret_cast<const unsigned*>(a - sh);
      unsigned t[5];
#pragma unroll
      for (int i = 0; i < 5; ++i) t[i] = q[i];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = __builtin_amdgcn_alignbyte(t[i + 1], t[i], sh);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = (unsigned)a[4 * i] | (unsigned)a[4 * i + 1] << 8 | (unsigned)a[4 * i + 2] << 16 | (unsigned)a[4 * i + 3] << 24;
    }
    *reinterpret_cast<uint4*>(g.dst + d0) = make_uint4(v[0], v[1], v[2], v[3]);
    return;
  }
  if (count == 16) {  // a whole chunk across source rows: every byte from its own row
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = 0;
    int c = col;
    long long s = s0;
    const long long skip = (long long)g.w * g.c - g.row_bytes;  // from the end of a crop's row to the start of its next
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      v[j >> 2] |= (unsigned)g.src[s] << (8 * (j & 3));
      ++s;
      if (++c == g.row_bytes) c = 0, s += skip;
    }
    *reinterpret_cast<uint4*>(g.dst + d0) = make_uint4(v[0], v[1], v[2], v[3]);
    return;
  }
  for (int j = 0; j < count; ++j) g.dst[d0 + j] = g.src[crop_source(g, d0 + j)];  // the crop's last chunk: its bytes and no more
}

}  // namespace ymk

extern "C" {

int ymk_crop_u8_record_words(void) { return ymk::CR_REC; }

int ymk_crop_u8(const int* blob_dev, int64_t blob_words, int n, int64_t total_chunks, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(n >= 0 && n <= 65535 && blob_words >= 0 && total_chunks >= 0, "bad argument");
  YMK_CHECK(total_chunks <= 0x7fffffffLL * ymk::CR_THREADS, "at most (2^31 - 1) * 256 chunks per launch");
  if (n == 0 || total_chunks == 0) return 0;
  YMK_CHECK(blob_dev && ((uintptr_t)blob_dev & 3) == 0 && blob_words >= (int64_t)n * ymk::CR_REC, "record table");
  const unsigned grid = (unsigned)((total_chunks + ymk::CR_THREADS - 1) / ymk::CR_THREADS);
  hipLaunchKernelGGL(ymk::k_crop_u8, dim3(grid), dim3(ymk::CR_THREADS), 0, (hipStream_t)stream, blob_dev, n, (long long)total_chunks);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}
}
