// What the page-file kernels share (ymk_jpeg.hip, ymk_flate.hip, ymk_ccitt.hip, ymk_binarize.hip, ymk_cc.hip, ymk_mrc.hip,
// ymk_deskew.hip; DESIGN.md, "Page-file helpers"): the 64-bit reader of a page record, the host checks of a page table and of a
// scratch pointer, the wave and block scans, the search of the word-per-thread file writers, and the length-limited Huffman
// construction of the two coders that make their own tables.  One definition each; tests/test_page_kernels_source.py holds the
// files to it.  The page records, their readers and the *Limits structs are NOT here: they differ per file and stay there.
#pragma once
#include "ymk_common.h"

#include <algorithm>

namespace ymk {

// ------------------------------------------------------------------------------------------------ page records and tables
// words k, k + 1 of a record as one 64-bit value (a device pointer, or an offset that may exceed 2^31), low word first
__device__ __forceinline__ long long page_word64(const int* r, int k) {
  return (long long)(((unsigned long long)(unsigned)r[k + 1] << 32) | (unsigned long long)(unsigned)r[k]);
}

static inline void check_aligned8(const void* p, const char* what) { YMK_CHECK(p && ((uintptr_t)p & 7) == 0, what); }

// n_pages records of rec_words words at blob_dev: 0..max_pages of them, the table aligned to align_mask + 1 bytes and as long as
// it says.  The two messages are the caller's.
static inline void check_page_table(const int* blob_dev, int64_t blob_words, int n_pages, int rec_words, uintptr_t align_mask, int max_pages,
                                    const char* pages_msg, const char* table_msg) {
  YMK_CHECK(n_pages >= 0 && n_pages <= max_pages, pages_msg);
  YMK_CHECK(blob_dev && ((uintptr_t)blob_dev & align_mask) == 0 && blob_words >= (int64_t)n_pages * rec_words, table_msg);
}

// blocks per page of a kernel whose threads write a file's 32-bit words: four words per thread where the largest file has that
// many; 1024 blocks per page at the most (the loop strides the rest)
static inline unsigned file_word_grid(int64_t max_capacity, int threads) {
  const int64_t per_block = (int64_t)threads * 4 * 4;
  return (unsigned)std::min<int64_t>(std::max<int64_t>((max_capacity + per_block - 1) / per_block, 1), 1024);
}

// ------------------------------------------------------------------------------------------------ scans and the search
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o);
    v = t < v ? t : v;
  }
  return v;
}

__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}

// part[0 .. THREADS) in LDS, written by its threads and a barrier passed: the inclusive scan in place, by all THREADS threads
template <int THREADS>
__device__ __forceinline__ void block_inclusive_scan_u64(unsigned long long* part, int t) {
  for (int o = 1; o < THREADS; o <<= 1) {
    const unsigned long long add = t >= o ? part[t - o] : 0ull;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
}

// off[0 .. pieces): the pieces' first bits, ascending (a piece has at least one bit) and off[0] <= bit: the last piece whose first
// bit is at or before `bit`
__device__ __forceinline__ int last_piece_at_or_before(const unsigned long long* off, int pieces, unsigned long long bit) {
  int r = 0, hi = pieces - 1;
  while (r < hi) {
    const int mid = (r + hi + 1) >> 1;
    if (off[mid] <= bit) r = mid; else hi = mid - 1;
  }
  return r;
}

// ------------------------------------------------------------------------------------------------ Huffman code lengths
// libjpeg's construction (jpeg_gen_optimal_table) by the 64 lanes of one wave: up to 320 symbols, symbol k * 64 + lane in register
// k of its lane (`lane`: its number in the wave).  The caller fills freq (0: the symbol is not used) and says how many rounds there
// can be; every lane gets the same `rounds`.  A round merges the two rarest live symbols - two wave arg-min reductions, among
// equals the LARGEST symbol, as libjpeg's upward scan with <= finds it: the tie rule is in the key - into the rarer one's place; a
// subtree id per symbol stands for libjpeg's chain: both subtrees get one bit longer and are one subtree from here on.  Ends when
// one live symbol is left.
// len: every symbol's code length before limiting, 0 for a symbol that is not used (and for the only one used).  freq is consumed.
__device__ __forceinline__ void huff_merge_lengths(unsigned (&freq)[5], int (&len)[5], int rounds, int lane) {
  int id[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) len[k] = 0, id[k] = k * 64 + lane;
  constexpr unsigned long long NONE = ~0ull;
  for (int merge = 0; merge < rounds; ++merge) {
    unsigned long long k1 = NONE, k2 = NONE;
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (freq[k]) k1 = min(k1, (unsigned long long)freq[k] << 32 | (unsigned)(0xffff - (k * 64 + lane)));
    k1 = wave_min_u64(k1);
    const int c1 = 0xffff - (int)(k1 & 0xffff);
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (freq[k] && k * 64 + lane != c1) k2 = min(k2, (unsigned long long)freq[k] << 32 | (unsigned)(0xffff - (k * 64 + lane)));
    k2 = wave_min_u64(k2);
    if (k2 == NONE) break;  // the same in every lane
    const int c2 = 0xffff - (int)(k2 & 0xffff);
    const unsigned long long sum64 = (k1 >> 32) + (k2 >> 32);
    const unsigned sum = sum64 > 0xfffffffeull ? 0xfffffffeu : (unsigned)sum64;  // saturates on counts no page has: NONE stays free
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int s = k * 64 + lane;
      if (s == c1) freq[k] = sum;
      if (s == c2) freq[k] = 0;
      if (id[k] == c1 || id[k] == c2) ++len[k], id[k] = c1;
    }
  }
}

// Figure K.3 of the JPEG standard, by one lane: bits[l] = codes of length l, l = 1 .. longest; afterwards none is longer than limit
__device__ __forceinline__ void huff_limit_counts(int* bits, int longest, int limit) {
  for (int i = longest; i > limit; --i)
    while (bits[i] > 0) {
      int j = i - 2;
      while (j > 0 && bits[j] == 0) --j;
      if (j == 0) {  // not a tree's counts: not reached with lengths from huff_merge_lengths
        bits[i] = 0;
        break;
      }
      bits[i] -= 2, bits[i - 1] += 1, bits[j + 1] += 2, bits[j] -= 1;
    }
}

// the length of the symbol at place `rank` by (length before limiting, symbol); cum[l]: the symbols shorter than l, l = 1 .. limit + 1
__device__ __forceinline__ int huff_length_of_rank(const int* cum, int rank, int limit) {
  int l = 1;
  while (l < limit && rank >= cum[l + 1]) ++l;
  return l;
}

}  // namespace ymk
