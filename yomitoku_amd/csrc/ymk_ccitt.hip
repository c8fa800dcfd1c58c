// CCITT Group 4 (ITU-T T.6) files of the two-valued pages of a wave (include/ymk.h, "Group 4 encoder"; yomitoku_amd/ccitt.py;
// DESIGN.md, "Two-valued pages").  tests/ccitt_ref.py is the definition; every stage equals it bit for bit.
//
//   k_g4_test_pack   per candidate page: is every sample 0 or 255 (and B == G == R)?  - an OR into the page's flag, as
//                    k_jpeg_pages_grey does - and, in the same pass, the page's rows as packed bits (1 = black, the leftmost
//                    pixel of a word in bit 31, rows padded to 32-bit words).  One wave per 64 pixels of a row: a ballot.
//   k_g4_rows        one THREAD per row of every page: the T.6 loop walks a0 along the row in sequence - the parallelism is
//                    across the thousands of rows of a wave of pages - against the packed row above (the SOURCE's row, so rows
//                    are independent), finding changing elements with bit scans on the packed words.  A block stages eight
//                    rows, the row above them and the code table in LDS first.  The codes go MSB first into the row's own
//                    slot of g4_slot_words(w) words, the row's bit count into rowbits.
//   k_g4_scan        one block per page: exclusive prefix sum of the page's bit counts -> each row's bit offset in the file,
//                    the file's length in bytes (rows + EOFB, padded to a byte), -1 where it exceeds the page's capacity.
//   k_g4_concat      gather, one thread per 32-bit word of a file: a binary search for the row that holds the word's first bit,
//                    then the bits of that row and of the rows behind it until the word is full; past the last row EOFB, then
//                    zeros.  Every word of a file is written exactly once by exactly one thread: no atomics, no cleared buffer.
//
// The slot bound.  A row of w pixels takes at most 7 w + 21 bits, so a slot has ceil((7 w + 32) / 32) words.  Proof: count the
// bits of a step of the row loop against the pixels a0 advances by (from a0 = -1 the advance is counted from column 0).
//   pass        4 bits; a0 -> b2 > b1 > a0: at least 2 pixels (1 from a0 = -1).
//   vertical    at most 7 bits; a0 -> a1 > a0: at least 1 pixel, except a1 = 0 from a0 = -1 (at most once a row: 7 extra bits).
//   horizontal  3 + T(r1) + T'(r2) bits for r1 + r2 pixels, T / T' the run codes of the two colours.  For runs of at least one
//               pixel T_white(r) <= 6 r (000111 for r = 1; 8 bits at most below 64; one make-up code of at most 9 bits per 64
//               pixels and one 12-bit code per 2560 beyond) and 3 + T_black(r) <= 6 r (3 + 3 for r = 1, 3 + 2 for r = 2, at
//               most 3 + 12 from r = 3 on, make-up codes of at most 13 bits per 64 pixels): at most 6 bits a pixel.  A run of 0
//               occurs only as the first run of a row (white, 8 bits: first pixel black) and as the last (a run to the row's
//               end is followed by the other colour's run of 0: 10 bits for black, 8 for white) - at most 8 and, with the 3
//               mode bits no black run absorbs, 13 extra bits.
// Every step costs at most 7 bits per pixel advanced, the steps' advances add up to w, and the extras to at most 8 + 13 (a
// first step is either vertical or horizontal).  tests/test_ccitt_host.py checks the bound exhaustively for narrow rows.
// k_g4_rows nevertheless never writes beyond a slot: a row that did not fit would be marked and its page get -1.

#include "ymk_pages.h"

#include "../../include/ymk.h"

namespace ymk {

constexpr int G4_REC = YMK_G4_PAGE_WORDS;
constexpr int G4_MAX_SIDE = 16383;
constexpr unsigned G4_OVERFLOW = 0xffffffffu;  // rowbits of a row that did not fit its slot

__host__ __device__ inline int g4_slot_words(int w) { return (7 * w + 32 + 31) >> 5; }

struct G4Limits {
  long long total_rows, packed_words, slot_words, out_bytes;
};

// (bits << 16 | code) of every code, one table so that a block can stage it in LDS: the terminating codes (index = run length)
// and the make-up codes (index = run length / 64 - 1) of white, then of black, the make-up codes 1792 ... 2560 of both colours,
// the vertical codes for a1 - b1 = -3 ... 3 (VL3 VL2 VL1 V0 VR1 VR2 VR3)
#define G4C(bits, code) ((unsigned)(bits) << 16 | (unsigned)(code))
constexpr int G4_WHITE_TERM = 0, G4_WHITE_MAKEUP = 64, G4_BLACK_TERM = 91, G4_BLACK_MAKEUP = 155, G4_EXT_MAKEUP = 182, G4_VERTICAL = 195,
              G4_TABLE_WORDS = 202;
__device__ const unsigned G4_TABLE[G4_TABLE_WORDS] = {
    // white, terminating
    G4C(8, 0x35), G4C(6, 0x07), G4C(4, 0x7), G4C(4, 0x8), G4C(4, 0xB), G4C(4, 0xC), G4C(4, 0xE), G4C(4, 0xF), G4C(5, 0x13),
    G4C(5, 0x14), G4C(5, 0x07), G4C(5, 0x08), G4C(6, 0x08), G4C(6, 0x03), G4C(6, 0x34), G4C(6, 0x35), G4C(6, 0x2A), G4C(6,
    0x2B), G4C(7, 0x27), G4C(7, 0x0C), G4C(7, 0x08), G4C(7, 0x17), G4C(7, 0x03), G4C(7, 0x04), G4C(7, 0x28), G4C(7, 0x2B),
    G4C(7, 0x13), G4C(7, 0x24), G4C(7, 0x18), G4C(8, 0x02), G4C(8, 0x03), G4C(8, 0x1A), G4C(8, 0x1B), G4C(8, 0x12), G4C(8,
    0x13), G4C(8, 0x14), G4C(8, 0x15), G4C(8, 0x16), G4C(8, 0x17), G4C(8, 0x28), G4C(8, 0x29), G4C(8, 0x2A), G4C(8, 0x2B),
    G4C(8, 0x2C), G4C(8, 0x2D), G4C(8, 0x04), G4C(8, 0x05), G4C(8, 0x0A), G4C(8, 0x0B), G4C(8, 0x52), G4C(8, 0x53), G4C(8,
    0x54), G4C(8, 0x55), G4C(8, 0x24), G4C(8, 0x25), G4C(8, 0x58), G4C(8, 0x59), G4C(8, 0x5A), G4C(8, 0x5B), G4C(8, 0x4A),
    G4C(8, 0x4B), G4C(8, 0x32), G4C(8, 0x33), G4C(8, 0x34),
    // white, make-up
    G4C(5, 0x1B), G4C(5, 0x12), G4C(6, 0x17), G4C(7, 0x37), G4C(8, 0x36), G4C(8, 0x37), G4C(8, 0x64), G4C(8, 0x65), G4C(8,
    0x68), G4C(8, 0x67), G4C(9, 0xCC), G4C(9, 0xCD), G4C(9, 0xD2), G4C(9, 0xD3), G4C(9, 0xD4), G4C(9, 0xD5), G4C(9, 0xD6),
    G4C(9, 0xD7), G4C(9, 0xD8), G4C(9, 0xD9), G4C(9, 0xDA), G4C(9, 0xDB), G4C(9, 0x98), G4C(9, 0x99), G4C(9, 0x9A), G4C(6,
    0x18), G4C(9, 0x9B),
    // black, terminating
    G4C(10, 0x37), G4C(3, 0x2), G4C(2, 0x3), G4C(2, 0x2), G4C(3, 0x3), G4C(4, 0x3), G4C(4, 0x2), G4C(5, 0x03), G4C(6, 0x05),
    G4C(6, 0x04), G4C(7, 0x04), G4C(7, 0x05), G4C(7, 0x07), G4C(8, 0x04), G4C(8, 0x07), G4C(9, 0x18), G4C(10, 0x17), G4C(10,
    0x18), G4C(10, 0x08), G4C(11, 0x67), G4C(11, 0x68), G4C(11, 0x6C), G4C(11, 0x37), G4C(11, 0x28), G4C(11, 0x17), G4C(11,
    0x18), G4C(12, 0xCA), G4C(12, 0xCB), G4C(12, 0xCC), G4C(12, 0xCD), G4C(12, 0x68), G4C(12, 0x69), G4C(12, 0x6A), G4C(12,
    0x6B), G4C(12, 0xD2), G4C(12, 0xD3), G4C(12, 0xD4), G4C(12, 0xD5), G4C(12, 0xD6), G4C(12, 0xD7), G4C(12, 0x6C), G4C(12,
    0x6D), G4C(12, 0xDA), G4C(12, 0xDB), G4C(12, 0x54), G4C(12, 0x55), G4C(12, 0x56), G4C(12, 0x57), G4C(12, 0x64), G4C(12,
    0x65), G4C(12, 0x52), G4C(12, 0x53), G4C(12, 0x24), G4C(12, 0x37), G4C(12, 0x38), G4C(12, 0x27), G4C(12, 0x28), G4C(12,
    0x58), G4C(12, 0x59), G4C(12, 0x2B), G4C(12, 0x2C), G4C(12, 0x5A), G4C(12, 0x66), G4C(12, 0x67),
    // black, make-up
    G4C(10, 0x0F), G4C(12, 0xC8), G4C(12, 0xC9), G4C(12, 0x5B), G4C(12, 0x33), G4C(12, 0x34), G4C(12, 0x35), G4C(13, 0x6C),
    G4C(13, 0x6D), G4C(13, 0x4A), G4C(13, 0x4B), G4C(13, 0x4C), G4C(13, 0x4D), G4C(13, 0x72), G4C(13, 0x73), G4C(13, 0x74),
    G4C(13, 0x75), G4C(13, 0x76), G4C(13, 0x77), G4C(13, 0x52), G4C(13, 0x53), G4C(13, 0x54), G4C(13, 0x55), G4C(13, 0x5A),
    G4C(13, 0x5B), G4C(13, 0x64), G4C(13, 0x65),
    // both colours, 1792 ... 2560
    G4C(11, 0x08), G4C(11, 0x0C), G4C(11, 0x0D), G4C(12, 0x12), G4C(12, 0x13), G4C(12, 0x14), G4C(12, 0x15), G4C(12, 0x16),
    G4C(12, 0x17), G4C(12, 0x1C), G4C(12, 0x1D), G4C(12, 0x1E), G4C(12, 0x1F),
    // vertical
    G4C(7, 2), G4C(6, 2), G4C(3, 2), G4C(1, 1), G4C(3, 3), G4C(6, 3), G4C(7, 3)};
constexpr unsigned G4_PASS = G4C(4, 1), G4_HORIZONTAL = G4C(3, 1);
constexpr unsigned G4_EOFB_TOP = 0x00100100u;  // 000000000001 twice, in the upper 24 bits of a word

// A page's record, read and checked against the buffers' sizes: every kernel takes a page whose record fails as absent, so no
// record, whatever it says, makes a kernel touch memory outside the buffers the caller named.
struct G4Page {
  const unsigned char* src;
  int h, w, ch, first_row, row_words, slot_row_words, capacity;
  long long packed_at, out_at, slot_at;
  bool ok;
};
__device__ __forceinline__ G4Page g4_page(const int* blob, int p, const G4Limits& lim) {
  const int* r = blob + (size_t)p * G4_REC;
  G4Page g;
  g.src = reinterpret_cast<const unsigned char*>((unsigned long long)page_word64(r, 0));
  g.h = r[2], g.w = r[3], g.ch = r[4], g.first_row = r[5];
  g.packed_at = page_word64(r, 6), g.out_at = page_word64(r, 8), g.capacity = r[10], g.slot_at = page_word64(r, 11);
  g.ok = g.h >= 1 && g.w >= 1 && g.h <= G4_MAX_SIDE && g.w <= G4_MAX_SIDE;
  g.row_words = g.ok ? (g.w + 31) >> 5 : 0;
  g.slot_row_words = g.ok ? g4_slot_words(g.w) : 0;
  g.ok = g.ok && g.packed_at >= 0 && g.packed_at + (long long)g.h * g.row_words <= lim.packed_words;
  return g;
}
// what the stages behind the test need on top: rows, slots and the file's place
__device__ __forceinline__ bool g4_coded_ok(const G4Page& g, const G4Limits& lim) {
  return g.ok && g.first_row >= 0 && (long long)g.first_row + g.h <= lim.total_rows && g.slot_at >= 0 &&
         g.slot_at + (long long)g.h * g.slot_row_words <= lim.slot_words && g.capacity >= 0 && g.out_at >= 0 && (g.out_at & 3) == 0 &&
         g.out_at + (((long long)g.capacity + 3) & ~3LL) <= lim.out_bytes;
}

// ------------------------------------------------------------------------------------------------ test and pack
constexpr int TP_THREADS = 256;
// flags[p] |= 1 where page p has a sample that is neither 0 nor 255, or a pixel with B != G or G != R; -1 for a record that is
// no page.  flags is zero before the launch.  packed: the page's rows as bits whether it qualifies or not (a page that does not
// is never coded).  A wave takes 64 pixels of a row at a time; its lanes' answers are the two words of a ballot, bit-reversed.
__global__ __launch_bounds__(TP_THREADS) void k_g4_test_pack(const int* __restrict__ blob, G4Limits lim, int* __restrict__ flags,
                                                             unsigned* __restrict__ packed) {
  const int p = blockIdx.y;
  const G4Page g = g4_page(blob, p, lim);
  if (!g.ok || g.src == nullptr || (g.ch != 1 && g.ch != 3)) {  // the whole block
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(flags + p, -1);
    return;
  }
  const int lane = threadIdx.x & 63, chunks = (g.w + 63) >> 6;
  const long long units = (long long)g.h * chunks, waves = (long long)gridDim.x * (TP_THREADS / 64);
  unsigned bad = 0;
  for (long long u = (long long)blockIdx.x * (TP_THREADS / 64) + (threadIdx.x >> 6); u < units; u += waves) {  // uniform in a wave
    const int y = (int)(u / chunks), c = (int)(u - (long long)y * chunks), x = c * 64 + lane;
    bool black = false;
    if (x < g.w) {
      const unsigned char* px = g.src + ((size_t)y * g.w + x) * g.ch;
      const unsigned v = px[0];
      if (g.ch == 3) {
        const unsigned gg = px[1], rr = px[2];
        bad |= (v ^ gg) | (gg ^ rr);
      }
      bad |= (v + 1u) & 0xfeu;  // 0 -> 1, 255 -> 256: nothing left; every other value leaves a bit
      black = v == 0;
    }
    const unsigned long long m = __ballot(black);
    unsigned* row = packed + g.packed_at + (long long)y * g.row_words;
    if (lane == 0) row[2 * c] = __brev((unsigned)m);
    if (lane == 1 && 2 * c + 1 < g.row_words) row[2 * c + 1] = __brev((unsigned)(m >> 32));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o);
  if (lane == 0 && bad) atomicOr(flags + p, 1);
}

// ------------------------------------------------------------------------------------------------ row coding
constexpr int RC_THREADS = 64, RC_ROWS = 8, RC_MAX_ROW_WORDS = (G4_MAX_SIDE + 31) / 32;

// the first column >= start whose bit, XORed with flip's, is set; w where there is none.  The padding behind column w is 0.
__device__ __forceinline__ int g4_next(const unsigned* q, int w, int start, unsigned flip) {
  if (start >= w) return w;
  const int nw = (w + 31) >> 5;
  int i = start >> 5;
  unsigned v = (q[i] ^ flip) & (0xffffffffu >> (start & 31));
  while (v == 0) {
    if (++i >= nw) return w;
    v = q[i] ^ flip;
  }
  return min((i << 5) + __clz((int)v), w);
}
// b1: the first column >= start of the reference row that differs from `colour` (cmask = all ones for black) while the column
// before it does not - a change to the opposite colour; the column before column 0 is white.  w where there is none.
__device__ __forceinline__ int g4_next_b1(const unsigned* q, int w, int start, unsigned cmask) {
  if (start >= w) return w;
  const int nw = (w + 31) >> 5;
  int i = start >> 5;
  unsigned prev = i ? q[i - 1] ^ cmask : cmask;  // its lowest bit: does the column before this word differ from colour
  unsigned v = q[i] ^ cmask;
  unsigned c = v & ~((v >> 1) | (prev << 31)) & (0xffffffffu >> (start & 31));
  while (c == 0) {
    if (++i >= nw) return w;
    prev = v;
    v = q[i] ^ cmask;
    c = v & ~((v >> 1) | (prev << 31));
  }
  return min((i << 5) + __clz((int)c), w);
}

struct G4Bits {
  const unsigned* tab;  // G4_TABLE, staged
  unsigned* out;
  int cap, pos;  // words of the slot, words written (pos may pass cap: nothing is stored beyond it)
  unsigned long long acc;
  int held;  // bits of acc not yet stored (< 32 between calls)
  unsigned total;
  __device__ __forceinline__ void put(unsigned entry) {  // bits << 16 | code, at most 13 bits
    const int n = (int)(entry >> 16);
    acc = (acc << n) | (entry & 0xffffu);
    held += n;
    total += (unsigned)n;
    if (held >= 32) {
      held -= 32;
      if (pos < cap) out[pos] = (unsigned)(acc >> held);
      ++pos;
    }
  }
  __device__ __forceinline__ void run(int n, bool black) {
    while (n >= 2624) {
      put(tab[G4_EXT_MAKEUP + 12]);
      n -= 2560;
    }
    if (n >= 64) {
      const int k = n >> 6;  // 1 ... 40
      put(tab[k <= 27 ? (black ? G4_BLACK_MAKEUP : G4_WHITE_MAKEUP) + k - 1 : G4_EXT_MAKEUP + k - 28]);
      n &= 63;
    }
    put(tab[(black ? G4_BLACK_TERM : G4_WHITE_TERM) + n]);
  }
  __device__ __forceinline__ void finish() {  // the last word, zero bits behind the row's
    if (held > 0) {
      if (pos < cap) out[pos] = (unsigned)(acc << (32 - held));
      ++pos;
    }
  }
};

// The row `cur` of w pixels against the row `ref` (both packed, (w + 31) / 32 words) into `out`, a slot of `cap` words; returns
// the row's bit count, G4_OVERFLOW where the slot was too small (nothing is written beyond it).
__device__ __forceinline__ unsigned g4_code_row(const unsigned* cur, const unsigned* ref, int w, const unsigned* tab, unsigned* out, int cap) {
  G4Bits bits{tab, out, cap, 0, 0ull, 0, 0u};
  int a0 = -1;
  unsigned cmask = 0;  // a0's colour: 0 white, all ones black
  while (a0 < w) {     // a0 grows with every step: at most w + 1 steps
    const int a1 = g4_next(cur, w, a0 + 1, cmask);
    const int b1 = g4_next_b1(ref, w, a0 + 1, cmask);
    const int b2 = g4_next(ref, w, b1 + 1, ~cmask);
    if (b2 < a1) {
      bits.put(G4_PASS);
      a0 = b2;
    } else if (abs(a1 - b1) <= 3) {
      bits.put(tab[G4_VERTICAL + a1 - b1 + 3]);
      a0 = a1;
      cmask = ~cmask;
    } else {
      const int a2 = g4_next(cur, w, a1 + 1, ~cmask);
      bits.put(G4_HORIZONTAL);
      bits.run(a1 - max(a0, 0), cmask != 0);
      bits.run(a2 - a1, cmask == 0);
      a0 = a2;
    }
  }
  bits.finish();
  return bits.pos <= bits.cap ? bits.total : G4_OVERFLOW;
}

// Block (x, p) codes the rows RC_ROWS x ... RC_ROWS x + RC_ROWS - 1 of page p.  The row loop is a chain of dependent reads - a
// word of the coding row, two or three of the reference row, a code - so the block first stages its rows, the row above them
// (zeros above row 0) and the code table in LDS, all 64 lanes loading; then lane r walks row r.  Few rows per block: the lanes of
// a wave take the three modes' branches in turn, and the launch ends with its slowest row, so thousands of short waves fill the
// chip where hundreds of long ones leave most of it idle.  Measured on a wave of 16 thresholded 1600 x 1200 pages (25 600 rows,
// about 360 bits a row): from global memory, one row per lane, 1.76 ms at 64 rows per block, 1.24 at 8, 1.14 at 2; from LDS
// 0.83 / 0.89 / 1.13 / 1.27 ms at 4 / 8 / 16 / 24.
__global__ __launch_bounds__(RC_THREADS) void k_g4_rows(const int* __restrict__ blob, G4Limits lim, const unsigned* __restrict__ packed,
                                                        unsigned* __restrict__ slots, unsigned* __restrict__ rowbits) {
  __shared__ unsigned tab[G4_TABLE_WORDS];
  __shared__ unsigned rows[(RC_ROWS + 1) * RC_MAX_ROW_WORDS];
  const int p = blockIdx.y, t = threadIdx.x;
  const G4Page g = g4_page(blob, p, lim);
  const int y0 = blockIdx.x * RC_ROWS;
  if (!g4_coded_ok(g, lim) || y0 >= g.h) return;  // the whole block; k_g4_scan gives a page whose record fails its -1
  const int n = min(RC_ROWS, g.h - y0), rw = g.row_words;
  for (int i = t; i < G4_TABLE_WORDS; i += RC_THREADS) tab[i] = G4_TABLE[i];
  for (int i = t; i < (n + 1) * rw; i += RC_THREADS) {
    const int r = i / rw, y = y0 - 1 + r;
    rows[i] = y < 0 ? 0u : packed[g.packed_at + (long long)y * rw + (i - r * rw)];
  }
  __syncthreads();
  if (t < n)
    rowbits[g.first_row + y0 + t] = g4_code_row(rows + (t + 1) * rw, rows + t * rw, g.w, tab, slots + g.slot_at + (long long)(y0 + t) * g.slot_row_words,
                                                g.slot_row_words);
}

// ------------------------------------------------------------------------------------------------ scan
constexpr int SC_THREADS = 256;
// rowoff: per page h + 1 offsets, page p's at first_row + p: offset of every row's first bit in the file, then the rows' total.
__global__ __launch_bounds__(SC_THREADS) void k_g4_scan(const int* __restrict__ blob, G4Limits lim, const unsigned* __restrict__ rowbits,
                                                        unsigned long long* __restrict__ rowoff, int* __restrict__ lengths) {
  __shared__ unsigned long long part[SC_THREADS];
  const int p = blockIdx.x, t = threadIdx.x;
  const G4Page g = g4_page(blob, p, lim);
  if (!g4_coded_ok(g, lim)) {  // the whole block
    if (t == 0) lengths[p] = -1;
    return;
  }
  const int per = (g.h + SC_THREADS - 1) / SC_THREADS, lo = min(t * per, g.h), hi = min(lo + per, g.h);
  const unsigned most = (unsigned)g.slot_row_words * 32u;
  unsigned long long sum = 0;
  int bad = 0;
  for (int y = lo; y < hi; ++y) {
    const unsigned b = rowbits[g.first_row + y];
    bad |= b == 0 || b > most;
    sum += b;
  }
  part[t] = sum;
  __syncthreads();
  block_inclusive_scan_u64<SC_THREADS>(part, t);  // of the threads' sums
  bad = __syncthreads_or(bad);
  unsigned long long at = part[t] - sum;
  unsigned long long* off = rowoff + g.first_row + p;
  for (int y = lo; y < hi; ++y) {
    off[y] = at;
    at += rowbits[g.first_row + y];
  }
  if (t == SC_THREADS - 1) {
    const unsigned long long total = part[t], bytes = (total + 24 + 7) >> 3;
    off[g.h] = total;
    lengths[p] = (!bad && bytes <= (unsigned long long)g.capacity) ? (int)bytes : -1;
  }
}

// ------------------------------------------------------------------------------------------------ concatenate
constexpr int CC_THREADS = 256;
__global__ __launch_bounds__(CC_THREADS) void k_g4_concat(const int* __restrict__ blob, G4Limits lim, const unsigned* __restrict__ slots,
                                                          const unsigned long long* __restrict__ rowoff, const int* __restrict__ lengths,
                                                          unsigned char* __restrict__ out) {
  const int p = blockIdx.y;
  const int len = lengths[p];
  if (len < 0) return;
  const G4Page g = g4_page(blob, p, lim);
  if (!g4_coded_ok(g, lim) || len > g.capacity) return;
  const unsigned long long* off = rowoff + g.first_row + p;
  const unsigned long long total = off[g.h];
  const int words = (len + 3) >> 2;  // the bytes of the last word behind the file's end lie within the capacity rounded up to 4
  unsigned* file = reinterpret_cast<unsigned*>(out + g.out_at);
  for (int k = blockIdx.x * CC_THREADS + threadIdx.x; k < words; k += gridDim.x * CC_THREADS) {
    const unsigned long long bit = 32ull * (unsigned)k;
    unsigned acc = 0;
    int filled = 0;
    if (bit < total) {
      int r = last_piece_at_or_before(off, g.h, bit);  // a row is a piece
      int s = (int)(bit - off[r]);
      while (filled < 32 && r < g.h) {
        const int nb = (int)(off[r + 1] - off[r]), take = min(32 - filled, nb - s);
        const unsigned* slot = slots + g.slot_at + (long long)r * g.slot_row_words;
        const int i = s >> 5, sh = s & 31;
        unsigned v = slot[i] << sh;
        if (sh + take > 32) v |= slot[i + 1] >> (32 - sh);
        if (take < 32) v &= ~(0xffffffffu >> take);
        acc |= v >> filled;
        filled += take;
        ++r;
        s = 0;
      }
    }
    if (filled < 32) {  // behind the last row: EOFB, then zeros
      const unsigned long long e = bit + (unsigned)filled - total;
      if (e < 24) acc |= (G4_EOFB_TOP << (int)e) >> filled;
    }
    file[k] = __builtin_bswap32(acc);  // the first bit of the stream is the top bit of byte 0
  }
}

static G4Limits g4_limits(int64_t total_rows, int64_t packed_bytes, int64_t slot_bytes, int64_t out_bytes) {
  YMK_CHECK(total_rows >= 0 && total_rows <= 0x7fffffffLL - 4096 && packed_bytes >= 0 && slot_bytes >= 0 && out_bytes >= 0, "bad sizes");
  return G4Limits{total_rows, packed_bytes / 4, slot_bytes / 4, out_bytes};
}
static void g4_check_table(const int* blob_dev, int64_t blob_words, int n_pages) {
  check_page_table(blob_dev, blob_words, n_pages, G4_REC, 3, 4096, "0..4096 pages", "page table: n records");
}

static void launch_g4_rows(hipStream_t s, const int* blob, int n_pages, const G4Limits& lim, int max_rows, const uint32_t* packed,
                           uint32_t* slots, uint32_t* rowbits) {
  YMK_CHECK(max_rows >= 1 && max_rows <= G4_MAX_SIDE, "max_rows: the largest page's rows");
  check_aligned8(packed, "packed rows: 8-byte aligned");
  check_aligned8(slots, "slots: 8-byte aligned");
  check_aligned8(rowbits, "row bit counts: 8-byte aligned");
  hipLaunchKernelGGL(k_g4_rows, dim3((unsigned)((max_rows + RC_ROWS - 1) / RC_ROWS), (unsigned)n_pages), dim3(RC_THREADS), 0, s, blob, lim, packed,
                     slots, rowbits);
  YMK_HIP(hipGetLastError());
}
static void launch_g4_scan(hipStream_t s, const int* blob, int n_pages, const G4Limits& lim, const uint32_t* rowbits, uint64_t* rowoff,
                           int* lengths) {
  check_aligned8(rowbits, "row bit counts: 8-byte aligned");
  check_aligned8(rowoff, "row offsets: 8-byte aligned");
  YMK_CHECK(lengths && ((uintptr_t)lengths & 3) == 0, "null or misaligned lengths");
  hipLaunchKernelGGL(k_g4_scan, dim3((unsigned)n_pages), dim3(SC_THREADS), 0, s, blob, lim, rowbits, (unsigned long long*)rowoff, lengths);
  YMK_HIP(hipGetLastError());
}
static void launch_g4_concat(hipStream_t s, const int* blob, int n_pages, const G4Limits& lim, const uint32_t* slots, const uint64_t* rowoff,
                             const int* lengths, unsigned char* out, int64_t max_capacity) {
  check_aligned8(slots, "slots: 8-byte aligned");
  check_aligned8(rowoff, "row offsets: 8-byte aligned");
  YMK_CHECK(out && ((uintptr_t)out & 15) == 0 && lengths, "output: 16-byte aligned");
  YMK_CHECK(max_capacity >= 0 && max_capacity <= 0x7fffffffLL, "bad capacity");
  hipLaunchKernelGGL(k_g4_concat, dim3(file_word_grid(max_capacity, CC_THREADS), (unsigned)n_pages), dim3(CC_THREADS), 0, s, blob, lim, slots,
                     (const unsigned long long*)rowoff, lengths, out);
  YMK_HIP(hipGetLastError());
}

}  // namespace ymk

extern "C" {

int ymk_g4_page_words(void) { return ymk::G4_REC; }

int ymk_g4_slot_words(int w) { return w >= 1 && w <= ymk::G4_MAX_SIDE ? ymk::g4_slot_words(w) : -1; }

int64_t ymk_g4_file_capacity(int h, int w) {
  if (h < 1 || w < 1 || h > ymk::G4_MAX_SIDE || w > ymk::G4_MAX_SIDE) return -1;
  return ((int64_t)h * (7 * (int64_t)w + 21) + 24 + 7) / 8;
}

int ymk_g4_scratch_bytes(const int* h, const int* w, int n_pages, int64_t* sizes5_out) {
  YMK_API_BEGIN
  YMK_CHECK(n_pages >= 0 && n_pages <= 4096 && sizes5_out && (n_pages == 0 || (h && w)), "bad argument");
  int64_t rows = 0, packed = 0, slots = 0;
  for (int k = 0; k < n_pages; ++k) {
    YMK_CHECK(h[k] >= 1 && w[k] >= 1 && h[k] <= ymk::G4_MAX_SIDE && w[k] <= ymk::G4_MAX_SIDE, "a page has 1..16383 pixels on a side");
    rows += h[k];
    packed += (int64_t)h[k] * ((w[k] + 31) >> 5);
    slots += (int64_t)h[k] * ymk::g4_slot_words(w[k]);
  }
  sizes5_out[0] = rows;
  sizes5_out[1] = ((packed + 1) & ~1LL) * 4;
  sizes5_out[2] = ((slots + 1) & ~1LL) * 4;
  sizes5_out[3] = ((rows + 1) & ~1LL) * 4;
  sizes5_out[4] = (rows + n_pages) * 8;
  YMK_API_END
}

int ymk_g4_test_pack(const int* blob_dev, int64_t blob_words, int n_pages, int64_t max_pixels, int* flags_dev, uint32_t* packed_dev,
                     int64_t packed_bytes, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(max_pixels >= 0 && max_pixels <= 16383LL * 16383LL, "bad argument");
  if (n_pages == 0) return 0;
  ymk::g4_check_table(blob_dev, blob_words, n_pages);
  YMK_CHECK(flags_dev && ((uintptr_t)flags_dev & 3) == 0, "null or misaligned flags");
  ymk::check_aligned8(packed_dev, "packed rows: 8-byte aligned");
  const ymk::G4Limits lim = ymk::g4_limits(0, packed_bytes, 0, 0);
  const hipStream_t s = (hipStream_t)stream;
  YMK_HIP(hipMemsetAsync(flags_dev, 0, (size_t)n_pages * sizeof(int), s));
  // 64 pixels per wave and step, sixteen steps per wave where the largest page has that many; 512 blocks per page at the most
  const int64_t per_block = (int64_t)ymk::TP_THREADS * 16;
  const unsigned gx = (unsigned)std::min<int64_t>(std::max<int64_t>((max_pixels + per_block - 1) / per_block, 1), 512);
  hipLaunchKernelGGL(ymk::k_g4_test_pack, dim3(gx, (unsigned)n_pages), dim3(ymk::TP_THREADS), 0, s, blob_dev, lim, flags_dev, packed_dev);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}

int ymk_g4_code_rows(const int* blob_dev, int64_t blob_words, int n_pages, int64_t total_rows, int max_rows, const uint32_t* packed_dev,
                     int64_t packed_bytes, uint32_t* slots_dev, int64_t slot_bytes, int64_t out_bytes, uint32_t* rowbits_dev, void* stream) {
  YMK_API_BEGIN
  if (n_pages == 0 || total_rows == 0) return 0;
  ymk::g4_check_table(blob_dev, blob_words, n_pages);
  const ymk::G4Limits lim = ymk::g4_limits(total_rows, packed_bytes, slot_bytes, out_bytes);
  ymk::launch_g4_rows((hipStream_t)stream, blob_dev, n_pages, lim, max_rows, packed_dev, slots_dev, rowbits_dev);
  YMK_API_END
}

int ymk_g4_scan(const int* blob_dev, int64_t blob_words, int n_pages, int64_t total_rows, int64_t packed_bytes, int64_t slot_bytes,
                int64_t out_bytes, const uint32_t* rowbits_dev, uint64_t* rowoff_dev, int* lengths_dev, void* stream) {
  YMK_API_BEGIN
  if (n_pages == 0) return 0;
  ymk::g4_check_table(blob_dev, blob_words, n_pages);
  const ymk::G4Limits lim = ymk::g4_limits(total_rows, packed_bytes, slot_bytes, out_bytes);
  ymk::launch_g4_scan((hipStream_t)stream, blob_dev, n_pages, lim, rowbits_dev, rowoff_dev, lengths_dev);
  YMK_API_END
}

int ymk_g4_concat(const int* blob_dev, int64_t blob_words, int n_pages, int64_t total_rows, int64_t packed_bytes, const uint32_t* slots_dev,
                  int64_t slot_bytes, const uint64_t* rowoff_dev, const int* lengths_dev, unsigned char* out_dev, int64_t out_bytes,
                  int64_t max_capacity, void* stream) {
  YMK_API_BEGIN
  if (n_pages == 0) return 0;
  ymk::g4_check_table(blob_dev, blob_words, n_pages);
  const ymk::G4Limits lim = ymk::g4_limits(total_rows, packed_bytes, slot_bytes, out_bytes);
  ymk::launch_g4_concat((hipStream_t)stream, blob_dev, n_pages, lim, slots_dev, rowoff_dev, lengths_dev, out_dev, max_capacity);
  YMK_API_END
}

int ymk_g4_encode_pages(const int* blob_dev, int64_t blob_words, int n_pages, int64_t total_rows, int max_rows, const uint32_t* packed_dev,
                        int64_t packed_bytes, uint32_t* slots_dev, int64_t slot_bytes, uint32_t* rowbits_dev, uint64_t* rowoff_dev,
                        unsigned char* out_dev, int64_t out_bytes, int64_t max_capacity, int* lengths_dev, void* stream) {
  YMK_API_BEGIN
  if (n_pages == 0) return 0;
  ymk::g4_check_table(blob_dev, blob_words, n_pages);
  YMK_CHECK(total_rows > 0, "pages without rows");
  const ymk::G4Limits lim = ymk::g4_limits(total_rows, packed_bytes, slot_bytes, out_bytes);
  const hipStream_t s = (hipStream_t)stream;
  ymk::launch_g4_rows(s, blob_dev, n_pages, lim, max_rows, packed_dev, slots_dev, rowbits_dev);
  ymk::launch_g4_scan(s, blob_dev, n_pages, lim, rowbits_dev, rowoff_dev, lengths_dev);
  ymk::launch_g4_concat(s, blob_dev, n_pages, lim, slots_dev, rowoff_dev, lengths_dev, out_dev, max_capacity);
  YMK_API_END
}
}
