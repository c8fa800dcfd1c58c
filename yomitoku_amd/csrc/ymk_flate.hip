// Lossless page files of a wave: a zlib stream of the page's PNG-filtered rows in one dynamic-Huffman Deflate block
// (include/ymk.h, "Lossless pages"; yomitoku_amd/flate.py; DESIGN.md, "Lossless pages").  tests/flate_ref.py is the definition;
// every stage equals it byte for byte.
//
//   k_fl_rows    one wave per row segment (at most 8192 filtered bytes; a row of up to 2730 colour pixels is one segment): the
//                five filter costs of the whole row reduced across the wave, the filtered bytes into LDS and out, the segment's
//                Adler sums, the six run lengths by a reverse scan in LDS (a lane a chunk, the carries by a suffix scan of the
//                lanes), the greedy parse by one lane walking best[i] in LDS, the tokens compacted in place and written out by
//                all lanes, the segment's symbol counts from LDS into the page's histogram with integer atomics.  Measured on a
//                wave of 16 pages of 1600 x 1200 x 3 (19 200 segments of 4801 bytes): 3.1 ms on document pages, 11.3 ms on
//                textured pages where nearly every byte is a literal - the walk's chain of dependent LDS reads is the step.
//   k_fl_tables  one wave per page: the three length sets (the shared construction of ymk_pages.h: libjpeg's merge rule across the
//                lanes, Figure K.3's limiter - the JPEG encoder's optimised tables come from the same code), the canonical codes,
//                the header's bits, the file's exact size, the page's Adler-32 folded from the segments' sums.
//   k_fl_code    one wave per segment: its tokens under the page's tables, LSB first, into LDS (a lane a chunk of tokens, the
//                chunks' bit offsets by a scan of the lanes) and from there into the segment's slot; its bit count.
//   k_fl_scan    one block per page: the segments' bit counts -> every piece's bit offset in the file; a page whose counts do
//                not add up to what k_fl_tables found gets -1.
//   k_fl_gather  one thread per 32-bit word of a file, as k_g4_concat: a binary search for the piece that holds the word's
//                first bit - the head (78 9C and the block's header), the segments, the tail (end-of-block, the pad, the
//                checksum) -, then bits until the word is full.  The last word's bytes behind the file's end are not written.
//
// Termination: no loop waits for another thread.  The merges of k_fl_tables end after at most n - 1 rounds (a round removes a
// live symbol); the walk of k_fl_rows advances i by at least 1 a step; the binary search halves; every other loop counts.
//
// The capacity (ymk_flate_file_capacity).  A literal costs at most 15 bits for one filtered byte.  A match costs at most 15 + 5
// bits for its length and 15 + 1 for its distance - the distances 1 2 3 4 6 8 are symbols 0-5, one extra bit at the most -: 36
// bits for at least 3 bytes.  So the tokens cost at most 15 bits a filtered byte, and a segment of n bytes fits a slot of
// ceil(15 n / 32) + 1 words.  End-of-block: 15.  The header: 17 bits, 19 x 3, and for each of at most 316 code lengths a symbol
// of at most 7 bits with at most 7 extra bits: 4498.  With 78 9C, the pad and the checksum: 2 + ceil((4498 + 15 N + 15) / 8) + 4
// bytes for N = h (1 + w c) filtered bytes.

#include "ymk_pages.h"

#include "../../include/ymk.h"

namespace ymk {

constexpr int FL_REC = YMK_FLATE_PAGE_WORDS, FL_HIST = YMK_FLATE_HIST_WORDS, FL_HEAD = YMK_FLATE_HEAD_WORDS;
constexpr int FL_MAX_SIDE = 16383, FL_SEG = 8192, FL_NLIT = 286, FL_NDIST = 30, FL_NCL = 19, FL_NSYM = FL_NLIT + FL_NDIST;
constexpr int FL_HEADER_BITS = 17 + 3 * FL_NCL + FL_NSYM * 14;
constexpr int FL_HEAD_TAIL = 8, FL_HEAD_BITS_AT = 10;  // words of a page's head: 0-7 the summary, 8-9 the tail's bits, 10.. the head's
constexpr unsigned FL_OVERFLOW = 0xffffffffu;
constexpr unsigned FL_ADLER = 65521u;
static_assert(FL_HEAD_BITS_AT + (16 + FL_HEADER_BITS + 31) / 32 <= FL_HEAD, "a page's head holds the header");

__host__ __device__ inline int fl_slot_words(int n) { return (15 * n + 31) / 32 + 1; }
__host__ __device__ inline int fl_row_bytes(int w, int ch) { return 1 + w * ch; }
__host__ __device__ inline int fl_row_segments(int w, int ch) { return (fl_row_bytes(w, ch) + FL_SEG - 1) / FL_SEG; }
__host__ __device__ inline int fl_row_slot_words(int w, int ch) {
  const int n = fl_row_bytes(w, ch), s = fl_row_segments(w, ch);
  return (s - 1) * fl_slot_words(FL_SEG) + fl_slot_words(n - (s - 1) * FL_SEG);
}

struct FlLimits {
  long long filt_bytes, segs, slot_words, out_bytes;
  int n_index;
};

// A page's record, read and checked against the buffers' sizes with the channels it ARRIVED with (the most it can take): a page
// whose record fails is absent for every kernel.  ch: the channels it is coded with - 1 for a three-channel page the grey test
// found grey.
struct FlPage {
  const unsigned char* src;
  int h, w, ch_src, ch, index, capacity, grey_at;
  long long filt_at, seg_at, slot_at, out_at;
  int row_bytes, nseg, row_slot;
  bool ok;
};
__device__ __forceinline__ FlPage fl_page(const int* blob, int p, const FlLimits& lim) {
  const int* r = blob + (size_t)p * FL_REC;
  FlPage g;
  g.src = reinterpret_cast<const unsigned char*>((unsigned long long)page_word64(r, 0));
  g.h = r[2], g.w = r[3], g.ch_src = r[4], g.index = r[5];
  g.filt_at = page_word64(r, 6), g.seg_at = page_word64(r, 8), g.slot_at = page_word64(r, 10), g.out_at = page_word64(r, 12);
  g.capacity = r[14], g.grey_at = r[15];
  g.ok = g.h >= 1 && g.w >= 1 && g.h <= FL_MAX_SIDE && g.w <= FL_MAX_SIDE && (g.ch_src == 1 || g.ch_src == 3) && g.src != nullptr &&
         g.index >= 0 && g.index < lim.n_index && g.grey_at >= 0 && g.grey_at <= lim.n_index;
  g.ch = g.ch_src, g.row_bytes = g.nseg = g.row_slot = 0;
  if (g.ok) {
    const long long rb = fl_row_bytes(g.w, g.ch_src), ns = fl_row_segments(g.w, g.ch_src), rs = fl_row_slot_words(g.w, g.ch_src);
    g.ok = g.filt_at >= 0 && g.filt_at + g.h * rb <= lim.filt_bytes && g.seg_at >= 0 && g.seg_at + g.h * ns <= lim.segs && g.slot_at >= 0 &&
           g.slot_at + g.h * rs <= lim.slot_words && g.capacity >= 0 && g.out_at >= 0 && (g.out_at & 3) == 0 &&
           g.out_at + (long long)g.capacity <= lim.out_bytes;
  }
  return g;
}
__device__ __forceinline__ void fl_coded_as(FlPage& g, int ch) {
  g.ch = (ch == 1 || ch == g.ch_src) ? ch : g.ch_src;
  g.row_bytes = fl_row_bytes(g.w, g.ch), g.nseg = fl_row_segments(g.w, g.ch), g.row_slot = fl_row_slot_words(g.w, g.ch);
}
// before there is a head: from the grey test's answer (0: every pixel has B == G == R)
__device__ __forceinline__ int fl_channels(const FlPage& g, const int* grey) {
  return g.ch_src == 3 && g.grey_at > 0 && grey != nullptr && grey[g.grey_at - 1] == 0 ? 1 : g.ch_src;
}

__device__ __forceinline__ int fl_length_symbol(int v) {  // v = length - 3
  if (v == 255) return 285;
  if (v < 8) return 257 + v;
  const int e = 29 - __clz(v);
  return 257 + 4 * (e + 1) + ((v >> e) & 3);
}
__device__ __forceinline__ int fl_length_extra(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }

// ------------------------------------------------------------------------------------------------ rows
__device__ __forceinline__ int fl_paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// sample j of row y: R G B of a B G R page, channel 0 of a grey-valued one; 0 outside the page.  No load outside the page.
__device__ __forceinline__ int fl_sample(const FlPage& g, int y, int j) {
  if (y < 0 || j < 0) return 0;
  if (g.ch == 3) {
    const int x = j / 3, k = j - 3 * x;
    return g.src[((size_t)y * g.w + x) * 3 + (2 - k)];
  }
  return g.src[((size_t)y * g.w + j) * g.ch_src];
}
__device__ __forceinline__ int fl_filtered(int type, int cur, int left, int up, int ul) {
  const int pred = type == 0 ? 0 : type == 1 ? left : type == 2 ? up : type == 3 ? (left + up) >> 1 : fl_paeth(left, up, ul);
  return (cur - pred) & 255;
}

__global__ __launch_bounds__(64) void k_fl_rows(const int* __restrict__ blob, FlLimits lim, const int* __restrict__ grey,
                                                unsigned char* __restrict__ filt, unsigned short* __restrict__ tokens,
                                                unsigned* __restrict__ segtok, unsigned* __restrict__ segadler, int* __restrict__ hist) {
  __shared__ unsigned char s_f[FL_SEG];
  __shared__ unsigned short s_best[FL_SEG];  // (index of the distance << 9 | length) of the best match at a position; then the tokens
  __shared__ int s_hist[FL_NSYM];
  __shared__ int s_ntok;
  const int p = blockIdx.z, y = blockIdx.y, sg = blockIdx.x, lane = threadIdx.x;
  FlPage g = fl_page(blob, p, lim);
  if (!g.ok) return;  // the whole block
  fl_coded_as(g, fl_channels(g, grey));
  if (y >= g.h || sg >= g.nseg) return;
  const int c = g.ch, nb = g.w * c, at = sg * FL_SEG, n = min(FL_SEG, g.row_bytes - at);
  for (int i = lane; i < FL_NSYM; i += 64) s_hist[i] = 0;
  // the filter: the five costs of the WHOLE row (every segment of a long row finds the same type)
  int cost[5] = {0, 0, 0, 0, 0};
  for (int j = lane; j < nb; j += 64) {
    const int cur = fl_sample(g, y, j), left = fl_sample(g, y, j - c), up = fl_sample(g, y - 1, j), ul = fl_sample(g, y - 1, j - c);
#pragma unroll
    for (int t = 0; t < 5; ++t) cost[t] += abs((int)(signed char)fl_filtered(t, cur, left, up, ul));
  }
  int type = 0, least = 0;
#pragma unroll
  for (int t = 0; t < 5; ++t) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cost[t] += __shfl_xor(cost[t], o);
    if (t == 0 || cost[t] < least) least = cost[t], type = t;
  }
  // the segment's filtered bytes and Adler sums: S = sum b, T = sum (n - q) b
  unsigned long long sum = 0, tri = 0;
  unsigned char* frow = filt + g.filt_at + (long long)y * g.row_bytes + at;
  for (int q = lane; q < n; q += 64) {
    const int j = at + q - 1;
    const int b = j < 0 ? type : fl_filtered(type, fl_sample(g, y, j), fl_sample(g, y, j - c), fl_sample(g, y - 1, j), fl_sample(g, y - 1, j - c));
    s_f[q] = (unsigned char)b;
    frow[q] = (unsigned char)b;
    sum += (unsigned)b, tri += (unsigned long long)(n - q) * (unsigned)b;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o), tri += __shfl_xor(tri, o);
  // the runs: lane l owns the positions [l ch, l ch + ch); ch / 4 is odd, so the lanes' byte reads fall into different banks
  const int ch0 = (n + 63) >> 6, chunk = ch0 + ((12 - (ch0 & 7)) & 7), lo = min(lane * chunk, n), hi = min(lo + chunk, n);
  for (int i = lo; i < hi; ++i) s_best[i] = 0;
  __syncthreads();
  constexpr int DIST[6] = {1, 2, 3, 4, 6, 8};
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int d = DIST[k];
    int run = 0;  // the run at the chunk's first position, had the chunk no neighbour
    for (int i = hi - 1; i >= lo; --i) run = (i >= d && s_f[i] == s_f[i - d]) ? run + 1 : 0;
    int all = run == hi - lo;  // an empty chunk: (0, true), the identity
    // suffix scan of (run, all) over the lanes: afterwards `run` is the run at the chunk's first position
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int r2 = __shfl_down(run, o), a2 = __shfl_down(all, o);
      if (lane + o < 64) {
        run = all ? run + r2 : run;
        all = all && a2;
      }
    }
    int carry = __shfl_down(run, 1);
    if (lane == 63) carry = 0;
    run = carry;
    for (int i = hi - 1; i >= lo; --i) {
      run = (i >= d && s_f[i] == s_f[i - d]) ? run + 1 : 0;
      const int r = min(run, 258);
      if (r > (s_best[i] & 0x1ff)) s_best[i] = (unsigned short)(k << 9 | r);  // strictly longer: a tie stays with the smaller d
    }
  }
  __syncthreads();
  // the parse: one lane walks.  A token takes at least one position, so token t lands at or before the position just read
  if (lane == 0) {
    int i = 0, nt = 0;
    while (i < n) {  // one LDS round trip a token: both reads go out together, the counts are adds nobody waits for
      const int v = s_best[i], b = s_f[i], len = v & 0x1ff;
      unsigned short tok;
      if (len >= 3) {
        tok = (unsigned short)(0x8000 | (v & 0xe00) | (len - 3));
        atomicAdd(&s_hist[fl_length_symbol(len - 3)], 1);
        atomicAdd(&s_hist[FL_NLIT + (v >> 9)], 1);
        i += len;
      } else {
        tok = (unsigned short)b;
        atomicAdd(&s_hist[b], 1);
        i += 1;
      }
      s_best[nt++] = tok;
    }
    if (y == 0 && sg == 0) atomicAdd(&s_hist[256], 1);  // end-of-block, once a page
    s_ntok = nt;
    const long long seg = g.seg_at + (long long)y * g.nseg + sg;
    segtok[seg] = (unsigned)nt;
    segadler[seg] = (unsigned)(tri % FL_ADLER) << 16 | (unsigned)(sum % FL_ADLER);
  }
  __syncthreads();
  unsigned short* trow = tokens + g.filt_at + (long long)y * g.row_bytes + at;
  for (int i = lane; i < s_ntok; i += 64) trow[i] = s_best[i];
  int* mine = hist + (size_t)g.index * FL_HIST;
  for (int i = lane; i < FL_NSYM; i += 64)
    if (s_hist[i]) atomicAdd(mine + i, s_hist[i]);
}

// ------------------------------------------------------------------------------------------------ tables
// The code lengths of `n` <= 320 frequencies (LDS) under `limit` <= 15 into out (LDS), by all 64 lanes of the one wave: symbol
// k * 64 + lane sits in register k.  The construction is ymk_pages.h's, the one k_jpeg_optimal_tables runs; what is flate's own:
// no reserved code point, so the Kraft sum stays 1, and a single used symbol gets a code of one bit.
__device__ void fl_huff(const unsigned* freq_in, int n, int limit, unsigned char* out, int* s_key, int* s_bits, int* s_cum) {
  const int lane = threadIdx.x;
  unsigned freq[5];
  int len[5], used = 0;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int s = k * 64 + lane;
    freq[k] = s < n ? min(freq_in[s], 0x3fffffffu) : 0u;
    used += __popcll(__ballot(freq[k] != 0));
  }
  huff_merge_lengths(freq, len, n - 1, lane);  // a round removes a live symbol
  s_bits[lane] = 0;
  __syncthreads();
  int longest = 0;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int s = k * 64 + lane;
    if (used == 1 && s < n && freq_in[s] != 0) len[k] = 1;  // one used symbol: length 1
    len[k] = min(len[k], 63);
    if (len[k] > 0) atomicAdd(&s_bits[len[k]], 1);
    s_key[s] = len[k] > 0 ? (len[k] << 9 | s) : 0x7fffffff;
    longest = max(longest, len[k]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) longest = max(longest, __shfl_xor(longest, o));
  __syncthreads();
  if (lane == 0) {  // Figure K.3 with `limit`, then the first place of every length
    huff_limit_counts(s_bits, longest, limit);
    int at = 0;
    for (int l = 1; l <= limit; ++l) s_cum[l] = at, at += s_bits[l];
    s_cum[limit + 1] = at;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int s = k * 64 + lane, key = s_key[s];
    if (s >= n) continue;
    int l = 0;
    if (key != 0x7fffffff) {
      int rank = 0;  // the symbol's place by (length before limiting, symbol)
      for (int o = 0; o < n; ++o) rank += s_key[o] < key;
      l = huff_length_of_rank(s_cum, rank, limit);
    }
    out[s] = (unsigned char)l;
  }
  __syncthreads();
}

struct FlBits {  // LSB first into LDS words, by one lane
  unsigned* out;
  unsigned long long acc;
  int held, pos, total;
  __device__ __forceinline__ void put(unsigned v, int n) {  // n <= 16
    acc |= (unsigned long long)(v & ((1u << n) - 1u)) << held;
    held += n, total += n;
    if (held >= 32) out[pos++] = (unsigned)acc, acc >>= 32, held -= 32;
  }
  __device__ __forceinline__ void finish() {
    if (held > 0) out[pos++] = (unsigned)acc;
  }
};

// canonical codes (RFC 1951, 3.2.2) of n lengths, each as (length << 16 | the code's bits reversed: LSB first), by one lane
__device__ void fl_codes(const unsigned char* len, int n, unsigned* out) {
  int count[16], next[16];
  for (int b = 0; b < 16; ++b) count[b] = 0;
  for (int s = 0; s < n; ++s) count[len[s] & 15] += len[s] != 0;
  int code = 0;
  next[0] = 0;
  for (int b = 1; b < 16; ++b) code = (code + count[b - 1]) << 1, next[b] = code;
  for (int s = 0; s < n; ++s) {
    const int l = len[s] & 15;
    out[s] = l ? (unsigned)l << 16 | (__brev((unsigned)next[l]++) >> (32 - l)) : 0u;
  }
}

__device__ const unsigned char FL_CL_ORDER[FL_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// sizes[2 index] = the file's bytes, -1 where it exceeds the capacity; sizes[2 index + 1] = the channels it is coded with.
__global__ __launch_bounds__(64) void k_fl_tables(const int* __restrict__ blob, FlLimits lim, const int* __restrict__ grey,
                                                  const int* __restrict__ hist, const unsigned* __restrict__ segadler,
                                                  unsigned* __restrict__ tables, unsigned* __restrict__ head, int* __restrict__ sizes) {
  __shared__ unsigned s_freq[320];
  __shared__ unsigned char s_len[320], s_cllen[32];
  __shared__ int s_key[320], s_bits[64], s_cum[18];
  __shared__ unsigned short s_rle[FL_NSYM];
  __shared__ unsigned s_clfreq[32], s_code[FL_NSYM], s_clcode[32], s_headbits[FL_HEAD];
  __shared__ int s_n[4];  // hlit, hdist, symbols of the run-length coded header, the head's bits
  const int p = blockIdx.x, lane = threadIdx.x;
  FlPage g = fl_page(blob, p, lim);
  if (!g.ok) {  // the whole block; a record without a place for its answer leaves none
    if (lane == 0 && g.index >= 0 && g.index < lim.n_index) sizes[2 * g.index] = -1, sizes[2 * g.index + 1] = 0;
    return;
  }
  fl_coded_as(g, fl_channels(g, grey));
  const int* mine = hist + (size_t)g.index * FL_HIST;
  for (int i = lane; i < 320; i += 64) s_freq[i] = i < FL_NSYM ? (unsigned)max(mine[i], 0) : 0u;
  __syncthreads();
  fl_huff(s_freq, FL_NLIT, 15, s_len, s_key, s_bits, s_cum);
  fl_huff(s_freq + FL_NLIT, FL_NDIST, 15, s_len + FL_NLIT, s_key, s_bits, s_cum);
  if (lane < 32) s_clfreq[lane] = 0;
  __syncthreads();
  if (lane == 0) {
    int hlit = FL_NLIT, hdist = FL_NDIST;
    while (hlit > 257 && s_len[hlit - 1] == 0) --hlit;
    while (hdist > 1 && s_len[FL_NLIT + hdist - 1] == 0) --hdist;
    if (hdist == 1 && s_len[FL_NLIT] == 0) s_len[FL_NLIT] = 1;  // no match: one distance code is declared
    const int total = hlit + hdist;
    int i = 0, nr = 0, prev = -1;
    while (i < total) {  // the greedy rule of the header
      const int v = s_len[i < hlit ? i : FL_NLIT + i - hlit];
      int r = 1;
      while (i + r < total && s_len[i + r < hlit ? i + r : FL_NLIT + i + r - hlit] == v) ++r;
      int sym, ev, eb;
      if (v == 0 && r >= 3) {
        r = min(r, 138);
        if (r >= 11) sym = 18, eb = 7, ev = r - 11; else sym = 17, eb = 3, ev = r - 3;
      } else if (prev == v && r >= 3) {
        r = min(r, 6), sym = 16, eb = 2, ev = r - 3;
      } else {
        r = 1, sym = v, eb = 0, ev = 0;
      }
      s_rle[nr++] = (unsigned short)(sym | eb << 5 | ev << 8);
      ++s_clfreq[sym];
      prev = v, i += r;
    }
    s_n[0] = hlit, s_n[1] = hdist, s_n[2] = nr;
  }
  __syncthreads();
  fl_huff(s_clfreq, FL_NCL, 7, s_cllen, s_key, s_bits, s_cum);
  if (lane == 0) {
    fl_codes(s_len, FL_NLIT, s_code);
    fl_codes(s_len + FL_NLIT, FL_NDIST, s_code + FL_NLIT);
    fl_codes(s_cllen, FL_NCL, s_clcode);
    int hclen = FL_NCL;
    while (hclen > 4 && s_cllen[FL_CL_ORDER[hclen - 1]] == 0) --hclen;
    FlBits w{s_headbits, 0ull, 0, 0, 0};
    w.put(0x9c78u, 16);  // 78 9C
    w.put(1u, 1), w.put(2u, 2);
    w.put((unsigned)(s_n[0] - 257), 5), w.put((unsigned)(s_n[1] - 1), 5), w.put((unsigned)(hclen - 4), 4);
    for (int k = 0; k < hclen; ++k) w.put(s_cllen[FL_CL_ORDER[k]], 3);
    for (int k = 0; k < s_n[2]; ++k) {
      const int e = s_rle[k], sym = e & 31, eb = (e >> 5) & 7, ev = e >> 8;
      w.put(s_clcode[sym] & 0xffffu, (int)(s_clcode[sym] >> 16));
      if (eb) w.put((unsigned)ev, eb);
    }
    w.finish();
    s_n[3] = w.total;
  }
  __syncthreads();
  // the tokens' bits from the histogram: every symbol's count times its length and extra bits (end-of-block is counted)
  unsigned long long bits = 0;
  for (int s = lane; s < FL_NSYM; s += 64) {
    const int extra = s < FL_NLIT ? fl_length_extra(s) : (s - FL_NLIT >= 4 ? ((s - FL_NLIT) >> 1) - 1 : 0);
    bits += (unsigned long long)s_freq[s] * (unsigned)(s_len[s] + extra);
  }
  // the page's Adler-32: a lane folds a run of segments, then the lanes' results in order
  const long long nsegs = (long long)g.h * g.nseg;
  const long long per = (nsegs + 63) / 64, s_lo = min((long long)lane * per, nsegs), s_hi = min(s_lo + per, nsegs);
  const unsigned last = (unsigned)(g.row_bytes - (g.nseg - 1) * FL_SEG);
  unsigned long long S = 0, T = 0, N = 0;
  for (long long s = s_lo; s < s_hi; ++s) {
    const unsigned a = segadler[g.seg_at + s], n2 = (s % g.nseg) == g.nseg - 1 ? last : (unsigned)FL_SEG;
    T = (T + (unsigned long long)(n2 % FL_ADLER) * S + (a >> 16)) % FL_ADLER;
    S = (S + (a & 0xffffu)) % FL_ADLER;
    N = (N + n2) % FL_ADLER;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bits += __shfl_xor(bits, o);
  unsigned long long S0 = 0, T0 = 0, N0 = 0;
  for (int j = 0; j < 64; ++j) {  // the same in every lane
    const unsigned long long s2 = __shfl(S, j), t2 = __shfl(T, j), n2 = __shfl(N, j);
    T0 = (T0 + n2 * S0 + t2) % FL_ADLER;
    S0 = (S0 + s2) % FL_ADLER;
    N0 = (N0 + n2) % FL_ADLER;
  }
  const unsigned adler = (unsigned)((N0 + T0) % FL_ADLER) << 16 | (unsigned)((1 + S0) % FL_ADLER);
  unsigned* mh = head + (size_t)g.index * FL_HEAD;
  unsigned* mt = tables + (size_t)g.index * FL_HIST;
  for (int i = lane; i < FL_NSYM; i += 64) mt[i] = s_code[i];
  for (int i = lane; i < FL_HEAD - FL_HEAD_BITS_AT; i += 64) mh[FL_HEAD_BITS_AT + i] = i < (s_n[3] + 31) / 32 ? s_headbits[i] : 0u;
  if (lane == 0) {
    const int eob_len = (int)(s_code[256] >> 16);
    const unsigned long long tail_at = (unsigned long long)s_n[3] + bits - (unsigned)eob_len, end = tail_at + (unsigned)eob_len;
    const int pad = (int)((8 - (end & 7)) & 7);
    const unsigned long long bytes = ((end + (unsigned)pad) >> 3) + 4;
    const unsigned long long tail = (unsigned long long)(s_code[256] & 0xffffu) | (unsigned long long)__builtin_bswap32(adler) << (eob_len + pad);
    const int fits = bytes <= (unsigned long long)g.capacity && bytes <= 0x7fffffffull;
    mh[0] = fits ? (unsigned)bytes : 0xffffffffu, mh[1] = (unsigned)g.ch, mh[2] = (unsigned)s_n[3], mh[3] = (unsigned)(eob_len + pad + 32);
    mh[4] = adler, mh[5] = (unsigned)tail_at, mh[6] = (unsigned)(tail_at >> 32), mh[7] = 0;
    mh[FL_HEAD_TAIL] = (unsigned)tail, mh[FL_HEAD_TAIL + 1] = (unsigned)(tail >> 32);
    sizes[2 * g.index] = fits ? (int)bytes : -1, sizes[2 * g.index + 1] = g.ch;
  }
}

// the stages behind the tables take the channels from the page's head; false: the page has no file
__device__ __forceinline__ bool fl_headed(FlPage& g, const unsigned* head) {
  if (!g.ok) return false;
  const unsigned* mh = head + (size_t)g.index * FL_HEAD;
  if ((int)mh[0] < 0) return false;
  fl_coded_as(g, (int)mh[1]);
  return true;
}

// ------------------------------------------------------------------------------------------------ code
__global__ __launch_bounds__(64) void k_fl_code(const int* __restrict__ blob, FlLimits lim, const unsigned short* __restrict__ tokens,
                                                const unsigned* __restrict__ segtok, const unsigned* __restrict__ tables,
                                                const unsigned* __restrict__ head, unsigned* __restrict__ slots, unsigned* __restrict__ segbits) {
  __shared__ unsigned s_tab[FL_NSYM];
  __shared__ unsigned s_out[(15 * FL_SEG + 31) / 32 + 2];
  const int p = blockIdx.z, y = blockIdx.y, sg = blockIdx.x, lane = threadIdx.x;
  FlPage g = fl_page(blob, p, lim);
  if (!fl_headed(g, head) || y >= g.h || sg >= g.nseg) return;  // the whole block
  const int at = sg * FL_SEG, n = min(FL_SEG, g.row_bytes - at), words = fl_slot_words(n);
  const long long seg = g.seg_at + (long long)y * g.nseg + sg;
  const int nt = (int)min(segtok[seg], (unsigned)n);
  const unsigned* mt = tables + (size_t)g.index * FL_HIST;
  for (int i = lane; i < FL_NSYM; i += 64) s_tab[i] = mt[i];
  for (int i = lane; i < words; i += 64) s_out[i] = 0;
  __syncthreads();
  const unsigned short* trow = tokens + g.filt_at + (long long)y * g.row_bytes + at;
  const int per = (nt + 63) >> 6, lo = min(lane * per, nt), hi = min(lo + per, nt);
  int mine = 0;
  for (int i = lo; i < hi; ++i) {
    const int t = trow[i];
    if (t & 0x8000) {
      const int sym = fl_length_symbol(t & 0xff), j = (t >> 9) & 7;
      mine += (int)((s_tab[sym] >> 16) & 15) + fl_length_extra(sym) + (int)((s_tab[FL_NLIT + min(j, 5)] >> 16) & 15) + (j >= 4);
    } else {
      mine += (int)((s_tab[t & 0xff] >> 16) & 15);
    }
  }
  const int incl = wave_inclusive_scan(mine, lane);
  const int total = __shfl(incl, 63);
  const bool fits = total <= 15 * n;  // always, with lengths of at most 15 bits and tokens of k_fl_rows
  if (fits) {
    int pos = incl - mine;
    auto put = [&](unsigned long long v, int nbits) {  // at most 20 bits
      const unsigned long long x = v << (pos & 31);
      atomicOr(&s_out[pos >> 5], (unsigned)x);
      if (x >> 32) atomicOr(&s_out[(pos >> 5) + 1], (unsigned)(x >> 32));
      pos += nbits;
    };
    for (int i = lo; i < hi; ++i) {
      const int t = trow[i];
      if (t & 0x8000) {
        const int v = t & 0xff, sym = fl_length_symbol(v), eb = fl_length_extra(sym), j = min((t >> 9) & 7, 5);
        const unsigned cl = s_tab[sym], cd = s_tab[FL_NLIT + j];
        const int ll = (int)((cl >> 16) & 15), ld = (int)((cd >> 16) & 15);
        put((unsigned long long)(cl & 0xffffu) | (unsigned long long)(v & ((1 << eb) - 1)) << ll, ll + eb);
        put((unsigned long long)(cd & 0xffffu) | (unsigned long long)(j >= 4) << ld, ld + (j >= 4));
      } else {
        const unsigned cl = s_tab[t & 0xff];
        put(cl & 0xffffu, (int)((cl >> 16) & 15));
      }
    }
  }
  __syncthreads();
  if (fits) {
    unsigned* slot = slots + g.slot_at + (long long)y * g.row_slot + (long long)sg * fl_slot_words(FL_SEG);
    for (int i = lane; i < (total + 31) >> 5; i += 64) slot[i] = s_out[i];
  }
  if (lane == 0) segbits[seg] = fits ? (unsigned)total : FL_OVERFLOW;
}

// ------------------------------------------------------------------------------------------------ scan
constexpr int FS_THREADS = 256;
// off: per page its pieces' bit offsets, at seg_at + 3 index: the head at 0, the segments, the tail, the file's end.
__global__ __launch_bounds__(FS_THREADS) void k_fl_scan(const int* __restrict__ blob, FlLimits lim, const unsigned* __restrict__ segbits,
                                                        unsigned* __restrict__ head, unsigned long long* __restrict__ off, int* __restrict__ sizes) {
  __shared__ unsigned long long part[FS_THREADS];
  const int p = blockIdx.x, t = threadIdx.x;
  FlPage g = fl_page(blob, p, lim);
  if (!fl_headed(g, head)) return;  // the whole block: k_fl_tables has said -1
  unsigned* mh = head + (size_t)g.index * FL_HEAD;
  const int nsegs = g.h * g.nseg;  // at most 16383 x 6
  const int per = (nsegs + FS_THREADS - 1) / FS_THREADS, lo = min(t * per, nsegs), hi = min(lo + per, nsegs);
  unsigned long long sum = 0;
  int bad = 0;
  for (int s = lo; s < hi; ++s) {
    const unsigned b = segbits[g.seg_at + s];
    bad |= b == 0 || b == FL_OVERFLOW;
    sum += b;
  }
  part[t] = sum;
  __syncthreads();
  block_inclusive_scan_u64<FS_THREADS>(part, t);
  const unsigned long long first = mh[2], tail_at = (unsigned long long)mh[6] << 32 | mh[5];
  bad |= first + part[FS_THREADS - 1] != tail_at;
  bad = __syncthreads_or(bad);
  unsigned long long* mo = off + g.seg_at + 3 * (long long)g.index;
  unsigned long long at = first + part[t] - sum;
  for (int s = lo; s < hi; ++s) {
    mo[1 + s] = at;
    at += segbits[g.seg_at + s];
  }
  if (t == 0) {
    mo[0] = 0, mo[1 + nsegs] = tail_at, mo[2 + nsegs] = tail_at + mh[3];
    if (bad) mh[0] = 0xffffffffu, sizes[2 * g.index] = -1;
  }
}

// ------------------------------------------------------------------------------------------------ gather
constexpr int FG_THREADS = 256;
__global__ __launch_bounds__(FG_THREADS) void k_fl_gather(const int* __restrict__ blob, FlLimits lim, const unsigned* __restrict__ slots,
                                                          const unsigned* __restrict__ head, const unsigned long long* __restrict__ off,
                                                          unsigned char* __restrict__ out) {
  const int p = blockIdx.y;
  FlPage g = fl_page(blob, p, lim);
  if (!fl_headed(g, head)) return;
  const unsigned* mh = head + (size_t)g.index * FL_HEAD;
  const int len = (int)mh[0];
  if (len > g.capacity) return;
  const unsigned long long* mo = off + g.seg_at + 3 * (long long)g.index;
  const int nsegs = g.h * g.nseg, pieces = nsegs + 2;
  if (mo[pieces] != 8ull * (unsigned)len) return;  // not this page's offsets
  const int words = (len + 3) >> 2;
  unsigned char* file = out + g.out_at;
  for (int k = blockIdx.x * FG_THREADS + threadIdx.x; k < words; k += gridDim.x * FG_THREADS) {
    const unsigned long long bit = 32ull * (unsigned)k;
    int r = last_piece_at_or_before(mo, pieces, bit);
    unsigned acc = 0;
    int filled = 0, s = (int)(bit - mo[r]);
    while (filled < 32 && r < pieces) {
      const int nb = (int)(mo[r + 1] - mo[r]), take = min(32 - filled, nb - s);
      const unsigned* piece;
      if (r == 0) piece = mh + FL_HEAD_BITS_AT;
      else if (r == pieces - 1) piece = mh + FL_HEAD_TAIL;
      else {
        const int y = (r - 1) / g.nseg, sg = (r - 1) - y * g.nseg;
        piece = slots + g.slot_at + (long long)y * g.row_slot + (long long)sg * fl_slot_words(FL_SEG);
      }
      const int i = s >> 5, sh = s & 31;
      unsigned v = piece[i] >> sh;
      if (sh + take > 32) v |= piece[i + 1] << (32 - sh);
      if (take < 32) v &= (1u << take) - 1u;
      acc |= v << filled;
      filled += take;
      ++r;
      s = 0;
    }
    if (4 * k + 4 <= len) {
      *reinterpret_cast<unsigned*>(file + 4 * (size_t)k) = acc;  // the first bit of the stream is the lowest of byte 0
    } else {
      for (int b = 4 * k; b < len; ++b) file[b] = (unsigned char)(acc >> (8 * (b - 4 * k)));  // nothing behind the file's end
    }
  }
}

// ------------------------------------------------------------------------------------------------ launches
static FlLimits fl_limits(int n_index, int64_t filt_bytes, int64_t segs, int64_t slot_bytes, int64_t out_bytes) {
  YMK_CHECK(n_index >= 0 && n_index <= 4096, "0..4096 pages");
  YMK_CHECK(filt_bytes >= 0 && segs >= 0 && segs <= 0x7fffffffLL - 3 * 4096 && slot_bytes >= 0 && out_bytes >= 0, "bad sizes");
  return FlLimits{filt_bytes, segs, slot_bytes / 4, out_bytes, n_index};
}
static void fl_check_table(const int* blob_dev, int64_t blob_words, int n_pages, int n_index) {
  check_page_table(blob_dev, blob_words, n_pages, FL_REC, 3, n_index, "0..n_index pages", "page table: n records");
}
static dim3 fl_segment_grid(int n_pages, int max_rows, int max_row_segments) {
  YMK_CHECK(max_rows >= 1 && max_rows <= FL_MAX_SIDE, "max_rows: the largest page's rows");
  YMK_CHECK(max_row_segments >= 1 && max_row_segments <= fl_row_segments(FL_MAX_SIDE, 3), "max_row_segments: the widest page's");
  return dim3((unsigned)max_row_segments, (unsigned)max_rows, (unsigned)n_pages);
}

static void launch_fl_rows(hipStream_t s, const int* blob, int n_pages, const FlLimits& lim, int max_rows, int max_row_segments, const int* grey,
                           unsigned char* filt, uint16_t* tokens, uint32_t* segtok, uint32_t* segadler, int* hist) {
  check_aligned8(filt, "filtered bytes: 8-byte aligned");
  check_aligned8(tokens, "tokens: 8-byte aligned");
  check_aligned8(segtok, "token counts: 8-byte aligned");
  check_aligned8(segadler, "checksum parts: 8-byte aligned");
  check_aligned8(hist, "histograms: 8-byte aligned");
  YMK_HIP(hipMemsetAsync(hist, 0, (size_t)lim.n_index * FL_HIST * sizeof(int), s));
  hipLaunchKernelGGL(k_fl_rows, fl_segment_grid(n_pages, max_rows, max_row_segments), dim3(64), 0, s, blob, lim, grey, filt,
                     (unsigned short*)tokens, segtok, segadler, hist);
  YMK_HIP(hipGetLastError());
}
static void launch_fl_tables(hipStream_t s, const int* blob, int n_pages, const FlLimits& lim, const int* grey, const int* hist,
                             const uint32_t* segadler, uint32_t* tables, uint32_t* head, int* sizes) {
  check_aligned8(hist, "histograms: 8-byte aligned");
  check_aligned8(segadler, "checksum parts: 8-byte aligned");
  check_aligned8(tables, "tables: 8-byte aligned");
  check_aligned8(head, "heads: 8-byte aligned");
  YMK_CHECK(sizes && ((uintptr_t)sizes & 3) == 0, "null or misaligned sizes");
  hipLaunchKernelGGL(k_fl_tables, dim3((unsigned)n_pages), dim3(64), 0, s, blob, lim, grey, hist, segadler, tables, head, sizes);
  YMK_HIP(hipGetLastError());
}
static void launch_fl_code(hipStream_t s, const int* blob, int n_pages, const FlLimits& lim, int max_rows, int max_row_segments,
                           const uint16_t* tokens, const uint32_t* segtok, const uint32_t* tables, const uint32_t* head, uint32_t* slots,
                           uint32_t* segbits) {
  check_aligned8(tokens, "tokens: 8-byte aligned");
  check_aligned8(segtok, "token counts: 8-byte aligned");
  check_aligned8(tables, "tables: 8-byte aligned");
  check_aligned8(head, "heads: 8-byte aligned");
  check_aligned8(slots, "slots: 8-byte aligned");
  check_aligned8(segbits, "bit counts: 8-byte aligned");
  hipLaunchKernelGGL(k_fl_code, fl_segment_grid(n_pages, max_rows, max_row_segments), dim3(64), 0, s, blob, lim, (const unsigned short*)tokens,
                     segtok, tables, head, slots, segbits);
  YMK_HIP(hipGetLastError());
}
static void launch_fl_scan(hipStream_t s, const int* blob, int n_pages, const FlLimits& lim, const uint32_t* segbits, uint32_t* head,
                           uint64_t* off, int* sizes) {
  check_aligned8(segbits, "bit counts: 8-byte aligned");
  check_aligned8(head, "heads: 8-byte aligned");
  check_aligned8(off, "offsets: 8-byte aligned");
  YMK_CHECK(sizes && ((uintptr_t)sizes & 3) == 0, "null or misaligned sizes");
  hipLaunchKernelGGL(k_fl_scan, dim3((unsigned)n_pages), dim3(FS_THREADS), 0, s, blob, lim, segbits, head, (unsigned long long*)off, sizes);
  YMK_HIP(hipGetLastError());
}
static void launch_fl_gather(hipStream_t s, const int* blob, int n_pages, const FlLimits& lim, const uint32_t* slots, const uint32_t* head,
                             const uint64_t* off, unsigned char* out, int64_t max_capacity) {
  check_aligned8(slots, "slots: 8-byte aligned");
  check_aligned8(head, "heads: 8-byte aligned");
  check_aligned8(off, "offsets: 8-byte aligned");
  YMK_CHECK(out && ((uintptr_t)out & 15) == 0, "output: 16-byte aligned");
  YMK_CHECK(max_capacity >= 0 && max_capacity <= 0x7fffffffLL, "bad capacity");
  hipLaunchKernelGGL(k_fl_gather, dim3(file_word_grid(max_capacity, FG_THREADS), (unsigned)n_pages), dim3(FG_THREADS), 0, s, blob, lim, slots, head, (const unsigned long long*)off, out);
  YMK_HIP(hipGetLastError());
}

}  // namespace ymk

extern "C" {

int ymk_flate_page_words(void) { return ymk::FL_REC; }

int64_t ymk_flate_file_capacity(int h, int w, int channels) {
  if (h < 1 || w < 1 || h > ymk::FL_MAX_SIDE || w > ymk::FL_MAX_SIDE || (channels != 1 && channels != 3)) return -1;
  const int64_t n = (int64_t)h * ymk::fl_row_bytes(w, channels);
  return 2 + (ymk::FL_HEADER_BITS + 15 * n + 15 + 7) / 8 + 4;
}

int ymk_flate_scratch_bytes(const int* h, const int* w, const int* channels, int n_pages, int64_t* sizes8_out) {
  YMK_API_BEGIN
  YMK_CHECK(n_pages >= 0 && n_pages <= 4096 && sizes8_out && (n_pages == 0 || (h && w && channels)), "bad argument");
  int64_t segs = 0, filt = 0, slots = 0;
  for (int k = 0; k < n_pages; ++k) {
    YMK_CHECK(h[k] >= 1 && w[k] >= 1 && h[k] <= ymk::FL_MAX_SIDE && w[k] <= ymk::FL_MAX_SIDE, "a page has 1..16383 pixels on a side");
    YMK_CHECK(channels[k] == 1 || channels[k] == 3, "a page has 1 or 3 channels");
    segs += (int64_t)h[k] * ymk::fl_row_segments(w[k], channels[k]);
    filt += (int64_t)h[k] * ymk::fl_row_bytes(w[k], channels[k]);
    slots += (int64_t)h[k] * ymk::fl_row_slot_words(w[k], channels[k]);
  }
  sizes8_out[0] = segs;
  sizes8_out[1] = (filt + 7) & ~7LL;                  // filt_dev
  sizes8_out[2] = ((filt + 7) & ~7LL) * 2;            // tokens_dev
  sizes8_out[3] = ((segs + 1) & ~1LL) * 4;            // segtok_dev, segadler_dev, segbits_dev, each
  sizes8_out[4] = (segs + 3 * (int64_t)n_pages) * 8;  // off_dev
  sizes8_out[5] = ((slots + 1) & ~1LL) * 4;           // slots_dev
  sizes8_out[6] = (int64_t)n_pages * ymk::FL_HIST * 4;  // hist_dev, tables_dev, each
  sizes8_out[7] = (int64_t)n_pages * ymk::FL_HEAD * 4;  // head_dev
  YMK_API_END
}

int ymk_flate_rows(const int* blob_dev, int64_t blob_words, int n_pages, int n_index, int64_t filt_bytes, int64_t segs, int64_t slot_bytes,
                   int64_t out_bytes, int max_rows, int max_row_segments, const int* grey_dev, unsigned char* filt_dev, uint16_t* tokens_dev,
                   uint32_t* segtok_dev, uint32_t* segadler_dev, int* hist_dev, void* stream) {
  YMK_API_BEGIN
  if (n_pages == 0) return 0;
  ymk::fl_check_table(blob_dev, blob_words, n_pages, n_index);
  const ymk::FlLimits lim = ymk::fl_limits(n_index, filt_bytes, segs, slot_bytes, out_bytes);
  ymk::launch_fl_rows((hipStream_t)stream, blob_dev, n_pages, lim, max_rows, max_row_segments, grey_dev, filt_dev, tokens_dev, segtok_dev,
                      segadler_dev, hist_dev);
  YMK_API_END
}

int ymk_flate_tables(const int* blob_dev, int64_t blob_words, int n_pages, int n_index, int64_t filt_bytes, int64_t segs, int64_t slot_bytes,
                     int64_t out_bytes, const int* grey_dev, const int* hist_dev, const uint32_t* segadler_dev, uint32_t* tables_dev,
                     uint32_t* head_dev, int* sizes_dev, void* stream) {
  YMK_API_BEGIN
  if (n_pages == 0) return 0;
  ymk::fl_check_table(blob_dev, blob_words, n_pages, n_index);
  const ymk::FlLimits lim = ymk::fl_limits(n_index, filt_bytes, segs, slot_bytes, out_bytes);
  ymk::launch_fl_tables((hipStream_t)stream, blob_dev, n_pages, lim, grey_dev, hist_dev, segadler_dev, tables_dev, head_dev, sizes_dev);
  YMK_API_END
}

int ymk_flate_code(const int* blob_dev, int64_t blob_words, int n_pages, int n_index, int64_t filt_bytes, int64_t segs, int64_t slot_bytes,
                   int64_t out_bytes, int max_rows, int max_row_segments, const uint16_t* tokens_dev, const uint32_t* segtok_dev,
                   const uint32_t* tables_dev, const uint32_t* head_dev, uint32_t* slots_dev, uint32_t* segbits_dev, void* stream) {
  YMK_API_BEGIN
  if (n_pages == 0) return 0;
  ymk::fl_check_table(blob_dev, blob_words, n_pages, n_index);
  const ymk::FlLimits lim = ymk::fl_limits(n_index, filt_bytes, segs, slot_bytes, out_bytes);
  ymk::launch_fl_code((hipStream_t)stream, blob_dev, n_pages, lim, max_rows, max_row_segments, tokens_dev, segtok_dev, tables_dev, head_dev,
                      slots_dev, segbits_dev);
  YMK_API_END
}

int ymk_flate_scan(const int* blob_dev, int64_t blob_words, int n_pages, int n_index, int64_t filt_bytes, int64_t segs, int64_t slot_bytes,
                   int64_t out_bytes, const uint32_t* segbits_dev, uint32_t* head_dev, uint64_t* off_dev, int* sizes_dev, void* stream) {
  YMK_API_BEGIN
  if (n_pages == 0) return 0;
  ymk::fl_check_table(blob_dev, blob_words, n_pages, n_index);
  const ymk::FlLimits lim = ymk::fl_limits(n_index, filt_bytes, segs, slot_bytes, out_bytes);
  ymk::launch_fl_scan((hipStream_t)stream, blob_dev, n_pages, lim, segbits_dev, head_dev, off_dev, sizes_dev);
  YMK_API_END
}

int ymk_flate_gather(const int* blob_dev, int64_t blob_words, int n_pages, int n_index, int64_t filt_bytes, int64_t segs, int64_t slot_bytes,
                     int64_t out_bytes, const uint32_t* slots_dev, const uint32_t* head_dev, const uint64_t* off_dev, unsigned char* out_dev,
                     int64_t max_capacity, void* stream) {
  YMK_API_BEGIN
  if (n_pages == 0) return 0;
  ymk::fl_check_table(blob_dev, blob_words, n_pages, n_index);
  const ymk::FlLimits lim = ymk::fl_limits(n_index, filt_bytes, segs, slot_bytes, out_bytes);
  ymk::launch_fl_gather((hipStream_t)stream, blob_dev, n_pages, lim, slots_dev, head_dev, off_dev, out_dev, max_capacity);
  YMK_API_END
}

int ymk_flate_encode_pages(const int* blob_dev, int64_t blob_words, int n_pages, int n_index, int64_t filt_bytes, int64_t segs,
                           int64_t slot_bytes, int64_t out_bytes, int max_rows, int max_row_segments, const int* grey_dev,
                           unsigned char* filt_dev, uint16_t* tokens_dev, uint32_t* segtok_dev, uint32_t* segadler_dev, uint32_t* segbits_dev,
                           int* hist_dev, uint32_t* tables_dev, uint32_t* head_dev, uint64_t* off_dev, uint32_t* slots_dev,
                           unsigned char* out_dev, int64_t max_capacity, int* sizes_dev, void* stream) {
  YMK_API_BEGIN
  if (n_pages == 0) return 0;
  ymk::fl_check_table(blob_dev, blob_words, n_pages, n_index);
  const ymk::FlLimits lim = ymk::fl_limits(n_index, filt_bytes, segs, slot_bytes, out_bytes);
  const hipStream_t s = (hipStream_t)stream;
  ymk::launch_fl_rows(s, blob_dev, n_pages, lim, max_rows, max_row_segments, grey_dev, filt_dev, tokens_dev, segtok_dev, segadler_dev, hist_dev);
  ymk::launch_fl_tables(s, blob_dev, n_pages, lim, grey_dev, hist_dev, segadler_dev, tables_dev, head_dev, sizes_dev);
  ymk::launch_fl_code(s, blob_dev, n_pages, lim, max_rows, max_row_segments, tokens_dev, segtok_dev, tables_dev, head_dev, slots_dev, segbits_dev);
  ymk::launch_fl_scan(s, blob_dev, n_pages, lim, segbits_dev, head_dev, off_dev, sizes_dev);
  ymk::launch_fl_gather(s, blob_dev, n_pages, lim, slots_dev, head_dev, off_dev, out_dev, max_capacity);
  YMK_API_END
}
}
