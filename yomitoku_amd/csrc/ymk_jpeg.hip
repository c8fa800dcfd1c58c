// Baseline JPEG encoder for a wave of pages resident in HBM (DocumentAnalyzer.serve(jpeg=...), yomitoku_amd/jpeg.py), and the
// uint8 form of the Pillow resample that shrinks a page first.  DESIGN.md, "JPEG encoder", has the pixel rules and the format;
// tests/jpeg_ref.py is the definition every stage equals byte for byte.  All arithmetic is integer.
//
//   k_jpeg_coefficients   one wave per tile (16 x 16 pixels of a colour page - the MCU at 4:2:0, two MCUs at 4:2:2, four at 4:4:4 -,
//                         8 x 8 of a one-component one), four tiles per block.  The tile's rows come in as 16-byte loads into LDS
//                         (an edge tile, or a page whose rows are not 16-byte aligned: byte loads with the coordinates clamped =
//                         edge replication), are converted to Y Cb Cr, the chroma averaged 2 x 2 / in pairs / not at all, and the
//                         six / eight / twelve 8 x 8 blocks go through libjpeg's `islow` DCT - 8 lanes per block, one row, then
//                         one column each; twelve blocks in two turns - and the quantiser.  Output: zig-zag int16 [block][64] in
//                         scan order; an MCU of an edge tile that is not the page's is not written.  A page's mode (word 15 of
//                         its record; tests/jpeg_modes_ref.py is the definition) also makes channel 0 of a three-channel page a
//                         one-component file: the same tile and loads, four MCUs of one block, no copy of the plane.
//   k_jpeg_pages_grey     whether a three-channel page has B == G == R everywhere (what decides that mode): an OR-reduction of
//                         the pixels' XORs, 16-byte loads, one int per page.
//   k_jpeg_entropy        one wave per restart interval (= one MCU row).  64 blocks at a time: their coefficients staged in LDS,
//                         each lane sizes ITS block (DC predictor = the previous block of the component, 0 at the start of the
//                         interval), a wave prefix sum turns the sizes into bit positions, the words the chunk will touch are
//                         zeroed, and each lane writes its block's codes.  A lane shares at most its first and its last 32-bit
//                         word with a neighbour: those two go out with atomicOr, the words in between with plain stores.  Then
//                         the pad bits, and a count of the FF bytes: the interval's record is (bytes, bytes after stuffing).
//   k_jpeg_compact        one wave per interval again: the stuffed lengths of the page's intervals summed (the file's length, and
//                         this interval's place in it), the header copied by interval 0, the interval copied with FF -> FF 00
//                         (a count per lane and a wave prefix sum give every lane its place), RSTm or EOI behind it.  A file that
//                         does not fit the page's capacity is not written at all; its length stays -1.
//   k_pil_resize_u8       k_pil_resize_batch (ymk_image.hip) with uint8 [oh][ow][C] outputs of differing sizes.
//
// Optimised Huffman tables (ymk_jpeg_encode_pages_opt; the definition is tests/jpeg_opt_ref.py) put two launches between the
// coefficients and the entropy stage, and the entropy and compaction stages run in their OPT form:
//   k_jpeg_histogram      k_jpeg_entropy's decomposition (one wave per interval, 64 blocks at a time in LDS, the same DC
//                         predecessor): the symbols the coder will emit are counted in LDS, the non-zero bins added to the page's
//                         histogram (integer atomicAdd: the sums do not depend on the order).
//   k_jpeg_optimal_tables one workgroup per page, one wave per table.  The construction is the shared one of ymk_pages.h, which
//                         the Deflate coder (ymk_flate.hip) runs too: libjpeg's rule - the two rarest symbols are merged until
//                         one is left - and the lengths limited to 16 bits (Annex K.3).  The kernel's own: the reserved symbol
//                         256 and the removal of its code point, the codes assigned (Annex C), the DHT segments.
//                         Output: the page's symbol -> code table in c_luts' layout, and its DHT segments as bytes.
//   k_jpeg_entropy<true>  s_lut filled from the page's table; YMK_JPEG_BLOCK_STREAM_BYTES_OPT per block (a DC code may have 16 bits).
//   k_jpeg_compact<true>  the header is the blob's up to SOF0, the page's DHT bytes, the blob's from DRI.
//
// Nothing is allocated and nothing waited for; no workgroup waits for another (every stage is a launch of its own).
#include "ymk_pages.h"

#include "../../include/ymk.h"

namespace ymk {

constexpr int JP_REC = YMK_JPEG_PAGE_WORDS;
constexpr int JP_BLOCK_WORDS = YMK_JPEG_BLOCK_STREAM_BYTES / 4;  // 32-bit words of the unstuffed stream reserved per block
constexpr int JP_WAVES = 4;                                      // tiles per block of k_jpeg_coefficients
constexpr int JP_TILE_BLOCKS = 12;                               // blocks of a 16 x 16 tile at 4:4:4 (4:2:2: 8, 4:2:0: 6)
static_assert(YMK_JPEG_BLOCK_STREAM_BYTES % 4 == 0 && YMK_JPEG_BLOCK_STREAM_BYTES * 8 >= 22 + 63 * 26,
              "a block's worst case: a 11 + 11 bit DC and 63 AC symbols of 16 + 10 bits");
constexpr int JP_BLOCK_WORDS_OPT = YMK_JPEG_BLOCK_STREAM_BYTES_OPT / 4;
static_assert(YMK_JPEG_BLOCK_STREAM_BYTES_OPT % 4 == 0 && YMK_JPEG_BLOCK_STREAM_BYTES_OPT * 8 >= 27 + 63 * 26,
              "with a page's own tables any code may have 16 bits: a 16 + 11 bit DC and 63 AC symbols of 16 + 10 bits");
constexpr int JP_LUT_WORDS = YMK_JPEG_TABLE_WORDS;  // one page's histogram or code table: [2][256 + 16]
constexpr int JP_DHT_BYTES = YMK_JPEG_DHT_BYTES;    // one page's DHT record: an int32 length, then the segments
constexpr int JP_SEG_BYTES = 2 + 2 + 1 + 16 + 256;  // the longest DHT segment
static_assert(JP_LUT_WORDS == 2 * (256 + 16) && JP_DHT_BYTES % 4 == 0 && JP_DHT_BYTES >= 4 + 2 * (JP_SEG_BYTES - 240) + 2 * JP_SEG_BYTES,
              "two DC segments of at most 16 symbols and two AC segments of at most 256 behind the length");

// ------------------------------------------------------------------------------------------------ tables (Annex K)
struct HuffSpec {
  unsigned char bits[16];   // codes of each length 1..16
  unsigned char vals[162];  // symbols in code order
  int n;
};
constexpr HuffSpec DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec AC_LUMA = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    162};
constexpr HuffSpec AC_CHROMA = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    162};

// symbol -> code | length << 16 (Annex C's canonical assignment); 0 for a symbol the table does not have
struct HuffLut {
  unsigned e[256];
};
constexpr HuffLut make_lut(const HuffSpec& s) {
  HuffLut t{};
  unsigned code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < s.bits[len - 1]; ++i) t.e[s.vals[k++]] = code++ | (unsigned)len << 16;
    code <<= 1;
  }
  return t;
}
// [0] luminance, [1] chrominance; the twelve DC entries follow the 256 AC entries of a table
struct HuffLuts {
  unsigned e[2][256 + 16];
};
constexpr HuffLuts make_luts() {
  HuffLuts t{};
  const HuffLut ac0 = make_lut(AC_LUMA), ac1 = make_lut(AC_CHROMA), dc0 = make_lut(DC_LUMA), dc1 = make_lut(DC_CHROMA);
  for (int i = 0; i < 256; ++i) t.e[0][i] = ac0.e[i], t.e[1][i] = ac1.e[i];
  for (int i = 0; i < 16; ++i) t.e[0][256 + i] = dc0.e[i], t.e[1][256 + i] = dc1.e[i];
  return t;
}
__constant__ HuffLuts c_luts = make_luts();

constexpr unsigned char ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
__constant__ unsigned char c_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                           41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                           30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr unsigned char LUMA_Q[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40, 57,
                                      69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,
                                      81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
constexpr unsigned char CHROMA_Q[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                        99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// the IJG quality rule; out: zig-zag order, luminance then chrominance
static void quant_tables(int quality, int* out128) {
  const int q = std::min(std::max(quality, 1), 100);
  const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k) {
      const int base = (t ? CHROMA_Q : LUMA_Q)[ZIGZAG[k]];
      out128[t * 64 + k] = std::min(std::max((base * scale + 50) / 100, 1), 255);
    }
}

// A page's mode (word 15 of its record), host and device.  The luminance sampling factors are 1 << lh and 1 << lv (a
// one-component file: 1 x 1, an MCU of one block).  A tile - the pixels a wave of k_jpeg_coefficients takes - has 1 << lt pixels on
// a side: 16 of a three-channel page in every mode (one, two or four MCUs), the MCU's 8 of a one-channel page.  Logarithms, so
// that the device derives a page's geometry with shifts.
struct JpegMode {
  int comps, lh, lv, lt;
};
__host__ __device__ inline bool jpeg_mode(int channels, int mode, JpegMode& m) {
  if (channels == 1 && mode == 0) {
    m = {1, 0, 0, 3};
  } else if (channels == 3 && mode == YMK_JPEG_MODE_GREY) {
    m = {1, 0, 0, 4};
  } else if (channels == 3 && (mode == YMK_JPEG_MODE_420 || mode == YMK_JPEG_MODE_422 || mode == YMK_JPEG_MODE_444)) {
    m = {3, mode == YMK_JPEG_MODE_444 ? 0 : 1, mode == YMK_JPEG_MODE_420 ? 1 : 0, 4};
  } else {
    return false;
  }
  return true;
}

static void put_segment(std::vector<unsigned char>& out, int marker, const std::vector<unsigned char>& payload) {
  out.push_back(0xff);
  out.push_back((unsigned char)marker);
  out.push_back((unsigned char)((payload.size() + 2) >> 8));
  out.push_back((unsigned char)((payload.size() + 2) & 255));
  out.insert(out.end(), payload.begin(), payload.end());
}

// SOI, APP0, DQT, SOF0, DHT, DRI, SOS: everything before the scan's first byte
// dht false: without the DHT segments, *split = the bytes before their place
static std::vector<unsigned char> jpeg_header(int h, int w, const JpegMode& mode, int quality, bool dht = true, int* split = nullptr) {
  const bool grey = mode.comps == 1;
  int q[128];
  quant_tables(quality, q);
  std::vector<unsigned char> out = {0xff, 0xd8};
  put_segment(out, 0xe0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (int t = 0; t < (grey ? 1 : 2); ++t) {
    std::vector<unsigned char> p = {(unsigned char)t};
    for (int k = 0; k < 64; ++k) p.push_back((unsigned char)q[t * 64 + k]);
    put_segment(out, 0xdb, p);
  }
  std::vector<unsigned char> sof = {8, (unsigned char)(h >> 8), (unsigned char)(h & 255), (unsigned char)(w >> 8), (unsigned char)(w & 255)};
  if (grey) {
    sof.insert(sof.end(), {1, 1, 0x11, 0});
  } else {
    sof.insert(sof.end(), {3, 1, (unsigned char)(1 << (mode.lh + 4) | 1 << mode.lv), 0, 2, 0x11, 1, 3, 0x11, 1});
  }
  put_segment(out, 0xc0, sof);
  const HuffSpec* specs[4] = {&DC_LUMA, &AC_LUMA, &DC_CHROMA, &AC_CHROMA};
  const unsigned char ids[4] = {0x00, 0x10, 0x01, 0x11};
  if (split) *split = (int)out.size();
  for (int t = 0; dht && t < (grey ? 2 : 4); ++t) {
    std::vector<unsigned char> p = {ids[t]};
    p.insert(p.end(), specs[t]->bits, specs[t]->bits + 16);
    p.insert(p.end(), specs[t]->vals, specs[t]->vals + specs[t]->n);
    put_segment(out, 0xc4, p);
  }
  const int mcus = (w + (8 << mode.lh) - 1) >> (3 + mode.lh);  // one MCU row per restart interval
  put_segment(out, 0xdd, {(unsigned char)(mcus >> 8), (unsigned char)(mcus & 255)});
  if (grey) {
    put_segment(out, 0xda, {1, 1, 0x00, 0, 63, 0});
  } else {
    put_segment(out, 0xda, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
  }
  return out;
}

// ------------------------------------------------------------------------------------------------ the page table
struct JpegLimits {
  long long blob_words, total_mcus, total_blocks, total_intervals, out_bytes;  // out_bytes < 0: the stage writes no output
};
struct JpegPage {
  const unsigned char* src;
  int h, w, ch, mcu_w, mcu_h, per;  // per: blocks per MCU
  int comps, lh, lv, lt;            // JpegMode's
  int tile_w, tile_h;               // the page in k_jpeg_coefficients' tiles
  long long first_mcu, first_block, first_interval, out_off;  // first_mcu (word 5) counts tiles
  int capacity, hdr_off, hdr_len, q_off, hdr_split;  // hdr_split (word 14): the header's bytes before the DHT segments' place
};
// Record p, checked against the limits: a record that does not fit is no page (never trusted).
__device__ __forceinline__ bool jpeg_page(const int* __restrict__ blob, const JpegLimits& lim, int p, JpegPage& g) {
  const int* r = blob + (size_t)p * JP_REC;
  g.src = reinterpret_cast<const unsigned char*>((unsigned long long)page_word64(r, 0));
  g.h = r[2], g.w = r[3], g.ch = r[4];
  JpegMode m;
  if (g.src == nullptr || g.h < 1 || g.w < 1 || g.h > 16383 || g.w > 16383 || !jpeg_mode(g.ch, r[15], m)) return false;
  g.comps = m.comps, g.lh = m.lh, g.lv = m.lv, g.lt = m.lt;
  g.per = m.comps == 3 ? (1 << (m.lh + m.lv)) + 2 : 1;
  g.mcu_w = (g.w + (8 << m.lh) - 1) >> (3 + m.lh), g.mcu_h = (g.h + (8 << m.lv) - 1) >> (3 + m.lv);
  g.tile_w = (g.w + (1 << m.lt) - 1) >> m.lt, g.tile_h = (g.h + (1 << m.lt) - 1) >> m.lt;
  g.first_mcu = r[5], g.first_block = r[6], g.first_interval = r[7];
  g.out_off = page_word64(r, 8);
  g.capacity = r[10], g.hdr_off = r[11], g.hdr_len = r[12], g.q_off = r[13];
  g.hdr_split = min(max(r[14], 0), max(g.hdr_len, 0));
  const long long mcus = (long long)g.mcu_w * g.mcu_h;
  if (g.first_mcu < 0 || g.first_block < 0 || g.first_interval < 0 || g.first_mcu + (long long)g.tile_w * g.tile_h > lim.total_mcus ||
      g.first_block + mcus * g.per > lim.total_blocks || g.first_interval + g.mcu_h > lim.total_intervals)
    return false;
  if (g.q_off < 0 || (long long)g.q_off + 128 > lim.blob_words) return false;
  if (g.hdr_off < 0 || g.hdr_len < 0 || (long long)g.hdr_off + g.hdr_len > lim.blob_words * 4) return false;
  if (lim.out_bytes >= 0 && (g.capacity < 0 || g.out_off < 0 || g.out_off + g.capacity > lim.out_bytes)) return false;
  return true;
}
// The page whose tiles (by_interval false) / restart intervals (true) contain global index `idx`, or -1: the first record that is
// a page (jpeg_page) and has the index.  Every wave of every stage searches, through half the table on average, and a whole
// jpeg_page per record passed was most of what a wave of k_jpeg_coefficients executed.  So a record is first asked whether the
// index could be its own, from the five words that say so - its first and its count as jpeg_page derives them, from words not
// yet checked (a record that is no page may answer anything: jpeg_page is asked next, and answers as it always did).
__device__ __forceinline__ int jpeg_find(const int* __restrict__ blob, const JpegLimits& lim, int n_pages, long long idx, bool by_interval,
                                         JpegPage& g) {
  for (int p = 0; p < n_pages; ++p) {
    const int* r = blob + (size_t)p * JP_REC;
    JpegMode m;
    if (!jpeg_mode(r[4], r[15], m)) continue;
    const unsigned h = (unsigned)r[2], w = (unsigned)r[3];
    const long long first = by_interval ? r[7] : r[5];
    const long long count = by_interval ? (long long)((h + (8u << m.lv) - 1) >> (3 + m.lv))
                                        : (long long)((w + (1u << m.lt) - 1) >> m.lt) * (long long)((h + (1u << m.lt) - 1) >> m.lt);
    if (idx < first || idx >= first + count) continue;
    if (jpeg_page(blob, lim, p, g)) return p;
  }
  return -1;
}

// ------------------------------------------------------------------------------------------------ coefficients
// libjpeg's jfdctint.c (`islow`), one pass over eight values `stride` apart: CONST_BITS 13, PASS1_BITS 2
template <bool FIRST>
__device__ __forceinline__ void fdct_pass(int* d, int stride) {
  constexpr int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299, F1847 = 15137,
                F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
  constexpr int SH = FIRST ? 11 : 15, RND = 1 << (SH - 1);
  const int d0 = d[0], d1 = d[stride], d2 = d[2 * stride], d3 = d[3 * stride], d4 = d[4 * stride], d5 = d[5 * stride],
            d6 = d[6 * stride], d7 = d[7 * stride];
  int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (FIRST) {
    d[0] = (t10 + t11) * 4;
    d[4 * stride] = (t10 - t11) * 4;
  } else {
    d[0] = (t10 + t11 + 2) >> 2;
    d[4 * stride] = (t10 - t11 + 2) >> 2;
  }
  int z1 = (t12 + t13) * F0541;
  d[2 * stride] = (z1 + t13 * F0765 + RND) >> SH;
  d[6 * stride] = (z1 - t12 * F1847 + RND) >> SH;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * F1175;
  t4 *= F0298, t5 *= F2053, t6 *= F3072, t7 *= F1501;
  z1 *= -F0899, z2 *= -F2562;
  z3 = z3 * -F1961 + z5, z4 = z4 * -F0390 + z5;
  d[7 * stride] = (t4 + z1 + z3 + RND) >> SH;
  d[5 * stride] = (t5 + z2 + z4 + RND) >> SH;
  d[3 * stride] = (t6 + z2 + z3 + RND) >> SH;
  d[stride] = (t7 + z1 + z4 + RND) >> SH;
}

__global__ __launch_bounds__(JP_WAVES * 64) void k_jpeg_coefficients(const int* __restrict__ blob, JpegLimits lim, int n_pages,
                                                                     short* __restrict__ coef) {
  __shared__ __align__(16) unsigned char s_raw[JP_WAVES][16 * 48];  // the tile's pixels, B G R
  // The tile's MCUs one after the other, each Y.. Cb Cr: samples - 128, then the DCT in place.  Only 4:4:4 has more than eight
  // blocks, and it needs no chroma at full resolution next to them: in the other modes blocks 8 - 11 hold that, Cb and Cr as
  // short [2][256].  15 KB of LDS per workgroup, where blocks and planes side by side would take 19 (4:2:0 alone took 13).
  __shared__ int s_blk[JP_WAVES][JP_TILE_BLOCKS][64];
  static_assert(JP_TILE_BLOCKS == 12 && 4 * 64 * sizeof(int) == 2 * 256 * sizeof(short), "the planes fill blocks 8 - 11");
  // the wave's index is the same in all its lanes; said so, the search for the tile's page and the page's geometry are scalar work
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const long long tile = (long long)blockIdx.x * JP_WAVES + wave;
  JpegPage g;
  const bool ok = tile < lim.total_mcus && jpeg_find(blob, lim, n_pages, tile, false, g) >= 0;  // the same in all lanes of a wave
  const bool colour = ok && g.comps == 3, grey = ok && g.comps == 1;
  const bool wide = ok && g.lt == 4;  // a 16 x 16 tile of a three-channel page: colour, or channel 0 alone
  int tx = 0, ty = 0;
  int d_luma = 8, d_chroma = 8;  // this lane's two divisors, asked for now: every block of the tile uses one of them at the end
  if (ok) {
    const long long local = tile - g.first_mcu;
    ty = (int)(local / g.tile_w), tx = (int)(local % g.tile_w);
    const int* qt = blob + g.q_off;
    d_luma = min(max(qt[lane], 1), 255) * 8, d_chroma = min(max(qt[64 + lane], 1), 255) * 8;
  }
  // The sampling factors are 1 or 2: sh, sv are their logarithms and the masks hs - 1, vs - 1 at once.  The tile has
  // mcus_x x mcus_y MCUs of `per` blocks, the first ny of them luminance.
  const int sh = ok ? g.lh : 0, sv = ok ? g.lv : 0;
  const int lx = wide ? 1 - sh : 0, mcus_x = 1 << lx, mcus_y = wide ? 2 >> sv : 1;
  const int per = ok ? g.per : 0, ny = 1 << (sh + sv);
  const bool full = colour && sh + sv == 0;  // 4:4:4: Cb and Cr go into their blocks as they are
  short* s_chroma = reinterpret_cast<short*>(&s_blk[wave][8][0]);
  if (wide) {
    const int x0 = tx * 16, y0 = ty * 16;
    const size_t pitch = (size_t)g.w * 3;
    const bool whole = x0 + 16 <= g.w && y0 + 16 <= g.h && (pitch & 15) == 0 && ((uintptr_t)g.src & 15) == 0;
    if (whole) {
      if (lane < 48) {  // 16 rows of 48 bytes: three 16-byte loads per row, adjacent lanes on adjacent segments
        const int row = lane / 3, seg = lane % 3;
        const uint4 v = *reinterpret_cast<const uint4*>(g.src + (size_t)(y0 + row) * pitch + (size_t)x0 * 3 + seg * 16);
        *reinterpret_cast<uint4*>(&s_raw[wave][row * 48 + seg * 16]) = v;
      }
    } else {
      for (int i = lane; i < 256; i += 64) {
        const int sy = min(y0 + (i >> 4), g.h - 1), sx = min(x0 + (i & 15), g.w - 1);
        const unsigned char* px = g.src + (size_t)sy * pitch + (size_t)sx * 3;
        s_raw[wave][i * 3] = px[0], s_raw[wave][i * 3 + 1] = px[1], s_raw[wave][i * 3 + 2] = px[2];
      }
    }
  }
  __syncthreads();
  if (colour) {
    for (int i = lane; i < 256; i += 64) {
      const int b = s_raw[wave][i * 3], gr = s_raw[wave][i * 3 + 1], r = s_raw[wave][i * 3 + 2];
      const int y = (19595 * r + 38470 * gr + 7471 * b + 32768) >> 16;
      const int cb = (-11059 * r - 21709 * gr + 32768 * b + (128 << 16) + 32767) >> 16;
      const int cr = (32768 * r - 27439 * gr - 5329 * b + (128 << 16) + 32767) >> 16;
      const int py = i >> 4, px = i & 15, by = py >> 3, bx = px >> 3;
      // block (by, bx) of the tile: its MCU, and its place among the MCU's luminance blocks (row-major)
      const int slot = (((by >> sv) << lx) + (bx >> sh)) * per + ((by & sv) << sh) + (bx & sh);
      s_blk[wave][slot][(py & 7) * 8 + (px & 7)] = y - 128;
      if (full) {
        s_blk[wave][slot + 1][(py & 7) * 8 + (px & 7)] = cb - 128;
        s_blk[wave][slot + 2][(py & 7) * 8 + (px & 7)] = cr - 128;
      } else {
        s_chroma[i] = (short)cb;
        s_chroma[256 + i] = (short)cr;
      }
    }
  } else if (wide) {  // the grey file of a three-channel page: channel 0, four MCUs of one block
    for (int i = lane; i < 256; i += 64) {
      const int py = i >> 4, px = i & 15;
      s_blk[wave][(py >> 3) * 2 + (px >> 3)][(py & 7) * 8 + (px & 7)] = (int)s_raw[wave][i * 3] - 128;
    }
  } else if (grey) {
    const int sy = min(ty * 8 + (lane >> 3), g.h - 1), sx = min(tx * 8 + (lane & 7), g.w - 1);
    s_blk[wave][0][lane] = (int)g.src[(size_t)sy * g.w + sx] - 128;
  }
  __syncthreads();
  if (colour && !full) {  // one MCU at 4:2:0, two (one below the other) at 4:2:2: blocks 0 - 7 at the most
    const int cy = lane >> 3, cx = lane & 7;
    for (int m = 0; m < mcus_y; ++m) {
      // the MCU's first row in the tile, then this lane's sample: 8 chroma columns per MCU, so cx's parity is the column's
      const int at = ((m * 8 + cy) << sv) * 16 + cx * 2;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const short* s = s_chroma + c * 256;
        const int v = sv ? (s[at] + s[at + 1] + s[at + 16] + s[at + 17] + 1 + (cx & 1)) >> 2 : (s[at] + s[at + 1] + (cx & 1)) >> 1;
        s_blk[wave][m * per + ny + c][lane] = v - 128;
      }
    }
  }
  __syncthreads();
  const int nb = mcus_x * mcus_y * per;  // 6, 8 or 12 of a colour page, 4 or 1 of a grey one
  for (int i = lane; i < nb * 8; i += 64) fdct_pass<true>(&s_blk[wave][i >> 3][(i & 7) * 8], 1);
  __syncthreads();
  for (int i = lane; i < nb * 8; i += 64) fdct_pass<false>(&s_blk[wave][i >> 3][i & 7], 8);
  __syncthreads();
  if (ok) {
    for (int m = 0; m < mcus_x * mcus_y; ++m) {
      const int mx = tx * mcus_x + (m & (mcus_x - 1)), my = ty * mcus_y + (m >> lx);
      if (mx >= g.mcu_w || my >= g.mcu_h) continue;  // a tile at the page's edge: the MCU is not the page's
      const long long first = g.first_block + ((long long)my * g.mcu_w + mx) * per;  // < first_block + MCUs * per: jpeg_page
      for (int b = 0; b < per; ++b) {
        const int v = s_blk[wave][m * per + b][c_zigzag[lane]];
        const int d = b >= ny ? d_chroma : d_luma;
        int c = (abs(v) + d / 2) / d;
        c = v < 0 ? -c : c;
        c = min(max(c, lane == 0 ? -1024 : -1023), 1023);
        coef[(size_t)(first + b) * 64 + lane] = (short)c;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ entropy
constexpr int EN_PITCH = 66;  // shorts between the staged blocks of two lanes: 33 words, so 32 lanes read 32 banks

struct BitWriter {
  unsigned* out;  // the interval's words, most significant bit first
  int w;          // next word
  unsigned long long acc;
  int n;          // bits of `acc` in use (< 32 between calls); the first word starts with the neighbour's bits as zeros
  bool first;
  __device__ __forceinline__ void put(unsigned code, int len) {
    acc = (acc << len) | code;
    n += len;
    if (n >= 32) {
      n -= 32;
      const unsigned word = (unsigned)(acc >> n);
      if (first) {
        atomicOr(out + w, word);  // shared with the block before
        first = false;
      } else {
        out[w] = word;  // every bit of it is this lane's
      }
      ++w;
      acc &= (1ull << n) - 1;
    }
  }
  __device__ __forceinline__ void finish() {
    if (n > 0) atomicOr(out + w, (unsigned)(acc << (32 - n)));  // shared with the block behind (or, `first`, with both)
  }
};

// Block `c` (zig-zag, in LDS) with DC predictor `pred`: counts its bits and, EMIT, writes them.
template <bool EMIT>
__device__ __forceinline__ int encode_block(const short* c, int pred, const unsigned* lut, BitWriter* wr) {
  int bits = 0;
  {
    const int diff = min(max((int)c[0] - pred, -2047), 2047);  // what the definition's clamps allow; a stray value cannot outgrow the block's words
    const int cat = 32 - __clz(abs(diff));
    const unsigned e = lut[256 + cat];
    bits += (int)(e >> 16) + cat;
    if (EMIT) wr->put((e & 0xffff) << cat | ((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1)), (int)(e >> 16) + cat);
  }
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = min(max((int)c[k], -1023), 1023);
    if (v == 0) {
      ++run;
      continue;
    }
    while (run > 15) {
      const unsigned z = lut[0xf0];
      bits += (int)(z >> 16);
      if (EMIT) wr->put(z & 0xffff, (int)(z >> 16));
      run -= 16;
    }
    const int cat = 32 - __clz(abs(v));
    const unsigned e = lut[run << 4 | cat];
    bits += (int)(e >> 16) + cat;
    if (EMIT) wr->put((e & 0xffff) << cat | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << cat) - 1)), (int)(e >> 16) + cat);
    run = 0;
  }
  if (run > 0) {
    const unsigned e = lut[0];
    bits += (int)(e >> 16);
    if (EMIT) wr->put(e & 0xffff, (int)(e >> 16));
  }
  return bits;
}

// Block `b` of a restart interval: its component (0 Y, 1 Cb, 2 Cr) - an MCU is per - 2 luminance blocks, then Cb, then Cr; a
// one-component page's is its block -
__device__ __forceinline__ int jpeg_component(const JpegPage& g, int b) { return g.comps == 3 ? max(b % g.per - (g.per - 3), 0) : 0; }
// - and the block before it of the same component, whose DC is its predictor (negative: none, the interval starts here).  Y
// follows Y inside an MCU and the last Y of the MCU before; Cb / Cr the MCU before.
__device__ __forceinline__ int jpeg_predecessor(const JpegPage& g, int b, int comp) {
  if (g.comps != 3) return b - 1;
  return comp == 0 ? (b % g.per == 0 ? b - 3 : b - 1) : b - g.per;
}

// OPT: the codes are the page's own (`tables`, k_jpeg_optimal_tables) and a block has JP_BLOCK_WORDS_OPT words
template <bool OPT>
__global__ __launch_bounds__(64) void k_jpeg_entropy(const int* __restrict__ blob, JpegLimits lim, int n_pages,
                                                     const short* __restrict__ coef, unsigned* __restrict__ stream,
                                                     int* __restrict__ intervals, const unsigned* __restrict__ tables) {
  constexpr int BLOCK_WORDS = OPT ? JP_BLOCK_WORDS_OPT : JP_BLOCK_WORDS;
  __shared__ unsigned s_lut[2][256 + 16];
  __shared__ __align__(16) short s_coef[64 * EN_PITCH];  // written as 32-bit words: a block starts at a multiple of 132 bytes
  const int lane = threadIdx.x;
  if (!OPT)
    for (int i = lane; i < 2 * (256 + 16); i += 64) (&s_lut[0][0])[i] = (&c_luts.e[0][0])[i];
  JpegPage g;
  const long long iv = blockIdx.x;
  const int page = jpeg_find(blob, lim, n_pages, iv, true, g);
  if (page < 0) return;  // the whole block
  if (OPT)               // a length above 16 is not one k_jpeg_optimal_tables writes: such an entry codes nothing
    for (int i = lane; i < JP_LUT_WORDS; i += 64) {
      const unsigned e = tables[(size_t)page * JP_LUT_WORDS + i];
      (&s_lut[0][0])[i] = (e >> 16) <= 16 ? e : 0u;
    }
  const int nb = g.mcu_w * g.per;  // blocks of the interval: <= 1024 * 6
  const long long blk0 = g.first_block + (iv - g.first_interval) * nb;
  unsigned* out = stream + (size_t)blk0 * BLOCK_WORDS;  // nb * BLOCK_WORDS words are this interval's
  int cum = 0, zeroed = 0;                                 // bits written so far (< 2^24); words zeroed so far
  for (int base = 0; base < nb; base += 64) {
    __syncthreads();  // the previous chunk's readers of s_coef (and, first time, the writers of s_lut)
    for (int i = lane; i < 64 * 8; i += 64) {
      const int blk = i >> 3, part = i & 7;
      if (base + blk < nb) {
        const uint4 v = *reinterpret_cast<const uint4*>(coef + (size_t)(blk0 + base + blk) * 64 + part * 8);
        unsigned* d = reinterpret_cast<unsigned*>(&s_coef[blk * EN_PITCH + part * 8]);
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
      }
    }
    __syncthreads();
    const int b = base + lane;
    const bool active = b < nb;
    const int comp = jpeg_component(g, b);  // 0 Y, 1 Cb, 2 Cr
    int pred = 0;
    if (active) {
      const int prev = jpeg_predecessor(g, b, comp);
      if (prev >= 0) pred = coef[(size_t)(blk0 + prev) * 64];
    }
    const unsigned* lut = s_lut[comp ? 1 : 0];
    const short* mine = &s_coef[lane * EN_PITCH];
    const int len = active ? encode_block<false>(mine, pred, lut, nullptr) : 0;
    const int incl = wave_inclusive_scan(len, lane);
    const int total = __shfl(incl, 63);
    const int need = (cum + total + 31) >> 5;  // <= nb * BLOCK_WORDS: a block is at most 1660 (OPT: 1665) bits
    for (int wd = zeroed + lane; wd < need; wd += 64) out[wd] = 0;
    zeroed = max(zeroed, need);
    __syncthreads();  // the zeros are in memory before any lane ORs into them
    if (active && len > 0) {
      const int start = cum + incl - len;
      BitWriter wr{out, start >> 5, 0ull, start & 31, true};
      encode_block<true>(mine, pred, lut, &wr);
      wr.finish();
    }
    cum += total;
  }
  if (lane == 0 && (cum & 7)) {  // pad with 1-bits to a byte
    const int pad = 8 - (cum & 7);
    atomicOr(out + (cum >> 5), ((1u << pad) - 1) << (32 - (cum & 31) - pad));
  }
  __syncthreads();
  const int nbytes = (cum + 7) >> 3;
  int ff = 0;
  for (int wd = lane; wd * 4 < nbytes; wd += 64) {
    // read at the L2: a neighbouring interval's block on this CU may have pulled the line that holds this interval's first
    // or last words into the L1 before they were complete
    const unsigned v = __hip_atomic_load(out + wd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int k = 0; k < 4; ++k) ff += ((v >> (24 - 8 * k)) & 255) == 255;  // bytes behind the last are zero
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ff += __shfl_xor(ff, o);
  if (lane == 0) {
    intervals[2 * iv] = nbytes;
    intervals[2 * iv + 1] = nbytes + ff;
  }
}

// ------------------------------------------------------------------------------------------------ histograms
// The symbols encode_block emits for block `c`, counted in `hist` (LDS, one class: 256 AC bins, then 16 DC bins).
__device__ __forceinline__ void count_block(const short* c, int pred, int* hist) {
  const int diff = min(max((int)c[0] - pred, -2047), 2047);
  atomicAdd(hist + 256 + (32 - __clz(abs(diff))), 1);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = min(max((int)c[k], -1023), 1023);
    if (v == 0) {
      ++run;
      continue;
    }
    while (run > 15) {
      atomicAdd(hist + 0xf0, 1);
      run -= 16;
    }
    atomicAdd(hist + (run << 4 | (32 - __clz(abs(v)))), 1);
    run = 0;
  }
  if (run > 0) atomicAdd(hist, 1);
}

// hist: int32 [n_pages][2][256 + 16], zero before the launch
__global__ __launch_bounds__(64) void k_jpeg_histogram(const int* __restrict__ blob, JpegLimits lim, int n_pages,
                                                       const short* __restrict__ coef, int* __restrict__ hist) {
  __shared__ int s_hist[2][256 + 16];
  __shared__ __align__(16) short s_coef[64 * EN_PITCH];
  const int lane = threadIdx.x;
  JpegPage g;
  const long long iv = blockIdx.x;
  const int page = jpeg_find(blob, lim, n_pages, iv, true, g);
  if (page < 0) return;  // the whole block
  for (int i = lane; i < JP_LUT_WORDS; i += 64) (&s_hist[0][0])[i] = 0;
  const int nb = g.mcu_w * g.per;
  const long long blk0 = g.first_block + (iv - g.first_interval) * nb;
  for (int base = 0; base < nb; base += 64) {
    __syncthreads();  // the previous chunk's readers of s_coef (and, first time, the zeros of s_hist)
    for (int i = lane; i < 64 * 8; i += 64) {
      const int blk = i >> 3, part = i & 7;
      if (base + blk < nb) {
        const uint4 v = *reinterpret_cast<const uint4*>(coef + (size_t)(blk0 + base + blk) * 64 + part * 8);
        unsigned* d = reinterpret_cast<unsigned*>(&s_coef[blk * EN_PITCH + part * 8]);
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
      }
    }
    __syncthreads();
    const int b = base + lane;
    if (b < nb) {
      const int comp = jpeg_component(g, b);
      const int prev = jpeg_predecessor(g, b, comp);  // as k_jpeg_entropy
      const int pred = prev >= 0 ? coef[(size_t)(blk0 + prev) * 64] : 0;
      count_block(&s_coef[lane * EN_PITCH], pred, s_hist[comp ? 1 : 0]);
    }
  }
  __syncthreads();
  int* mine = hist + (size_t)page * JP_LUT_WORDS;
  for (int i = lane; i < JP_LUT_WORDS; i += 64) {
    const int v = (&s_hist[0][0])[i];
    if (v) atomicAdd(mine + i, v);
  }
}

// ------------------------------------------------------------------------------------------------ optimal tables
// One workgroup per page, wave t makes table t of DC 0, AC 0, DC 1, AC 1 (a grey page: the first two; the other two come out
// empty).  Symbol s = k * 64 + lane sits in register k of its lane (huff_merge_lengths, ymk_pages.h); the reserved symbol 256 in lane 0.
// Frequencies: a symbol's count is at most the symbols of one class of a 16383 x 16383 page - the most are the chrominance's at
// 4:4:4, 2 * 2048 * 2048 blocks of at most 64 -, and so is the sum of a table's, 5.4e8: below libjpeg's 1e9 sentinel ("no
// symbol") and inside an int.  Counts from elsewhere are
// clamped to that sum's range per symbol; whatever they are, the merges build a tree, so the lengths stay below 257.
__global__ __launch_bounds__(256) void k_jpeg_optimal_tables(const int* __restrict__ blob, JpegLimits lim, int n_pages,
                                                             const int* __restrict__ hist, unsigned* __restrict__ tables,
                                                             unsigned char* __restrict__ dht) {
  __shared__ int s_key[4][256];   // code length before limiting << 9 | symbol; INT_MAX: the symbol has no code
  __shared__ int s_bits[4][260];  // codes of each length 0..256
  __shared__ int s_first[4][17], s_cum[4][18];
  __shared__ unsigned char s_seg[4][JP_SEG_BYTES + 3];
  __shared__ int s_seglen[4];
  const int t = threadIdx.x >> 6, lane = threadIdx.x & 63, page = blockIdx.x;
  JpegPage g;
  if (!jpeg_page(blob, lim, page, g)) return;  // the whole block
  const int cls = t >> 1, ac = t & 1;
  const int n = t < (g.comps == 3 ? 4 : 2) ? (ac ? 256 : 16) : 0;  // symbols this table may have
  const int* src = hist + (size_t)page * JP_LUT_WORDS + cls * (256 + 16) + (ac ? 0 : 256);
  unsigned freq[5];
  int len[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int s = k * 64 + lane;
    freq[k] = k < 4 ? (s < n ? (unsigned)min(max(src[s], 0), 0x3fffffff) : 0u) : (lane == 0 ? 1u : 0u);
  }
  huff_merge_lengths(freq, len, 256, lane);  // at most 257 live symbols
  for (int i = lane; i < 260; i += 64) s_bits[t][i] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int s = k * 64 + lane;
    if (s <= 256 && len[k] > 0) atomicAdd(&s_bits[t][min(len[k], 256)], 1);
    if (k < 4) s_key[t][s] = len[k] > 0 ? (len[k] << 9 | s) : 0x7fffffff;
  }
  __syncthreads();
  int longest = 0;
#pragma unroll
  for (int k = 0; k < 5; ++k) longest = max(longest, min(len[k], 256));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) longest = max(longest, __shfl_xor(longest, o));
  if (lane == 0) {  // tens of steps: Figure K.3, then the first code and the first place of every length
    int* bits = s_bits[t];
    huff_limit_counts(bits, longest, 16);
    int top = 16;
    while (top > 0 && bits[top] == 0) --top;
    if (top > 0) --bits[top];  // the reserved symbol's code
    int code = 0, at = 0;
    for (int l = 1; l <= 16; ++l) {
      s_first[t][l] = code, s_cum[t][l] = at;
      code = (code + bits[l]) << 1, at += bits[l];
    }
    s_cum[t][17] = at;
  }
  __syncthreads();
  const int total = min(max(s_cum[t][17], 0), n);
  unsigned* lut = tables + (size_t)page * JP_LUT_WORDS + cls * (256 + 16) + (ac ? 0 : 256);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int s = k * 64 + lane, key = s_key[t][s];
    unsigned entry = 0;
    if (key != 0x7fffffff) {
      int rank = 0;  // the symbol's place by (length before limiting, value)
      for (int o = 0; o < 256; ++o) rank += s_key[t][o] < key;
      if (rank < total) {
        const int l = huff_length_of_rank(s_cum[t], rank, 16);
        entry = (unsigned)(s_first[t][l] + rank - s_cum[t][l]) | (unsigned)l << 16;
        s_seg[t][5 + 16 + rank] = (unsigned char)s;
      }
    }
    if (s < (ac ? 256 : 16)) lut[s] = entry;
  }
  if (lane < 16) s_seg[t][5 + lane] = (unsigned char)s_bits[t][lane + 1];
  if (lane == 0) {
    const int seg = n > 0 ? 5 + 16 + total : 0;
    s_seg[t][0] = 0xff, s_seg[t][1] = 0xc4, s_seg[t][2] = (unsigned char)((seg - 2) >> 8), s_seg[t][3] = (unsigned char)((seg - 2) & 255);
    s_seg[t][4] = (unsigned char)(ac << 4 | cls);
    s_seglen[t] = seg;
  }
  __syncthreads();
  unsigned char* rec = dht + (size_t)page * JP_DHT_BYTES;
  int at = 4;
  for (int u = 0; u < t; ++u) at += s_seglen[u];
  for (int i = lane; i < s_seglen[t]; i += 64) rec[at + i] = s_seg[t][i];
  if (threadIdx.x == 0) *reinterpret_cast<int*>(rec) = s_seglen[0] + s_seglen[1] + s_seglen[2] + s_seglen[3];
}

// ------------------------------------------------------------------------------------------------ compaction
// OPT: the page's DHT record (k_jpeg_optimal_tables) stands between the header's two parts, and a block has JP_BLOCK_WORDS_OPT words
template <bool OPT>
__global__ __launch_bounds__(64) void k_jpeg_compact(const int* __restrict__ blob, JpegLimits lim, int n_pages,
                                                     const unsigned* __restrict__ stream, const int* __restrict__ intervals,
                                                     unsigned char* __restrict__ out, int* __restrict__ lengths,
                                                     const unsigned char* __restrict__ dht) {
  constexpr int BLOCK_WORDS = OPT ? JP_BLOCK_WORDS_OPT : JP_BLOCK_WORDS;
  const int lane = threadIdx.x;
  JpegPage g;
  const long long iv = blockIdx.x;
  const int p = jpeg_find(blob, lim, n_pages, iv, true, g);
  if (p < 0) return;
  const unsigned char* dht_rec = OPT ? dht + (size_t)p * JP_DHT_BYTES : nullptr;
  const int dht_len = OPT ? min(max(*reinterpret_cast<const int*>(dht_rec), 0), JP_DHT_BYTES - 4) : 0;
  const int hdr_len = g.hdr_len + dht_len;  // SOI .. SOF0, the page's tables, DRI, SOS
  const int row = (int)(iv - g.first_interval), n_iv = g.mcu_h;
  long long before = 0, total = 0;
  for (int i = lane; i < n_iv; i += 64) {
    const long long s = max(intervals[2 * (g.first_interval + i) + 1], 0);
    total += s;
    if (i < row) before += s;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    total += __shfl_xor(total, o);
    before += __shfl_xor(before, o);
  }
  const long long file_len = (long long)hdr_len + total + 2LL * (n_iv - 1) + 2;
  if (file_len > g.capacity) return;  // lengths[p] stays -1 and not a byte of the page's output is written
  unsigned char* page_out = out + g.out_off;
  const long long cap = g.capacity;
  if (row == 0) {
    const unsigned char* hdr = reinterpret_cast<const unsigned char*>(blob) + g.hdr_off;
    if (OPT) {
      for (int i = lane; i < hdr_len; i += 64)
        page_out[i] = i < g.hdr_split ? hdr[i] : (i < g.hdr_split + dht_len ? dht_rec[4 + i - g.hdr_split] : hdr[i - dht_len]);
    } else {
      for (int i = lane; i < hdr_len; i += 64) page_out[i] = hdr[i];
    }
  }
  const int nb = g.mcu_w * g.per;
  const unsigned* src = stream + (size_t)(g.first_block + (long long)row * nb) * BLOCK_WORDS;
  const int nbytes = min(max(intervals[2 * iv], 0), nb * BLOCK_WORDS * 4);
  long long pos = (long long)hdr_len + before + 2LL * row;  // where this interval starts in the file
  for (int wbase = 0; wbase * 4 < nbytes; wbase += 64) {
    const int wd = wbase + lane;
    const int valid = min(max(nbytes - wd * 4, 0), 4);
    const unsigned v = valid > 0 ? src[wd] : 0u;
    int mine = valid;
    for (int k = 0; k < valid; ++k) mine += ((v >> (24 - 8 * k)) & 255) == 255;
    const int incl = wave_inclusive_scan(mine, lane);
    long long at = pos + incl - mine;
    for (int k = 0; k < valid; ++k) {
      const unsigned char byte = (unsigned char)(v >> (24 - 8 * k));
      if (at < cap) page_out[at] = byte;  // always true when `intervals` is what k_jpeg_entropy wrote for this stream
      ++at;
      if (byte == 255) {
        if (at < cap) page_out[at] = 0;
        ++at;
      }
    }
    pos += __shfl(incl, 63);
  }
  if (lane == 0 && pos + 2 <= cap) {
    page_out[pos] = 0xff;
    page_out[pos + 1] = row + 1 < n_iv ? (unsigned char)(0xd0 + (row & 7)) : (unsigned char)0xd9;  // RSTm | EOI
    if (row + 1 == n_iv) lengths[p] = (int)file_len;
  }
}

// ------------------------------------------------------------------------------------------------ grey test
constexpr int GT_THREADS = 256, GT_GROUP = 48;  // a group: 16 pixels = three 16-byte loads
// diff[p] |= the OR over page p of (B ^ G) | (G ^ R) - zero exactly where (B ^ G) | (B ^ R) is: a page all of whose pixels have
// B == G == R.  diff is zero before the launch.  Of a record only words 0 - 4 are read (the pixels, h, w, channels); one that is
// not a three-channel page of 1..16383 pixels on a side gets -1.  The page is h * w * 3 contiguous bytes: where its address is
// 16-byte aligned a thread takes whole groups - XOR of every byte with the byte behind it, kept where the byte is a B or a G -
// and the pixels behind the last whole group (all of them where it is not aligned) go one at a time.  Every page is read to its
// end: stopping once another wave has found a difference was tried - a look at the page's word (at the L2) before each step - and
// made the launch slower on colour pages, 0.23 against 0.10 ms per wave of 16 pages.
__global__ __launch_bounds__(GT_THREADS) void k_jpeg_pages_grey(const int* __restrict__ blob, int* __restrict__ diff) {
  const int p = blockIdx.y;
  const int* r = blob + (size_t)p * JP_REC;
  const unsigned char* src = reinterpret_cast<const unsigned char*>((unsigned long long)page_word64(r, 0));
  const int h = r[2], w = r[3];
  if (src == nullptr || h < 1 || w < 1 || h > 16383 || w > 16383 || r[4] != 3) {  // the whole block
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(diff + p, -1);
    return;
  }
  const long long pixels = (long long)h * w;
  const long long groups = ((uintptr_t)src & 15) == 0 ? pixels / 16 : 0;
  const long long tid = (long long)blockIdx.x * GT_THREADS + threadIdx.x, step = (long long)gridDim.x * GT_THREADS;
  unsigned acc = 0;
  for (long long i = tid; i < groups; i += step) {
    const uint4* q = reinterpret_cast<const uint4*>(src + i * GT_GROUP);
    const uint4 a = q[0], b = q[1], c = q[2];
    const unsigned v[13] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, 0u};  // byte 47 is an R: nothing behind it is looked at
#pragma unroll
    for (int k = 0; k < 12; k += 3) {  // bytes 12 k / 4 ...: B G R B | G R B G | R B G R
      acc |= (v[k] ^ (v[k] >> 8 | v[k + 1] << 24)) & 0xff00ffffu;
      acc |= (v[k + 1] ^ (v[k + 1] >> 8 | v[k + 2] << 24)) & 0xffff00ffu;
      acc |= (v[k + 2] ^ (v[k + 2] >> 8 | v[k + 3] << 24)) & 0x00ffff00u;
    }
  }
  for (long long i = groups * 16 + tid; i < pixels; i += step) {
    const unsigned char* px = src + i * 3;
    acc |= (unsigned)((px[0] ^ px[1]) | (px[1] ^ px[2]));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc |= __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0 && acc) atomicOr(diff + p, 1);
}

// ------------------------------------------------------------------------------------------------ Pillow resample -> uint8
constexpr int RS_REC = YMK_PIL_RESIZE_U8_WORDS;
__device__ __forceinline__ int clip8_22(int v) {
  v >>= 22;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}
template <int C>
__device__ __forceinline__ void pil_resize_pixel(const unsigned char* __restrict__ src, int W, const int* xb, const int* xk, int ksx,
                                                 const int* yb, const int* yk, int ksy, int x, int y, unsigned char* __restrict__ dst) {
  const int xmin = xb[2 * x], xn = xb[2 * x + 1], ymin = yb[2 * y], yn = yb[2 * y + 1];
  const int* kx = xk + (size_t)x * ksx;
  const int* ky = yk + (size_t)y * ksy;
  int acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 1 << 21;
  for (int r = 0; r < yn; ++r) {
    const unsigned char* row = src + ((size_t)(ymin + r) * W + xmin) * C;
    int hsum[C];
#pragma unroll
    for (int c = 0; c < C; ++c) hsum[c] = 1 << 21;
    for (int t = 0; t < xn; ++t) {
      const int k = kx[t];
#pragma unroll
      for (int c = 0; c < C; ++c) hsum[c] += row[t * C + c] * k;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] += clip8_22(hsum[c]) * ky[r];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) dst[c] = (unsigned char)clip8_22(acc[c]);
}
__global__ void k_pil_resize_u8(const int* __restrict__ blob, long long blob_words) {
  const int* rec = blob + (size_t)blockIdx.z * RS_REC;
  const int H = rec[2], W = rec[3], C = rec[4], oh = rec[5], ow = rec[6], ksx = rec[7], ksy = rec[8];
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= ow || y >= oh || H < 1 || W < 1 || ksx < 1 || ksy < 1) return;
  const long long off[4] = {rec[9], rec[10], rec[11], rec[12]}, len[4] = {2LL * ow, (long long)ow * ksx, 2LL * oh, (long long)oh * ksy};
  for (int i = 0; i < 4; ++i)
    if (off[i] < 0 || off[i] + len[i] > blob_words) return;  // a table outside the blob: nothing is read through it
  const int *xb = blob + off[0], *xk = blob + off[1], *yb = blob + off[2], *yk = blob + off[3];
  // a tap outside the page is not read: the bounds are the caller's, the page's size is the record's
  if (xb[2 * x] < 0 || xb[2 * x + 1] < 0 || xb[2 * x + 1] > ksx || xb[2 * x] + xb[2 * x + 1] > W) return;
  if (yb[2 * y] < 0 || yb[2 * y + 1] < 0 || yb[2 * y + 1] > ksy || yb[2 * y] + yb[2 * y + 1] > H) return;
  const unsigned char* src = reinterpret_cast<const unsigned char*>(((unsigned long long)(unsigned)rec[1] << 32) | (unsigned)rec[0]);
  unsigned char* dst = reinterpret_cast<unsigned char*>(((unsigned long long)(unsigned)rec[14] << 32) | (unsigned)rec[13]);
  if (C == 3)
    pil_resize_pixel<3>(src, W, xb, xk, ksx, yb, yk, ksy, x, y, dst + ((size_t)y * ow + x) * 3);
  else if (C == 1)
    pil_resize_pixel<1>(src, W, xb, xk, ksx, yb, yk, ksy, x, y, dst + (size_t)y * ow + x);
}

static JpegLimits limits(int64_t blob_words, int64_t total_mcus, int64_t total_blocks, int64_t total_intervals, int64_t out_bytes) {
  YMK_CHECK(blob_words >= 0 && total_mcus >= 0 && total_blocks >= 0 && total_intervals >= 0, "bad argument");
  YMK_CHECK(total_mcus <= 0x7fffffffLL / JP_WAVES && total_blocks <= 0x7fffffffLL && total_intervals <= 0x7fffffffLL,
            "a wave of at most 2^31 - 1 blocks");
  return JpegLimits{blob_words, total_mcus, total_blocks, total_intervals, out_bytes};
}
static JpegMode checked_mode(int channels, int mode) {
  JpegMode m;
  YMK_CHECK(jpeg_mode(channels, mode, m), "mode: 0 for a one-channel page; YMK_JPEG_MODE_420 / _422 / _444 / _GREY for a three-channel one");
  return m;
}
static void check_table(const int* blob_dev, int64_t blob_words, int n_pages) {
  check_page_table(blob_dev, blob_words, n_pages, JP_REC, 15, 4096, "0..4096 pages", "page table: 16-byte aligned, n records");
}

static void launch_coefficients(hipStream_t s, const int* blob, const JpegLimits& lim, int n_pages, int16_t* coef) {
  YMK_CHECK(coef && ((uintptr_t)coef & 15) == 0, "coefficients: 16-byte aligned");
  const unsigned grid = (unsigned)((lim.total_mcus + JP_WAVES - 1) / JP_WAVES);
  hipLaunchKernelGGL(k_jpeg_coefficients, dim3(grid), dim3(JP_WAVES * 64), 0, s, blob, lim, n_pages, (short*)coef);
  YMK_HIP(hipGetLastError());
}
// tables: null = the Annex K codes; else the pages' own (k_jpeg_optimal_tables) and the larger reservation per block
static void launch_entropy(hipStream_t s, const int* blob, const JpegLimits& lim, int n_pages, const int16_t* coef, uint32_t* stream_dev,
                           int64_t stream_bytes, int* intervals, const uint32_t* tables = nullptr) {
  YMK_CHECK(coef && ((uintptr_t)coef & 15) == 0 && stream_dev && ((uintptr_t)stream_dev & 3) == 0 && intervals, "null or misaligned scratch");
  if (tables) {
    YMK_CHECK(((uintptr_t)tables & 3) == 0, "misaligned tables");
    YMK_CHECK(stream_bytes >= lim.total_blocks * YMK_JPEG_BLOCK_STREAM_BYTES_OPT, "stream scratch smaller than ymk_jpeg_scratch_bytes_opt says");
    hipLaunchKernelGGL(k_jpeg_entropy<true>, dim3((unsigned)lim.total_intervals), dim3(64), 0, s, blob, lim, n_pages, (const short*)coef,
                       (unsigned*)stream_dev, intervals, (const unsigned*)tables);
  } else {
    YMK_CHECK(stream_bytes >= lim.total_blocks * YMK_JPEG_BLOCK_STREAM_BYTES, "stream scratch smaller than ymk_jpeg_scratch_bytes says");
    hipLaunchKernelGGL(k_jpeg_entropy<false>, dim3((unsigned)lim.total_intervals), dim3(64), 0, s, blob, lim, n_pages, (const short*)coef,
                       (unsigned*)stream_dev, intervals, (const unsigned*)nullptr);
  }
  YMK_HIP(hipGetLastError());
}
// dht: null = the header is the blob's; else the pages' DHT records go into it
static void launch_compact(hipStream_t s, const int* blob, const JpegLimits& lim, int n_pages, const uint32_t* stream_dev,
                           int64_t stream_bytes, const int* intervals, unsigned char* out, int* lengths, const unsigned char* dht = nullptr) {
  YMK_CHECK(stream_dev && intervals && out && lengths && lim.out_bytes >= 0, "null scratch / output");
  YMK_CHECK(stream_bytes >= lim.total_blocks * (dht ? YMK_JPEG_BLOCK_STREAM_BYTES_OPT : YMK_JPEG_BLOCK_STREAM_BYTES),
            "stream scratch smaller than ymk_jpeg_scratch_bytes says");
  YMK_CHECK(((uintptr_t)dht & 3) == 0, "misaligned DHT records");
  YMK_HIP(hipMemsetAsync(lengths, 0xff, (size_t)n_pages * sizeof(int), s));  // -1 until a page's last interval is in place
  if (dht)
    hipLaunchKernelGGL(k_jpeg_compact<true>, dim3((unsigned)lim.total_intervals), dim3(64), 0, s, blob, lim, n_pages,
                       (const unsigned*)stream_dev, intervals, out, lengths, dht);
  else
    hipLaunchKernelGGL(k_jpeg_compact<false>, dim3((unsigned)lim.total_intervals), dim3(64), 0, s, blob, lim, n_pages,
                       (const unsigned*)stream_dev, intervals, out, lengths, (const unsigned char*)nullptr);
  YMK_HIP(hipGetLastError());
}
static void launch_histogram(hipStream_t s, const int* blob, const JpegLimits& lim, int n_pages, const int16_t* coef, int* hist) {
  YMK_CHECK(coef && ((uintptr_t)coef & 15) == 0 && hist && ((uintptr_t)hist & 3) == 0, "null or misaligned scratch");
  // on this stream, on every call: the caller's scratch holds the counts of its last wave
  YMK_HIP(hipMemsetAsync(hist, 0, (size_t)n_pages * JP_LUT_WORDS * sizeof(int), s));
  hipLaunchKernelGGL(k_jpeg_histogram, dim3((unsigned)lim.total_intervals), dim3(64), 0, s, blob, lim, n_pages, (const short*)coef, hist);
  YMK_HIP(hipGetLastError());
}
static void launch_tables(hipStream_t s, const int* blob, const JpegLimits& lim, int n_pages, const int* hist, uint32_t* tables,
                          unsigned char* dht) {
  YMK_CHECK(hist && tables && dht && (((uintptr_t)hist | (uintptr_t)tables | (uintptr_t)dht) & 3) == 0, "null or misaligned scratch");
  hipLaunchKernelGGL(k_jpeg_optimal_tables, dim3((unsigned)n_pages), dim3(256), 0, s, blob, lim, n_pages, hist, (unsigned*)tables, dht);
  YMK_HIP(hipGetLastError());
}

}  // namespace ymk

extern "C" {
int ymk_jpeg_page_words(void) { return ymk::JP_REC; }

int ymk_jpeg_quant_tables(int quality, int* zigzag128_out) {
  YMK_API_BEGIN
  YMK_CHECK(zigzag128_out, "null output");
  ymk::quant_tables(quality, zigzag128_out);
  YMK_API_END
}

int ymk_jpeg_header(int h, int w, int channels, int quality, unsigned char* out, int capacity) {
  return ymk_jpeg_header_mode(h, w, channels, 0, quality, out, capacity);
}

int ymk_jpeg_header_mode(int h, int w, int channels, int mode, int quality, unsigned char* out, int capacity) {
  YMK_API_BEGIN
  YMK_CHECK(h >= 1 && w >= 1 && h <= 16383 && w <= 16383 && (channels == 1 || channels == 3), "page: 1..16383 pixels on a side, 1 or 3 channels");
  const std::vector<unsigned char> hdr = ymk::jpeg_header(h, w, ymk::checked_mode(channels, mode), quality);
  YMK_CHECK(out && capacity >= (int)hdr.size(), "header buffer too small");
  std::memcpy(out, hdr.data(), hdr.size());
  return (int)hdr.size();
  YMK_API_END_OR(-1)
}

int ymk_jpeg_header_opt(int h, int w, int channels, int quality, unsigned char* out, int capacity, int* split_out) {
  return ymk_jpeg_header_opt_mode(h, w, channels, 0, quality, out, capacity, split_out);
}

int ymk_jpeg_header_opt_mode(int h, int w, int channels, int mode, int quality, unsigned char* out, int capacity, int* split_out) {
  YMK_API_BEGIN
  YMK_CHECK(h >= 1 && w >= 1 && h <= 16383 && w <= 16383 && (channels == 1 || channels == 3), "page: 1..16383 pixels on a side, 1 or 3 channels");
  YMK_CHECK(split_out, "null output");
  const std::vector<unsigned char> hdr = ymk::jpeg_header(h, w, ymk::checked_mode(channels, mode), quality, false, split_out);
  YMK_CHECK(out && capacity >= (int)hdr.size(), "header buffer too small");
  std::memcpy(out, hdr.data(), hdr.size());
  return (int)hdr.size();
  YMK_API_END_OR(-1)
}

int ymk_jpeg_scratch_bytes_opt(const int* h, const int* w, const int* channels, int n_pages, int64_t* sizes9_out) {
  return ymk_jpeg_scratch_bytes_opt_mode(h, w, channels, nullptr, n_pages, sizes9_out);
}

int ymk_jpeg_scratch_bytes_opt_mode(const int* h, const int* w, const int* channels, const int* modes, int n_pages, int64_t* sizes9_out) {
  YMK_API_BEGIN
  YMK_CHECK(sizes9_out, "bad argument");
  if (ymk_jpeg_scratch_bytes_mode(h, w, channels, modes, n_pages, sizes9_out)) return 1;
  sizes9_out[4] = sizes9_out[1] * YMK_JPEG_BLOCK_STREAM_BYTES_OPT;
  sizes9_out[6] = sizes9_out[7] = (int64_t)n_pages * YMK_JPEG_TABLE_WORDS * (int64_t)sizeof(int);
  sizes9_out[8] = (int64_t)n_pages * YMK_JPEG_DHT_BYTES;
  YMK_API_END
}

int ymk_jpeg_scratch_bytes(const int* h, const int* w, const int* channels, int n_pages, int64_t* sizes6_out) {
  return ymk_jpeg_scratch_bytes_mode(h, w, channels, nullptr, n_pages, sizes6_out);
}

int ymk_jpeg_scratch_bytes_mode(const int* h, const int* w, const int* channels, const int* modes, int n_pages, int64_t* sizes6_out) {
  YMK_API_BEGIN
  YMK_CHECK(n_pages >= 0 && n_pages <= 4096 && sizes6_out && (n_pages == 0 || (h && w && channels)), "bad argument");
  int64_t tiles = 0, blocks = 0, intervals = 0;
  for (int p = 0; p < n_pages; ++p) {
    YMK_CHECK(h[p] >= 1 && w[p] >= 1 && h[p] <= 16383 && w[p] <= 16383 && (channels[p] == 1 || channels[p] == 3),
              "page: 1..16383 pixels on a side, 1 or 3 channels");
    const ymk::JpegMode m = ymk::checked_mode(channels[p], modes ? modes[p] : 0);
    const int64_t mw = (w[p] + (8 << m.lh) - 1) >> (3 + m.lh), mh = (h[p] + (8 << m.lv) - 1) >> (3 + m.lv);
    tiles += (int64_t)((w[p] + (1 << m.lt) - 1) >> m.lt) * ((h[p] + (1 << m.lt) - 1) >> m.lt);
    blocks += mw * mh * (m.comps == 3 ? (1 << (m.lh + m.lv)) + 2 : 1);
    intervals += mh;
  }
  sizes6_out[0] = tiles, sizes6_out[1] = blocks, sizes6_out[2] = intervals;
  sizes6_out[3] = blocks * 64 * (int64_t)sizeof(int16_t);
  sizes6_out[4] = blocks * YMK_JPEG_BLOCK_STREAM_BYTES;
  sizes6_out[5] = intervals * 2 * (int64_t)sizeof(int);
  YMK_API_END
}

int ymk_jpeg_coefficients(const int* blob_dev, int64_t blob_words, int n_pages, int64_t total_mcus, int16_t* coef_dev,
                          int64_t total_blocks, void* stream) {
  YMK_API_BEGIN
  const ymk::JpegLimits lim = ymk::limits(blob_words, total_mcus, total_blocks, 0x7fffffffLL, -1);
  if (n_pages == 0 || total_mcus == 0) return 0;
  ymk::check_table(blob_dev, blob_words, n_pages);
  ymk::launch_coefficients((hipStream_t)stream, blob_dev, lim, n_pages, coef_dev);
  YMK_API_END
}

int ymk_jpeg_entropy(const int* blob_dev, int64_t blob_words, int n_pages, const int16_t* coef_dev, int64_t total_blocks,
                     uint32_t* stream_dev, int64_t stream_bytes, int* intervals_dev, int64_t total_intervals, void* stream) {
  YMK_API_BEGIN
  const ymk::JpegLimits lim = ymk::limits(blob_words, 0x7fffffffLL / ymk::JP_WAVES, total_blocks, total_intervals, -1);
  if (n_pages == 0 || total_intervals == 0) return 0;
  ymk::check_table(blob_dev, blob_words, n_pages);
  ymk::launch_entropy((hipStream_t)stream, blob_dev, lim, n_pages, coef_dev, stream_dev, stream_bytes, intervals_dev);
  YMK_API_END
}

int ymk_jpeg_compact(const int* blob_dev, int64_t blob_words, int n_pages, const uint32_t* stream_dev, int64_t stream_bytes,
                     int64_t total_blocks, const int* intervals_dev, int64_t total_intervals, unsigned char* out_dev, int64_t out_bytes,
                     int* lengths_dev, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(out_bytes >= 0, "bad argument");
  const ymk::JpegLimits lim = ymk::limits(blob_words, 0x7fffffffLL / ymk::JP_WAVES, total_blocks, total_intervals, out_bytes);
  if (n_pages == 0) return 0;
  ymk::check_table(blob_dev, blob_words, n_pages);
  if (total_intervals == 0) {
    YMK_CHECK(lengths_dev, "null lengths");
    YMK_HIP(hipMemsetAsync(lengths_dev, 0xff, (size_t)n_pages * sizeof(int), (hipStream_t)stream));
    return 0;
  }
  ymk::launch_compact((hipStream_t)stream, blob_dev, lim, n_pages, stream_dev, stream_bytes, intervals_dev, out_dev, lengths_dev);
  YMK_API_END
}

int ymk_jpeg_encode_pages(const int* blob_dev, int64_t blob_words, int n_pages, int64_t total_mcus, int64_t total_blocks,
                          int64_t total_intervals, int16_t* coef_dev, uint32_t* stream_dev, int64_t stream_bytes, int* intervals_dev,
                          unsigned char* out_dev, int64_t out_bytes, int* lengths_dev, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(out_bytes >= 0, "bad argument");
  const ymk::JpegLimits lim = ymk::limits(blob_words, total_mcus, total_blocks, total_intervals, out_bytes);
  if (n_pages == 0) return 0;
  ymk::check_table(blob_dev, blob_words, n_pages);
  YMK_CHECK(total_mcus > 0 && total_intervals > 0, "pages without MCUs");
  const hipStream_t s = (hipStream_t)stream;
  ymk::launch_coefficients(s, blob_dev, lim, n_pages, coef_dev);
  ymk::launch_entropy(s, blob_dev, lim, n_pages, coef_dev, stream_dev, stream_bytes, intervals_dev);
  ymk::launch_compact(s, blob_dev, lim, n_pages, stream_dev, stream_bytes, intervals_dev, out_dev, lengths_dev);
  YMK_API_END
}

int ymk_jpeg_histogram(const int* blob_dev, int64_t blob_words, int n_pages, const int16_t* coef_dev, int64_t total_blocks,
                       int64_t total_intervals, int* hist_dev, void* stream) {
  YMK_API_BEGIN
  const ymk::JpegLimits lim = ymk::limits(blob_words, 0x7fffffffLL / ymk::JP_WAVES, total_blocks, total_intervals, -1);
  if (n_pages == 0) return 0;
  ymk::check_table(blob_dev, blob_words, n_pages);
  if (total_intervals == 0) {
    YMK_CHECK(hist_dev, "null histograms");
    YMK_HIP(hipMemsetAsync(hist_dev, 0, (size_t)n_pages * ymk::JP_LUT_WORDS * sizeof(int), (hipStream_t)stream));
    return 0;
  }
  ymk::launch_histogram((hipStream_t)stream, blob_dev, lim, n_pages, coef_dev, hist_dev);
  YMK_API_END
}

int ymk_jpeg_optimal_tables(const int* blob_dev, int64_t blob_words, int n_pages, const int* hist_dev, uint32_t* tables_dev,
                            unsigned char* dht_dev, void* stream) {
  YMK_API_BEGIN
  const ymk::JpegLimits lim = ymk::limits(blob_words, 0x7fffffffLL / ymk::JP_WAVES, 0x7fffffffLL, 0x7fffffffLL, -1);
  if (n_pages == 0) return 0;
  ymk::check_table(blob_dev, blob_words, n_pages);
  ymk::launch_tables((hipStream_t)stream, blob_dev, lim, n_pages, hist_dev, tables_dev, dht_dev);
  YMK_API_END
}

int ymk_jpeg_entropy_opt(const int* blob_dev, int64_t blob_words, int n_pages, const int16_t* coef_dev, int64_t total_blocks,
                         const uint32_t* tables_dev, uint32_t* stream_dev, int64_t stream_bytes, int* intervals_dev,
                         int64_t total_intervals, void* stream) {
  YMK_API_BEGIN
  const ymk::JpegLimits lim = ymk::limits(blob_words, 0x7fffffffLL / ymk::JP_WAVES, total_blocks, total_intervals, -1);
  if (n_pages == 0 || total_intervals == 0) return 0;
  ymk::check_table(blob_dev, blob_words, n_pages);
  YMK_CHECK(tables_dev, "null tables");
  ymk::launch_entropy((hipStream_t)stream, blob_dev, lim, n_pages, coef_dev, stream_dev, stream_bytes, intervals_dev, tables_dev);
  YMK_API_END
}

int ymk_jpeg_compact_opt(const int* blob_dev, int64_t blob_words, int n_pages, const uint32_t* stream_dev, int64_t stream_bytes,
                         int64_t total_blocks, const int* intervals_dev, int64_t total_intervals, const unsigned char* dht_dev,
                         unsigned char* out_dev, int64_t out_bytes, int* lengths_dev, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(out_bytes >= 0, "bad argument");
  const ymk::JpegLimits lim = ymk::limits(blob_words, 0x7fffffffLL / ymk::JP_WAVES, total_blocks, total_intervals, out_bytes);
  if (n_pages == 0) return 0;
  ymk::check_table(blob_dev, blob_words, n_pages);
  if (total_intervals == 0) {
    YMK_CHECK(lengths_dev, "null lengths");
    YMK_HIP(hipMemsetAsync(lengths_dev, 0xff, (size_t)n_pages * sizeof(int), (hipStream_t)stream));
    return 0;
  }
  YMK_CHECK(dht_dev, "null DHT records");
  ymk::launch_compact((hipStream_t)stream, blob_dev, lim, n_pages, stream_dev, stream_bytes, intervals_dev, out_dev, lengths_dev, dht_dev);
  YMK_API_END
}

int ymk_jpeg_encode_pages_opt(const int* blob_dev, int64_t blob_words, int n_pages, int64_t total_mcus, int64_t total_blocks,
                              int64_t total_intervals, int16_t* coef_dev, int* hist_dev, uint32_t* tables_dev, unsigned char* dht_dev,
                              uint32_t* stream_dev, int64_t stream_bytes, int* intervals_dev, unsigned char* out_dev, int64_t out_bytes,
                              int* lengths_dev, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(out_bytes >= 0, "bad argument");
  const ymk::JpegLimits lim = ymk::limits(blob_words, total_mcus, total_blocks, total_intervals, out_bytes);
  if (n_pages == 0) return 0;
  ymk::check_table(blob_dev, blob_words, n_pages);
  YMK_CHECK(total_mcus > 0 && total_intervals > 0, "pages without MCUs");
  YMK_CHECK(tables_dev && dht_dev, "null scratch");
  const hipStream_t s = (hipStream_t)stream;
  ymk::launch_coefficients(s, blob_dev, lim, n_pages, coef_dev);
  ymk::launch_histogram(s, blob_dev, lim, n_pages, coef_dev, hist_dev);
  ymk::launch_tables(s, blob_dev, lim, n_pages, hist_dev, tables_dev, dht_dev);
  ymk::launch_entropy(s, blob_dev, lim, n_pages, coef_dev, stream_dev, stream_bytes, intervals_dev, tables_dev);
  ymk::launch_compact(s, blob_dev, lim, n_pages, stream_dev, stream_bytes, intervals_dev, out_dev, lengths_dev, dht_dev);
  YMK_API_END
}

int ymk_jpeg_pages_grey(const int* blob_dev, int64_t blob_words, int n_pages, int64_t max_pixels, int* diff_dev, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(max_pixels >= 0 && max_pixels <= 16383LL * 16383LL, "bad argument");
  if (n_pages == 0) return 0;
  ymk::check_table(blob_dev, blob_words, n_pages);
  YMK_CHECK(diff_dev && ((uintptr_t)diff_dev & 3) == 0, "null or misaligned output");
  const hipStream_t s = (hipStream_t)stream;
  YMK_HIP(hipMemsetAsync(diff_dev, 0, (size_t)n_pages * sizeof(int), s));
  // four groups per thread where the largest page has that many; 256 blocks per page at the most (the loops stride the rest)
  const int64_t per_block = (int64_t)ymk::GT_THREADS * 16 * 4;
  const unsigned gx = (unsigned)std::min<int64_t>(std::max<int64_t>((max_pixels + per_block - 1) / per_block, 1), 256);
  hipLaunchKernelGGL(ymk::k_jpeg_pages_grey, dim3(gx, (unsigned)n_pages), dim3(ymk::GT_THREADS), 0, s, blob_dev, diff_dev);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}

int ymk_pil_resize_u8_record_words(void) { return ymk::RS_REC; }

int ymk_pil_resize_u8(const int* blob_dev, int64_t blob_words, int n, int max_oh, int max_ow, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(n >= 0 && n <= 65535 && max_oh >= 0 && max_oh <= 65535 && max_ow >= 0, "at most 65535 images and output rows per launch");
  if (n == 0 || max_oh == 0 || max_ow == 0) return 0;
  YMK_CHECK(blob_dev && blob_words >= (int64_t)n * ymk::RS_REC, "record table");
  hipLaunchKernelGGL(ymk::k_pil_resize_u8, dim3((max_ow + 255) / 256, max_oh, n), dim3(256), 0, (hipStream_t)stream, blob_dev,
                     (long long)blob_words);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}
}
