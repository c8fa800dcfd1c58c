// The fp16-plane arithmetic of every fp16-split kernel (device side): the vector types, the power-of-two scale, the cut of
// fp32 values into a high and a low fp16 plane, and the layout of planes kept in HBM.  conv_igemm_split and the weight-panel
// splitter (ymk_conv_split.hip), conv_f16_dma, conv_f16_astat, k_vit_mlp_f16, k_flash_attn_f16 (ymk_seq.hip) and the
// plane-writing epilogue (ymk_conv_kernel.h) all cut their operands HERE, which is what lets the tests hold the convolution
// kernels to bit identity with each other: a change to the cut is a change in this file, for all of them at once.
//
// Error analysis.  An fp32 operand x is multiplied by a power of two sa (exact) and cut into
//   hi = f16(x sa)   lo = f16(x sa - hi)      round-to-nearest at both cuts
// * the subtraction is exact: hi keeps the leading 11 significand bits of x sa, so the remainder is at most half a unit of
//   hi's last place and a multiple of the unit of x's last place - at most 13 significant bits, an fp32 value;
// * lo keeps 11 bits of that remainder: hi + lo carries 22 of the 24 significand bits, |x sa - hi - lo| <= 2^-22 |x sa|;
// * a product x y is evaluated as lo_x hi_y + hi_x lo_y + hi_x hi_y - three v_mfma_f32_32x32x16_f16, smallest terms first,
//   each term exact in the MFMA's fp32 accumulator; what is dropped (lo_x lo_y and the two cut errors) is <= 2^-21 |x y|.
//   For K >= 64 the fp32 accumulation's own rounding (2^-24 of a partial sum ~sqrt(K) products large) is the larger term;
// * fp16 lacks range, not precision: sa puts max|x| of the whole operand into [2^14, 2^15), so nothing overflows (fp16
//   ends at 65504) and elements more than 2^18 below the maximum lose low-plane bits gradually (fp16 subnormals);
// * the scale comes from the biased exponent e of max|x|, clamped to 27 .. 227: sa = 2^(141 - e) and 1 / sa = 2^(e - 141) then
//   have biased exponents 41 .. 241 and 13 .. 213, i.e. both are normal, finite floats whatever the record holds - an all-zero
//   or denormal operand (e < 27) is scaled by 2^114 and stays far below 2^15; an operand beyond 2^101 would saturate the planes.
#pragma once
#include <hip/hip_runtime.h>

namespace ymk {

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));  // native vectors: stay in SSA registers
typedef float f32x16 __attribute__((ext_vector_type(16)));

// max|x| bits -> {sa, 1 / sa}, sa the power of two that puts max|x| into [2^14, 2^15); both kept normal whatever the input
__device__ __forceinline__ float2 f16_plane_scales(unsigned amax_bits) {
  int e = (int)(amax_bits >> 23);  // biased exponent, 0 .. 255
  e = e < 27 ? 27 : (e > 227 ? 227 : e);
  float2 r;
  r.x = __uint_as_float((unsigned)(268 - e) << 23);  // 2^(14 - (e - 127))
  r.y = __uint_as_float((unsigned)(e - 14) << 23);
  return r;
}

// 8 values -> hi and lo planes of 8 halves each, one MFMA operand per plane; scaled(i) = pair i of the values, times sa.
// (A callable, not an array: the front ends below differ only in how a scaled pair is formed, and each pair is formed where
// it is cut - the order the kernels' instruction schedules were measured with.)
template <class ScaledPair>
__device__ __forceinline__ void f16_split8_pairs(ScaledPair scaled, f16x8& hi, f16x8& lo) {
  f16x2 h[4], l[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f32x2 x = scaled(i);
    h[i] = __builtin_convertvector(x, f16x2);
    x -= __builtin_convertvector(h[i], f32x2);  // exact
    l[i] = __builtin_convertvector(x, f16x2);
  }
  hi = f16x8{h[0].x, h[0].y, h[1].x, h[1].y, h[2].x, h[2].y, h[3].x, h[3].y};
  lo = f16x8{l[0].x, l[0].y, l[1].x, l[1].y, l[2].x, l[2].y, l[3].x, l[3].y};
}
// 8 fp32 (u then v: two 16-byte loads), times the power of two sa
__device__ __forceinline__ void f16_split8(const f32x4 u, const f32x4 v, float sa, f16x8& hi, f16x8& lo) {
  const f32x2 x[4] = {{u.x, u.y}, {u.z, u.w}, {v.x, v.y}, {v.z, v.w}};
  f16_split8_pairs([&](int i) { return x[i] * sa; }, hi, lo);
}
// the same from 8 scalars: each multiplied on its own, then paired (the attention kernel's gathered operands)
__device__ __forceinline__ void f16_split8(const float (&v)[8], float sa, f16x8& hi, f16x8& lo) {
  f16_split8_pairs([&](int i) { return f32x2{v[2 * i] * sa, v[2 * i + 1] * sa}; }, hi, lo);
}

// 4 values ALREADY times sa, as the pairs (0, 1) and (2, 3) -> 4 high halves and 4 low halves, 8 bytes each
__device__ __forceinline__ void f16_split4(f32x2 a, f32x2 b, uint2& hi, uint2& lo) {
  const f16x2 ha = __builtin_convertvector(a, f16x2), hb = __builtin_convertvector(b, f16x2);
  a -= __builtin_convertvector(ha, f32x2);  // exact
  b -= __builtin_convertvector(hb, f32x2);
  const f16x2 la = __builtin_convertvector(a, f16x2), lb = __builtin_convertvector(b, f16x2);
  hi = make_uint2(__builtin_bit_cast(unsigned, ha), __builtin_bit_cast(unsigned, hb));
  lo = make_uint2(__builtin_bit_cast(unsigned, la), __builtin_bit_cast(unsigned, lb));
}

// one value (the weight-panel splitter)
__device__ __forceinline__ void f16_split1(float x, float sa, _Float16& hi, _Float16& lo) {
  float r = x * sa;
  hi = (_Float16)r;
  r -= (float)hi;  // exact
  lo = (_Float16)r;
}

// ---- planes in HBM (Tensor::planes): a pixel's 32-channel slice occupies the 128 bytes its 32 floats would - 32 high halves,
// then 32 low halves - so a planes tensor has the size and the pixel stride of the fp32 one
constexpr int PLANE_SLICE_LOG2 = 5;
constexpr int PLANE_SLICE_CH = 1 << PLANE_SLICE_LOG2;  // channels per slice
constexpr int PLANE_SLICE_BYTES = 4 * PLANE_SLICE_CH;  // bytes per slice
constexpr int PLANE_LO_BYTES = 2 * PLANE_SLICE_CH;     // byte offset of the low plane inside a slice
// where the high half of channel c of the pixel at `pixel` lives (its low half: + PLANE_LO_BYTES)
__device__ __forceinline__ char* plane_channel_ptr(char* pixel, int c) {
  return pixel + (size_t)(c >> PLANE_SLICE_LOG2) * PLANE_SLICE_BYTES + (size_t)(c & (PLANE_SLICE_CH - 1)) * 2;
}

}  // namespace ymk
