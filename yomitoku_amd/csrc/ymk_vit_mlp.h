// The launch record of the fused ViT MLP kernel (ymk_vit_mlp.hip), filled by vit_mlp_split_launch (ymk_conv_split.hip).  MlpK is
// passed BY VALUE as the kernel argument: this is its one definition.
#pragma once
#include "ymk_common.h"

namespace ymk {

struct MlpK {
  const float* x;   // [M][ld] token rows in
  float* out;       // [M][ld] out (may be x)
  int M, ld;
  const float *ln_g, *ln_b;  // [D]
  float ln_eps, ln_bound;    // LayerNorm epsilon; its static output bound (scale of the row planes)
  const uint4* w1;           // fc1 planes [F^256][KT][2][32] halves (the standard fp16 panel: rows = hidden units)
  unsigned w1_bytes;
  const float *s1, *b1;      // [F]: epilogue scale (row's power of two taken back out) and bias of fc1
  const uint4* w2;           // fc2 planes [D^256][F / 32][2][32] halves, hidden units of every 32-chunk in accumulator order
  unsigned w2_bytes;
  const float *s2, *b2;      // [D]
  float g_bound;             // bound on |GELU(fc1(..))|: scale of the hidden planes
};

// false = not a shape the kernel is built for (nothing was launched)
bool vit_mlp_f16_launch(hipStream_t s, const MlpK& k, int D, int F);

}  // namespace ymk
