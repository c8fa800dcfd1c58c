// Fused PARSeq decoder step (ymk_decstep.hip).
#pragma once
#include "ymk_common.h"

namespace ymk {

// device pointers; *_t matrices are transposed nn.Linear weights: [in][out]
struct DecStepW {
  const float *emb, *posq, *qsa;
  const float *ncg, *ncb, *n1g, *n1b, *n2g, *n2b, *dng, *dnb;
  const float *Wkv_t, *bkv, *Wo1_t, *bo1, *Wq_t, *bq, *Wo2_t, *bo2, *W1_t, *b1, *W2_t, *b2;
  int D, H, F;
};

// the decoder layer's matrices as the state dict holds them (host, nn.Linear layout [out][in]): self / cross attention
// in_proj_weight [3 D][D] + in_proj_bias [3 D], the two out_proj, linear1 [F][D], linear2 [D][F]
struct DecStepHostW {
  const float *sa_in_w, *sa_in_b, *sa_out_w, *sa_out_b, *ca_in_w, *ca_in_b, *ca_out_w, *ca_out_b, *l1_w, *l1_b, *l2_w, *l2_b;
  int D, H, F;
};
// uploads the transposed copies ([in][out]) and the biases the fused step reads and fills W's matrix fields and D, H, F: the K|V
// rows of the self attention's in_proj, the query rows of the cross attention's.  The tables (emb, posq, qsa) and the LayerNorm
// vectors stay the caller's.  One function for ymk_parseq.cpp finalize and for ymk_op_parseq_dec_step.
void make_dec_step_weights(DevicePool& pool, const DecStepHostW& h, DecStepW& W);

bool parseq_dec_step_supported(int D, int H, int F, int L, int NS);
// gid / gopen (grouped forward): row b belongs to mini-batch gid[b]; gopen[step][g] = rows of g still lacking an <eos>
// after that step.  A block whose mini-batch closed at an earlier step does nothing.
// L: encoder-memory rows per sample, or - with mem_off / mem_len (device, per sample: first row, row count) - the
// longest sample of a ragged batch
void parseq_dec_step(hipStream_t s, const DecStepW& W, const int* tok, int ld_tok, int step, float* skv, int NS,
                     const float* memkv, int L, const int* mem_off, const int* mem_len, float* out, const int* prev_not_done,
                     int B, const int* gid = nullptr, const int* gopen = nullptr, int ng = 1, const int* state = nullptr);
// state (optional, the greedy kernel's [B][4] words, "retire_rows"): a row whose state[b][3] != 0 has been retired - it is
// treated as a row of a closed mini-batch is (neither skv nor out written; a block of such rows only returns)
bool decstep_debug_option(const std::string& key, int value);

}  // namespace ymk
