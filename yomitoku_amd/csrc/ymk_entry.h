// Host-side entry points behind the C ABI (ymk_api.cpp): the models' forwards, the per-launch timing spans and the debug /
// stat hooks, each declared here once and defined in the file named.  Every defining file includes this header, so a
// changed signature is a compile error, not a link that still succeeds.
#pragma once
#include "ymk_common.h"

namespace ymk {

// ymk_dbnet.cpp, ymk_parseq.cpp, ymk_rtdetr.cpp (create_dbnet: ymk_common.h)
void dbnet_forward(Model* m, const float* x, int n, int h, int w, float* prob, hipStream_t s);
Model* create_parseq();
void parseq_forward(Model* m, const float* x, int B, int W, float* logits, int* out_len, int* ar_steps, hipStream_t s);
void parseq_forward_groups(Model* m, const float* const* x, const int* b, const int* w, int ng, float* logits, int* out_len,
                           int* ar_steps, hipStream_t s);
void parseq_dims(Model* m, int* num_steps, int* num_classes);
bool parseq_debug_option(const std::string& key, int value);
bool parseq_stat(const std::string& key, long long* value);
Model* create_rtdetr();
void rtdetr_forward(Model* m, const float* x, int B, int H, int W, float* logits, float* boxes, hipStream_t s);

// ymk_conv.hip: timed spans around the convolution launches (bench.py roofline leg)
void prof_begin();
void prof_end(double* ms, double* flop, int64_t* launches);
double prof_bytes();
int64_t prof_launch_table(double* ms, double* flop, double* bytes, double* products, int64_t capacity);
bool conv_debug_option(const std::string& key, int value);

// ymk_conv_split.hip, ymk_conv_astat.hip
bool conv_split_debug_option(const std::string& key, int value);
bool conv_split_stat(const std::string& key, long long* value);
void amax_check_counters(long long* out4);
bool gemm_takes_astat(int M, int K, const ConvW& w, bool with_res, int ld);

}  // namespace ymk
