// extern "C" surface of libymk_hip.so (declared in include/ymk.h).
#include "../../include/ymk.h"
#include "ymk_common.h"
#include "ymk_decstep.h"
#include "ymk_det.h"
#include "ymk_entry.h"
#include "ymk_seq.h"

struct ymk_model {
  ymk::Model* impl = nullptr;
  int device = 0;
};

// roctx ranges around the forwards and the pre-processing entry points ("rocprofv3 / roctx ranges around each
// C-ABI call"), so that a `rocprofv3 --marker-trace` timeline shows which call a kernel belongs to.  Off unless YMK_ROCTX=1: the
// library links only libamdhip64, the marker library (librocprofiler-sdk-roctx.so, else libroctx64.so) is opened at the first
// range and a box without it simply gets no ranges.
#include <dlfcn.h>
namespace {
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    const char* on = std::getenv("YMK_ROCTX");
    if (on == nullptr || on[0] == '\0' || on[0] == '0') return;
    for (const char* name : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
      if (void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) {
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (push && pop) return;
        push = nullptr;
        pop = nullptr;
      }
    }
  }
};
struct RoctxRange {
  explicit RoctxRange(const char* name) {
    static Roctx r;
    pop_ = r.pop;
    if (r.push) (void)r.push(name);
    else pop_ = nullptr;
  }
  ~RoctxRange() {
    if (pop_) (void)pop_();
  }
  int (*pop_)() = nullptr;
};
}  // namespace

extern "C" {

int ymk_version(void) { return 100; }

const char* ymk_last_error(void) { return ymk::last_error().c_str(); }

int ymk_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return -1;
  return n;
}

ymk_model* ymk_model_create(const char* kind, int device) {
  YMK_API_BEGIN
  YMK_CHECK(kind != nullptr, "kind is null");
  YMK_HIP(hipSetDevice(device));
  std::string k(kind);
  ymk::Model* impl = nullptr;
  if (k == "dbnet") impl = ymk::create_dbnet();
  else if (k == "parseq") impl = ymk::create_parseq();
  else if (k == "rtdetr") impl = ymk::create_rtdetr();
  else throw ymk::Error("unknown model kind: " + k);
  auto* m = new ymk_model();
  m->impl = impl;
  m->device = device;
  return m;
  YMK_API_END_OR(nullptr)
}

void ymk_model_destroy(ymk_model* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  delete m->impl;
  delete m;
}

int ymk_model_set_param(ymk_model* m, const char* key, double value) {
  YMK_API_BEGIN
  YMK_CHECK(m && key, "null argument");
  const std::string k(key);
  if (k == "workspace_reuse") {
    YMK_CHECK(value == 0.0 || value == 1.0 || value == -1.0, "workspace_reuse must be 0 or 1 (-1: follow the process-wide default)");
    YMK_CHECK(!ymk::in_forward(), "workspace_reuse cannot change inside a forward");
  }
  m->impl->params[key] = value;
  if (m->impl->finalized && (k == "conv_split" || k == "conv_split_encoder")) {  // a precision switched between forwards: its copies now
    YMK_HIP(hipSetDevice(m->device));
    m->impl->prebuild_split();
  }
  YMK_API_END
}

int ymk_model_set_tensor(ymk_model* m, const char* name, const float* host_data, int ndim, const int64_t* dims) {
  YMK_API_BEGIN
  YMK_CHECK(m && name && host_data && (ndim == 0 || dims), "null argument");
  YMK_CHECK(!m->impl->finalized, "model already finalized");
  m->impl->ws.put(name, host_data, ndim, dims);
  YMK_API_END
}

int ymk_model_finalize(ymk_model* m) {
  YMK_API_BEGIN
  RoctxRange roctx_range("ymk_model_finalize");
  YMK_CHECK(m, "null model");
  YMK_HIP(hipSetDevice(m->device));
  m->impl->finalize();
  // the split copies of the weight panels for the precision the model runs, and its max|x| words: built here, so that no
  // forward ever allocates, builds or waits for them (ymk_common.h: "device allocations and the forwards")
  m->impl->prebuild_split();
  // finalize() uploads the weights with synchronous copies from pageable host memory and fills a few words with hipMemset: all
  // work of the null stream, which the forwards' non-blocking streams do not order with.  Whatever the runtime's guarantee at
  // the return of such a call (staged vs. landed), after this line every byte is in place before a first forward can start
  if (!ymk::debug_hazard_no_finalize_sync()) YMK_HIP(hipDeviceSynchronize());
  YMK_API_END
}

int ymk_model_reserve(ymk_model* m, int n, int h, int w, void* stream) {
  YMK_API_BEGIN
  RoctxRange roctx_range("ymk_model_reserve");
  YMK_CHECK(m && m->impl, "null argument");
  YMK_HIP(hipSetDevice(m->device));
  m->impl->reserve(n, h, w, (hipStream_t)stream);
  YMK_API_END
}

int64_t ymk_model_weight_bytes(const ymk_model* m) { return m ? (int64_t)m->impl->pool.bytes() : -1; }
int64_t ymk_model_workspace_bytes(const ymk_model* m) { return m ? (int64_t)m->impl->arena.capacity() : -1; }

int ymk_dbnet_forward(ymk_model* m, const float* x_dev, int n, int h, int w, float* prob_dev, void* stream) {
  YMK_API_BEGIN
  RoctxRange roctx_range("ymk_dbnet_forward");
  YMK_CHECK(m && x_dev && prob_dev, "null argument");
  YMK_HIP(hipSetDevice(m->device));
  ymk::dbnet_forward(m->impl, x_dev, n, h, w, prob_dev, (hipStream_t)stream);
  YMK_API_END
}

int ymk_parseq_dims(ymk_model* m, int* num_steps, int* num_classes) {
  YMK_API_BEGIN
  YMK_CHECK(m && num_steps && num_classes, "null argument");
  ymk::parseq_dims(m->impl, num_steps, num_classes);
  YMK_API_END
}

int ymk_parseq_forward(ymk_model* m, const float* x_dev, int b, int w, float* logits_dev, int* out_len, int* ar_steps,
                       void* stream) {
  YMK_API_BEGIN
  RoctxRange roctx_range("ymk_parseq_forward");
  YMK_CHECK(m && x_dev && logits_dev && out_len && ar_steps, "null argument");
  YMK_HIP(hipSetDevice(m->device));
  ymk::parseq_forward(m->impl, x_dev, b, w, logits_dev, out_len, ar_steps, (hipStream_t)stream);
  YMK_API_END
}

int ymk_parseq_forward_groups(ymk_model* m, const float* const* x_dev, const int* b, const int* w, int n_groups,
                              float* logits_dev, int* out_len, int* ar_steps, void* stream) {
  YMK_API_BEGIN
  RoctxRange roctx_range("ymk_parseq_forward_groups");
  YMK_CHECK(m && x_dev && b && w && logits_dev && out_len && ar_steps, "null argument");
  YMK_HIP(hipSetDevice(m->device));
  ymk::parseq_forward_groups(m->impl, x_dev, b, w, n_groups, logits_dev, out_len, ar_steps, (hipStream_t)stream);
  YMK_API_END
}

int ymk_parseq_token_stats(const float* logits_dev, int rows, int num_classes, int* ids_dev, float* probs_dev,
                           void* stream) {
  YMK_API_BEGIN
  RoctxRange roctx_range("ymk_parseq_token_stats");
  YMK_CHECK(logits_dev && ids_dev && probs_dev, "null argument");
  ymk::row_maxprob((hipStream_t)stream, logits_dev, rows, num_classes, ids_dev, probs_dev);
  YMK_API_END
}

int ymk_rtdetr_forward(ymk_model* m, const float* x_dev, int b, int h, int w, float* logits_dev, float* boxes_dev,
                       void* stream) {
  YMK_API_BEGIN
  RoctxRange roctx_range("ymk_rtdetr_forward");
  YMK_CHECK(m && x_dev && logits_dev && boxes_dev, "null argument");
  YMK_HIP(hipSetDevice(m->device));
  ymk::rtdetr_forward(m->impl, x_dev, b, h, w, logits_dev, boxes_dev, (hipStream_t)stream);
  YMK_API_END
}

int ymk_debug_option(const char* key, int value) {
  YMK_API_BEGIN
  YMK_CHECK(key != nullptr, "null key");
  const std::string k(key);
  YMK_CHECK(ymk::conv_debug_option(k, value) || ymk::parseq_debug_option(k, value) || ymk::decstep_debug_option(k, value) ||
                ymk::conv_split_debug_option(k, value) || ymk::runtime_debug_option(k, value),
            "unknown debug option: " + k);
  YMK_API_END
}

int ymk_stat(const char* key, int64_t* value) {
  YMK_API_BEGIN
  YMK_CHECK(key != nullptr && value != nullptr, "null argument");
  long long v = 0;
  YMK_CHECK(ymk::conv_split_stat(std::string(key), &v) || ymk::runtime_stat(std::string(key), &v) || ymk::parseq_stat(std::string(key), &v), std::string("unknown counter: ") + key);
  *value = v;
  YMK_API_END
}

int ymk_amax_check_counters(int64_t* out4) {
  YMK_API_BEGIN
  YMK_CHECK(out4 != nullptr, "null argument");
  long long v[4];
  ymk::amax_check_counters(v);
  for (int i = 0; i < 4; ++i) out4[i] = v[i];
  YMK_API_END
}

int ymk_prof_begin(void) {
  YMK_API_BEGIN
  ymk::prof_begin();
  YMK_API_END
}

int ymk_prof_end(double* conv_ms, double* conv_flop, int64_t* conv_launches) {
  YMK_API_BEGIN
  YMK_CHECK(conv_ms && conv_flop && conv_launches, "null argument");
  ymk::prof_end(conv_ms, conv_flop, conv_launches);
  YMK_API_END
}

int ymk_prof_bytes(double* conv_bytes) {
  YMK_API_BEGIN
  YMK_CHECK(conv_bytes, "null argument");
  *conv_bytes = ymk::prof_bytes();
  YMK_API_END
}

int ymk_prof_launch_table(double* ms, double* flop, double* bytes, double* mfma_products, int64_t capacity, int64_t* count) {
  YMK_API_BEGIN
  YMK_CHECK(count != nullptr && capacity >= 0 && (capacity == 0 || (ms && flop && bytes && mfma_products)), "null argument");
  *count = ymk::prof_launch_table(ms, flop, bytes, mfma_products, capacity);
  YMK_API_END
}

// ------------------------------------------------------------------ single operators
int ymk_op_plan_workspace(int64_t n, const int64_t* sizes, const int64_t* release_pos, int64_t* offsets_out, int64_t* peak_out,
                          int64_t* live_bound_out) {
  YMK_API_BEGIN
  YMK_CHECK(n >= 0 && (n == 0 || (sizes && offsets_out)), "plan_workspace: bad argument");
  std::vector<size_t> sz((size_t)n), off((size_t)n);
  for (int64_t k = 0; k < n; ++k) {
    YMK_CHECK(sizes[k] >= 0, "plan_workspace: negative size");
    sz[(size_t)k] = (size_t)sizes[k];
  }
  size_t peak = 0, live = 0;
  ymk::plan_workspace((size_t)n, sz.data(), release_pos, off.data(), &peak, &live);
  for (int64_t k = 0; k < n; ++k) offsets_out[k] = (int64_t)off[(size_t)k];
  if (peak_out) *peak_out = (int64_t)peak;
  if (live_bound_out) *live_bound_out = (int64_t)live;
  YMK_API_END
}

int ymk_op_conv2d(const float* x_dev, int n, int h, int w, int c, const float* w_host_oihw, int cout, int cin, int kh,
                  int kw, const float* scale_host, const float* bias_host, const float* res_dev, int stride, int pad,
                  int dil, int act, int tap4, float* y_dev, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  DevicePool pool;
  ConvW cw;
  cw.cout = cout;
  cw.cin = tap4 ? 4 : cin;
  cw.kh = kh;
  cw.kw = kw;
  cw.mode = tap4 ? 1 : 0;
  std::vector<float> panel;
  pack_conv_weight(w_host_oihw, cout, cin, kh, kw, tap4 != 0, panel, cw.kpad, cw.ctiles);
  cw.w = pool.upload(panel);
  if (scale_host) cw.scale = pool.upload(scale_host, cout);
  if (bias_host) cw.bias = pool.upload(bias_host, cout);
  Tensor in{const_cast<float*>(x_dev), n, h, w, c, c};
  const int oh = conv_out_dim(h, kh, stride, pad, dil), ow = conv_out_dim(w, kw, stride, pad, dil);
  Tensor out{y_dev, n, oh, ow, cout, cout};
  Tensor res{const_cast<float*>(res_dev), n, oh, ow, cout, cout};
  ConvArgs a;
  a.stride = stride;
  a.pad = pad;
  a.dil = dil;
  a.act = act;
  a.res = res_dev ? &res : nullptr;
  SplitCtxOwner split_ctx;  // split copies of this call's panel live and die with it
  ConvSplitScope scope(-1, split_ctx.get(), 0);  // single operators: exact fp32 unless the process-wide option says otherwise
  conv2d((hipStream_t)stream, in, cw, a, out);
  YMK_HIP(hipStreamSynchronize((hipStream_t)stream));  // pool frees the panel on return
  YMK_API_END
}

// a layer of one single-operator call: the packed panel, scale / bias and the plane bound, as make_conv builds them
static ymk::ConvW op_conv_weight(ymk::DevicePool& pool, const float* w_host_oihw, int cout, int cin, int kh, int kw, bool tap4,
                                 const float* scale_host, const float* bias_host) {
  using namespace ymk;
  ConvW cw;
  cw.cout = cout;
  cw.cin = tap4 ? 4 : cin;
  cw.kh = kh;
  cw.kw = kw;
  cw.mode = tap4 ? 1 : 0;
  std::vector<float> panel;
  pack_conv_weight(w_host_oihw, cout, cin, kh, kw, tap4, panel, cw.kpad, cw.ctiles);
  cw.w = pool.upload(panel);
  std::vector<float> scale, bias;
  if (scale_host) scale.assign(scale_host, scale_host + cout);
  if (bias_host) bias.assign(bias_host, bias_host + cout);
  if (scale_host) cw.scale = pool.upload(scale);
  if (bias_host) cw.bias = pool.upload(bias);
  plane_bound(cw, w_host_oihw, (size_t)cin * kh * kw, scale, bias);
  return cw;
}

int ymk_op_conv2d_view(const float* x_dev, int n, int h, int w, int c, int in_ld, const float* w_host_oihw, int cout, int kh, int kw,
                       int tap4, const float* scale_host, const float* bias_host, const float* res_dev, int res_ld, int res_post,
                       int stride_h, int stride_w, int pad, int dil, int act, const int* row_group_dev, const int* group_open_dev,
                       const unsigned* amax_in_dev, unsigned* amax_out_dev, float* y_dev, int out_ld, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  YMK_CHECK(x_dev && w_host_oihw && y_dev, "null argument");
  YMK_CHECK(n > 0 && h > 0 && w > 0 && c > 0 && in_ld > 0 && cout > 0 && kh > 0 && kw > 0 && res_ld >= 0 && out_ld > 0 &&
                stride_h > 0 && stride_w > 0 && pad >= 0 && dil > 0,
            "conv2d_view: sizes, strides and leading dimensions are positive (res_ld may be 0)");
  hipStream_t s = (hipStream_t)stream;
  DevicePool pool;
  const ConvW cw = op_conv_weight(pool, w_host_oihw, cout, c, kh, kw, tap4 != 0, scale_host, bias_host);
  SplitCtxOwner split_ctx;
  ConvSplitScope scope(-1, split_ctx.get(), 0);  // as ymk_op_conv2d: exact fp32 unless the process-wide option says otherwise
  if (row_group_dev || group_open_dev) {
    // skipped rows exist for linear layers only, and those reach the kernels through gemm() (its row chunks included)
    YMK_CHECK(kh == 1 && kw == 1 && stride_h == 1 && stride_w == 1 && pad == 0 && !res_post && !tap4,
              "conv2d_view: a row predicate comes with a plain linear layer");
    gemm(s, x_dev, n * h * w, c, in_ld, cw, act, res_dev, res_ld, y_dev, out_ld, row_group_dev, group_open_dev, EPI_STORE, amax_in_dev,
         amax_out_dev);
  } else {
    Tensor in{const_cast<float*>(x_dev), n, h, w, c, in_ld};
    const int oh = conv_out_dim(h, kh, stride_h, pad, dil), ow = conv_out_dim(w, kw, stride_w, pad, dil);
    Tensor out{y_dev, n, oh, ow, cout, out_ld};
    Tensor res{const_cast<float*>(res_dev), n, oh, ow, cout, res_ld};
    ConvArgs a;
    a.stride = stride_h;
    a.stride_w = stride_w;
    a.pad = pad;
    a.dil = dil;
    a.act = act;
    a.res = res_dev ? &res : nullptr;
    a.res_post = res_post != 0;
    a.amax_in = amax_in_dev;
    a.amax_out = amax_out_dev;
    conv2d(s, in, cw, a, out);
  }
  YMK_HIP(hipStreamSynchronize(s));  // pool frees the panel on return
  YMK_API_END
}

int ymk_op_conv_planes_pair(const float* x_dev, int n, int h, int w, int c, const unsigned* amax_in_dev, const float* w1_host_oihw,
                            int cout1, int kh1, int kw1, int stride1, int pad1, int dil1, int act1, const float* scale1_host,
                            const float* bias1_host, const float* res1_dev, const float* w2_host_oihw, int cout2, int kh2, int kw2,
                            int stride2, int pad2, int dil2, int act2, const float* scale2_host, const float* bias2_host,
                            const float* res2_dev, float* mid_dev, unsigned* mid_amax_dev, float* y_dev, int* planes_taken,
                            float* pl_a, float* pl_b, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  YMK_CHECK(x_dev && w1_host_oihw && w2_host_oihw && mid_dev && mid_amax_dev && y_dev && planes_taken && pl_a && pl_b, "null argument");
  YMK_CHECK(n > 0 && h > 0 && w > 0 && c > 0 && cout1 > 0 && kh1 > 0 && kw1 > 0 && stride1 > 0 && pad1 >= 0 && dil1 > 0 && cout2 > 0 &&
                kh2 > 0 && kw2 > 0 && stride2 > 0 && pad2 >= 0 && dil2 > 0,
            "conv_planes_pair: sizes and strides are positive");
  hipStream_t s = (hipStream_t)stream;
  DevicePool pool;
  const ConvW c1 = op_conv_weight(pool, w1_host_oihw, cout1, c, kh1, kw1, false, scale1_host, bias1_host);
  const ConvW c2 = op_conv_weight(pool, w2_host_oihw, cout2, cout1, kh2, kw2, false, scale2_host, bias2_host);
  Tensor in{const_cast<float*>(x_dev), n, h, w, c, c};
  in.amax = const_cast<unsigned*>(amax_in_dev);
  Tensor mid{mid_dev, n, conv_out_dim(h, kh1, stride1, pad1, dil1), conv_out_dim(w, kw1, stride1, pad1, dil1), cout1, cout1};
  mid.amax = mid_amax_dev;
  Tensor out{y_dev, n, conv_out_dim(mid.h, kh2, stride2, pad2, dil2), conv_out_dim(mid.w, kw2, stride2, pad2, dil2), cout2, cout2};
  Tensor r1{const_cast<float*>(res1_dev), mid.n, mid.h, mid.w, cout1, cout1};
  Tensor r2{const_cast<float*>(res2_dev), out.n, out.h, out.w, cout2, cout2};
  ConvArgs a1, a2;
  a1.stride = stride1;
  a1.pad = pad1;
  a1.dil = dil1;
  a1.act = act1;
  a1.res = res1_dev ? &r1 : nullptr;
  a2.stride = stride2;
  a2.pad = pad2;
  a2.dil = dil2;
  a2.act = act2;
  a2.res = res2_dev ? &r2 : nullptr;
  SplitCtxOwner split_ctx;  // the fp16 planes of this call's panels live and die with it
  ConvSplitScope scope(SPLIT_F16X2, split_ctx.get(), 0);
  // as DBNetModel::bottleneck: the intermediate always has a record, and is planes where the pair qualifies
  mid.planes = conv_planes_pair_ok(in, c1, a1, c2, a2);
  a1.out_planes = mid.planes;
  YMK_HIP(hipMemsetAsync(mid_amax_dev, 0, AMAX_REC_WORDS * sizeof(unsigned), s));
  conv2d(s, in, c1, a1, mid);
  conv2d(s, mid, c2, a2, out);
  YMK_HIP(hipStreamSynchronize(s));
  *planes_taken = mid.planes ? 1 : 0;
  *pl_a = c1.pl_a;
  *pl_b = c1.pl_b;
  YMK_API_END
}

int ymk_op_conv1x1_astat(const float* x_dev, int m, int c, const float* w_host_oc, int cout, const float* scale_host,
                         const float* bias_host, const float* res_dev, int act, const float* ln_g_host, const float* ln_b_host, float ln_eps,
                         float* y_dev, int reps, float* kernel_ms, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  YMK_CHECK(x_dev && w_host_oc && y_dev && m > 0 && c > 0 && cout > 0, "bad argument");
  YMK_CHECK((ln_g_host == nullptr) == (ln_b_host == nullptr), "LayerNorm: gamma and beta come together");
  hipStream_t s = (hipStream_t)stream;
  DevicePool pool;
  ConvW cw;
  cw.cout = cout;
  cw.cin = c;
  std::vector<float> panel;
  YMK_CHECK(c % 4 == 0, "astat: channels must be a multiple of 4");
  pack_conv_weight(w_host_oc, cout, c, 1, 1, false, panel, cw.kpad, cw.ctiles);
  YMK_CHECK(cw.kpad <= 256, "astat: K <= 256");
  cw.w = pool.upload(panel);
  if (scale_host) cw.scale = pool.upload(scale_host, cout);
  if (bias_host) cw.bias = pool.upload(bias_host, cout);
  // the input's max|x| record: measured - or, in front of a fused LayerNorm, the static bound of its output, as the models do
  unsigned* rec = nullptr;
  const float *g_dev = nullptr, *b_dev = nullptr;
  if (ln_g_host) {
    const std::vector<float> g(ln_g_host, ln_g_host + c), b(ln_b_host, ln_b_host + c);
    g_dev = pool.upload(g);
    b_dev = pool.upload(b);
    rec = make_layernorm_amax_record(pool, g, b);
  } else {
    rec = reinterpret_cast<unsigned*>(pool.alloc(AMAX_REC_WORDS));
    YMK_HIP(hipMemsetAsync(rec, 0, AMAX_REC_WORDS * sizeof(unsigned), s));
    absmax_record(s, x_dev, (size_t)m * c, rec);
  }
  struct Events {  // freed on every way out (a failing HIP call throws)
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() {
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
    }
  } ev;
  YMK_HIP(hipEventCreate(&ev.e0));
  YMK_HIP(hipEventCreate(&ev.e1));
  SplitCtxOwner split_ctx;  // the fp16 planes of this call's panel live and die with it
  ConvSplitScope scope(SPLIT_F16X2, split_ctx.get(), 0);
  ConvSplitTileScope tile_scope(30);  // the A-stationary kernel for whatever it can run - this thread's launches only
  for (int r = 0; r < std::max(1, reps); ++r) {
    if (r == std::max(1, reps) - 1) YMK_HIP(hipEventRecord(ev.e0, s));
    if (ln_g_host) {
      YMK_CHECK(gemm_ln_fused(s, x_dev, m, c, c, g_dev, b_dev, ln_eps, cw, act, res_dev, cout, y_dev, cout, rec),
                "astat: this launch cannot carry a fused LayerNorm (C must be 128 or 192)");
    } else {
      YMK_CHECK(gemm_takes_astat(m, c, cw, res_dev != nullptr, cout), "astat: not a launch the A-stationary kernel runs");
      gemm(s, x_dev, m, c, c, cw, act, res_dev, cout, y_dev, cout, nullptr, nullptr, EPI_STORE, rec);
    }
    if (r == std::max(1, reps) - 1) YMK_HIP(hipEventRecord(ev.e1, s));
  }
  YMK_HIP(hipStreamSynchronize(s));
  float ms = 0.f;
  YMK_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  if (kernel_ms) *kernel_ms = ms;
  YMK_API_END
}

int ymk_op_vit_mlp(const float* x_dev, int m, int d, int f, const float* ln_g_host, const float* ln_b_host, float ln_eps,
                   const float* w1_host_fd, const float* b1_host, const float* w2_host_df, const float* b2_host, float* y_dev, int reps,
                   float* kernel_ms, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  YMK_CHECK(x_dev && y_dev && ln_g_host && ln_b_host && w1_host_fd && b1_host && w2_host_df && b2_host && m > 0, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  DevicePool pool;
  const std::vector<float> g(ln_g_host, ln_g_host + d), b(ln_b_host, ln_b_host + d);
  const float* g_dev = pool.upload(g);
  const float* b_dev = pool.upload(b);
  ConvW fc1 = make_linear_raw(pool, w1_host_fd, b1_host, f, d), fc2 = make_linear_raw(pool, w2_host_df, b2_host, d, f);
  struct Events {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() {
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
    }
  } ev;
  YMK_HIP(hipEventCreate(&ev.e0));
  YMK_HIP(hipEventCreate(&ev.e1));
  SplitCtxOwner split_ctx;
  ConvSplitScope scope(SPLIT_F16X2, split_ctx.get(), 0);
  YMK_HIP(hipMemcpyAsync(y_dev, x_dev, (size_t)m * d * sizeof(float), hipMemcpyDeviceToDevice, s));
  for (int r = 0; r < std::max(1, reps); ++r) {  // in place on y: repetitions (timing) keep transforming it
    if (r == std::max(1, reps) - 1) YMK_HIP(hipEventRecord(ev.e0, s));
    YMK_CHECK(vit_mlp_fused(s, y_dev, m, d, g_dev, b_dev, ln_eps, layernorm_output_bound(g, b), fc1, fc2),
              "the fused ViT MLP runs D = 192, F = 768 and at least 256 blocks of 128 rows");
    if (r == std::max(1, reps) - 1) YMK_HIP(hipEventRecord(ev.e1, s));
  }
  YMK_HIP(hipStreamSynchronize(s));
  float ms = 0.f;
  YMK_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  if (kernel_ms) *kernel_ms = ms;
  YMK_API_END
}

int ymk_op_layernorm(const float* x_dev, int rows, int d, const float* g_dev, const float* b_dev, float eps,
                     float* y_dev, void* stream) {
  YMK_API_BEGIN
  ymk::layernorm((hipStream_t)stream, x_dev, d, 0, g_dev, b_dev, eps, y_dev, d, rows, d);
  YMK_API_END
}

int ymk_op_attention(const float* q_dev, const float* k_dev, const float* v_dev, float* o_dev, int b, int heads, int lq,
                     int lk, int hd, float scale, const unsigned char* mask_qk_dev, const unsigned char* kpm_dev,
                     int use_small, void* stream) {
  YMK_API_BEGIN
  const int D = heads * hd;
  if (use_small || mask_qk_dev || kpm_dev)
    ymk::small_attention((hipStream_t)stream, q_dev, k_dev, v_dev, o_dev, b, heads, lq, lk, hd, D, D, D, D, (long)lq * D,
                         (long)lk * D, (long)lk * D, (long)lq * D, scale, mask_qk_dev, lk, kpm_dev, lk);
  else if (ymk::conv_effective_split() == ymk::SPLIT_F16X2) {
    // ymk_debug_option("conv_split", 16): the fp16-split form, its three max|x| records measured here (tests)
    unsigned* rec = (unsigned*)ymk::dev_malloc(3 * ymk::AMAX_REC_WORDS * sizeof(unsigned));
    YMK_HIP(hipMemsetAsync(rec, 0, 3 * ymk::AMAX_REC_WORDS * sizeof(unsigned), (hipStream_t)stream));
    ymk::absmax_record((hipStream_t)stream, q_dev, (size_t)b * lq * D, rec);
    ymk::absmax_record((hipStream_t)stream, k_dev, (size_t)b * lk * D, rec + ymk::AMAX_REC_WORDS);
    ymk::absmax_record((hipStream_t)stream, v_dev, (size_t)b * lk * D, rec + 2 * ymk::AMAX_REC_WORDS);
    ymk::flash_attention((hipStream_t)stream, q_dev, k_dev, v_dev, o_dev, b, heads, lq, lk, hd, D, D, D, D, (long)lq * D,
                         (long)lk * D, (long)lk * D, (long)lq * D, scale, nullptr, rec, rec + ymk::AMAX_REC_WORDS, rec + 2 * ymk::AMAX_REC_WORDS);
    YMK_HIP(hipStreamSynchronize((hipStream_t)stream));
    ymk::dev_free(rec);
  } else
    ymk::flash_attention((hipStream_t)stream, q_dev, k_dev, v_dev, o_dev, b, heads, lq, lk, hd, D, D, D, D, (long)lq * D,
                         (long)lk * D, (long)lk * D, (long)lq * D, scale);
  YMK_API_END
}

int ymk_op_nar_cross_attention(const float* q_dev, const float* k_dev, const float* v_dev, float* o_dev, int b, int heads, int lq,
                               int lk, int hd, float scale, const int* koff_dev, const int* klen_dev, void* stream) {
  YMK_API_BEGIN
  const int D = heads * hd;
  YMK_CHECK((koff_dev == nullptr) == (klen_dev == nullptr), "offset and length tables come in pairs");
  ymk::SeqTab tab;
  tab.koff = koff_dev;
  tab.klen = klen_dev;
  ymk::nar_cross_attention((hipStream_t)stream, q_dev, k_dev, v_dev, o_dev, b, heads, lq, lk, hd, D, D, D, D, (long)lk * D, (long)lk * D,
                           (long)lq * D, scale, koff_dev ? &tab : nullptr);
  YMK_API_END
}

int ymk_op_layernorm_view(const float* x_dev, int ldx, int in_rows_mod, int rows, int d, const float* g_dev, const float* b_dev,
                          float eps, float* y_dev, int ldy, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(x_dev && g_dev && b_dev && y_dev, "null argument");
  YMK_CHECK(rows >= 0 && d > 0 && ldx >= d && ldy >= d && in_rows_mod >= 0, "layernorm_view: rows of at least d floats, in_rows_mod >= 0");
  ymk::layernorm((hipStream_t)stream, x_dev, ldx, in_rows_mod, g_dev, b_dev, eps, y_dev, ldy, rows, d);
  YMK_API_END
}

int ymk_op_attention_view(int kernel, const float* q_dev, const float* k_dev, const float* v_dev, float* o_dev, int b, int heads, int lq,
                          int lk, int hd, float scale, int ldq, int ldk, int ldv, int ldo, int64_t bsq, int64_t bsk, int64_t bsv,
                          int64_t bso, const unsigned char* mask_qk_dev, int ld_mask, const unsigned char* kpm_dev, int ld_kpm,
                          const int* qoff_dev, const int* qlen_dev, const int* koff_dev, const int* klen_dev,
                          const unsigned* amax_q_dev, const unsigned* amax_k_dev, const unsigned* amax_v_dev, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  YMK_CHECK(q_dev && k_dev && v_dev && o_dev, "null argument");
  YMK_CHECK(kernel >= 0 && kernel <= 2, "attention_view: kernel is 0 (flash), 1 (small) or 2 (nar cross)");
  YMK_CHECK((qoff_dev == nullptr) == (qlen_dev == nullptr) && (koff_dev == nullptr) == (klen_dev == nullptr),
            "offset and length tables come in pairs");
  YMK_CHECK(kernel == 1 || (!mask_qk_dev && !kpm_dev), "attention_view: masks come with the small kernel");
  YMK_CHECK(kernel != 2 || (!qoff_dev && bsq == 0), "attention_view: the nar kernel has one query table and no query batch stride");
  hipStream_t s = (hipStream_t)stream;
  SeqTab tab;
  tab.qoff = qoff_dev;
  tab.qlen = qlen_dev;
  tab.koff = koff_dev;
  tab.klen = klen_dev;
  const SeqTab* tp = (qoff_dev || koff_dev) ? &tab : nullptr;
  if (kernel == 0)
    flash_attention(s, q_dev, k_dev, v_dev, o_dev, b, heads, lq, lk, hd, ldq, ldk, ldv, ldo, (long)bsq, (long)bsk, (long)bsv, (long)bso, scale,
                    tp, amax_q_dev, amax_k_dev, amax_v_dev);
  else if (kernel == 1)
    small_attention(s, q_dev, k_dev, v_dev, o_dev, b, heads, lq, lk, hd, ldq, ldk, ldv, ldo, (long)bsq, (long)bsk, (long)bsv, (long)bso, scale,
                    mask_qk_dev, ld_mask, kpm_dev, ld_kpm, tp);
  else
    nar_cross_attention(s, q_dev, k_dev, v_dev, o_dev, b, heads, lq, lk, hd, ldq, ldk, ldv, ldo, (long)bsk, (long)bsv, (long)bso, scale, tp);
  YMK_API_END
}

int ymk_op_maxpool3x3s2(const float* x_dev, int n, int h, int w, int c, float* y_dev, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  Tensor in{const_cast<float*>(x_dev), n, h, w, c, c};
  Tensor out{y_dev, n, (h + 2 - 3) / 2 + 1, (w + 2 - 3) / 2 + 1, c, c};
  maxpool3x3s2((hipStream_t)stream, in, out);
  YMK_API_END
}

int ymk_op_upsample_bilinear(const float* x_dev, int n, int h, int w, int c, int oh, int ow, const float* add_dev,
                             float* y_dev, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  Tensor in{const_cast<float*>(x_dev), n, h, w, c, c};
  Tensor out{y_dev, n, oh, ow, c, c};
  Tensor add{const_cast<float*>(add_dev), n, oh, ow, c, c};
  upsample_bilinear((hipStream_t)stream, in, out, add_dev ? &add : nullptr);
  YMK_API_END
}

// ---- single operators of the detection transformer and of the DBNet++ head (the launch functions the models call)
namespace {
// level_hw = {h0, w0, h1, w1, h2, w2} (host) -> the geometry ymk_rtdetr.cpp builds for B images
ymk::DetGeom det_geom_arg(int b, const int* level_hw) {
  YMK_CHECK(level_hw != nullptr && b >= 1, "det op: b >= 1 and a level_hw array");
  const int h[3] = {level_hw[0], level_hw[2], level_hw[4]}, w[3] = {level_hw[1], level_hw[3], level_hw[5]};
  long ntok = 0;
  for (int l = 0; l < 3; ++l) {
    YMK_CHECK(h[l] >= 1 && w[l] >= 1, "det op: every level needs at least one token");
    ntok += (long)h[l] * w[l];
  }
  YMK_CHECK((long)b * ntok < (1L << 30), "det op: too many tokens");
  return ymk::make_det_geom(b, h, w);
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

int ymk_op_topk_tokens(const float* logits_dev, int b, const int* level_hw, int nc, int k, int* idx_dev, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  const DetGeom g = det_geom_arg(b, level_hw);
  YMK_CHECK(logits_dev && idx_dev && nc >= 1, "topk: bad argument");
  YMK_CHECK(k >= 1 && k <= 2048 && k <= g.ntok, "topk: 1 <= k <= min(2048, tokens)");
  hipStream_t s = (hipStream_t)stream;
  DevicePool pool;  // the b * ntok key words
  unsigned* keys = reinterpret_cast<unsigned*>(pool.alloc((size_t)g.B * g.ntok));
  topk_tokens(s, logits_dev, nc, g, k, keys, idx_dev);
  YMK_HIP(hipStreamSynchronize(s));  // pool frees the keys on return
  YMK_API_END
}

int ymk_op_gather_queries(const float* om_dev, const float* bbox_dev, const float* anchors_dev, const int* idx_dev, int b,
                          const int* level_hw, int k, int d, float* content_dev, float* ref_dev, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  const DetGeom g = det_geom_arg(b, level_hw);
  YMK_CHECK(om_dev && bbox_dev && anchors_dev && idx_dev && content_dev && ref_dev && k >= 1 && d >= 1, "gather: bad argument");
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> idx((size_t)b * k);  // the kernel trusts its indices: a test entry point checks them first
  YMK_HIP(hipMemcpyAsync(idx.data(), idx_dev, idx.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  YMK_HIP(hipStreamSynchronize(s));
  for (int v : idx) YMK_CHECK(v >= 0 && v < g.ntok, "gather: token index out of range");
  gather_queries(s, om_dev, bbox_dev, anchors_dev, idx_dev, g, k, d, content_dev, ref_dev);
  YMK_API_END
}

int ymk_op_refine_boxes(const float* delta_dev, const float* ref_dev, float* out_dev, int64_t n, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(delta_dev && ref_dev && out_dev && n >= 0, "refine: bad argument");
  ymk::refine_boxes((hipStream_t)stream, delta_dev, ref_dev, out_dev, (size_t)n);
  YMK_API_END
}

int ymk_op_mask_rows(const float* in_dev, const float* valid_dev, int b, const int* level_hw, int d, float* out_dev, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  const DetGeom g = det_geom_arg(b, level_hw);
  YMK_CHECK(in_dev && valid_dev && out_dev && d >= 4 && d % 4 == 0, "mask_rows: d must be a positive multiple of 4");
  YMK_CHECK(aligned16(in_dev) && aligned16(out_dev), "mask_rows: rows must be 16 B aligned");
  mask_rows((hipStream_t)stream, in_dev, valid_dev, out_dev, g, d);
  YMK_API_END
}

int ymk_op_deform_sample(const float* offs_dev, const float* attw_dev, const float* ref_dev, const float* value_dev, int ldv, int b,
                         const int* level_hw, int k, float* out_dev, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  const DetGeom g = det_geom_arg(b, level_hw);
  YMK_CHECK(offs_dev && attw_dev && ref_dev && value_dev && out_dev && k >= 1, "deform_sample: bad argument");
  // 8 heads x 32 channels per value row, read as float4; ref rows and output rows as float4
  YMK_CHECK(ldv >= 256 && ldv % 4 == 0, "deform_sample: ldv >= 256, a multiple of 4");
  YMK_CHECK(aligned16(value_dev) && aligned16(ref_dev) && aligned16(out_dev), "deform_sample: value / ref / out must be 16 B aligned");
  deform_sample((hipStream_t)stream, offs_dev, attw_dev, ref_dev, value_dev, ldv, g, k, out_dev);
  YMK_API_END
}

int ymk_op_avgpool2x2_ceil(const float* x_dev, int n, int h, int w, int c, float* y_dev, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  YMK_CHECK(x_dev && y_dev && n >= 1 && h >= 1 && w >= 1 && c >= 4 && c % 4 == 0, "avgpool: c must be a positive multiple of 4");
  Tensor in{const_cast<float*>(x_dev), n, h, w, c, c};
  Tensor out{y_dev, n, (h + 1) / 2, (w + 1) / 2, c, c};
  avgpool2x2_ceil((hipStream_t)stream, in, out);
  YMK_API_END
}

int ymk_op_upsample_nearest2x(const float* x_dev, int n, int h, int w, int c, float* y_dev, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  YMK_CHECK(x_dev && y_dev && n >= 1 && h >= 1 && w >= 1 && c >= 4 && c % 4 == 0, "nearest2x: c must be a positive multiple of 4");
  Tensor in{const_cast<float*>(x_dev), n, h, w, c, c};
  Tensor out{y_dev, n, 2 * h, 2 * w, c, c};
  upsample_nearest2x((hipStream_t)stream, in, out);
  YMK_API_END
}

// ---- the NHWC glue kernels and the max|x| passes in the forms the models launch them (tests/test_glue_views_gpu.py): the
// caller's leading dimensions into the launch functions the models call; nothing allocated, nothing waited for
namespace {
// what every kernel of ymk_elem.hip trusts of a view, said once more here so that a test gets the message of the entry it called
void glue_view_arg(const char* op, const char* what, const float* p, int c, int ld) {
  const std::string at = std::string(op) + ": " + what;
  YMK_CHECK(p != nullptr, at + " is null");
  YMK_CHECK(c >= 4 && c % 4 == 0, at + ": c must be a positive multiple of 4");
  YMK_CHECK(ld % 4 == 0 && ld >= c, at + ": ld must be a multiple of 4, at least c");
  YMK_CHECK(aligned16(p), at + " must be 16 B aligned");
}
ymk::Tensor glue_tensor(const float* p, int n, int h, int w, int c, int ld) {
  ymk::Tensor t;
  t.p = const_cast<float*>(p);
  t.n = n;
  t.h = h;
  t.w = w;
  t.c = c;
  t.ld = ld;
  return t;
}
}  // namespace

int ymk_op_maxpool3x3s2_view(const float* x_dev, int n, int h, int w, int c, int in_ld, float* y_dev, int out_ld, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  YMK_CHECK(n >= 1 && h >= 1 && w >= 1, "maxpool_view: n, h, w >= 1");
  glue_view_arg("maxpool_view", "x", x_dev, c, in_ld);
  glue_view_arg("maxpool_view", "y", y_dev, c, out_ld);
  maxpool3x3s2((hipStream_t)stream, glue_tensor(x_dev, n, h, w, c, in_ld), glue_tensor(y_dev, n, (h - 1) / 2 + 1, (w - 1) / 2 + 1, c, out_ld));
  YMK_API_END
}

int ymk_op_avgpool2x2_ceil_view(const float* x_dev, int n, int h, int w, int c, int in_ld, float* y_dev, int out_ld, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  YMK_CHECK(n >= 1 && h >= 1 && w >= 1, "avgpool_view: n, h, w >= 1");
  glue_view_arg("avgpool_view", "x", x_dev, c, in_ld);
  glue_view_arg("avgpool_view", "y", y_dev, c, out_ld);
  avgpool2x2_ceil((hipStream_t)stream, glue_tensor(x_dev, n, h, w, c, in_ld), glue_tensor(y_dev, n, (h + 1) / 2, (w + 1) / 2, c, out_ld));
  YMK_API_END
}

int ymk_op_upsample_nearest2x_view(const float* x_dev, int n, int h, int w, int c, int in_ld, float* y_dev, int out_ld, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  YMK_CHECK(n >= 1 && h >= 1 && w >= 1, "nearest2x_view: n, h, w >= 1");
  glue_view_arg("nearest2x_view", "x", x_dev, c, in_ld);
  glue_view_arg("nearest2x_view", "y", y_dev, c, out_ld);
  upsample_nearest2x((hipStream_t)stream, glue_tensor(x_dev, n, h, w, c, in_ld), glue_tensor(y_dev, n, 2 * h, 2 * w, c, out_ld));
  YMK_API_END
}

int ymk_op_upsample_bilinear_view(const float* x_dev, int n, int h, int w, int c, int in_ld, int oh, int ow, const float* add_dev,
                                  int add_ld, float* y_dev, int out_ld, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  YMK_CHECK(n >= 1 && h >= 1 && w >= 1 && oh >= 1 && ow >= 1, "bilinear_view: n, h, w, oh, ow >= 1");
  glue_view_arg("bilinear_view", "x", x_dev, c, in_ld);
  glue_view_arg("bilinear_view", "y", y_dev, c, out_ld);
  if (add_dev) glue_view_arg("bilinear_view", "add", add_dev, c, add_ld);
  const Tensor add = glue_tensor(add_dev, n, oh, ow, c, add_ld);
  upsample_bilinear((hipStream_t)stream, glue_tensor(x_dev, n, h, w, c, in_ld), glue_tensor(y_dev, n, oh, ow, c, out_ld), add_dev ? &add : nullptr);
  YMK_API_END
}

int ymk_op_nchw3_to_nhwc4(const float* x_nchw_dev, int n, int h, int w, float* y_dev, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  YMK_CHECK(x_nchw_dev && y_dev && n >= 1 && h >= 1 && w >= 1, "nchw3_to_nhwc4: null argument or an empty image");
  YMK_CHECK(aligned16(y_dev), "nchw3_to_nhwc4: y must be 16 B aligned");
  nchw3_to_nhwc4((hipStream_t)stream, x_nchw_dev, n, h, w, glue_tensor(y_dev, n, h, w, 4, 4));
  YMK_API_END
}

int ymk_op_add_bcast(const float* a_dev, const float* b_dev, int rows_mod, int m, int d, float* out_dev, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(a_dev && b_dev && out_dev, "add_bcast: null argument");
  YMK_CHECK(m >= 1 && rows_mod >= 1 && d >= 4 && d % 4 == 0, "add_bcast: m, rows_mod >= 1, d a positive multiple of 4");
  YMK_CHECK(aligned16(a_dev) && aligned16(b_dev) && aligned16(out_dev), "add_bcast: rows must be 16 B aligned");
  ymk::add_bcast((hipStream_t)stream, a_dev, b_dev, rows_mod, out_dev, m, d);
  YMK_API_END
}

int ymk_op_absmax(const float* x_dev, int64_t pixels, int c, int ld, unsigned* slot_dev, unsigned* next_dev, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(slot_dev && next_dev && pixels >= 1, "absmax: null record or no pixels");
  glue_view_arg("absmax", "x", x_dev, c, ld);
  ymk::absmax_launch((hipStream_t)stream, x_dev, (size_t)pixels, c, ld, slot_dev, next_dev);
  YMK_HIP(hipGetLastError());
  YMK_API_END
}

int ymk_op_amax_merge(unsigned* dst_dev, const unsigned* src_dev, void* stream) {
  YMK_API_BEGIN
  ymk::amax_merge((hipStream_t)stream, dst_dev, src_dev);  // a null record is "no record": nothing is launched
  YMK_API_END
}

int ymk_op_deconv2x2(const float* x_dev, int n, int h, int w, int cin, const float* w_host, int cout, const float* scale_host,
                     const float* bias_host, int act, float* y_dev, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  YMK_CHECK(x_dev && w_host && y_dev && n >= 1 && h >= 1 && w >= 1, "deconv2x2: bad argument");
  YMK_CHECK(cin >= 4 && cin % 4 == 0 && cout >= 4 && cout % 4 == 0, "deconv2x2: cin and cout must be positive multiples of 4");
  DevicePool pool;
  const ConvW cw = make_deconv2x2_panel(pool, w_host, cin, cout, scale_host, bias_host);
  Tensor in{const_cast<float*>(x_dev), n, h, w, cin, cin};
  Tensor out{y_dev, n, 2 * h, 2 * w, cout, cout};
  ConvArgs a;
  a.act = act;
  a.epi = EPI_DECONV2X2;
  SplitCtxOwner split_ctx;  // as ymk_op_conv2d: exact fp32 unless the process-wide option says otherwise
  ConvSplitScope scope(-1, split_ctx.get(), 0);
  conv2d((hipStream_t)stream, in, cw, a, out);
  YMK_HIP(hipStreamSynchronize((hipStream_t)stream));  // pool frees the panel on return
  YMK_API_END
}

int ymk_op_deconv2x2_to1_sigmoid(const float* x_dev, int n, int h, int w, const float* w_host, float bias, float* y_dev,
                                 void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  YMK_CHECK(x_dev && w_host && y_dev && n >= 1 && h >= 1 && w >= 1, "deconv_to1: bad argument");
  YMK_CHECK(aligned16(x_dev), "deconv_to1: input must be 16 B aligned");
  DevicePool pool;
  const float* wd = pool.upload(w_host, 64 * 4);
  Tensor in{const_cast<float*>(x_dev), n, h, w, 64, 64};
  deconv2x2_to1_sigmoid((hipStream_t)stream, in, wd, bias, y_dev);
  YMK_HIP(hipStreamSynchronize((hipStream_t)stream));  // pool frees the weights on return
  YMK_API_END
}

int ymk_op_dbnet_asf(const float* ax_dev, const float* fuse_dev, int n, int h, int w, const float* w1_host, const float* w2_host,
                     int cmid, const float* sp33_host, float sp11, const float* watt_host, float* out_dev, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  YMK_CHECK(ax_dev && fuse_dev && out_dev && w1_host && w2_host && sp33_host && watt_host && n >= 1 && h >= 1 && w >= 1,
            "asf: bad argument");
  YMK_CHECK(cmid >= 1 && cmid <= 64, "asf: 1 <= cmid <= 64");
  YMK_CHECK(aligned16(ax_dev) && aligned16(fuse_dev) && aligned16(out_dev), "asf: tensors must be 16 B aligned");
  hipStream_t s = (hipStream_t)stream;
  DevicePool pool;
  const float* w1 = pool.upload(w1_host, (size_t)cmid * 64);
  const float* w2 = pool.upload(w2_host, (size_t)64 * cmid);
  const float* sp33 = pool.upload(sp33_host, 9);
  const float* watt = pool.upload(watt_host, 4 * 64);
  float* gap_scr = pool.alloc((size_t)GAP_CHUNKS * n * 64);
  float* gap = pool.alloc((size_t)n * 64);
  float* gate = pool.alloc((size_t)n * 64);
  float* cmean = pool.alloc((size_t)n * h * w);
  Tensor x{const_cast<float*>(ax_dev), n, h, w, 64, 64};
  Tensor fuse{const_cast<float*>(fuse_dev), n, h, w, 256, 256};
  Tensor out{out_dev, n, h, w, 256, 256};
  asf_block(s, x, w1, w2, cmid, sp33, sp11, watt, fuse, gap_scr, gap, gate, cmean, out);
  YMK_HIP(hipStreamSynchronize(s));  // pool frees weights and scratch on return
  YMK_API_END
}

// ---- single operators of the PARSeq greedy decode (the launch functions ymk_parseq.cpp calls)
int ymk_op_parseq_dec_step(int d, int heads, int f, const float* sa_in_w_host, const float* sa_in_b_host, const float* sa_out_w_host,
                           const float* sa_out_b_host, const float* ca_in_w_host, const float* ca_in_b_host,
                           const float* ca_out_w_host, const float* ca_out_b_host, const float* lin1_w_host, const float* lin1_b_host,
                           const float* lin2_w_host, const float* lin2_b_host, const float* const* ln_host, const float* emb_host,
                           int ntok, const float* posq_host, const float* qsa_host, const int* tok_dev, float* skv_dev,
                           const float* memkv_dev, const int* mem_off_dev, const int* mem_len_dev, const int* prev_not_done_dev,
                           const int* gid_dev, const int* gopen_dev, int ng, int step, int b, int l, int ns, float* out_dev,
                           void* stream) {
  return ymk_op_parseq_dec_step_state(d, heads, f, sa_in_w_host, sa_in_b_host, sa_out_w_host, sa_out_b_host, ca_in_w_host, ca_in_b_host,
                                      ca_out_w_host, ca_out_b_host, lin1_w_host, lin1_b_host, lin2_w_host, lin2_b_host, ln_host, emb_host,
                                      ntok, posq_host, qsa_host, tok_dev, skv_dev, memkv_dev, mem_off_dev, mem_len_dev, prev_not_done_dev,
                                      gid_dev, gopen_dev, ng, /*state_dev=*/nullptr, step, b, l, ns, out_dev, stream);
}

int ymk_op_parseq_dec_step_state(int d, int heads, int f, const float* sa_in_w_host, const float* sa_in_b_host,
                                 const float* sa_out_w_host, const float* sa_out_b_host, const float* ca_in_w_host,
                                 const float* ca_in_b_host, const float* ca_out_w_host, const float* ca_out_b_host,
                                 const float* lin1_w_host, const float* lin1_b_host, const float* lin2_w_host, const float* lin2_b_host,
                                 const float* const* ln_host, const float* emb_host, int ntok, const float* posq_host,
                                 const float* qsa_host, const int* tok_dev, float* skv_dev, const float* memkv_dev,
                                 const int* mem_off_dev, const int* mem_len_dev, const int* prev_not_done_dev, const int* gid_dev,
                                 const int* gopen_dev, int ng, const int* state_dev, int step, int b, int l, int ns, float* out_dev,
                                 void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  // refused before anything is uploaded or launched (parseq_dec_step checks again)
  YMK_CHECK(d >= 4 && heads >= 1 && f >= 4 && l >= 1 && ns >= 1 && parseq_dec_step_supported(d, heads, f, l, ns),
            "fused decoder step: unsupported geometry");
  YMK_CHECK(sa_in_w_host && sa_in_b_host && sa_out_w_host && sa_out_b_host && ca_in_w_host && ca_in_b_host && ca_out_w_host &&
                ca_out_b_host && lin1_w_host && lin1_b_host && lin2_w_host && lin2_b_host && ln_host && emb_host && posq_host && qsa_host,
            "dec_step: a host weight is null");
  for (int i = 2; i < 10; ++i) YMK_CHECK(ln_host[i] != nullptr, "dec_step: a LayerNorm vector is null");
  YMK_CHECK(tok_dev && skv_dev && memkv_dev && out_dev && b >= 1 && ntok >= 1 && step >= 0 && step < ns, "dec_step: bad argument");
  YMK_CHECK((mem_off_dev == nullptr) == (mem_len_dev == nullptr), "dec_step: mem_off and mem_len come in pairs");
  YMK_CHECK((gid_dev == nullptr) == (gopen_dev == nullptr) && ng >= 1, "dec_step: gid and gopen come in pairs, ng >= 1");
  YMK_CHECK(aligned16(skv_dev) && aligned16(memkv_dev) && aligned16(out_dev), "dec_step: skv / memkv / out must be 16 B aligned");
  hipStream_t s = (hipStream_t)stream;
  DevicePool pool;
  DecStepW w{};
  const DecStepHostW hw{sa_in_w_host, sa_in_b_host, sa_out_w_host, sa_out_b_host, ca_in_w_host, ca_in_b_host, ca_out_w_host,
                        ca_out_b_host, lin1_w_host, lin1_b_host, lin2_w_host, lin2_b_host, d, heads, f};
  make_dec_step_weights(pool, hw, w);
  w.emb = pool.upload(emb_host, (size_t)ntok * d);
  w.posq = pool.upload(posq_host, (size_t)ns * d);
  w.qsa = pool.upload(qsa_host, (size_t)ns * d);
  w.ncg = pool.upload(ln_host[2], d); w.ncb = pool.upload(ln_host[3], d);
  w.n1g = pool.upload(ln_host[4], d); w.n1b = pool.upload(ln_host[5], d);
  w.n2g = pool.upload(ln_host[6], d); w.n2b = pool.upload(ln_host[7], d);
  w.dng = pool.upload(ln_host[8], d); w.dnb = pool.upload(ln_host[9], d);
  parseq_dec_step(s, w, tok_dev, ns, step, skv_dev, ns, memkv_dev, l, mem_off_dev, mem_len_dev, out_dev, prev_not_done_dev, b, gid_dev,
                  gopen_dev, ng, state_dev);
  YMK_HIP(hipStreamSynchronize(s));  // pool frees the weights on return
  YMK_API_END
}

int ymk_op_greedy_step(const float* logits_dev, int64_t ld_b, int c, int step, int num_steps, int* tok_dev, int* raw_dev, int ld_tok,
                       int* state_dev, int eos_id, int rep_on, int period_max, int min_run_p1, int min_repeats, int* not_done_dev,
                       const int* prev_not_done_dev, const int* gid_dev, int* gopen_dev, int ng, int partials, int b, void* stream) {
  return ymk_op_greedy_step_retire(logits_dev, ld_b, c, step, num_steps, tok_dev, raw_dev, ld_tok, state_dev, eos_id, rep_on, period_max,
                                   min_run_p1, min_repeats, not_done_dev, prev_not_done_dev, gid_dev, gopen_dev, ng, partials,
                                   /*retire_rows=*/0, b, stream);
}

int ymk_op_greedy_step_retire(const float* logits_dev, int64_t ld_b, int c, int step, int num_steps, int* tok_dev, int* raw_dev,
                              int ld_tok, int* state_dev, int eos_id, int rep_on, int period_max, int min_run_p1, int min_repeats,
                              int* not_done_dev, const int* prev_not_done_dev, const int* gid_dev, int* gopen_dev, int ng, int partials,
                              int retire_rows, int b, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(retire_rows == 0 || retire_rows == 1, "greedy_step: retire_rows is 0 or 1");
  YMK_CHECK(logits_dev && tok_dev && raw_dev && state_dev && not_done_dev && b >= 1 && c >= 1, "greedy_step: bad argument");
  YMK_CHECK(step >= 0 && step < num_steps && num_steps <= ld_tok, "greedy_step: 0 <= step < num_steps <= ld_tok");
  YMK_CHECK(ld_b >= (int64_t)c * (partials ? 2 : 1), "greedy_step: rows overlap");
  YMK_CHECK(!partials || (((uintptr_t)logits_dev | (uintptr_t)(ld_b * 4)) & 7) == 0, "greedy_step: (max, column) pairs must be 8 B aligned");
  YMK_CHECK((gid_dev == nullptr) == (gopen_dev == nullptr) && ng >= 1, "greedy_step: gid and gopen come in pairs, ng >= 1");
  YMK_CHECK(period_max >= 0, "greedy_step: period_max >= 0");
  ymk::greedy_step((hipStream_t)stream, logits_dev, (long)ld_b, c, step, num_steps, tok_dev, raw_dev, ld_tok, state_dev, eos_id, rep_on,
                   period_max, min_run_p1, min_repeats, not_done_dev, prev_not_done_dev, /*arrived=*/nullptr, /*host_flag=*/nullptr, b,
                   gid_dev, gopen_dev, ng, partials, retire_rows);
  YMK_API_END
}

int ymk_op_rowmax_head(const float* x_dev, int m, int k, const float* w_host, int cout, const float* bias_host, int split,
                       const int* row_group_dev, const int* group_open_dev, const int* row_dead_dev, int row_dead_ld,
                       const unsigned* amax_in_dev, float* pairs_dev, void* stream) {
  YMK_API_BEGIN
  using namespace ymk;
  YMK_CHECK(x_dev && w_host && pairs_dev && m > 0 && k > 0 && k % 4 == 0 && cout > 0, "rowmax_head: bad argument");
  YMK_CHECK((row_group_dev == nullptr) == (group_open_dev == nullptr), "rowmax_head: row_group and group_open come in pairs");
  YMK_CHECK(row_dead_dev == nullptr || row_dead_ld >= 1, "rowmax_head: row_dead_ld >= 1");
  YMK_CHECK(split == 0 || (split == SPLIT_F16X2 && amax_in_dev != nullptr), "rowmax_head: split is 0 or 16 (with the input's record)");
  hipStream_t s = (hipStream_t)stream;
  DevicePool pool;
  const ConvW cw = op_conv_weight(pool, w_host, cout, k, 1, 1, false, nullptr, bias_host);
  SplitCtxOwner split_ctx;
  ConvSplitScope scope(split, split_ctx.get(), 0);
  const int tiles = (cout + ROWMAX_TILE_N - 1) / ROWMAX_TILE_N;
  gemm(s, x_dev, m, k, k, cw, ACT_NONE, nullptr, 0, pairs_dev, 2 * tiles, row_group_dev, group_open_dev, EPI_ROWMAX, amax_in_dev, nullptr,
       row_dead_dev, row_dead_ld);
  YMK_HIP(hipStreamSynchronize(s));  // pool frees the weights on return
  YMK_API_END
}

int ymk_op_refine_prep(const int* raw_dev, int ld_tok, int s_len, int bos_id, int eos_id, int* tok2_dev, unsigned char* kpm_dev, int b,
                       const int* gid_dev, const int* gsteps_dev, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(raw_dev && tok2_dev && kpm_dev && b >= 1 && s_len >= 1 && s_len <= ld_tok, "refine_prep: bad argument");
  YMK_CHECK((gid_dev == nullptr) == (gsteps_dev == nullptr), "refine_prep: gid and gsteps come in pairs");
  ymk::refine_prep((hipStream_t)stream, raw_dev, ld_tok, s_len, bos_id, eos_id, tok2_dev, kpm_dev, b, gid_dev, gsteps_dev);
  YMK_API_END
}

int ymk_op_rep_cut(float* logits_dev, int64_t ld_b, int c, int s_len, const int* state_dev, int eos_id, int b, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(logits_dev && state_dev && b >= 1 && c >= 1 && s_len >= 0 && ld_b >= (int64_t)s_len * c, "rep_cut: bad argument");
  ymk::rep_cut((hipStream_t)stream, logits_dev, (long)ld_b, c, s_len, state_dev, eos_id, b);
  YMK_API_END
}

int ymk_op_row_argmax(const float* logits_dev, int rows, int c, int* out_dev, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(logits_dev && out_dev && rows >= 0 && c >= 1, "row_argmax: bad argument");
  ymk::row_argmax((hipStream_t)stream, logits_dev, rows, c, out_dev);
  YMK_API_END
}

int ymk_op_ctx_embed_ln(const int* tok_dev, int ld_tok, int pos0, int npos, const float* emb_dev, const float* posq_dev,
                        const float* g_dev, const float* b_dev, float eps, float* out_dev, int out_rows, int d, int b, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(tok_dev && emb_dev && posq_dev && g_dev && b_dev && out_dev && b >= 1 && d >= 1, "ctx_embed_ln: bad argument");
  YMK_CHECK(pos0 >= 0 && npos >= 0 && pos0 + npos <= ld_tok && pos0 + npos <= out_rows, "ctx_embed_ln: positions outside the rows");
  ymk::ctx_embed_ln((hipStream_t)stream, tok_dev, ld_tok, pos0, npos, emb_dev, posq_dev, g_dev, b_dev, eps, out_dev, out_rows, d, b);
  YMK_API_END
}

int ymk_op_init_decode(int* tok_dev, int ld_tok, int* state_dev, int bos_id, int pad_id, int b, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(tok_dev && state_dev && b >= 0, "init_decode: bad argument");
  ymk::init_decode((hipStream_t)stream, tok_dev, ld_tok, state_dev, bos_id, pad_id, b);
  YMK_API_END
}

int ymk_op_tile_rows(const float* src_dev, int rows, int d, float* dst_dev, int b, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(src_dev && dst_dev && rows >= 0 && d >= 0 && b >= 0 && ((size_t)rows * d) % 4 == 0, "tile_rows: rows * d must be a multiple of 4");
  YMK_CHECK(aligned16(src_dev) && aligned16(dst_dev), "tile_rows: tensors must be 16 B aligned");
  ymk::tile_rows((hipStream_t)stream, src_dev, rows, d, dst_dev, b);
  YMK_API_END
}

int ymk_op_add_pos_embed(float* x_dev, const float* pos_dev, int b, int gh, int gw, int full_gw, int d, void* stream) {
  YMK_API_BEGIN
  YMK_CHECK(x_dev && pos_dev && b >= 1 && gh >= 1 && gw >= 1 && gw <= full_gw && d >= 4 && d % 4 == 0, "add_pos_embed: bad argument");
  YMK_CHECK(aligned16(x_dev) && aligned16(pos_dev), "add_pos_embed: tensors must be 16 B aligned");
  ymk::add_pos_embed((hipStream_t)stream, x_dev, pos_dev, b, gh, gw, full_gw, d);
  YMK_API_END
}

}  // extern "C"
