// Host runtime of libymk_hip.so: error slot, arena, weight store, state-dict -> packed panels.
#include "ymk_common.h"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>

namespace ymk {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
const std::string& last_error() { return g_err; }

// ---------------------------------------------------------------- allocation accounting (ymk_common.h)
static thread_local int t_forward_depth = 0;
static std::atomic<long long> g_allocs_in_forward{0}, g_arena_grows_in_forward{0}, g_lazy_panel_builds{0}, g_syncs_in_forward{0};
ForwardScope::ForwardScope() { ++t_forward_depth; }
ForwardScope::~ForwardScope() { --t_forward_depth; }
bool in_forward() { return t_forward_depth > 0; }
static void count_alloc() {
  if (t_forward_depth > 0) ++g_allocs_in_forward;
}
void* dev_malloc(size_t bytes) {
  void* p = nullptr;
  count_alloc();
  YMK_HIP(hipMalloc(&p, bytes ? bytes : 4));
  return p;
}
void dev_free(void* p) {
  if (!p) return;
  count_alloc();
  (void)hipFree(p);
}
void* host_malloc_pinned(size_t bytes, unsigned flags) {
  void* p = nullptr;
  count_alloc();
  YMK_HIP(hipHostMalloc(&p, bytes ? bytes : 4, flags));
  return p;
}
void host_free_pinned(void* p) {
  if (!p) return;
  count_alloc();
  (void)hipHostFree(p);
}
void forward_sync(hipStream_t s) {
  if (t_forward_depth > 0) ++g_syncs_in_forward;
  YMK_HIP(hipStreamSynchronize(s));
}
void note_lazy_panel_build() {
  if (t_forward_depth > 0) ++g_lazy_panel_builds;
}
void note_arena_grow() {
  if (t_forward_depth > 0) ++g_arena_grows_in_forward;
}
static bool workspace_stat(const std::string& key, long long* value);
bool runtime_stat(const std::string& key, long long* value) {
  if (key == "allocs_in_forward") *value = g_allocs_in_forward.load();
  else if (key == "arena_grows_in_forward") *value = g_arena_grows_in_forward.load();
  else if (key == "lazy_panel_builds") *value = g_lazy_panel_builds.load();
  else if (key == "syncs_in_forward") *value = g_syncs_in_forward.load();
  else return workspace_stat(key, value);
  return true;
}
static bool env_flag(const char* name) {
  const char* v = std::getenv(name);
  return v != nullptr && v[0] != '\0' && v[0] != '0';
}
bool debug_lazy_split() {
  static const bool on = env_flag("YMK_DEBUG_LAZY_SPLIT");
  return on;
}
bool debug_hazard_null_memset() {
  static const bool on = env_flag("YMK_DEBUG_HAZARD_NULL_MEMSET");
  return on;
}
bool debug_hazard_no_finalize_sync() {
  static const bool on = env_flag("YMK_DEBUG_HAZARD_NO_FINALIZE_SYNC");
  return on;
}

// ---------------------------------------------------------------- workspace planner (ymk_common.h)
namespace {
struct Placed {
  size_t off, end;
  int64_t from, to;  // alive over positions [from, to)
};
// greedy best-fit of the allocations in `order`; returns the peak
size_t place_in_order(const std::vector<uint32_t>& order, const std::vector<size_t>& sz, const std::vector<int64_t>& to, std::vector<size_t>& off) {
  std::vector<Placed> placed;  // sorted by offset
  placed.reserve(order.size());
  size_t peak = 0;
  for (uint32_t k : order) {
    const int64_t from = (int64_t)k, until = to[k];
    const size_t need = sz[k];
    // walk the placed buffers whose lifetime meets this one's, lowest first; keep the tightest gap that fits
    size_t cursor = 0, best = SIZE_MAX, best_gap = SIZE_MAX;
    for (const Placed& p : placed) {
      if (p.to <= from || until <= p.from) continue;
      if (p.off > cursor) {
        const size_t gap = p.off - cursor;
        if (gap >= need && gap < best_gap) {
          best_gap = gap;
          best = cursor;
        }
      }
      if (p.end > cursor) cursor = p.end;
    }
    if (best == SIZE_MAX) best = cursor;  // above everything it overlaps with
    off[k] = best;
    const Placed me{best, best + need, from, until};
    auto it = placed.begin();
    while (it != placed.end() && it->off <= best) ++it;
    placed.insert(it, me);
    if (me.end > peak) peak = me.end;
  }
  return peak;
}
}  // namespace

void plan_workspace(size_t n, const size_t* size, const int64_t* release_pos, size_t* offsets, size_t* peak, size_t* live_bound) {
  YMK_CHECK(n < (size_t)1 << 31, "plan_workspace: too many allocations");
  std::vector<size_t> sz(n);
  std::vector<int64_t> to(n);
  size_t sum = 0;
  for (size_t k = 0; k < n; ++k) {
    sz[k] = (size[k] + WS_ALIGN - 1) & ~(WS_ALIGN - 1);
    sum += sz[k];
    const int64_t r = release_pos ? release_pos[k] : WS_NEVER;
    YMK_CHECK(r < 0 || r > (int64_t)k, "plan_workspace: allocation " + std::to_string(k) + " released before it was made");
    to[k] = (r < 0 || r > (int64_t)n) ? (int64_t)n : r;
  }
  // the lower bound: bytes alive at each position
  std::vector<int64_t> delta(n + 1, 0);
  for (size_t k = 0; k < n; ++k) {
    delta[k] += (int64_t)sz[k];
    delta[(size_t)to[k]] -= (int64_t)sz[k];
  }
  int64_t live = 0, live_max = 0;
  for (size_t k = 0; k < n; ++k) {
    live += delta[k];
    live_max = std::max(live_max, live);
  }
  std::vector<uint32_t> order(n);
  std::vector<size_t> off(n), best_off(n);
  size_t best_peak = SIZE_MAX;
  for (int pass = 0; pass < 3 && best_peak != (size_t)live_max; ++pass) {
    for (size_t k = 0; k < n; ++k) order[k] = (uint32_t)k;
    if (pass == 0)
      std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const int64_t la = to[a] - (int64_t)a, lb = to[b] - (int64_t)b;
        return la != lb ? la > lb : sz[a] > sz[b];
      });
    else if (pass == 1)
      std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return sz[a] > sz[b]; });
    const size_t pk = place_in_order(order, sz, to, off);
    if (pk < best_peak) {
      best_peak = pk;
      best_off.swap(off);
    }
  }
  if (n == 0) best_peak = 0;
  YMK_CHECK(best_peak <= sum && (size_t)live_max <= best_peak, "plan_workspace: inconsistent plan");
  for (size_t k = 0; k < n; ++k) offsets[k] = best_off[k];
  if (peak) *peak = best_peak;
  if (live_bound) *live_bound = (size_t)live_max;
}

// ---------------------------------------------------------------- Arena
static std::atomic<int> g_ws_reuse_default{0}, g_ws_poison{0};
static std::atomic<long long> g_ws_planned_forwards{0}, g_ws_plan_bytes{0}, g_ws_bump_bytes{0}, g_ws_live_bound{0};
bool runtime_debug_option(const std::string& key, int value) {
  if (key == "workspace_reuse") g_ws_reuse_default = value != 0;
  else if (key == "workspace_poison") g_ws_poison = value != 0;
  else return false;
  return true;
}
bool workspace_reuse_default() { return g_ws_reuse_default.load(std::memory_order_relaxed) != 0; }
static bool workspace_stat(const std::string& key, long long* value) {
  if (key == "workspace_planned_forwards") *value = g_ws_planned_forwards.load();
  else if (key == "ws_plan_bytes_last") *value = g_ws_plan_bytes.load();
  else if (key == "ws_bump_bytes_last") *value = g_ws_bump_bytes.load();
  else if (key == "ws_live_bound_last") *value = g_ws_live_bound.load();
  else return false;
  return true;
}

Arena::~Arena() { dev_free(base_); }
void Arena::reserve(size_t bytes) {
  if (bytes <= cap_ && !resize_pending_) return;
  YMK_CHECK(off_ == 0 && k_ == 0, "arena reserve while in use");
  if (bytes == cap_) {
    resize_pending_ = false;
    return;
  }
  if (bytes < cap_) {  // the mode changed: plans made for the old slab go with it (set_planned dropped them; be sure)
    plans_.clear();
    cur_ = nullptr;  // (the bounds stay: the reservation being made is sized from them)
  }
  note_arena_grow();
  dev_free(base_);
  base_ = nullptr;
  cap_ = 0;
  base_ = (char*)dev_malloc(bytes);
  cap_ = bytes;
  resize_pending_ = false;
}
void Arena::reset() {
  off_ = 0;
  k_ = r_ = 0;
  if (dry_run && planned_) {
    t_size_.clear();
    t_at_.clear();
    t_rel_.clear();
    t_rel_order_.clear();
  }
}
bool Arena::set_planned(bool on) {
  if (on == planned_) return false;
  planned_ = on;
  plans_.clear();
  bounds_.clear();
  cur_ = nullptr;
  resize_pending_ = true;
  return true;
}
void* Arena::alloc_bytes(size_t bytes) {
  const size_t a = (bytes + WS_ALIGN - 1) & ~(WS_ALIGN - 1);
  if (planned_ && !dry_run) {  // replay: a table lookup
    YMK_CHECK(cur_ != nullptr && k_ < cur_->size.size(), "planned workspace: allocation " + std::to_string(k_) + " is not in the plan");
    YMK_CHECK(cur_->size[k_] == a, "planned workspace: allocation " + std::to_string(k_) + " asks " + std::to_string(a) +
                                       " bytes, the plan recorded " + std::to_string(cur_->size[k_]));
    const size_t at = cur_->off[k_++];
    YMK_CHECK(at + a <= cap_, "arena overflow: need " + std::to_string(at + a) + " have " + std::to_string(cap_));
    return base_ + at;
  }
  const size_t at = off_;
  off_ += a;
  if (off_ > high_) high_ = off_;
  if (dry_run) {
    if (planned_) {
      t_size_.push_back(a);
      t_at_.push_back(at);
      t_rel_.push_back(WS_NEVER);
    }
    return (void*)(uintptr_t)(4096 + at);  // aligned fake address, never dereferenced
  }
  YMK_CHECK(off_ <= cap_, "arena overflow: need " + std::to_string(off_) + " have " + std::to_string(cap_));
  return base_ + at;
}
void Arena::release(const void* p) {
  if (!planned_ || p == nullptr) return;
  if (dry_run) {  // the fake addresses grow with the call order: find the allocation by bisection
    const size_t at = (size_t)(uintptr_t)p - 4096;
    const auto it = std::lower_bound(t_at_.begin(), t_at_.end(), at);
    YMK_CHECK(it != t_at_.end() && *it == at, "workspace release: not the start of an allocation of this forward");
    const size_t k = (size_t)(it - t_at_.begin());
    YMK_CHECK(t_rel_[k] == WS_NEVER, "workspace release: allocation " + std::to_string(k) + " released twice");
    t_rel_[k] = (int64_t)t_size_.size();
    t_rel_order_.push_back((uint32_t)k);
    return;
  }
  YMK_CHECK(cur_ != nullptr && r_ < cur_->rel_order.size(), "planned workspace: release " + std::to_string(r_) + " is not in the plan");
  const uint32_t k = cur_->rel_order[r_++];
  YMK_CHECK((const char*)p == base_ + cur_->off[k], "planned workspace: release " + std::to_string(r_ - 1) + " does not match the plan");
  if (g_ws_poison.load(std::memory_order_relaxed)) YMK_HIP(hipMemsetAsync(base_ + cur_->off[k], 0xFF, cur_->size[k], stream_));
}
size_t Arena::plan_commit(uint64_t key, bool bound) {
  if (!planned_) return off_;
  if (plans_.size() >= 64) {  // ragged workloads change shape on every call: keep the cache small
    plans_.clear();
    cur_ = nullptr;
  }
  Plan& p = plans_[key];
  p.size = t_size_;
  p.rel = t_rel_;
  p.rel_order = t_rel_order_;
  p.off.assign(t_size_.size(), 0);
  p.bump = off_;
  plan_workspace(p.size.size(), p.size.data(), p.rel.data(), p.off.data(), &p.peak, &p.live);
  if (!bound && p.peak > cap_) {
    for (const Plan& b : bounds_) {
      bool covers = b.peak <= cap_ && b.size.size() == p.size.size() && b.rel == p.rel;
      for (size_t k = 0; covers && k < p.size.size(); ++k) covers = p.size[k] <= b.size[k];
      if (!covers) continue;
      p.off = b.off;
      p.peak = 0;
      for (size_t k = 0; k < p.size.size(); ++k) p.peak = std::max(p.peak, p.off[k] + p.size[k]);
      break;
    }
  }
  if (bound) {
    if (bounds_.size() >= 8) bounds_.erase(bounds_.begin());
    bounds_.push_back(p);
  }
  cur_ = &p;
  publish(p);
  return p.peak;
}
bool Arena::plan_select(uint64_t key, size_t* need) {
  if (!planned_) return false;
  const auto it = plans_.find(key);
  if (it == plans_.end()) return false;
  cur_ = &it->second;
  *need = cur_->peak;
  reset();
  return true;
}
void Arena::publish(const Plan& p) const {
  g_ws_plan_bytes = (long long)p.peak;
  g_ws_bump_bytes = (long long)p.bump;
  g_ws_live_bound = (long long)p.live;
}
void Arena::forward_begin() {
  reset();
  if (!planned_) return;
  YMK_CHECK(cur_ != nullptr, "planned workspace: no plan selected");
  ++g_ws_planned_forwards;
  publish(*cur_);
}
void Arena::amax_begin(hipStream_t s, int records) {
  stream_ = s;
  amax_n_ = records;
  amax_used_ = 0;
  const size_t bytes = (size_t)records * AMAX_REC_WORDS * sizeof(unsigned);
  amax_pool_ = (unsigned*)alloc_bytes(bytes);
  if (!dry_run) YMK_HIP(hipMemsetAsync(amax_pool_, 0, bytes, s));
}
unsigned* Arena::amax_next() {
  if (amax_pool_ == nullptr || amax_used_ >= amax_n_) return nullptr;
  return amax_pool_ + (size_t)(amax_used_++) * AMAX_REC_WORDS;
}
float* Arena::alloc_f(size_t count) { return (float*)alloc_bytes(count * sizeof(float)); }
Tensor Arena::tensor(int n, int h, int w, int c) {
  Tensor t;
  t.n = n;
  t.h = h;
  t.w = w;
  t.c = c;
  t.ld = c;
  t.p = alloc_f((size_t)n * h * w * c);
  return t;
}

// ---------------------------------------------------------------- DevicePool
DevicePool::~DevicePool() {
  for (void* p : ptrs_) dev_free(p);
}
void DevicePool::note(const ConvW& c, bool perm) {
  std::vector<ConvW>& list = perm ? perm_ : convs_;
  for (ConvW& have : list)
    if (have.w == c.w) {
      have = c;
      return;
    }
  list.push_back(c);
}
float* DevicePool::alloc(size_t n) {
  const size_t b = (n ? n : 1) * sizeof(float);
  void* p = dev_malloc(b);
  ptrs_.push_back(p);
  bytes_ += b;
  return (float*)p;
}
float* DevicePool::upload(const float* src, size_t n) {
  float* d = alloc(n);
  if (n) YMK_HIP(hipMemcpy(d, src, n * sizeof(float), hipMemcpyHostToDevice));
  return d;
}
float* DevicePool::upload(const std::vector<float>& v) { return upload(v.data(), v.size()); }

// ---------------------------------------------------------------- WeightStore
void WeightStore::put(const std::string& name, const float* data, int ndim, const int64_t* dims) {
  HostTensor t;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    t.dims.push_back(dims[i]);
    n *= (size_t)dims[i];
  }
  t.data.assign(data, data + n);
  t_[name] = std::move(t);
}
const HostTensor& WeightStore::get(const std::string& name) const {
  auto it = t_.find(name);
  if (it == t_.end()) throw Error("missing weight tensor: " + name);
  return it->second;
}

// ---------------------------------------------------------------- packing helpers
// ConvW::pl_a / pl_b from the OIHW weights and the folded scale / bias (1 / 0 where absent); a little head room for the
// rounding of the fp32 sums and of the bound's own arithmetic
void plane_bound(ConvW& c, const float* oihw, size_t per_out, const std::vector<float>& scale, const std::vector<float>& bias) {
  double a = 0.0, b = 0.0;
  for (int o = 0; o < c.cout; ++o) {
    double l1 = 0.0;
    for (size_t i = 0; i < per_out; ++i) l1 += std::fabs((double)oihw[(size_t)o * per_out + i]);
    a = std::max(a, l1 * (scale.empty() ? 1.0 : std::fabs((double)scale[o])));
    if (!bias.empty()) b = std::max(b, std::fabs((double)bias[o]));
  }
  c.pl_a = (float)(a * 1.001);
  c.pl_b = (float)(b * 1.001);
}

ConvW make_conv(DevicePool& pool, const WeightStore& ws, const std::string& conv_prefix, const std::string& bn_prefix,
                bool tap4, float bn_eps) {
  const HostTensor& w = ws.get(conv_prefix + ".weight");
  YMK_CHECK(w.dims.size() == 4, conv_prefix + ".weight must be OIHW");
  ConvW c;
  c.cout = (int)w.dims[0];
  c.cin = (int)w.dims[1];
  c.kh = (int)w.dims[2];
  c.kw = (int)w.dims[3];
  c.mode = tap4 ? 1 : 0;
  std::vector<float> panel;
  pack_conv_weight(w.data.data(), c.cout, c.cin, c.kh, c.kw, tap4, panel, c.kpad, c.ctiles);
  if (tap4) c.cin = 4;
  c.w = pool.upload(panel);
  std::vector<float> scale, bias;
  const bool has_cb = ws.has(conv_prefix + ".bias");
  if (!bn_prefix.empty()) {
    // eval BatchNorm: y = (x - mean) / sqrt(var + eps) * gamma + beta    (x may carry a conv bias)
    const HostTensor& g = ws.get(bn_prefix + ".weight");
    const HostTensor& b = ws.get(bn_prefix + ".bias");
    const HostTensor& m = ws.get(bn_prefix + ".running_mean");
    const HostTensor& v = ws.get(bn_prefix + ".running_var");
    YMK_CHECK((int)g.numel() == c.cout, bn_prefix + ": channel mismatch");
    scale.resize(c.cout);
    bias.resize(c.cout);
    for (int i = 0; i < c.cout; ++i) {
      const float s = g.data[i] / std::sqrt(v.data[i] + bn_eps);
      const float cb = has_cb ? ws.get(conv_prefix + ".bias").data[i] : 0.f;
      scale[i] = s;
      bias[i] = b.data[i] + (cb - m.data[i]) * s;
    }
    c.scale = pool.upload(scale);
    c.bias = pool.upload(bias);
  } else if (has_cb) {
    bias = ws.get(conv_prefix + ".bias").data;
    c.bias = pool.upload(bias);
  }
  plane_bound(c, w.data.data(), w.numel() / (size_t)w.dims[0], scale, bias);
  pool.note(c);
  return c;
}

ConvW make_linear_raw(DevicePool& pool, const float* w_out_in, const float* bias, int out, int in) {
  ConvW c;
  c.cout = out;
  c.cin = in;
  c.kh = c.kw = 1;
  c.mode = 0;
  std::vector<float> panel;
  pack_conv_weight(w_out_in, out, in, 1, 1, false, panel, c.kpad, c.ctiles);
  c.w = pool.upload(panel);
  if (bias) c.bias = pool.upload(bias, out);
  plane_bound(c, w_out_in, (size_t)in, {}, bias ? std::vector<float>(bias, bias + out) : std::vector<float>());
  pool.note(c);
  return c;
}

ConvW make_deconv2x2_panel(DevicePool& pool, const float* w, int ci, int co, const float* scale, const float* bias) {
  std::vector<float> lin((size_t)4 * co * ci);
  for (int c = 0; c < ci; ++c)
    for (int o = 0; o < co; ++o)
      for (int ab = 0; ab < 4; ++ab) lin[((size_t)ab * co + o) * ci + c] = w[((size_t)c * co + o) * 4 + ab];
  ConvW p = make_linear_raw(pool, lin.data(), nullptr, 4 * co, ci);
  if (scale == nullptr && bias == nullptr) return p;
  std::vector<float> sc(scale ? 4 * co : 0), bi(bias ? 4 * co : 0);
  for (int ab = 0; ab < 4; ++ab)
    for (int o = 0; o < co; ++o) {
      if (scale) sc[ab * co + o] = scale[o];
      if (bias) bi[ab * co + o] = bias[o];
    }
  if (scale) p.scale = pool.upload(sc);
  if (bias) p.bias = pool.upload(bi);
  pool.note(p);  // (the panel with its scale: what the split copy folds the row's power of two into)
  return p;
}

float layernorm_output_bound(const std::vector<float>& gamma, const std::vector<float>& beta) {
  float g = 0.f, b = 0.f;
  for (float v : gamma) g = std::max(g, std::fabs(v));
  for (float v : beta) b = std::max(b, std::fabs(v));
  return std::sqrt((float)gamma.size()) * g + b;
}

unsigned* make_layernorm_amax_record(DevicePool& pool, const std::vector<float>& gamma, const std::vector<float>& beta) {
  const float bound = layernorm_output_bound(gamma, beta);
  std::vector<float> rec(AMAX_REC_WORDS, 0.f);  // all-zero bit patterns but word 0
  rec[0] = bound;                                // the record holds fp32 bit patterns: upload the float as it is
  return reinterpret_cast<unsigned*>(pool.upload(rec));
}

ConvW make_linear(DevicePool& pool, const WeightStore& ws, const std::string& prefix, bool has_bias) {
  const HostTensor& w = ws.get(prefix + ".weight");
  YMK_CHECK(w.dims.size() == 2, prefix + ".weight must be [out][in]");
  const float* b = nullptr;
  if (has_bias && ws.has(prefix + ".bias")) b = ws.get(prefix + ".bias").data.data();
  return make_linear_raw(pool, w.data.data(), b, (int)w.dims[0], (int)w.dims[1]);
}

}  // namespace ymk
