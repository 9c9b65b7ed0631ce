// train_core.inc -- what the float32 engine (train.inc, dh_train) and the bf16 engine (train2.inc, dh_train2) share on the host:
// the parameter store (arenas, slot maps, allocations), the Adam launch, the gradient buckets of the data-parallel exchange and the
// side stream's hand-off.  Included in resnet_kernels.hip in front of train.inc.  The engines differ in their kernels and in the ORDER
// of their arenas (float32: forward order, bf16: backward-completion order); nothing here depends on that order.
namespace {

__global__ void fill_kernel(float* p, int64_t n, float v) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

// Adam (torch.optim.Adam defaults, no weight decay, no amsgrad) over one flat parameter arena
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n, float lr, float b1, float b2,
                                                   float eps, float bc1, float bc2_sqrt) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float gi = g[i];
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = p[i] - (lr / bc1) * (mi / denom);
  }
}

inline int grid_for(int64_t n, int per = 256, int cap = 256 * 16) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, cap));
}

}  // namespace

// A plain struct: it owns nothing by itself (no destructor); the engine that holds it calls store_free_all.  A test hook may fill
// one on the stack with borrowed pointers.
struct TrainStore {
  typedef std::pair<int64_t, int64_t> Range;   // (offset, count) in an arena, in elements
  std::map<std::string, Range> slot;    // parameter name -> its range in Pm / G / M / V
  std::map<std::string, Range> rslot;   // running_mean / running_var -> its range in R
  int64_t n_params = 0, n_running = 0;
  float *Pm = nullptr, *G = nullptr, *M = nullptr, *V = nullptr, *R = nullptr;   // masters, gradients, Adam moments, running statistics
  int64_t adam_t = 0;                   // Adam steps taken (bias correction when the caller passes step <= 0)
  std::vector<void*> allocs;            // live as long as the engine: arenas, packed weights, per-channel buffers
  std::vector<void*> shape_allocs;      // sized by (B, P): activations and workspaces, re-made when the batch shape changes
  bool shape_phase = false;             // store_alloc target
  // Data-parallel gradient buckets.  `items`: consecutive arena ranges in the order the backward pass completes them (the engine
  // lists them once).  A bucket is the union of consecutive items; bucket_last[k] is the last item of bucket k.
  std::vector<Range> items, buckets;
  std::vector<size_t> bucket_last;
  dh_bucket_cb bucket_cb = nullptr;
  void* bucket_user = nullptr;
  size_t items_done = 0, next_bucket = 0;   // progress of the running backward pass (store_begin_backward)
  // Weight gradients (and the fused optimiser) on a side stream of the lowest priority, behind one event of the main stream per
  // hand-off; null when the engine's side-stream switch is off.
  hipStream_t side = nullptr;
  hipEvent_t ev_dz = nullptr, ev_join = nullptr;
};

namespace {

template <typename V> int store_alloc(TrainStore& s, V** p, int64_t n) {
  DH_HIP(hipMalloc(reinterpret_cast<void**>(p), std::max<size_t>((size_t)std::max<int64_t>(n, 1) * sizeof(V), 16)));
  (s.shape_phase ? s.shape_allocs : s.allocs).push_back(*p);
  return DH_OK;
}

// layout: every tensor starts on a 4-element (16-byte) boundary; n_params / n_running are the running ends of the arenas
void store_add(TrainStore& s, const std::string& k, int64_t cnt) { s.slot[k] = {s.n_params, cnt}; s.n_params += (cnt + 3) & ~(int64_t)3; }
void store_radd(TrainStore& s, const std::string& k, int64_t cnt) { s.rslot[k] = {s.n_running, cnt}; s.n_running += (cnt + 3) & ~(int64_t)3; }

// the five arenas of the finished layout, zero-filled on `st`
int store_alloc_arenas(TrainStore& s, hipStream_t st) {
  int rc;
  for (float** a : {&s.Pm, &s.G, &s.M, &s.V}) {
    if ((rc = store_alloc(s, a, s.n_params))) return rc;
    DH_HIP(hipMemsetAsync(*a, 0, s.n_params * sizeof(float), st));
  }
  if ((rc = store_alloc(s, &s.R, s.n_running))) return rc;
  DH_HIP(hipMemsetAsync(s.R, 0, s.n_running * sizeof(float), st));
  return DH_OK;
}

void store_free_shape(TrainStore& s) {   // hipFree waits for work that still uses the buffers
  for (void* q : s.shape_allocs) (void)hipFree(q);
  s.shape_allocs.clear();
}
void store_free_all(TrainStore& s) {
  store_free_shape(s);
  for (void* q : s.allocs) (void)hipFree(q);
  s.allocs.clear();
  for (hipEvent_t e : {s.ev_dz, s.ev_join}) if (e) (void)hipEventDestroy(e);
  if (s.side) (void)hipStreamDestroy(s.side);
  s.side = nullptr; s.ev_dz = s.ev_join = nullptr;
}

// kind: 0 parameter, 1 gradient, 2 running statistic; to_lib != 0 copies caller -> library.  `ptr` may be host or device memory
// (hipMemcpyDefault).  `what` names the entry point in the error text.
int store_tensor(TrainStore& s, const char* what, const char* name, int32_t kind, void* ptr, int64_t n_elem, int32_t to_lib, hipStream_t st) {
  if (std::string(name).find("num_batches_tracked") != std::string::npos) return DH_OK;
  float* base = kind == 0 ? s.Pm : kind == 1 ? s.G : s.R;
  const auto& table = kind == 2 ? s.rslot : s.slot;
  auto it = table.find(name);
  DH_REQUIRE(it != table.end(), "%s: unknown tensor '%s' (kind %d)", what, name, kind);
  DH_REQUIRE(it->second.second == n_elem, "%s: '%s' has %lld elements, got %lld", what, name, (long long)it->second.second, (long long)n_elem);
  if (to_lib) DH_HIP(hipMemcpyAsync(base + it->second.first, ptr, n_elem * 4, hipMemcpyDefault, st));
  else DH_HIP(hipMemcpyAsync(ptr, base + it->second.first, n_elem * 4, hipMemcpyDefault, st));
  return DH_OK;
}

// a whole arena (data-parallel training all-reduces the gradient arena in place): kind 0 parameters, 1 gradients, 2 running statistics
void store_flat(const TrainStore& s, int32_t kind, void** ptr_out, int64_t* n_out) {
  *ptr_out = kind == 0 ? s.Pm : kind == 1 ? s.G : s.R;
  *n_out = kind == 2 ? s.n_running : s.n_params;
}

// ---- gradient buckets ---------------------------------------------------------------------------------------------------------
// The gradient arena is cut into buckets of about `bucket_bytes` (whole items; 0 = one bucket) in the order in which the backward
// pass completes them.  `cb` (may be NULL) is called on the calling thread from inside the backward pass right after the kernels
// that finish a bucket have been enqueued on the backward stream: the caller records an event there and starts that bucket's
// all-reduce on a stream of its own.
void store_set_buckets(TrainStore& s, int64_t bucket_bytes, dh_bucket_cb cb, void* user, int32_t* n_buckets_out) {
  s.bucket_cb = cb; s.bucket_user = user;
  s.buckets.clear(); s.bucket_last.clear();
  int64_t lo = 0, hi = 0;
  bool open = false;
  for (size_t i = 0; i < s.items.size(); ++i) {
    const int64_t a = s.items[i].first, b = a + s.items[i].second;
    lo = open ? std::min(lo, a) : a; hi = open ? std::max(hi, b) : b;
    open = true;
    if (i + 1 == s.items.size() || (bucket_bytes > 0 && (hi - lo) * 4 >= bucket_bytes)) {
      if (hi > lo) { s.buckets.push_back({lo, hi - lo}); s.bucket_last.push_back(i); }
      open = false;
    }
  }
  if (n_buckets_out) *n_buckets_out = (int32_t)s.buckets.size();
}
int store_bucket(const TrainStore& s, const char* what, int32_t i, int64_t* offset, int64_t* count) {
  DH_REQUIRE(offset && count && i >= 0 && (size_t)i < s.buckets.size(), "%s: index out of range", what);
  *offset = s.buckets[i].first; *count = s.buckets[i].second;
  return DH_OK;
}
void store_begin_backward(TrainStore& s) { s.items_done = s.next_bucket = 0; }
// a bucket completes with the item about to be marked done: its gradients must precede the caller's event
bool store_bucket_due(const TrainStore& s) {
  return s.bucket_cb != nullptr && s.next_bucket < s.buckets.size() && s.bucket_last[s.next_bucket] <= s.items_done;
}
// the kernels of the next completion item have been enqueued: fire the buckets that end with it
void store_mark_done(TrainStore& s) {
  for (; s.next_bucket < s.buckets.size() && s.bucket_last[s.next_bucket] <= s.items_done; ++s.next_bucket)
    if (s.bucket_cb) s.bucket_cb((int32_t)s.next_bucket, s.buckets[s.next_bucket].first, s.buckets[s.next_bucket].second, s.bucket_user);
  ++s.items_done;
}

// ---- optimiser ----------------------------------------------------------------------------------------------------------------
struct AdamArgs { float lr, beta1, beta2, eps, bc1, bc2s; };
// step <= 0: the store's own count (it survives batch-shape changes with the moments)
AdamArgs adam_args(TrainStore& s, float lr, float beta1, float beta2, float eps, int64_t step) {
  if (step <= 0) step = s.adam_t + 1;
  s.adam_t = step;
  return {lr, beta1, beta2, eps, 1.f - powf(beta1, (float)step), sqrtf(1.f - powf(beta2, (float)step))};
}
void adam_range(TrainStore& s, const AdamArgs& a, int64_t off, int64_t n, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, st, s.Pm + off, s.G + off, s.M + off, s.V + off, n, a.lr, a.beta1, a.beta2,
                     a.eps, a.bc1, a.bc2s);
}

// ---- side stream --------------------------------------------------------------------------------------------------------------
int store_open_side(TrainStore& s) {
  int pr_lo = 0, pr_hi = 0;   // the side stream is filler next to the critical path: lowest priority
  (void)hipDeviceGetStreamPriorityRange(&pr_lo, &pr_hi);
  if (pr_lo == pr_hi || hipStreamCreateWithPriority(&s.side, hipStreamNonBlocking, pr_lo) != hipSuccess) {
    (void)hipGetLastError();   // the failed attempt's error is sticky: without this the next DH_LAUNCH_CHECK reports it as a launch failure
    DH_HIP(hipStreamCreateWithFlags(&s.side, hipStreamNonBlocking));   // (no priorities on this device: a plain stream)
  }
  DH_HIP(hipEventCreateWithFlags(&s.ev_dz, hipEventDisableTiming));
  DH_HIP(hipEventCreateWithFlags(&s.ev_join, hipEventDisableTiming));
  return DH_OK;
}
// what `st` has enqueued so far precedes what the side stream is given next
int side_handoff(TrainStore& s, hipStream_t st) {
  DH_HIP(hipEventRecord(s.ev_dz, st));
  DH_HIP(hipStreamWaitEvent(s.side, s.ev_dz, 0));
  return DH_OK;
}
// everything handed to the side stream so far precedes what `st` does next
int side_join(TrainStore& s, hipStream_t st) {
  DH_HIP(hipEventRecord(s.ev_join, s.side));
  DH_HIP(hipStreamWaitEvent(st, s.ev_join, 0));
  return DH_OK;
}

}  // namespace
