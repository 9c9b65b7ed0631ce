// train_core.inc -- what the float32 engine (train.inc, dh_train) and the bf16 engine (train2.inc, dh_train2) share on the host:
// the parameter store (arenas, slot maps, allocations), the Adam launch, the gradient buckets of the data-parallel exchange, the
// side stream's hand-off, the record of one convolution with what is derived from it (slots, BN buffers, map sizes, pack table, stem
// slab split) and the scheduler of a backward pass (BwdSched: every cross-stream ordering rule of a training step).  Included in
// resnet_kernels.hip behind train_core_kernels.inc (the kernels both engines launch) and in front of train.inc.  The engines differ in
// their kernels and in the ORDER of their arenas (float32: forward order, bf16: backward-completion order); nothing here depends on
// that order.

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

// ---- one convolution of a training engine ---------------------------------------------------------------------------------------
// The description (net_desc.inc) plus the engine's buffers; E = the element type of its activations (float / bf16_t).
template <typename E> struct TrainConvT : ConvDesc {
  int Hi = 0, Wi = 0, Ho = 0, Wo = 0;   // input / output map of the current batch shape (conv_shapes)
  void* wp_f = nullptr;   // packed forward operand, in E (the stem: its own layout; float32 1x1: unused, the GEMM reads the master tensor)
  void* wp_d = nullptr;   // packed data-gradient operand, in E; not for the stem
  E* Z = nullptr;         // conv output (pre-BN), NHWC
  E* Y = nullptr;         // BN (+identity) (+ReLU) output, NHWC
  E* dZ = nullptr;        // with a side stream: this conv's own dZ (the side stream's weight-gradient kernels read it long after it was written)
  BnBufs bnb{};
};
typedef TrainConvT<float> TrainConv;

namespace {

template <typename C> void convs_from_desc(std::vector<C>& convs, const NetDesc& d) {
  for (const ConvDesc& cd : d.convs) { convs.emplace_back(); static_cast<ConvDesc&>(convs.back()) = cd; }
}

// the five slots of a conv at the running ends of the arenas.  The order of the calls IS the arena order, inside a conv too: the float32
// engine (forward order) puts the conv weight first, the bf16 engine (backward-completion order) last.
void store_add_conv(TrainStore& s, const ConvDesc& c, bool weight_first) {
  const int64_t nw = (int64_t)c.cout * c.cin * c.ks * c.ks;
  if (weight_first) store_add(s, c.name + ".weight", nw);
  store_add(s, c.bn + ".weight", c.cout); store_add(s, c.bn + ".bias", c.cout);
  if (!weight_first) store_add(s, c.name + ".weight", nw);
  store_radd(s, c.bn + ".running_mean", c.cout); store_radd(s, c.bn + ".running_var", c.cout);
}

int store_alloc_bn(TrainStore& s, BnBufs& b, int C) {
  for (float** q : {&b.mean, &b.invstd, &b.scale, &b.shift, &b.k0, &b.k1, &b.k2})
    if (int rc = store_alloc(s, q, C)) return rc;
  return DH_OK;
}

// The map sizes of patch size P: every conv gets Hi / Ho, then `setup(conv, index, top)` runs (the engine's allocations; top: the last
// conv of a block), in forward order: the stem, then block by block its convs and its downsample conv.
template <typename C, typename Setup>
int conv_shapes(std::vector<C>& convs, const std::vector<BlockDesc>& blocks, int P, Setup setup) {
  auto place = [&](int i, int hi, bool top) -> int {
    C& c = convs[i];
    c.Hi = c.Wi = hi;
    c.Ho = c.Wo = (hi + 2 * (c.ks / 2) - c.ks) / c.stride + 1;
    return setup(c, i, top);
  };
  int rc = place(0, P, false);
  if (rc) return rc;
  int H = (convs[0].Ho + 2 - 3) / 2 + 1;   // behind the 3x3/2 maxpool
  for (const BlockDesc& b : blocks) {
    int h = H;
    for (int i = 0; i < b.nconv; ++i) {
      if ((rc = place(b.conv[i], h, i + 1 == b.nconv))) return rc;
      h = convs[b.conv[i]].Ho;
    }
    if (b.ds >= 0 && (rc = place(b.ds, H, false))) return rc;
    H = h;
  }
  return DH_OK;
}

// The descriptor table of an engine's pack-everything kernel: one Desc (with a field blk0 = its first workgroup) per packed conv, in
// conv order.  `add` them all, `upload` once (the descriptors hold device addresses that stay put for the life of the engine), then
// `range(j0, j1)` is the launch over descriptors [j0, j1): grid, first descriptor, count, blk0 of the first.
template <typename Desc> struct PackTable {
  Desc* dev = nullptr;
  std::vector<Desc> host;   // until upload
  std::vector<int> blk0;    // first workgroup of every descriptor (+ the total)
  int blocks = 0;
  void add(Desc d, int n_blocks) { d.blk0 = blocks; blk0.push_back(blocks); host.push_back(d); blocks += n_blocks; }
  int upload(TrainStore& s) {
    DH_HIP(hipMalloc(reinterpret_cast<void**>(&dev), host.size() * sizeof(Desc)));
    s.allocs.push_back(dev);   // freed with the engine (not with the batch-shape buffers)
    DH_HIP(hipMemcpy(dev, host.data(), host.size() * sizeof(Desc), hipMemcpyHostToDevice));
    blk0.push_back(blocks);
    host.clear();
    return DH_OK;
  }
  struct Launch { int grid; const Desc* first; int count, blk_base; };
  Launch range(int j0, int j1) const { return {blk0[j1] - blk0[j0], dev + j0, j1 - j0, blk0[j0]}; }
};

// The stem's weight gradient: at most STEM_WGRAD_SLABS runs of `rows_per_slab` output rows (b, oy), one workgroup of the engine's kernel
// and one 64 x 160 slab each, then the fixed-order sum of the slabs into dw [64][3][7][7].
struct StemSlabs { int rows_per_slab, n_slabs; };
StemSlabs stem_wgrad_split(int B, int Ho) {
  const int total_rows = B * Ho;
  const int rpb = (total_rows + STEM_WGRAD_SLABS - 1) / STEM_WGRAD_SLABS;
  return {rpb, (total_rows + rpb - 1) / rpb};
}
int stem_wgrad_reduce(const float* slabs, int n_slabs, float* dw, hipStream_t st) {
  hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3((64 * 147 + 31) / 32), dim3(256), 0, st, slabs, n_slabs, dw);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// the element range of the completion items [i0, i1): consecutive items are contiguous in the arena (ascending for the bf16 engine,
// descending for the float32 engine), so their union is one range; count 0 when they are not (or the interval is empty)
TrainStore::Range store_item_range(const TrainStore& s, size_t i0, size_t i1) {
  if (i0 >= i1 || i1 > s.items.size()) return {0, 0};
  int64_t lo = s.items[i0].first, hi = lo, sum = 0;
  for (size_t i = i0; i < i1; ++i) {
    lo = std::min(lo, s.items[i].first); hi = std::max(hi, s.items[i].first + s.items[i].second);
    sum += s.items[i].second;
  }
  return {lo, sum == hi - lo ? sum : 0};
}

// ---- the scheduler of a backward pass --------------------------------------------------------------------------------------------
// Which stream a weight gradient runs on, and what orders the two streams: the ONE copy of the rules both engines' passes follow.
// Without a side stream (s.side null) a weight gradient is launched on the main stream where it is queued and flush / join do nothing.
// With one, every convolution owns its dZ buffer (HBM is plentiful), so the main stream never waits for the side stream inside the pass;
// queued weight gradients are handed over in groups behind ONE event of the main stream (an event record or wait stalls the recording
// queue for about 6 us: one hand-off per convolution cost 0.67 ms of a 7.7 ms ResNet-50 step, profiles/r03_exp_side_handoff.txt).
//   queue   a conv's weight gradient (conv index, its input x, its dZ)
//   flush   one side_handoff, the queued gradients in queue order on the side stream; in a fused pass then the Adam update of the
//           completion items that are complete once the side stream gets there, and the repack of the flushed convs [lo, hi]
//   join    flush + side_join: everything handed over so far precedes what the main stream does next.  A gradient bucket's gradients,
//           the side stream's included, must precede the callback that fires it (store_mark_done): the engine joins before it marks
//           such an item done.  The optimiser after the pass needs one too.
//   tail    after the last item is marked done (and a join): in a fused pass Adam over what the side stream has not updated and the
//           repack of those convs, on the main stream -- the stem; the whole arena without a side stream
// `fused` (single-rank training): the Adam update and the repack of a group's tensors follow that group's weight gradients on the side
// stream, instead of one update of the whole arena after the pass (same arithmetic per element: identical parameters).  The cursor of
// that update counts COMPLETION ITEMS: items [0, cursor) are updated.  `completes` (flush, join) = how many items beyond those already
// marked done the queued gradients complete (float32 flushes a block before it marks it: 1; bf16 after: 0).
// The engine supplies  wgrad(conv, x, dz, stream)  and  repack(lo, hi, stream)  (convs lo .. hi inclusive; conv 0 is the stem).
// no_adam / no_side_repack: the timing-only ablations of diagnostic builds (DH_T1_ABL / DH_T2_ABL), false in the shipped library.
template <typename E, typename Wgrad, typename Repack> struct BwdSched {
  TrainStore& s;
  hipStream_t st;          // the main stream of the pass
  const AdamArgs* fused;   // null: no optimiser in the pass
  int n_convs;
  Wgrad wgrad;
  Repack repack;
  bool no_adam, no_side_repack;
  struct Pending { int conv; const E* x; const E* dz; };
  std::vector<Pending> pending;
  size_t cursor = 0;

  int queue(int conv, const E* x, const E* dz) {
    if (!s.side) return wgrad(conv, x, dz, st);
    pending.push_back({conv, x, dz});
    return DH_OK;
  }
  int flush(size_t completes) {
    if (pending.empty()) return DH_OK;
    int rc = side_handoff(s, st);
    if (rc) return rc;
    int lo = n_convs, hi = -1;
    for (const Pending& w : pending) {
      if ((rc = wgrad(w.conv, w.x, w.dz, s.side))) return rc;
      lo = std::min(lo, w.conv); hi = std::max(hi, w.conv);
    }
    if (fused) {
      const size_t upto = s.items_done + completes;
      const TrainStore::Range r = store_item_range(s, cursor, upto);
      DH_REQUIRE(hi - lo + 1 == (int)pending.size() && r.second > 0, "backward: the convolutions of a hand-off are not a contiguous range");
      if (!no_adam) adam_range(s, *fused, r.first, r.second, s.side);
      cursor = upto;
      if (!no_side_repack && (rc = repack(lo, hi, s.side))) return rc;
    }
    pending.clear();
    return DH_OK;
  }
  int join(size_t completes) {
    if (!s.side) return DH_OK;
    const int rc = flush(completes);
    return rc ? rc : side_join(s, st);
  }
  int tail() {
    if (!fused) return DH_OK;
    const TrainStore::Range r = store_item_range(s, cursor, s.items.size());
    if (!no_adam) adam_range(s, *fused, r.first, r.second, st);
    return repack(0, cursor == 0 ? n_convs - 1 : 0, st);
  }
};
template <typename E, typename Wgrad, typename Repack>
BwdSched<E, Wgrad, Repack> bwd_sched(TrainStore& s, hipStream_t st, const AdamArgs* fused, int n_convs, Wgrad wgrad, Repack repack,
                                     bool no_adam = false, bool no_side_repack = false) {
  return {s, st, fused, n_convs, wgrad, repack, no_adam, no_side_repack, {}, 0};
}

}  // namespace
