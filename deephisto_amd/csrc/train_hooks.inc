// train_hooks.inc -- included once by resnet_kernels.hip, after train2.inc.
//
// The test hooks of both training engines (train.inc: float32, train2.inc: bf16): every entry point here is declared and described
// in include/deephisto_hip_debug.h.  Each runs ONE building block of a training step on caller data through the engines' own launch
// code (tr_* / t2_*), so the GPU parity tests can hold every kernel against a float64 reference on its own instead of through the
// whole network; the three taps copy out what a real step left in memory.  The hooks allocate their own scratch and synchronise
// (the taps are stream-ordered); the product path never calls them, and no kernel is defined here.

namespace {
struct DbgScratch {
  std::vector<void*> a;
  ~DbgScratch() { for (void* p : a) (void)hipFree(p); }
  template <typename V> int get(V** p, int64_t n) { DH_HIP(hipMalloc((void**)p, (size_t)std::max<int64_t>(n, 1) * sizeof(V))); a.push_back(*p); return DH_OK; }
};
int dbg_finish(hipStream_t st, const char* what) {
  hipError_t e = hipStreamSynchronize(st);
  if (e != hipSuccess) { dh::set_error("%s: %s", what, hipGetErrorString(e)); return DH_EHIP; }
  return DH_OK;
}

// ---- fixtures of the float32 hooks -----------------------------------------------------------------------------------------
// a BnView over caller data: scratch per-channel buffers and reduction workspace, running statistics starting from (0, 1)
int dbg_bn_view(DbgScratch& sc, hipStream_t st, const float* z, const float* gamma, const float* beta, float* dgamma, float* dbeta, int64_t rows,
                int B, int Ho, int Wo, int C, BnView* v) {
  float *partial, *buf;
  int rc;
  if ((rc = sc.get(&partial, (int64_t)RED_NB * 2 * 512)) || (rc = sc.get(&buf, 9 * (int64_t)C))) return rc;
  *v = {z, gamma, beta, buf + 7 * C, buf + 8 * C, dgamma, dbeta,
        BnBufs{buf, buf + C, buf + 2 * C, buf + 3 * C, buf + 4 * C, buf + 5 * C, buf + 6 * C}, rows, C, B, Ho, Wo, partial};
  hipLaunchKernelGGL(fill_kernel, dim3(2), dim3(256), 0, st, v->run_mean, (int64_t)C, 0.0f);
  hipLaunchKernelGGL(fill_kernel, dim3(2), dim3(256), 0, st, v->run_var, (int64_t)C, 1.0f);
  return DH_OK;
}

// one convolution's weights w[cout][cin][ks][ks] through pack_all_f32_kernel, the grid as tr_pack counts it; waits for the descriptor copy
int dbg_pack_f32(DbgScratch& sc, hipStream_t st, const float* w, float* wf, float* wd, int cout, int cin, int ks) {
  const PackDescF hd{w, wf, wd, cout, cin, ks, 0};
  PackDescF* dd;
  int rc;
  if ((rc = sc.get(&dd, 1))) return rc;
  DH_HIP(hipMemcpyAsync(dd, &hd, sizeof hd, hipMemcpyHostToDevice, st));
  DH_HIP(hipStreamSynchronize(st));   // `hd` is a stack object
  hipLaunchKernelGGL(pack_all_f32_kernel, dim3(packf_blocks(cout, cin, ks)), dim3(256), PACKF_LDS, st, dd, 1, 0);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// ---- fixtures of the bf16 hooks --------------------------------------------------------------------------------------------
// A bf16 engine of one BN layer `c` over caller data (and a second one, `d`, the downsample branch of a join): one zeroed scratch
// buffer holds the parameter / gradient / running-statistic "arenas" (two channels-sized slots per layer each: gamma | beta, their
// gradients, running mean | var from zero) and each layer's coefficient arrays; t.partial has the engine's T2_PARTIAL_FLOATS.
struct DbgBn2 {
  dh_train2 t;
  T2Conv c, d;
};
int dbg_bn2_engine(DbgBn2& e, DbgScratch& sc, hipStream_t st, int B, int Ho, int Wo, int C, int ks, const float* gamma, const float* beta,
                   float* mean, float* invstd, const float* gamma2 = nullptr, const float* beta2 = nullptr, float* mean2 = nullptr,
                   float* invstd2 = nullptr) {
  dh_train2& t = e.t;
  t.B = B;
  int rc;
  float* buf;
  if ((rc = sc.get(&buf, (int64_t)22 * C)) || (rc = sc.get(&t.partial, T2_PARTIAL_FLOATS))) return rc;
  DH_HIP(hipMemsetAsync(buf, 0, 22 * C * sizeof(float), st));
  t.Pm = buf; t.G = buf + 4 * C; t.R = buf + 8 * C;
  const auto layer = [&](T2Conv& c, int i, const char* name, int lks, const float* g, const float* b, float* m, float* is) -> int {
    c.name = name; c.bn = name; c.cout = C; c.Ho = Ho; c.Wo = Wo; c.ks = lks;
    const int64_t o = (int64_t)2 * i * C;
    t.slot[c.bn + ".weight"] = {o, C}; t.slot[c.bn + ".bias"] = {o + C, C};
    t.rslot[c.bn + ".running_mean"] = {o, C}; t.rslot[c.bn + ".running_var"] = {o + C, C};
    DH_HIP(hipMemcpyAsync(t.Pm + o, g, C * sizeof(float), hipMemcpyDeviceToDevice, st));
    DH_HIP(hipMemcpyAsync(t.Pm + o + C, b, C * sizeof(float), hipMemcpyDeviceToDevice, st));
    float* k = buf + (12 + 5 * i) * (int64_t)C;
    c.bnb.mean = m; c.bnb.invstd = is; c.bnb.scale = k; c.bnb.shift = k + C; c.bnb.k0 = k + 2 * C; c.bnb.k1 = k + 3 * C; c.bnb.k2 = k + 4 * C;
    return DH_OK;
  };
  if ((rc = layer(e.c, 0, "dbgbn", ks, gamma, beta, mean, invstd))) return rc;
  return gamma2 ? layer(e.d, 1, "dbgds", 1, gamma2, beta2, mean2, invstd2) : DH_OK;
}

// dh_debug_bn2_bf16 and dh_debug_bn2_paths_bf16 behind their own argument checks.  fold < 0: the engine's default; z2 given: the join.
int dbg_bn2(const char* what, const uint16_t* z, const uint16_t* res, const float* gamma, const float* beta, int relu, int fold, uint16_t* y,
            uint8_t* bits, float* mean, float* invstd, const uint16_t* z2, const float* gamma2, const float* beta2, float* mean2, float* invstd2,
            const uint16_t* dy, int relu_mode, uint16_t* dz, uint16_t* g_out, float* dgamma, float* dbeta, int64_t rows, int C, hipStream_t st) {
  DbgScratch sc;
  DbgBn2 e;
  int rc;
  if ((rc = dbg_bn2_engine(e, sc, st, 1, 1, (int)rows, C, 3, gamma, beta, mean, invstd, z2 ? gamma2 : nullptr, beta2, mean2, invstd2))) return rc;
  if (fold >= 0) e.t.fold = fold != 0;
  e.c.Z = const_cast<bf16_t*>(z); e.c.Y = y;
  if (z2) {   // the branch BN: statistics and coefficients only, applied inside the top BN's pass
    e.d.Z = const_cast<bf16_t*>(z2);
    if ((rc = t2_bn_fwd(&e.t, e.d, nullptr, false, true, st, false, nullptr, nullptr, false))) return rc;
  }
  if ((rc = t2_bn_fwd(&e.t, e.c, res, relu != 0, true, st, false, nullptr, nullptr, true, z2 ? &e.d : nullptr, 0, bits))) return rc;
  if (dy) {
    if ((rc = t2_bn_bwd(&e.t, e.c, dy, relu_mode == 1 ? y : nullptr, relu_mode, dz, g_out, st))) return rc;
    DH_HIP(hipMemcpyAsync(dgamma, e.t.G, C * sizeof(float), hipMemcpyDeviceToDevice, st));
    DH_HIP(hipMemcpyAsync(dbeta, e.t.G + C, C * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  return dbg_finish(st, what);
}

// a scratch convolution "dbg" of the bf16 engine: the description and its map sizes (pad ks / 2), no buffers
T2Conv dbg_conv_bf16(int cin, int cout, int ks, int stride, int Hi, int Wi) {
  T2Conv c;
  c.name = "dbg"; c.cin = cin; c.cout = cout; c.ks = ks; c.stride = stride;
  c.Hi = Hi; c.Wi = Wi; c.Ho = (Hi + 2 * (ks / 2) - ks) / stride + 1; c.Wo = (Wi + 2 * (ks / 2) - ks) / stride + 1;
  return c;
}

// one convolution's weights w[cout][cin][ks][ks] (ks 1 or 3) through pack_all_kernel, the grid as t2_pack counts it; waits for the descriptor copy
int dbg_pack_bf16(DbgScratch& sc, hipStream_t st, const float* w, bf16_t* wf, bf16_t* wd, int cout, int cin, int ks) {
  const PackDesc hd{w, wf, wd, cout, cin, ks, 0};
  PackDesc* dd;
  int rc;
  if ((rc = sc.get(&dd, 1))) return rc;
  DH_HIP(hipMemcpyAsync(dd, &hd, sizeof hd, hipMemcpyHostToDevice, st));
  DH_HIP(hipStreamSynchronize(st));   // `hd` is a stack object
  if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(&pack_all_kernel), PACK3_LDS))) return rc;
  const int tiles = (cout / 64) * (cin / 64);
  hipLaunchKernelGGL(pack_all_kernel, dim3(ks == 3 ? tiles : std::min(64, tiles)), dim3(256), PACK3_LDS, st, dd, 1, 0);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// the ReLU pattern of a bf16 tensor [M][N] as bytes (st8_bits), the form the engine hands a GEMM its mask in
int dbg_mask_bits(DbgScratch& sc, hipStream_t st, const uint16_t* mask, int64_t M, int N, const uint8_t** bits) {
  uint8_t* mb = nullptr;
  int rc;
  if ((rc = sc.get(&mb, M * N / 8))) return rc;
  hipLaunchKernelGGL(relu_bits_pack_kernel, dim3(grid_for(M * N / 8)), dim3(256), 0, st, mask, mb, M * N / 8);
  *bits = mb;
  return DH_OK;
}

int dbg_maxpool2(const char* what, const uint16_t* x, uint16_t* y, uint8_t* idx, const uint16_t* dy, uint16_t* dx, int B, int Hi, int Wi, int C,
                 hipStream_t st) {
  const int Ho = (Hi + 2 - 3) / 2 + 1, Wo = (Wi + 2 - 3) / 2 + 1;
  hipLaunchKernelGGL(maxpool2_fwd_idx_kernel, dim3(grid_for((int64_t)B * Ho * Wo * C / 8)), dim3(256), 0, st, x, y, idx, B, Hi, Wi, C, Ho, Wo);
  if (dy)
    hipLaunchKernelGGL(maxpool2_bwd_kernel, dim3(grid_for((int64_t)B * Hi * Wi * C / 8)), dim3(256), 0, st, idx, dy, dx, B, Hi, Wi, C, Ho, Wo);
  DH_LAUNCH_CHECK();
  return dbg_finish(st, what);
}
}  // namespace

// =====================================================================================
// Taps: tensors of the last training forward / backward
// =====================================================================================
// float32 engine.  The stem's dZ lives in BIG1, which nothing else uses; read-only: the stem's Y, which the engine never stores, is refused.
extern "C" int dh_resnet18_train_debug_act(dh_resnet18* net, const char* conv_name, int32_t what, float* out_dev, int64_t n_elem, void* stream) {
  DH_REQUIRE(net && net->train && conv_name && out_dev && net->train->B > 0 && net->train->x_in, "train debug: bad arguments / no training forward");
  DH_REQUIRE(what >= 0 && what <= 3, "train debug: what = %d (0 Z, 1 Y, 2 dZ, 3 X1)", what);
  const dh_train* t = net->train;
  for (size_t i = 0; i < t->convs.size(); ++i)
    if (t->convs[i].name == conv_name) {
      const TrainConv& tc = t->convs[i];
      DH_REQUIRE(what != 3 || i == 0, "train debug: what = 3 (X1, the pooled block input) goes with 'conv1', not '%s'", conv_name);
      DH_REQUIRE(what != 1 || i != 0, "train debug: what = 1 (Y) of 'conv1' is not kept (the stem pools in its BN pass: what = 3)");
      const int H2 = (tc.Ho + 2 - 3) / 2 + 1;
      const int64_t n = what == 3 ? (int64_t)t->B * H2 * H2 * 64 : (int64_t)t->B * tc.Ho * tc.Wo * tc.cout;
      DH_REQUIRE(n == n_elem, "train debug: n_elem = %lld, '%s' (what = %d) has %lld elements", (long long)n_elem, conv_name, what, (long long)n);
      if (what == 2) {
        DH_REQUIRE(t->side != nullptr, "train debug: what = 2 (dZ) needs the per-convolution dZ buffers of the side-stream engine (created with DH_T1_SIDE=0)");
        DH_REQUIRE(t->bwd_done, "train debug: what = 2 (dZ): no backward has run since the last forward");
      }
      const float* src = what == 0 ? tc.Z : what == 1 ? tc.Y : what == 3 ? t->X1 : i == 0 ? t->BIG1 : tc.dZ;
      DH_HIP(hipMemcpyAsync(out_dev, src, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, dh::as_stream(stream)));
      return DH_OK;
    }
  dh::set_error("train debug: unknown conv_name '%s'", conv_name);
  return DH_EINVAL;
}

// bf16 engine.  The stem's dZ lives in GB[2], which the side-stream engine uses for nothing else; read-only but for what = 1 on the
// stem, which rebuilds Y from Z.
extern "C" int dh_train2_debug_act(dh_train2* t, const char* conv_name, int32_t what, float* out_dev, int64_t n_elem, void* stream) {
  DH_REQUIRE(t && conv_name && out_dev && t->B > 0, "train2 debug: bad arguments / no forward");
  DH_REQUIRE(what >= 0 && what <= 3, "train2 debug: what = %d (0 Z, 1 Y, 2 dZ, 3 X1)", what);
  hipStream_t st = dh::as_stream(stream);
  for (const T2Conv& c : t->convs)
    if (c.name == conv_name) {
      const bool stem = &c == &t->convs[0];
      DH_REQUIRE(what != 3 || stem, "train2 debug: what = 3 (X1, the pooled block input) goes with 'conv1', not '%s'", conv_name);
      const int H2 = (c.Ho + 2 - 3) / 2 + 1;
      const int64_t n = what == 3 ? (int64_t)t->B * H2 * H2 * 64 : (int64_t)t->B * c.Ho * c.Wo * c.cout;
      DH_REQUIRE(n == n_elem, "train2 debug: n_elem = %lld, '%s' (what = %d) has %lld elements", (long long)n_elem, conv_name, what, (long long)n);
      const bf16_t* src = what == 0 ? c.Z : what == 1 ? c.Y : what == 3 ? t->X1 : stem ? t->GB[2] : c.dZ;
      if (what == 2) {
        DH_REQUIRE(t->side_wgrad, "train2 debug: what = 2 (dZ) needs the per-convolution dZ buffers of the side-stream engine (created with DH_T2_SIDE=0)");
        DH_REQUIRE(t->bwd_done, "train2 debug: what = 2 (dZ): no backward has run since the last forward");
      }
      if (what == 1 && stem)   // the stem's normalised map is not kept (bn2_apply_pool_kernel): made here from Z and the saved coefficients
        hipLaunchKernelGGL(bn2_apply_kernel, dim3(grid_for(n / 8)), dim3(256), 0, st, c.Z, c.bnb.scale, c.bnb.shift,
                           static_cast<const bf16_t*>(nullptr), c.Y, n / 8, c.cout, 1);
      hipLaunchKernelGGL(bf16_to_f32_kernel, dim3(grid_for(n)), dim3(256), 0, st, src, out_dev, n);
      DH_LAUNCH_CHECK();
      return DH_OK;
    }
  dh::set_error("train2 debug: unknown conv_name '%s'", conv_name);
  return DH_EINVAL;
}

// The same t2_backward, the same launches in the same order; the copies read buffers of the pass between their writer and their next
// writer, on the same stream.
extern "C" int dh_train2_debug_backward_tap(dh_train2* t, const float* dlogits, const char* conv_name, float* grad_in_dev, int64_t n_elem,
                                            float* g_out_dev, float* mean_dev, float* invstd_dev, int32_t* route_host, void* stream) {
  DH_REQUIRE(t && dlogits && conv_name && grad_in_dev && mean_dev && invstd_dev && route_host, "train2 backward tap: null argument");
  DH_REQUIRE(t->B > 0 && t->last_training && !t->bwd_done,
             "train2 backward tap: no training forward has run since the last backward (every tapped backward follows a forward of its own)");
  hipStream_t st = dh::as_stream(stream);
  for (size_t ci = 0; ci < t->convs.size(); ++ci) {
    const T2Conv& c = t->convs[ci];
    if (c.name != conv_name) continue;
    const int Hp = (c.Ho + 2 - 3) / 2 + 1, Wp = (c.Wo + 2 - 3) / 2 + 1;
    const int64_t n = ci == 0 ? (int64_t)t->B * Hp * Wp * c.cout : (int64_t)t->B * c.Ho * c.Wo * c.cout;
    DH_REQUIRE(n == n_elem, "train2 backward tap: n_elem = %lld, grad_in of '%s' has %lld elements", (long long)n_elem, conv_name, (long long)n);
    bool writes_g_out = false;   // the top BN of a block that is not pre-masked
    for (int bi = 0; bi < (int)t->blocks.size(); ++bi) {
      const BlockDesc& b = t->blocks[bi];
      if (b.conv[b.nconv - 1] == (int)ci) writes_g_out = !t2_premasked(t, bi);
    }
    DH_REQUIRE(!g_out_dev || writes_g_out, "train2 backward tap: g_out_dev given, but the BN of '%s' writes no masked gradient (pass NULL)", conv_name);
    const T2BwdTap tap{&c, grad_in_dev, g_out_dev, route_host};
    for (int i = 0; i < T2R_N; ++i) route_host[i] = -1;
    int rc = t2_backward(t, dlogits, st, nullptr, &tap);
    if (rc) return rc;
    DH_HIP(hipMemcpyAsync(mean_dev, c.bnb.mean, (size_t)c.cout * sizeof(float), hipMemcpyDeviceToDevice, st));
    DH_HIP(hipMemcpyAsync(invstd_dev, c.bnb.invstd, (size_t)c.cout * sizeof(float), hipMemcpyDeviceToDevice, st));
    return DH_OK;
  }
  dh::set_error("train2 backward tap: unknown conv_name '%s'", conv_name);
  return DH_EINVAL;
}

// =====================================================================================
// Float32 engine: one backward building block per hook, as dh_resnet18_backward launches it
// =====================================================================================
// mode 0 = the path backward takes, 1 = force the per-tap kernel
extern "C" int dh_debug_wgrad_f32(const float* dz_dev, const float* x_dev, float* dw_dev, int32_t B, int32_t Hi, int32_t Wi, int32_t cin,
                                  int32_t cout, int32_t ks, int32_t stride, int32_t mode, void* stream) {
  DH_REQUIRE(dz_dev && x_dev && dw_dev && (ks == 1 || ks == 3) && cin % 64 == 0 && cout % 64 == 0, "debug wgrad: bad arguments");
  hipStream_t st = dh::as_stream(stream);
  DbgScratch sc;
  float* slabs;
  int rc = sc.get(&slabs, (int64_t)WGRAD3_WGS * 9 * 64 * 64);
  if (rc) return rc;
  TrainConv c;
  c.name = c.bn = "dbg"; c.cin = cin; c.cout = cout; c.ks = ks; c.stride = stride;
  c.Hi = Hi; c.Wi = Wi; c.Ho = (Hi + 2 * (ks / 2) - ks) / stride + 1; c.Wo = (Wi + 2 * (ks / 2) - ks) / stride + 1;
  if ((rc = tr_wgrad(slabs, dw_dev, c, x_dev, dz_dev, B, st, mode == 1))) return rc;
  return dbg_finish(st, "debug wgrad");
}

extern "C" int dh_debug_stem_wgrad_f32(const float* dz_dev, const float* x_nchw_dev, float* dw_dev, int32_t B, int32_t P, void* stream) {
  DH_REQUIRE(dz_dev && x_nchw_dev && dw_dev && B > 0 && P >= 32 && P % 2 == 0, "debug stem wgrad: bad arguments");
  hipStream_t st = dh::as_stream(stream);
  DbgScratch sc;
  float* slabs;
  int rc = sc.get(&slabs, (int64_t)STEM_WGRAD_SLABS * 64 * 160);
  if (rc) return rc;
  if ((rc = tr_stem_wgrad(dz_dev, x_nchw_dev, slabs, dw_dev, B, P, P / 2, P / 2, st))) return rc;
  return dbg_finish(st, "debug stem wgrad");
}

// the training step's sub-tile kernel (wf_tile, wd_tile) next to the element-wise kernel of the inference load path (wf_elem, wd_elem)
extern "C" int dh_debug_pack_f32(const float* w_dev, int32_t cout, int32_t cin, float* wf_tile, float* wd_tile, float* wf_elem,
                                 float* wd_elem, void* stream) {
  DH_REQUIRE(w_dev && wf_tile && wd_tile && wf_elem && wd_elem && cout > 0 && cin > 0 && cout % 64 == 0 && cin % 64 == 0, "debug pack: bad arguments");
  hipStream_t st = dh::as_stream(stream);
  DbgScratch sc;
  int rc;
  if ((rc = dbg_pack_f32(sc, st, w_dev, wf_tile, wd_tile, cout, cin, 3))) return rc;
  const int64_t nw = (int64_t)cout * cin * 9;
  hipLaunchKernelGGL((pack_conv_dev_kernel<float, false>), dim3(grid_for(nw)), dim3(256), 0, st, w_dev, cout, cin, 3, wf_elem);
  hipLaunchKernelGGL((pack_conv_dev_kernel<float, true>), dim3(grid_for(nw)), dim3(256), 0, st, w_dev, cout, cin, 3, wd_elem);
  DH_LAUNCH_CHECK();
  return dbg_finish(st, "debug pack");
}

// the flipped / transposed operand is packed on the device; stride 2 goes through the four parity classes of dX (3x3) or the
// low-resolution product (1x1)
extern "C" int dh_debug_dgrad_f32(const float* dz_dev, const float* w_dev, const float* res_dev, float* dx_dev, int32_t B, int32_t Hi,
                                  int32_t Wi, int32_t cin, int32_t cout, int32_t ks, int32_t stride, void* stream) {
  DH_REQUIRE(dz_dev && w_dev && dx_dev && (ks == 1 || ks == 3) && (stride == 1 || stride == 2) && cin % 64 == 0 && cout % 64 == 0,
             "debug dgrad: bad arguments");
  hipStream_t st = dh::as_stream(stream);
  DbgScratch sc;
  const int Ho = (Hi + 2 * (ks / 2) - ks) / stride + 1, Wo = (Wi + 2 * (ks / 2) - ks) / stride + 1;
  const int64_t nw = (int64_t)cout * cin * ks * ks;
  float *wp_d, *ones, *zeros;
  int rc;
  if ((rc = sc.get(&wp_d, nw)) || (rc = sc.get(&ones, 512)) || (rc = sc.get(&zeros, 512))) return rc;
  const UnitAffine u{ones, zeros};
  hipLaunchKernelGGL(fill_kernel, dim3(2), dim3(256), 0, st, ones, (int64_t)512, 1.0f);
  hipLaunchKernelGGL(fill_kernel, dim3(2), dim3(256), 0, st, zeros, (int64_t)512, 0.0f);
  if (ks == 1) {   // the 1x1 data gradient is a GEMM over the transposed weights Wt[cin][cout] (what pack_all_f32_kernel keeps)
    if ((rc = dbg_pack_f32(sc, st, w_dev, wp_d, wp_d, cout, cin, 1))) return rc;
  } else {
    hipLaunchKernelGGL((pack_conv_dev_kernel<float, true>), dim3(grid_for(nw)), dim3(256), 0, st, w_dev, cout, cin, ks, wp_d);
  }
  if (ks == 3 && stride == 1) rc = tr_conv(u, cout, cin, 3, 1, wp_d, dz_dev, res_dev, dx_dev, B, Ho, Wo, st);
  else if (ks == 3) rc = tr_dgrad_s2(u, cout, cin, wp_d, dz_dev, res_dev, dx_dev, B, Ho, Wo, Hi, Wi, st);   // the parity classes of dX over dZ itself
  else if (stride == 1) rc = tr_conv(u, cout, cin, 1, 1, wp_d, dz_dev, res_dev, dx_dev, B, Ho, Wo, st);
  else {   // 1x1 stride 2 (downsample branch): dx (+)= upsample(conv1x1(dz)); dx starts from res (or zero)
    float* up;
    if ((rc = sc.get(&up, (int64_t)B * Ho * Wo * cin))) return rc;
    const int64_t nx = (int64_t)B * Hi * Wi * cin;
    if (res_dev) (void)hipMemcpyAsync(dx_dev, res_dev, nx * 4, hipMemcpyDeviceToDevice, st);
    else (void)hipMemsetAsync(dx_dev, 0, nx * 4, st);
    rc = tr_conv(u, cout, cin, 1, 1, wp_d, dz_dev, nullptr, up, B, Ho, Wo, st);
    const int64_t m4 = (int64_t)B * Ho * Wo * cin / 4;
    if (!rc) hipLaunchKernelGGL(upsample2_add_kernel, dim3(grid_for(m4)), dim3(256), 0, st, up, dx_dev, B, Ho, Wo, cin);
  }
  if (rc) return rc;
  DH_LAUNCH_CHECK();
  return dbg_finish(st, "debug dgrad");
}

// through tr_bn_forward / tr_bn_backward
extern "C" int dh_debug_bn_f32(const float* z_dev, const float* gamma_dev, const float* beta_dev, const float* res_dev, int32_t relu,
                               float* y_dev, const float* dy_dev, float* dz_dev, float* g_dev, float* dgamma_dev, float* dbeta_dev,
                               float* stats_out_dev, int64_t rows, int32_t C, void* stream) {
  DH_REQUIRE(z_dev && gamma_dev && beta_dev && y_dev && rows > 0 && C % 4 == 0 && C <= 512 && 256 % (C / 4) == 0, "debug bn: bad arguments");
  DH_REQUIRE(relu >= 0 && relu <= 2, "debug bn: relu=%d (0 none, 1 pattern from y, 2 pattern recomputed from z)", relu);
  DH_REQUIRE(relu != 2 || (!res_dev && !g_dev), "debug bn: relu=2 (pattern recomputed from z) takes neither res_dev nor g_dev");
  DH_REQUIRE(!dy_dev || (dz_dev && dgamma_dev && dbeta_dev), "debug bn: backward outputs missing");
  hipStream_t st = dh::as_stream(stream);
  DbgScratch sc;
  BnView v;
  int rc;
  if ((rc = dbg_bn_view(sc, st, z_dev, gamma_dev, beta_dev, dgamma_dev, dbeta_dev, rows, 0, 0, 0, C, &v))) return rc;
  if ((rc = tr_bn_forward(v, res_dev, relu != 0, y_dev, st))) return rc;
  if (dy_dev && (rc = tr_bn_backward(v, dy_dev, relu == 1 ? y_dev : nullptr, relu != 0, dz_dev, g_dev, st))) return rc;
  if (stats_out_dev) {
    (void)hipMemcpyAsync(stats_out_dev, v.bn.mean, C * 4, hipMemcpyDeviceToDevice, st);
    (void)hipMemcpyAsync(stats_out_dev + C, v.bn.invstd, C * 4, hipMemcpyDeviceToDevice, st);
    (void)hipMemcpyAsync(stats_out_dev + 2 * C, v.run_mean, 2 * (size_t)C * 4, hipMemcpyDeviceToDevice, st);
  }
  DH_LAUNCH_CHECK();
  return dbg_finish(st, "debug bn");
}

// through tr_bn_forward with a pooled target and tr_bn_pool_backward
extern "C" int dh_debug_bn_pool_f32(const float* z_dev, const float* gamma_dev, const float* beta_dev, float* pooled_dev, uint8_t* idx_dev,
                                    const float* dpool_dev, float* dz_dev, float* dgamma_dev, float* dbeta_dev, int32_t B, int32_t Hi, int32_t Wi,
                                    int32_t C, void* stream) {
  DH_REQUIRE(z_dev && gamma_dev && beta_dev && pooled_dev && idx_dev && B > 0 && Hi > 0 && Wi > 0 && C % 4 == 0 && C <= 512 && 256 % (C / 4) == 0,
             "debug bn pool: bad arguments");
  DH_REQUIRE(!dpool_dev || (dz_dev && dgamma_dev && dbeta_dev), "debug bn pool: backward outputs missing");
  hipStream_t st = dh::as_stream(stream);
  DbgScratch sc;
  BnView v;
  int rc;
  if ((rc = dbg_bn_view(sc, st, z_dev, gamma_dev, beta_dev, dgamma_dev, dbeta_dev, (int64_t)B * Hi * Wi, B, Hi, Wi, C, &v))) return rc;
  if ((rc = tr_bn_forward(v, nullptr, true, nullptr, st, pooled_dev, idx_dev))) return rc;
  if (dpool_dev && (rc = tr_bn_pool_backward(v, dpool_dev, idx_dev, dz_dev, st))) return rc;
  return dbg_finish(st, "debug bn pool");
}

extern "C" int dh_debug_maxpool_f32(const float* x_dev, float* y_dev, const float* dy_dev, float* dx_dev, int32_t B, int32_t Hi, int32_t Wi,
                                    int32_t C, void* stream) {
  DH_REQUIRE(x_dev && y_dev && C % 4 == 0 && B > 0, "debug maxpool: bad arguments");
  hipStream_t st = dh::as_stream(stream);
  const int Ho = (Hi + 2 - 3) / 2 + 1, Wo = (Wi + 2 - 3) / 2 + 1;
  DbgScratch sc;
  uint8_t* idx;
  int rc = sc.get(&idx, (int64_t)B * Ho * Wo * C);
  if (rc) return rc;
  const int64_t n4 = (int64_t)B * Ho * Wo * C / 4;
  hipLaunchKernelGGL(maxpool_fwd_idx_kernel, dim3(grid_for(n4)), dim3(256), 0, st, x_dev, y_dev, idx, B, Hi, Wi, C, Ho, Wo);
  if (dy_dev) {
    DH_REQUIRE(dx_dev != nullptr, "debug maxpool: dx missing");
    const int64_t m4 = (int64_t)B * Hi * Wi * C / 4;
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(grid_for(m4)), dim3(256), 0, st, idx, dy_dev, dx_dev, B, Hi, Wi, C, Ho, Wo);
  }
  DH_LAUNCH_CHECK();
  return dbg_finish(st, "debug maxpool");
}

// =====================================================================================
// bf16 engine: one kernel or one piece of the step's launch code per hook (bf16 bits as uint16 on the device)
// =====================================================================================
// the engine's re-pack kernel (wf_tile, wd_tile) next to the element-wise packer of the inference load path (wf_elem, wd_elem)
extern "C" int dh_debug_pack_bf16(const float* w_dev, int32_t cout, int32_t cin, uint16_t* wf_tile, uint16_t* wd_tile, uint16_t* wf_elem,
                                  uint16_t* wd_elem, void* stream) {
  DH_REQUIRE(w_dev && wf_tile && wd_tile && wf_elem && wd_elem && cout > 0 && cin > 0 && cout % 64 == 0 && cin % 64 == 0, "debug pack: bad arguments");
  hipStream_t st = dh::as_stream(stream);
  DbgScratch sc;
  int rc;
  if ((rc = dbg_pack_bf16(sc, st, w_dev, wf_tile, wd_tile, cout, cin, 3))) return rc;
  const int64_t nw = (int64_t)cout * cin * 9;
  hipLaunchKernelGGL((pack_conv_dev_kernel<uint16_t, false>), dim3(grid_for(nw)), dim3(256), 0, st, w_dev, cout, cin, 3, wf_elem);
  hipLaunchKernelGGL((pack_conv_dev_kernel<uint16_t, true>), dim3(grid_for(nw)), dim3(256), 0, st, w_dev, cout, cin, 3, wd_elem);
  DH_LAUNCH_CHECK();
  return dbg_finish(st, "debug pack");
}

extern "C" int dh_debug_gemm1x1_bf16(const uint16_t* a_dev, const uint16_t* w_dev, const uint16_t* res_dev, uint16_t* out_dev, int64_t M,
                                     int32_t N, int32_t K, int32_t stride, int32_t Ho, int32_t Wo, int32_t Hi, int32_t Wi, int32_t repeat,
                                     void* stream) {
  DH_REQUIRE(a_dev && w_dev && out_dev && repeat >= 1, "debug gemm: bad arguments");
  hipStream_t st = dh::as_stream(stream);
  for (int i = 0; i < repeat; ++i) {
    GemmFuse fu;
    fu.res = res_dev;
    int rc = t2_gemm(a_dev, w_dev, out_dev, M, N, K, stride, Ho, Wo, Hi, Wi, fu, st);
    if (rc) return rc;
  }
  return dbg_finish(st, "debug gemm");
}

// mean / invstd as the BN coefficients come out of the fixed-point accumulator (eps 1e-5, biased variance) from the per-tile partial
// rows and the finalize launch
extern "C" int dh_debug_gemm1x1_fused_bf16(const uint16_t* a_dev, const uint16_t* w_dev, const uint16_t* res_dev, const uint16_t* mask_dev,
                                           uint16_t* out_dev, float* mean_dev, float* invstd_dev, int64_t M, int32_t N, int32_t K,
                                           int32_t stride, int32_t Ho, int32_t Wo, int32_t Hi, int32_t Wi, int32_t repeat, void* stream) {
  DH_REQUIRE(a_dev && w_dev && out_dev && repeat >= 1 && N > 0 && N <= 2048, "debug gemm fused: bad arguments");
  DH_REQUIRE((mean_dev == nullptr) == (invstd_dev == nullptr), "debug gemm fused: mean and invstd come together");
  hipStream_t st = dh::as_stream(stream);
  DbgScratch sc;
  GemmFuse fu;
  fu.res = res_dev;
  int rc;
  if (mask_dev) {
    DH_REQUIRE(stride == 1, "debug gemm fused: the mask rides on the stride-1 GEMM");
    if ((rc = dbg_mask_bits(sc, st, mask_dev, M, N, &fu.mask_bits))) return rc;
  }
  float* tmp = nullptr;
  BnFinal f{};
  const int64_t MB = (M + G2_BM - 1) / G2_BM;
  if (mean_dev) {
    DH_REQUIRE(MB * 2 * N <= T2_PARTIAL_FLOATS, "debug gemm fused: too many pixel tiles for the statistics buffer");
    if ((rc = sc.get(&fu.partial, MB * 2 * N)) || (rc = sc.get(&tmp, (int64_t)6 * N))) return rc;
    DH_HIP(hipMemsetAsync(tmp, 0, 6 * N * sizeof(float), st));
    hipLaunchKernelGGL(fill_kernel, dim3(8), dim3(256), 0, st, tmp, (int64_t)N, 1.0f);   // gamma = 1 (beta = 0)
    f.mean = mean_dev; f.invstd = invstd_dev; f.gamma = tmp; f.beta = tmp + N; f.scale = tmp + 2 * N;
    f.shift = tmp + 3 * N; f.run_mean = tmp + 4 * N; f.run_var = tmp + 5 * N; f.n_rows = (double)M;
  }
  for (int i = 0; i < repeat; ++i) {
    if ((rc = t2_gemm(a_dev, w_dev, out_dev, M, N, K, stride, Ho, Wo, Hi, Wi, fu, st))) return rc;
    if (fu.partial) {
      hipLaunchKernelGGL(bn_stat_finalize_onepass_kernel, dim3((N + FIN_CH - 1) / FIN_CH), dim3(256), 0, st, fu.partial, (int)MB, N, f.n_rows, f.mean, f.invstd,
                         f.gamma, f.beta, f.scale, f.shift, f.run_mean, f.run_var);
      DH_LAUNCH_CHECK();
    }
  }
  return dbg_finish(st, "debug gemm fused");
}

// sums_dev: the per-tile rows added up in double, as the finalize launch does
extern "C" int dh_debug_gemm1x1_bwdsums_bf16(const uint16_t* a_dev, const uint16_t* w_dev, const uint16_t* res_dev, const uint16_t* mask_dev,
                                             uint16_t* out_dev, const uint16_t* z_dev, const float* mean_dev, const float* invstd_dev,
                                             const float* scale_dev, const float* shift_dev, int32_t relu_mode, float* sums_dev, int64_t M,
                                             int32_t N, int32_t K, void* stream) {
  DH_REQUIRE(a_dev && w_dev && out_dev && z_dev && mean_dev && invstd_dev && sums_dev && (relu_mode == 0 || (relu_mode == 2 && scale_dev && shift_dev)),
             "debug gemm bwd sums: bad arguments");
  hipStream_t st = dh::as_stream(stream);
  DbgScratch sc;
  const int64_t MB = (M + G2_BM - 1) / G2_BM;
  DH_REQUIRE(MB * 2 * N <= T2_PARTIAL_FLOATS, "debug gemm bwd sums: too many pixel tiles for the rows buffer");
  GemmFuse fu;
  fu.res = res_dev;
  float *ones, *scratch;
  int rc;
  if (mask_dev && (rc = dbg_mask_bits(sc, st, mask_dev, M, N, &fu.mask_bits))) return rc;
  if ((rc = sc.get(&fu.partial, MB * 2 * N)) || (rc = sc.get(&ones, (int64_t)N)) || (rc = sc.get(&scratch, (int64_t)3 * N))) return rc;
  T2Conv bn;
  bn.cout = N; bn.Z = const_cast<bf16_t*>(z_dev);
  bn.bnb.mean = const_cast<float*>(mean_dev); bn.bnb.invstd = const_cast<float*>(invstd_dev);
  bn.bnb.scale = const_cast<float*>(scale_dev); bn.bnb.shift = const_cast<float*>(shift_dev);
  fu.bwd_of = &bn; fu.bwd_relu = relu_mode;
  if ((rc = t2_gemm(a_dev, w_dev, out_dev, M, N, K, 1, 1, 1, 1, 1, fu, st))) return rc;
  // column sums of the rows through the engine's finalize kernel: dgamma = sum g xhat, dbeta = sum g
  hipLaunchKernelGGL(fill_kernel, dim3(8), dim3(256), 0, st, ones, (int64_t)N, 1.0f);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((N + FIN_CH - 1) / FIN_CH), dim3(256), 0, st, fu.partial, (int)MB, N, (double)M, ones, mean_dev, invstd_dev,
                     sums_dev + N, sums_dev, scratch, scratch + N, scratch + 2 * N);
  DH_LAUNCH_CHECK();
  return dbg_finish(st, "debug gemm bwd sums");
}

// through t2_bn_fwd / t2_bn_bwd: the engine's default fold, no pattern bytes, no join
extern "C" int dh_debug_bn2_bf16(const uint16_t* z_dev, const uint16_t* res_dev, const float* gamma_dev, const float* beta_dev, int32_t relu,
                                 uint16_t* y_dev, float* mean_dev, float* invstd_dev, const uint16_t* dy_dev, int32_t relu_mode,
                                 uint16_t* dz_dev, uint16_t* g_out_dev, float* dgamma_dev, float* dbeta_dev, int64_t rows, int32_t C,
                                 void* stream) {
  DH_REQUIRE(z_dev && gamma_dev && beta_dev && y_dev && mean_dev && invstd_dev && rows > 0 && C >= 64 && C <= 2048 && C % 64 == 0 &&
             (256 % (C / 8) == 0 || (C / 8) % 256 == 0), "debug bn2: bad arguments");
  DH_REQUIRE(!dy_dev || (dz_dev && dgamma_dev && dbeta_dev && relu_mode >= 0 && relu_mode <= 2), "debug bn2: backward needs dz, dgamma, dbeta");
  DH_REQUIRE(rows < ((int64_t)1 << 31), "debug bn2: too many rows");
  return dbg_bn2("debug bn2", z_dev, res_dev, gamma_dev, beta_dev, relu, -1, y_dev, nullptr, mean_dev, invstd_dev, nullptr, nullptr, nullptr, nullptr,
                 nullptr, dy_dev, relu_mode, dz_dev, g_out_dev, dgamma_dev, dbeta_dev, rows, C, dh::as_stream(stream));
}

extern "C" int dh_debug_bn2_paths_bf16(const uint16_t* z_dev, const uint16_t* res_dev, const float* gamma_dev, const float* beta_dev, int32_t relu,
                                       int32_t fold, uint16_t* y_dev, uint8_t* bits_dev, float* mean_dev, float* invstd_dev,
                                       const uint16_t* z2_dev, const float* gamma2_dev, const float* beta2_dev, float* mean2_dev,
                                       float* invstd2_dev, const uint16_t* dy_dev, int32_t relu_mode, uint16_t* dz_dev, uint16_t* g_out_dev,
                                       float* dgamma_dev, float* dbeta_dev, int64_t rows, int32_t C, void* stream) {
  DH_REQUIRE(z_dev && gamma_dev && beta_dev, "debug bn2 paths: null input (z_dev, gamma_dev or beta_dev)");
  DH_REQUIRE(y_dev && mean_dev && invstd_dev, "debug bn2 paths: null output (y_dev, mean_dev or invstd_dev)");
  DH_REQUIRE(rows > 0 && rows < ((int64_t)1 << 31), "debug bn2 paths: rows=%lld", (long long)rows);
  DH_REQUIRE(C >= 64 && C <= 2048 && C % 64 == 0 && (256 % (C / 8) == 0 || (C / 8) % 256 == 0), "debug bn2 paths: C=%d (64 ... 2048, C / 8 divides 256)", C);
  DH_REQUIRE(fold == 0 || fold == 1, "debug bn2 paths: fold=%d (0 or 1)", fold);
  DH_REQUIRE(relu == 0 || relu == 1, "debug bn2 paths: relu=%d (0 or 1)", relu);
  const bool join = z2_dev || gamma2_dev || beta2_dev || mean2_dev || invstd2_dev;
  DH_REQUIRE(!join || (z2_dev && gamma2_dev && beta2_dev && mean2_dev && invstd2_dev),
             "debug bn2 paths: the join needs z2_dev, gamma2_dev, beta2_dev, mean2_dev and invstd2_dev together");
  DH_REQUIRE(!join || (relu == 1 && !res_dev), "debug bn2 paths: the join is a ReLU'd BN without res_dev (relu=%d)", relu);
  DH_REQUIRE(!dy_dev || (dz_dev && dgamma_dev && dbeta_dev), "debug bn2 paths: backward (dy_dev given) needs dz_dev, dgamma_dev and dbeta_dev");
  DH_REQUIRE(!dy_dev || (relu_mode >= 0 && relu_mode <= 2), "debug bn2 paths: relu_mode=%d (0, 1 or 2)", relu_mode);
  DH_REQUIRE(!g_out_dev || (dy_dev && relu_mode == 1), "debug bn2 paths: g_out_dev goes with dy_dev and relu_mode 1");
  return dbg_bn2("debug bn2 paths", z_dev, res_dev, gamma_dev, beta_dev, relu, fold, y_dev, bits_dev, mean_dev, invstd_dev, z2_dev, gamma2_dev,
                 beta2_dev, mean2_dev, invstd2_dev, dy_dev, relu_mode, dz_dev, g_out_dev, dgamma_dev, dbeta_dev, rows, C, dh::as_stream(stream));
}

// through t2_bn_fwd with a pooled target and t2_bn_pool_bwd
extern "C" int dh_debug_bn2_pool_bf16(const uint16_t* z_dev, const float* gamma_dev, const float* beta_dev, uint16_t* pooled_dev, uint8_t* idx_dev,
                                      float* mean_dev, float* invstd_dev, const uint16_t* dpool_dev, uint16_t* dz_dev, float* dgamma_dev,
                                      float* dbeta_dev, int32_t B, int32_t Hi, int32_t Wi, int32_t C, void* stream) {
  DH_REQUIRE(z_dev && gamma_dev && beta_dev && pooled_dev && idx_dev && mean_dev && invstd_dev && B > 0 && Hi > 0 && Wi > 0 && C >= 64 &&
             C <= 2048 && C % 64 == 0 && 256 % (C / 8) == 0, "debug bn2 pool: bad arguments");
  DH_REQUIRE(!dpool_dev || (dz_dev && dgamma_dev && dbeta_dev), "debug bn2 pool: backward needs dz, dgamma, dbeta");
  hipStream_t st = dh::as_stream(stream);
  DbgScratch sc;
  DbgBn2 e;
  int rc;
  if ((rc = dbg_bn2_engine(e, sc, st, B, Hi, Wi, C, 7, gamma_dev, beta_dev, mean_dev, invstd_dev))) return rc;
  e.c.Z = const_cast<bf16_t*>(z_dev);
  rc = t2_bn_fwd(&e.t, e.c, nullptr, true, true, st, false, pooled_dev, idx_dev);
  if (!rc && dpool_dev) {
    rc = t2_bn_pool_bwd(&e.t, e.c, dpool_dev, idx_dev, dz_dev, st);
    if (!rc && (hipMemcpyAsync(dgamma_dev, e.t.G, C * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess ||
                hipMemcpyAsync(dbeta_dev, e.t.G + C, C * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)) rc = DH_EHIP;
  }
  if (rc) { (void)hipStreamSynchronize(st); return rc; }
  return dbg_finish(st, "debug bn2 pool");
}

// x is rounded to bf16 on its way into LDS, as the forward stem does
extern "C" int dh_debug_stem_wgrad_bf16(const uint16_t* dz_dev, const float* x_nchw_dev, float* dw_dev, int32_t B, int32_t P, void* stream) {
  DH_REQUIRE(dz_dev && x_nchw_dev && dw_dev && B > 0 && P >= 32 && P % 2 == 0, "debug stem wgrad: bad arguments");
  hipStream_t st = dh::as_stream(stream);
  DbgScratch sc;
  float* slabs;
  int rc = sc.get(&slabs, (int64_t)STEM_WGRAD_SLABS * 64 * 160);
  if (rc) return rc;
  if ((rc = t2_stem_wgrad(dz_dev, x_nchw_dev, slabs, dw_dev, B, P, P / 2, P / 2, st))) return rc;
  return dbg_finish(st, "debug stem wgrad bf16");
}

extern "C" int dh_debug_maxpool2_bf16(const uint16_t* x_dev, uint16_t* y_dev, const uint16_t* dy_dev, uint16_t* dx_dev, int32_t B, int32_t Hi,
                                      int32_t Wi, int32_t C, void* stream) {
  DH_REQUIRE(x_dev && y_dev && B > 0 && Hi > 0 && Wi > 0 && C % 8 == 0 && (!dy_dev || dx_dev), "debug maxpool2: bad arguments");
  DbgScratch sc;
  uint8_t* idx;
  int rc = sc.get(&idx, (int64_t)B * ((Hi + 2 - 3) / 2 + 1) * ((Wi + 2 - 3) / 2 + 1) * C);
  if (rc) return rc;
  return dbg_maxpool2("debug maxpool2", x_dev, y_dev, idx, dy_dev, dx_dev, B, Hi, Wi, C, dh::as_stream(stream));
}
extern "C" int dh_debug_maxpool2_idx_bf16(const uint16_t* x_dev, uint16_t* y_dev, uint8_t* idx_dev, const uint16_t* dy_dev, uint16_t* dx_dev,
                                          int32_t B, int32_t Hi, int32_t Wi, int32_t C, void* stream) {
  DH_REQUIRE(x_dev, "debug maxpool2 idx: null input (x_dev)");
  DH_REQUIRE(y_dev && idx_dev, "debug maxpool2 idx: null output (y_dev or idx_dev)");
  DH_REQUIRE(!dy_dev || dx_dev, "debug maxpool2 idx: backward (dy_dev given) needs dx_dev");
  DH_REQUIRE(B > 0 && Hi > 0 && Wi > 0, "debug maxpool2 idx: B=%d Hi=%d Wi=%d", B, Hi, Wi);
  DH_REQUIRE(C > 0 && C % 8 == 0, "debug maxpool2 idx: C=%d (a positive multiple of 8)", C);
  return dbg_maxpool2("debug maxpool2 idx", x_dev, y_dev, idx_dev, dy_dev, dx_dev, B, Hi, Wi, C, dh::as_stream(stream));
}
extern "C" int dh_debug_upsample2_add_bf16(const uint16_t* t_dev, uint16_t* dx_dev, int32_t B, int32_t Ho, int32_t Wo, int32_t Hi, int32_t Wi,
                                           int32_t C, void* stream) {
  DH_REQUIRE(t_dev && dx_dev && B > 0 && C % 8 == 0 && 2 * (Ho - 1) < Hi && 2 * (Wo - 1) < Wi, "debug upsample2: bad arguments");
  hipStream_t st = dh::as_stream(stream);
  hipLaunchKernelGGL(upsample2_add_bf16_kernel, dim3(grid_for((int64_t)B * Ho * Wo * C / 8)), dim3(256), 0, st, t_dev, dx_dev, B, Ho, Wo, Hi, Wi, C);
  DH_LAUNCH_CHECK();
  return dbg_finish(st, "debug upsample2");
}
extern "C" int dh_debug_avgpool_fc_dgrad2(const float* dlogits_dev, const float* w_dev, uint16_t* dx_dev, int32_t B, int32_t HW, int32_t C,
                                          int32_t n_cls, void* stream) {
  DH_REQUIRE(dlogits_dev && w_dev && dx_dev && B > 0 && HW > 0 && C % 8 == 0 && n_cls > 0, "debug avgpool fc: bad arguments");
  hipStream_t st = dh::as_stream(stream);
  hipLaunchKernelGGL(avgpool_fc_dgrad2_kernel, dim3(B), dim3(256), 0, st, dlogits_dev, w_dev, HW, C, n_cls, dx_dev);
  DH_LAUNCH_CHECK();
  return dbg_finish(st, "debug avgpool fc");
}

// through t2_conv_fwd (t2_conv3 / t2_gemm) or t2_conv_dgrad on a scratch engine object, which pick tile and variant as in a step
extern "C" int dh_debug_conv_bf16(const uint16_t* in_dev, const float* w_dev, const uint16_t* res_dev, uint16_t* out_dev, int32_t B,
                                  int32_t Hi, int32_t Wi, int32_t cin, int32_t cout, int32_t ks, int32_t stride, int32_t dgrad,
                                  void* stream) {
  DH_REQUIRE(in_dev && w_dev && out_dev, "debug conv bf16: in, w and out must be given");
  DH_REQUIRE(B > 0 && Hi > 0 && Wi > 0, "debug conv bf16: B=%d Hi=%d Wi=%d must be positive", B, Hi, Wi);
  DH_REQUIRE(ks == 1 || ks == 3, "debug conv bf16: ks=%d is not 1 or 3", ks);
  DH_REQUIRE(stride == 1 || stride == 2, "debug conv bf16: stride=%d is not 1 or 2", stride);
  DH_REQUIRE(cin > 0 && cin % 64 == 0, "debug conv bf16: cin=%d is not a multiple of 64", cin);
  DH_REQUIRE(cout > 0 && cout % 64 == 0, "debug conv bf16: cout=%d is not a multiple of 64", cout);
  DH_REQUIRE(stride == 1 || Hi % 2 == 0, "debug conv bf16: Hi=%d is odd at stride 2 (the engine's maps are even: P %% 32 == 0)", Hi);
  DH_REQUIRE(stride == 1 || Wi % 2 == 0, "debug conv bf16: Wi=%d is odd at stride 2 (the engine's maps are even: P %% 32 == 0)", Wi);
  DH_REQUIRE(dgrad == 0 || dgrad == 1, "debug conv bf16: dgrad=%d is not 0 or 1", dgrad);
  DH_REQUIRE(dgrad == 1 || !res_dev, "debug conv bf16: res belongs to the data gradient (dgrad = 1); the forward conv is raw Z");
  hipStream_t st = dh::as_stream(stream);
  DbgScratch sc;
  dh_train2 t;
  t.B = B;
  T2Conv c = dbg_conv_bf16(cin, cout, ks, stride, Hi, Wi);
  const int64_t nw = (int64_t)cout * cin * ks * ks, nx = (int64_t)B * Hi * Wi * cin, nz = (int64_t)B * c.Ho * c.Wo * cout;
  DH_REQUIRE(std::max(nx, nz) * 2 < ((int64_t)1 << 32), "debug conv bf16: B=%d makes a tensor of 4 GiB or more", B);
  bf16_t *wf, *wd, *scratch = nullptr;
  int rc;
  if ((rc = sc.get(&wf, nw)) || (rc = sc.get(&wd, nw)) || (rc = sc.get(&t.ones, 2048)) || (rc = sc.get(&t.zeros, 2048))) return rc;
  DH_HIP(hipMemsetAsync(t.zeros, 0, 2048 * sizeof(float), st));
  hipLaunchKernelGGL(fill_kernel, dim3(8), dim3(256), 0, st, t.ones, (int64_t)2048, 1.0f);
  if ((rc = dbg_pack_bf16(sc, st, w_dev, wf, wd, cout, cin, ks))) return rc;
  c.wp_f = wf; c.wp_d = wd;
  if (!dgrad) {
    c.Z = out_dev;
    rc = t2_conv_fwd(&t, c, in_dev, st);
  } else if (ks == 1 && stride == 2) {   // a downsample branch: the step has already written the other branch's gradient into dX
    if ((rc = sc.get(&scratch, nz / cout * cin))) return rc;
    if (res_dev) DH_HIP(hipMemcpyAsync(out_dev, res_dev, nx * sizeof(bf16_t), hipMemcpyDeviceToDevice, st));
    else DH_HIP(hipMemsetAsync(out_dev, 0, nx * sizeof(bf16_t), st));
    rc = t2_conv_dgrad(&t, c, in_dev, nullptr, out_dev, scratch, true, st);
  } else {
    rc = t2_conv_dgrad(&t, c, in_dev, res_dev, out_dev, nullptr, false, st);
  }
  if (rc) { (void)hipStreamSynchronize(st); return rc; }
  return dbg_finish(st, "debug conv bf16");
}

extern "C" int dh_debug_wgrad_bf16(const uint16_t* dz_dev, const uint16_t* x_dev, float* dw_dev, int32_t B, int32_t Hi, int32_t Wi,
                                   int32_t cin, int32_t cout, int32_t ks, int32_t stride, int32_t repeat, void* stream) {
  DH_REQUIRE(dz_dev && x_dev && dw_dev && (ks == 1 || ks == 3) && cin % 64 == 0 && cout % 64 == 0 && repeat >= 1, "debug wgrad bf16: bad arguments");
  hipStream_t st = dh::as_stream(stream);
  dh_train2 t;
  t.B = B;
  const T2Conv c = dbg_conv_bf16(cin, cout, ks, stride, Hi, Wi);
  Wg2Plan q;
  int rc = t2_wgrad_plan(c, B, &q);
  if (rc) return rc;
  DbgScratch sc;
  const int64_t nw = (int64_t)cout * cin * ks * ks;
  t.wgrad_slab_floats = (int64_t)q.n_slabs * nw;
  if ((rc = sc.get(&t.wgrad_slabs, t.wgrad_slab_floats))) return rc;
  t.G = dw_dev;
  t.slot["dbg.weight"] = {0, nw};
  for (int i = 0; i < repeat; ++i)
    if ((rc = t2_wgrad(&t, c, x_dev, dz_dev, st))) return rc;
  return dbg_finish(st, "debug wgrad bf16");
}

// =====================================================================================
// The classifier head of both engines, in the order a step launches it: global average pool (avgpool_kernel on float32 x /
// avgpool2_kernel on bf16 x), fc_fwd_kernel, fc_wgrad_kernel on the caller's dlogits and the pooled features just made, and the
// matching avgpool_fc_dgrad kernel
// =====================================================================================
extern "C" int dh_debug_head(const void* x_dev, int32_t x_bf16, const float* w_dev, const float* bias_dev, const float* dlogits_dev,
                             float* pooled_dev, float* logits_dev, float* dw_dev, float* db_dev, void* dx_dev, int32_t B, int32_t HW,
                             int32_t C, int32_t n_cls, void* stream) {
  DH_REQUIRE(x_dev && w_dev && bias_dev && dlogits_dev, "debug head: null input (x_dev, w_dev, bias_dev or dlogits_dev)");
  DH_REQUIRE(pooled_dev && logits_dev && dw_dev && db_dev && dx_dev, "debug head: null output (pooled_dev, logits_dev, dw_dev, db_dev or dx_dev)");
  DH_REQUIRE(x_bf16 == 0 || x_bf16 == 1, "debug head: x_bf16=%d (0 float32, 1 bf16)", x_bf16);
  DH_REQUIRE(B > 0 && B <= 65535, "debug head: B=%d", B);
  DH_REQUIRE(HW > 0, "debug head: HW=%d", HW);
  DH_REQUIRE(C > 0 && C % 8 == 0, "debug head: C=%d (a positive multiple of 8)", C);
  DH_REQUIRE(n_cls > 0 && n_cls <= 1024, "debug head: n_cls=%d", n_cls);
  hipStream_t st = dh::as_stream(stream);
  if (x_bf16) hipLaunchKernelGGL(avgpool2_kernel, dim3(B), dim3(256), 0, st, static_cast<const bf16_t*>(x_dev), HW, C, pooled_dev);
  else hipLaunchKernelGGL(avgpool_kernel, dim3(B), dim3(256), 0, st, static_cast<const float*>(x_dev), HW, C, pooled_dev);
  hipLaunchKernelGGL(fc_fwd_kernel, dim3((B * n_cls + 3) / 4), dim3(256), 0, st, pooled_dev, w_dev, bias_dev, B, C, n_cls, logits_dev);
  hipLaunchKernelGGL(fc_wgrad_kernel, dim3((n_cls * C + 255) / 256), dim3(256), 0, st, dlogits_dev, pooled_dev, B, C, n_cls, dw_dev, db_dev);
  if (x_bf16) hipLaunchKernelGGL(avgpool_fc_dgrad2_kernel, dim3(B), dim3(256), 0, st, dlogits_dev, w_dev, HW, C, n_cls, static_cast<bf16_t*>(dx_dev));
  else hipLaunchKernelGGL(avgpool_fc_dgrad_kernel, dim3(B), dim3(256), 0, st, dlogits_dev, w_dev, HW, C, n_cls, static_cast<float*>(dx_dev));
  DH_LAUNCH_CHECK();
  return dbg_finish(st, "debug head");
}
