// resnet50_infer.inc -- bf16 INFERENCE engine of the ResNet-50 patch classifier (dh_resnet50_*), the counterpart of dh_resnet18's
// bf16 path for the network get_model(..., arch="resnet50") trains (torchvision resnet50 v1.5 + fc[n_cls, 2048]).
// Included at the end of resnet_kernels.hip, after gemm1x1_infer.inc.  The handle's common state, the parameter entry, finalize's checks
// and the tiles / tap / operands entries are infer_core.inc's, shared with dh_resnet18; the network itself is net_desc.inc's.
//
// Eval-mode BN is folded at finalize (host, double): W' = W * s, b' = beta - mean * s with s = gamma / sqrt(var + 1e-5).  Every
// convolution is then ONE kernel pass that writes its final bf16 activation:
//   stem      stem_pool_kernel (stem_pool.inc): conv 7x7/2 + bias + ReLU + maxpool 3x3/2 straight from the uint8 slide (or the float
//             NCHW input of dh_resnet50_forward), scale = 1, shift = b'
//   3x3       conv3x3.inc on the channel-blocked layout, scale = 1, shift = b', ReLU (stride 1 and 2)
//   1x1       gemm1x1_infer.inc: bias, ReLU; the block's conv3 also adds the identity (or the downsample's output) before its ReLU;
//             the downsample (stride 2 reads every second pixel of every second row) runs with bias only
//   head      r50_head_kernel: average pool over 2048 channels + fc in a fixed order
// Activations are bf16 in the channel-blocked layout [image][C/32][H][W][32] throughout (the stem writes it, both conv kernels read and
// write it): no layout conversion pass anywhere.  Four buffers per launch shape, reused by every block: X (block input, overwritten by
// the block output), T1 (conv1 out), T2 (conv2 out), D (downsample out).  The training workspace (dh_train2) is never allocated.
// Launch limit: R50_MAX_TILES tiles (see below); per-tile results do not depend on the launch: every kernel computes a tile's outputs
// from that tile's inputs in a fixed order (no float atomics).

// Largest map of a launch: the 256-channel maps of stage 1, 256 x (P/4)^2 bf16 = 2 MiB per 256^2 tile.  The engine keeps every
// activation tensor within 2^31 bytes (the signed 32-bit range of the conv3x3 schedule tables' and the 1x1 kernel's per-image offsets,
// with headroom for the 4 GiB bound of conv3x3 inputs), which caps a launch at 1 024 tiles of 256^2.
constexpr int R50_MAX_P = 256;
constexpr int64_t R50_MAX_TILES = ((int64_t)1 << 31) / ((int64_t)256 * (R50_MAX_P / 4) * (R50_MAX_P / 4) * 2);
static_assert(R50_MAX_TILES == DH_RESNET50_MAX_TILES, "include/deephisto_hip.h states the launch limit");

struct dh_resnet50 : InferNet {   // convs: w_dev = folded bf16 operand, shift_dev = folded bias, scale_dev = ones
  float* ones = nullptr;          // scale = 1 for the stem / 3x3 epilogues (shared by every layer)
  std::vector<int32_t> yx_host;   // origin check of forward_tiles
};

namespace {

// Tile shape per GEMM shape.  128 x 128 (NMT = 4: a third less operand ingest through L2) where the channel count allows it and K <= 1024;
// 128 x 64 at K = 2048 (measured on the training engine, profiles/r04_exp_gemm_wide.txt: the wide tile is 14-22 % faster at K <= 1024,
// 12-32 % slower at K = 2048, where four workgroups per CU hide more of the K loop).  Ring depth 2 (gemm1x1.inc: never slower than depth 3
// below K = 1024).
struct R50GemmCfg { int nmt, nstage; };
R50GemmCfg r50_gemm_cfg(int N, int K) {
  R50GemmCfg c;
  c.nmt = (N % 128 == 0 && K <= 1024) ? 4 : 2;
  c.nstage = std::min(K / G2_BK, 2);
  return c;
}

int r50_gemm(const ConvLayer& L, const bf16_t* in, const bf16_t* res, bf16_t* out, int B, int Hi, int Wi, bool relu, hipStream_t st) {
  const int Ho = (Hi - 1) / L.stride + 1, Wo = (Wi - 1) / L.stride + 1;
  const int64_t M = (int64_t)B * Ho * Wo;
  DH_REQUIRE(L.ks == 1 && L.cout % 64 == 0 && L.cin % 64 == 0 && M > 0 && M < ((int64_t)1 << 31),
             "resnet50 1x1 %s: M=%lld N=%d K=%d unsupported", L.name.c_str(), (long long)M, L.cout, L.cin);
  const R50GemmCfg cfg = r50_gemm_cfg(L.cout, L.cin);
  GemmInferParams p{};
  p.a = in; p.w = static_cast<const bf16_t*>(L.w_dev); p.bias = L.shift_dev; p.res = res; p.out = out;
  p.M = (int)M; p.N = L.cout; p.K = L.cin; p.HWo = Ho * Wo;
  p.stride = L.stride; p.Ho = Ho; p.Wo = Wo; p.Hi = Hi; p.Wi = Wi;
  p.MB = (int)((M + G2_BM - 1) / G2_BM); p.NB = L.cout / (32 * cfg.nmt);
  p.nstage = cfg.nstage; p.relu = relu ? 1 : 0;
  const int grid = ((p.MB + 7) / 8) * 8 * p.NB;
  if (cfg.nmt == 4) {
    if (int rc = ensure_dyn_lds(reinterpret_cast<const void*>(&gemm1x1_infer_kernel<4>), G2_LDS)) return rc;
    hipLaunchKernelGGL(gemm1x1_infer_kernel<4>, dim3(grid), dim3(256), (size_t)p.nstage * G2Cfg<4>::STAGE, st, p);
  } else {
    if (int rc = ensure_dyn_lds(reinterpret_cast<const void*>(&gemm1x1_infer_kernel<2>), G2_LDS)) return rc;
    hipLaunchKernelGGL(gemm1x1_infer_kernel<2>, dim3(grid), dim3(256), (size_t)p.nstage * G2Cfg<2>::STAGE, st, p);
  }
  DH_LAUNCH_CHECK();
  return DH_OK;
}

int r50_forward_impl(dh_resnet50* net, const float* x, const uint8_t* slide, int64_t slide_h, int64_t slide_w, const int32_t* yx,
                     int B, int P, float* logits, hipStream_t st, Tap* tap = nullptr, float* feat = nullptr, float* cam = nullptr) {
  const int H2 = P / 4;   // stem 7x7/2 -> P/2, maxpool 3x3/2 -> P/4 (P % 32 == 0)
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t px = (size_t)B * H2 * H2 * 2;   // bytes per channel of a stage-1 map
  const size_t big = al(256 * px), t1 = al(128 * px), t2 = al(64 * px);
  const size_t need = 2 * big + t1 + t2;
  int rc;
  if ((rc = infer_workspace(net, need))) return rc;
  char* base = static_cast<char*>(net->ws);
  bf16_t* X = reinterpret_cast<bf16_t*>(base);
  bf16_t* D = reinterpret_cast<bf16_t*>(base + big);
  bf16_t* T1 = reinterpret_cast<bf16_t*>(base + 2 * big);
  bf16_t* T2 = reinterpret_cast<bf16_t*>(base + 2 * big + t1);
  DH_REQUIRE(stem_seam_bytes(B, P) <= t1, "resnet50 forward: seam scratch larger than the bottleneck buffer");
  if ((rc = launch_stem_pool(net->convs[0], x, slide, slide_h, slide_w, yx, B, P, X, T1, st))) return rc;   // T1: free until conv1
  for (const char* nm : {"conv1", "maxpool"})   // the fused stem stores only the pooled map
    if ((rc = tap_after<__bf16>(tap, nm, X, 64, H2, H2, 32, st))) return rc;
  int H = H2;
  for (const BlockDesc& b : net->desc->blocks) {
    const ConvLayer &c1 = net->convs[b.conv[0]], &c2 = net->convs[b.conv[1]], &c3 = net->convs[b.conv[2]];
    const int Ho = (H - 1) / b.stride + 1;
    if ((rc = r50_gemm(c1, X, nullptr, T1, B, H, H, true, st))) return rc;
    if ((rc = tap_after<__bf16>(tap, c1.name, T1, c1.cout, H, H, 32, st))) return rc;
    rc = launch_conv3x3<__bf16>(b.stride, c2, T1, nullptr, T2, B, H, H, true, st, Ho, Ho, nullptr, nullptr, true);
    if (rc) return rc;
    if ((rc = tap_after<__bf16>(tap, c2.name, T2, c2.cout, Ho, Ho, 32, st))) return rc;
    const bf16_t* idt = X;
    if (b.ds >= 0) {
      if ((rc = r50_gemm(net->convs[b.ds], X, nullptr, D, B, H, H, false, st))) return rc;
      if ((rc = tap_after<__bf16>(tap, net->convs[b.ds].name, D, c3.cout, Ho, Ho, 32, st))) return rc;
      idt = D;
    }
    // the join: conv3 + identity, ReLU.  Without a downsample the output overwrites the identity in place (every lane reads its residual
    // pieces before it stores them); with one, X is dead once conv1 and the downsample have run (stream order)
    if ((rc = r50_gemm(c3, T2, idt, X, B, Ho, Ho, true, st))) return rc;
    if ((rc = tap_after<__bf16>(tap, c3.name, X, c3.cout, Ho, Ho, 32, st))) return rc;
    H = Ho;
  }
  if (feat)   // dh_resnet50_features_tiles: the same head, the pooled vector stored as well
    hipLaunchKernelGGL(r50_head_kernel<true>, dim3(B), dim3(256), 0, st, X, H * H, net->fc_w_dev, net->fc_b_dev, net->n_classes, logits, feat);
  else if (logits)   // null only in dh_resnet50_cam_tiles without logits
    hipLaunchKernelGGL(r50_head_kernel<false>, dim3(B), dim3(256), 0, st, X, H * H, net->fc_w_dev, net->fc_b_dev, net->n_classes, logits, nullptr);
  DH_LAUNCH_CHECK();
  if (cam) return launch_cam_head<__bf16>(net, X, B, H * H, cam, st);   // dh_resnet50_cam_tiles: fc per position of the same activation
  return DH_OK;
}

int r50_check_forward(const InferNet* net, int64_t n, int32_t P, const void* logits, const char* what) {
  DH_REQUIRE(net != nullptr, "%s: null handle", what);
  DH_REQUIRE(net->finalized, "%s: call dh_resnet50_finalize after setting parameters", what);
  DH_REQUIRE(P >= 64 && P <= R50_MAX_P && P % 32 == 0, "%s: patch %d unsupported (64 <= P <= %d, P %% 32 == 0)", what, P, R50_MAX_P);
  DH_REQUIRE(n >= 0 && n <= R50_MAX_TILES, "%s: %lld tiles exceed the launch limit of %lld tiles (DH_RESNET50_MAX_TILES)", what,
             (long long)n, (long long)R50_MAX_TILES);
  DH_REQUIRE(logits || n == 0, "%s: null logits", what);
  return DH_OK;
}

// feat rows are written as float4: 16-byte aligned; 1x1 operands are gemm1x1_infer.inc's plain bf16 [cout][cin]
const InferEngine R50_ENGINE = {"resnet50", r50_check_forward, 16, true};

// The origins are device memory: they are read back (n pairs, one synchronisation of `st`) and checked before any launch, so that an
// origin outside the slide is an error, not a read past the tile (the stem itself never reads outside the slide allocation either).
int r50_check_origins(dh_resnet50* net, int64_t h, int64_t w, const int32_t* yx, int64_t n, int32_t P, hipStream_t st, const char* what) {
  net->yx_host.resize((size_t)n * 2);
  DH_HIP(hipMemcpyAsync(net->yx_host.data(), yx, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  DH_HIP(hipStreamSynchronize(st));
  for (int64_t i = 0; i < n; ++i) {
    const int32_t y = net->yx_host[2 * i], x = net->yx_host[2 * i + 1];
    DH_REQUIRE(y >= 0 && x >= 0 && y <= h - P && x <= w - P, "%s: origin %lld (y=%d, x=%d) puts a %d-pixel tile outside the %lldx%lld slide",
               what, (long long)i, y, x, P, (long long)h, (long long)w);
  }
  return DH_OK;
}

// the tiles entries: the origin check, then the forward
int r50_tiles(dh_resnet50* net, const uint8_t* slide, int64_t h, int64_t w, const int32_t* yx, int64_t n, int32_t P, float* feat,
              float* logits, const float* out, void* stream, const char* what, float* cam = nullptr) {
  hipStream_t st = dh::as_stream(stream);
  return infer_tiles(R50_ENGINE, net, slide, h, w, yx, n, P, feat, out, what, [&](Tap* tap) {
    if (int rc = r50_check_origins(net, h, w, yx, n, P, st, what)) return rc;
    return r50_forward_impl(net, nullptr, slide, h, w, yx, (int)n, P, logits, st, tap, feat, cam);
  });
}

}  // namespace

extern "C" int dh_resnet50_create(dh_resnet50** out, int32_t n_classes) {
  DH_REQUIRE(out != nullptr, "resnet50 create: null output");
  DH_REQUIRE(n_classes > 0 && n_classes <= 1024, "resnet50 create: n_classes=%d", n_classes);
  if (int erc = dh::env_check()) return erc;
  auto* net = new dh_resnet50();
  infer_init(net, "resnet50", n_classes);
  *out = net;
  return DH_OK;
}

extern "C" void dh_resnet50_destroy(dh_resnet50* net) {
  if (!net) return;
  for (auto& c : net->convs) c.scale_dev = nullptr;   // every conv's scale is net->ones
  if (net->ones) (void)hipFree(net->ones);
  infer_free(net);
  delete net;
}

extern "C" int dh_resnet50_set_param(dh_resnet50* net, const char* name, const float* data, int64_t n_elem) {
  return infer_set_param(R50_ENGINE, net, name, data, n_elem);
}

extern "C" int dh_resnet50_finalize(dh_resnet50* net, void* stream) {
  (void)stream;   // uploads are synchronous (hipMemcpy), like dh_resnet18_finalize
  int rc = infer_finalize_begin(R50_ENGINE, net);
  if (rc) return rc;
  if (!net->ones) {
    const std::vector<float> one(net->desc->feat, 1.0f);
    if ((rc = upload(one, reinterpret_cast<void**>(&net->ones)))) return rc;
  }
  std::vector<double> scale, shift;
  for (auto& c : net->convs) {
    const std::vector<float>& w = *infer_param(net, c.name + ".weight");
    // eval-mode BN folded into the weights and a bias
    infer_bn_affine(net, c, scale, shift);
    const int64_t per = (int64_t)c.cin * c.ks * c.ks;
    std::vector<float> wf(w.size());
    const std::vector<float> bias(shift.begin(), shift.end());
    for (int k = 0; k < c.cout; ++k)
      for (int64_t i = 0; i < per; ++i) wf[k * per + i] = (float)((double)w[k * per + i] * scale[k]);
    if (c.ks == 1) {   // W'[cout][cin], bf16 (gemm1x1_infer.inc's W operand)
      std::vector<uint16_t> wb(wf.size());
      for (size_t i = 0; i < wf.size(); ++i) wb[i] = host_bf16(wf[i]);
      rc = upload(wb, &c.w_dev);
    } else {
      std::vector<uint8_t> packed;
      if (c.ks == 7) pack_stem_pool_weights(wf.data(), packed);
      else pack_conv_weights(wf.data(), c.cout, c.cin, c.ks, 2, packed);
      rc = upload(packed, &c.w_dev);
    }
    if (rc || (rc = upload(bias, reinterpret_cast<void**>(&c.shift_dev)))) return rc;
    c.scale_dev = net->ones;
  }
  return infer_finalize_end(net);
}

extern "C" int dh_resnet50_forward(dh_resnet50* net, const float* x, int64_t n, int32_t P, float* logits, void* stream) {
  if (int rc = r50_check_forward(net, n, P, logits, "resnet50 forward")) return rc;
  if (n == 0) return DH_OK;
  DH_REQUIRE(x != nullptr, "resnet50 forward: null input");
  return r50_forward_impl(net, x, nullptr, 0, 0, nullptr, (int)n, P, logits, dh::as_stream(stream));
}

extern "C" int dh_resnet50_forward_tiles(dh_resnet50* net, const uint8_t* slide, int64_t h, int64_t w, const int32_t* yx, int64_t n,
                                         int32_t P, float* logits, void* stream) {
  return r50_tiles(net, slide, h, w, yx, n, P, nullptr, logits, logits, stream, "resnet50 forward_tiles");
}

extern "C" int dh_resnet50_features_tiles(dh_resnet50* net, const uint8_t* slide, int64_t h, int64_t w, const int32_t* yx, int64_t n,
                                          int32_t P, float* feat, float* logits, void* stream) {
  return r50_tiles(net, slide, h, w, yx, n, P, feat, logits, feat, stream, "resnet50 features_tiles");
}

extern "C" int dh_resnet50_cam_tiles(dh_resnet50* net, const uint8_t* slide, int64_t h, int64_t w, const int32_t* yx, int64_t n,
                                     int32_t P, float* cam, float* logits, void* stream) {
  if (int rc = cam_check(R50_ENGINE, net, P, "resnet50 cam_tiles")) return rc;
  return r50_tiles(net, slide, h, w, yx, n, P, nullptr, logits, cam, stream, "resnet50 cam_tiles", cam);
}

// Test hooks (include/deephisto_hip_debug.h): the forward of forward_tiles with one stored activation tapped (no origin check), and a
// conv's operands as the engine holds them after finalize: the folded, bf16-rounded weight, scale (1) and the folded bias.
extern "C" int dh_debug_resnet50_forward_tap(dh_resnet50* net, const uint8_t* slide, int64_t h, int64_t w, const int32_t* yx_dev, int64_t n,
                                             int32_t P, const char* conv_name, const int32_t* sel_dev, int32_t k, float* out_dev,
                                             int64_t out_elems, float* logits_dev, void* stream) {
  hipStream_t st = dh::as_stream(stream);
  return infer_tap(R50_ENGINE, net, slide, h, w, yx_dev, n, P, conv_name, sel_dev, k, out_dev, out_elems, logits_dev, st, [&](Tap* tap) {
    return r50_forward_impl(net, nullptr, slide, h, w, yx_dev, (int)n, P, logits_dev, st, tap);
  });
}

extern "C" int dh_debug_resnet50_operands(dh_resnet50* net, const char* conv_name, float* w_host, int64_t w_elems, float* scale_host,
                                          float* shift_host, int64_t c_elems) {
  return infer_operands(R50_ENGINE, net, 2, conv_name, w_host, w_elems, scale_host, shift_host, c_elems);
}
