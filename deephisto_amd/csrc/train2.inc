// train2.inc -- bf16 training / evaluation engine for the patch classifiers of BASELINE configs[4]:
// ResNet-18 (BasicBlock) and ResNet-50 (Bottleneck, torchvision v1.5) with bf16 activations and bf16 MFMA
// (f32 accumulation), f32 master weights, f32 gradients, Adam in f32.  Host side; kernels in train2_kernels.inc and
// conv3x3.inc.  Included at the end of resnet_kernels.hip.  The file ends with its last product entry point: the test hooks over
// this code are train_hooks.inc's, declared in include/deephisto_hip_debug.h.
//
// Replaces, for `get_model` with a ResNet-50 backbone (models/patch_cls_simple/model.py:5-11 builds the torchvision
// network; BASELINE.json configs[4] names the ResNet-50 variant), the step of models/patch_cls_simple/train.py:166-172:
//   outputs = model(inputs); loss = criterion(outputs, labels); loss.backward(); optimizer.step()
// with CrossEntropyLoss(mean) (:117), Adam(lr) (:118), BatchNorm in training mode (batch statistics, momentum 0.1,
// eps 1e-5, unbiased running variance).
//
// Data flow per conv: Z = conv(X) (bf16, raw) -> per-channel batch statistics of Z (sum, sum of squares: from the GEMM's own
// epilogue for 1x1 convolutions, one pass over Z otherwise; fixed-point integer accumulators, see train2_kernels.inc) ->
// Y = [relu](Z*scale + shift [+ identity]) (bf16; the coefficients are made in the apply kernel's prologue).  Backward:
// g = dY * (Y > 0) (the mask of a block's join is applied by the dgrad GEMM that produces dY where one exists),
// BN backward as two per-channel sums + one elementwise pass (dz = k0 g + k1 z + k2), dgrad = the forward kernels on
// transposed (1x1) / flipped-transposed (3x3) weights, wgrad = pixel-reduction GEMM through transposed LDS reads.
// The parameter arenas (masters Pm, gradients G, Adam moments M / V) are laid out in BACKWARD order (fc first, stem
// last): gradient buckets complete front to back while the backward pass runs, which is what the bucketed, overlapped
// data-parallel all-reduce needs (dh_train2_set_buckets).  The parameter store, the buckets, the Adam launch and the side
// stream's hand-off are train_core.inc's, shared with the float32 engine.
#include <type_traits>

struct T2Conv : TrainConvT<bf16_t> {   // the shared record (train_core.inc); operands: 3x3 fragment order | 1x1 W[cout][cin] / Wt[cin][cout] | 7x7 stem layout
  uint8_t* Ybits = nullptr;   // top conv of a block: ReLU pattern of Y, one byte per 8 channels (st8_bits; read by the successor's dgrad GEMM)
};

struct dh_train2 : TrainStore {   // the arenas are in BACKWARD-completion order: every completion item is one convolution (or fc)
  int n_classes = 0, feat = 0;   // feat, blocks and the describing part of convs: copies of the architecture's NetDesc (net_desc.inc)
  std::vector<T2Conv> convs;     // index 0 = stem
  std::vector<BlockDesc> blocks;
  float *ones = nullptr, *zeros = nullptr, *partial = nullptr;
  int B = 0, P = 0;
  bf16_t* X1 = nullptr;          // pooled stem output = input of the first block
  uint8_t* pool_idx = nullptr;
  float *pooled = nullptr;
  bf16_t* GB[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // gradient ping-pong buffers (largest activation each)
  bool side_wgrad = false;  // weight gradients beside the dgrad / BN-backward chain, on TrainStore::side; every convolution owns its dZ buffer
  bool fold = true;         // small maps: the BN apply passes add the partial rows themselves, no finalize launch (bn_fold.inc; DH_T2_FOLD=0 at create: A/B, tests)
  bool join_fused = true;   // the downsample branch's BN is applied inside the join BN's pass (DH_T2_JOIN=0 at create: it writes its own Y; A/B, tests)
  float* stem_slabs = nullptr;
  float* wgrad_slabs = nullptr;
  int64_t wgrad_slab_floats = 0;
  const float* x_in = nullptr;
  bool last_training = false;
  bool bwd_done = false;    // a backward pass has run since the last forward: every dZ buffer holds THIS step's gradient (the dZ tap, train_hooks.inc)
  bool packed = false;
  PackTable<PackDesc> pack;        // table of pack_all_kernel (one launch packs every conv); descriptor j = conv j
};

namespace {

// Timing-only ablations of a training step: a COMPILE-TIME macro of diagnostic builds (tools/abl_train.sh builds one library per value with
// tools/build_variant.sh -DDH_T2_ABL=<bits>; results are garbage).  The shipped library is built without it: g_t2_abl is the constant 0, every
// test below folds away and no such switch exists at run time (tests/test_abi.py::test_no_ablation_switch_in_shipped_library).
// 1 no weight-gradient launches, 2 no BN finalize launches, 4 no forward BN apply passes, 8 no Adam / repack, 16 no slab reduce launches,
// 32 no BN-backward apply passes, 64 no BN-backward reduce passes, 128 no 1x1 GEMMs, 256 no 3x3 convolutions,
// 512 no forward apply pass in front of a 1x1 consumer (the bound of "apply on the operand path" for the bottleneck's conv3), 1024 the same in
// front of a 3x3 consumer, 2048 no forward statistics pass over a 3x3 convolution's output (NOT a bound: stale statistics zero the activations)
#ifndef DH_T2_ABL
#define DH_T2_ABL 0
#endif
constexpr int g_t2_abl = DH_T2_ABL;
#if DH_T2_ABL
int g_abl_consumer_ks = 0;   // kernel size of the convolution that consumes the BN output being produced (0: a block output)
#define DH_ABL_SKIP_APPLY() ((g_abl_consumer_ks == 1 && (g_t2_abl & 512)) || (g_abl_consumer_ks == 3 && (g_t2_abl & 1024)))
#define DH_ABL_SKIP_STATS(c) ((c).ks == 3 && (g_t2_abl & 2048))
#else
#define DH_ABL_SKIP_APPLY() false
#define DH_ABL_SKIP_STATS(c) false
#endif

// arenas in backward-completion order: fc, then blocks last to first (inside a block: last conv ... first conv, downsample), stem;
// each of them is one completion item
void t2_layout(dh_train2* t) {
  int64_t done = 0;   // the arena up to here is covered by items
  auto item_done = [&]() { t->items.push_back({done, t->n_params - done}); done = t->n_params; };
  auto add_conv = [&](int i) {
    store_add_conv(*t, t->convs[i], false);
    item_done();
  };
  store_add(*t, "fc.weight", (int64_t)t->n_classes * t->feat); store_add(*t, "fc.bias", t->n_classes);
  item_done();
  for (int b = (int)t->blocks.size() - 1; b >= 0; --b) {
    const BlockDesc& blk = t->blocks[b];
    for (int i = blk.nconv - 1; i >= 0; --i) add_conv(blk.conv[i]);
    if (blk.ds >= 0) add_conv(blk.ds);
  }
  add_conv(0);
}

// packs the weights of convs [i0, i1) (all of them by default)
int t2_pack(dh_train2* t, hipStream_t st, int i0 = 0, int i1 = -1) {
  if (!t->pack.dev) {
    for (const T2Conv& c : t->convs) {
      const int64_t n = c.ks == 7 ? 7 * 2 * 2 * 64 * 8 : (int64_t)c.cout * c.cin * c.ks * c.ks;
      t->pack.add({t->Pm + t->slot[c.name + ".weight"].first, static_cast<bf16_t*>(c.wp_f), static_cast<bf16_t*>(c.wp_d), c.cout, c.cin, c.ks, 0},
                  c.ks == 3 ? (c.cout / 64) * (c.cin / 64)                                   // one workgroup per 64 x 64 tile (pack3_tile)
                  : c.ks == 1 ? std::min(64, (c.cout / 64) * (c.cin / 64))                   // 64 x 64 tiles, a few per workgroup
                              : (int)std::max<int64_t>(1, std::min<int64_t>(64, (n + 8191) / 8192)));   // stem: 32 elements per thread
    }
    if (int rc = t->pack.upload(*t)) return rc;
  }
  if (i1 < 0) i1 = (int)t->convs.size();
  if (int arc = ensure_dyn_lds(reinterpret_cast<const void*>(&pack_all_kernel), PACK3_LDS)) return arc;
  const auto l = t->pack.range(i0, i1);
  hipLaunchKernelGGL(pack_all_kernel, dim3(l.grid), dim3(256), PACK3_LDS, st, l.first, l.count, l.blk_base);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
int t2_pack_all(dh_train2* t, hipStream_t st) {
  int rc = t2_pack(t, st);
  if (rc == DH_OK) t->packed = true;
  return rc;
}

// ---- convolution launches ------------------------------------------------------------------------------------
// Optional fused work of a 1x1 GEMM launch (gemm1x1.inc): + res, ReLU mask of another tensor, batch statistics of the output.
struct GemmFuse {
  const bf16_t* res = nullptr;
  const uint8_t* mask_bits = nullptr;   // ReLU pattern bytes of the tensor the output is masked by ([M][N / 8], st8_bits)
  float* partial = nullptr;       // statistics: [pixel tiles][2][N] partial sums of the output (capacity T2_PARTIAL_FLOATS)
  // backward mode: the output is the dY of the BN `bwd_of` (its Z and saved statistics): partial rows = {sum g, sum g xhat}
  const T2Conv* bwd_of = nullptr;
  int bwd_relu = 0;               // 0: g = the stored output (no ReLU, or masked by `mask`); 2: the BN's own ReLU, recomputed from Z
};
constexpr int64_t T2_PARTIAL_FLOATS = (int64_t)RED_NB * 2 * 2048;

int t2_gemm(const bf16_t* a, const void* w, bf16_t* out, int64_t M, int N, int K, int stride, int Ho, int Wo, int Hi, int Wi,
            const GemmFuse& fu, hipStream_t st) {
  DH_REQUIRE(N % G2_BN == 0 && K % G2_BK == 0 && M > 0 && M < ((int64_t)1 << 31), "gemm1x1: M=%lld N=%d K=%d unsupported", (long long)M, N, K);
  Gemm2Params p{};
  p.a = a; p.w = static_cast<const bf16_t*>(w); p.res = fu.res; p.mbits = fu.mask_bits; p.out = out;
  p.M = (int)M; p.N = N; p.K = K; p.stride = stride; p.Ho = Ho; p.Wo = Wo; p.Hi = Hi; p.Wi = Wi;
  p.MB = (int)((M + G2_BM - 1) / G2_BM); p.NB = N / G2_BN;
  p.partial = fu.partial;
  if (fu.bwd_of) {
    DH_REQUIRE(fu.partial && fu.bwd_of->cout == N, "gemm1x1: the fused BN-backward sums need the rows buffer and a BN of %d channels", N);
    p.bz = fu.bwd_of->Z; p.bmean = fu.bwd_of->bnb.mean; p.binvstd = fu.bwd_of->bnb.invstd; p.bscale = fu.bwd_of->bnb.scale;
    p.bshift = fu.bwd_of->bnb.shift; p.brelu = fu.bwd_relu;
  }
  if (g_t2_abl & 128) return DH_OK;
  static const int force_ns = dh::env_int("DH_G2_NSTAGE");
  // 128 x 128 tiles (gemm1x1.inc, NMT = 4; a third less operand ingest) for GEMMs of up to DH_G2_WIDE_M pixels: OFF by default --
  // measured in round 4 (profiles/r04_exp_gemm_wide.txt): 14-22 % faster where K <= 1024 and N >= 512, 12-32 % slower at K = 2048 (two
  // workgroups per CU instead of four hide less of the K loop's latency), ResNet-50 step 6.97 -> 7.02 ms.  Kept as an A/B switch.
  static const int64_t wide_m = dh::env_int("DH_G2_WIDE_M");
  const bool wide = N % 128 == 0 && M <= wide_m;
  if (wide) p.NB = N / 128;
  const int grid = ((p.MB + 7) / 8) * 8 * p.NB;
  // K from which the ring runs three stages deep (72 KB: two workgroups per CU).  Stand-alone depth 3 loses at K <= 512 (r03_exp_gemm_sweep.txt);
  // inside the step, next to the side stream, K >= 512 gains 0.7 % twice on one box (round 4: 7.00 / 6.99 -> 6.95 / 6.95 ms), 192 / 256 / 1024 are noise
  static const int ns3_k = dh::env_int("DH_G2_NS3_K");
  p.nstage = std::min(K / G2_BK, force_ns ? force_ns : (K >= ns3_k ? 3 : G2_NSTAGE));
  if (wide) {
    if (int rc = ensure_dyn_lds(reinterpret_cast<const void*>(&gemm1x1_ring_kernel<4>), G2_LDS)) return rc;
    const size_t lds = std::max<size_t>((size_t)p.nstage * G2Cfg<4>::STAGE, fu.bwd_of ? (size_t)G2Cfg<4>::BWD_LDS : fu.partial ? (size_t)G2Cfg<4>::STATS_LDS : 0);
    hipLaunchKernelGGL(gemm1x1_ring_kernel<4>, dim3(grid), dim3(256), lds, st, p);
  } else {
    if (int rc = ensure_dyn_lds(reinterpret_cast<const void*>(&gemm1x1_ring_kernel<2>), G2_LDS)) return rc;
    const size_t lds = std::max<size_t>((size_t)p.nstage * G2Cfg<2>::STAGE, fu.bwd_of ? (size_t)G2Cfg<2>::BWD_LDS : fu.partial ? (size_t)G2Cfg<2>::STATS_LDS : 0);
    hipLaunchKernelGGL(gemm1x1_ring_kernel<2>, dim3(grid), dim3(256), lds, st, p);
  }
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// workgroups of a per-channel reduction over `rows` rows of C bf16 channels: every CU gets one (256) before the count grows with
// the bytes (one per ~48 KiB, at most RED_NB).  Measured: one per 96 KiB from 16 up made the finalize kernels 30 % shorter and the
// reductions themselves 30-50 % longer (half the chip idle on the 12 MB maps): a net loss.
int t2_red_blocks(int64_t rows, int C) {
  const int tpr = std::min(C / 8, 256), rpi = 256 / tpr;
  const int64_t by_rows = (rows + rpi - 1) / rpi, by_bytes = std::max<int64_t>(256, rows * C * 2 / (48 * 1024));
  return (int)std::max<int64_t>(1, std::min<int64_t>(RED_NB, std::min(by_rows, by_bytes)));
}

int t2_conv3(dh_train2* t, int cin, int cout, int stride, const void* wp, const bf16_t* in, const bf16_t* res, bf16_t* out, int B, int Hi,
             int Wi, hipStream_t st) {
  if (g_t2_abl & 256) return DH_OK;
  ConvLayer L{{"t2", "t2", cin, cout, 3, stride}};
  L.w_dev = const_cast<void*>(wp); L.scale_dev = t->ones; L.shift_dev = t->zeros;
  const int Ho = (Hi + 2 - 3) / stride + 1, Wo = (Wi + 2 - 3) / stride + 1;
  DH_REQUIRE((int64_t)B * Hi * Wi * cin * 2 < ((int64_t)1 << 32), "conv3x3: input larger than 4 GiB, reduce the batch");
  return launch_conv3x3<__bf16>(stride, L, in, res, out, B, Hi, Wi, false, st, Ho, Wo);
}

struct BnFinal {   // per-channel arrays of one BN layer (forward statistics) and its affine parameters
  float *mean, *invstd, *scale, *shift, *run_mean, *run_var;
  const float *gamma, *beta;
  double n_rows;
};
BnFinal t2_bn_final(dh_train2* t, const T2Conv& c) {
  BnFinal f{};
  f.mean = c.bnb.mean; f.invstd = c.bnb.invstd; f.scale = c.bnb.scale; f.shift = c.bnb.shift;
  f.run_mean = t->R + t->rslot[c.bn + ".running_mean"].first;
  f.run_var = t->R + t->rslot[c.bn + ".running_var"].first;
  f.gamma = t->Pm + t->slot[c.bn + ".weight"].first;
  f.beta = t->Pm + t->slot[c.bn + ".bias"].first;
  f.n_rows = (double)((int64_t)t->B * c.Ho * c.Wo);
  return f;
}

// Small maps (stages 3-4): no finalize launches -- the channel-sliced consumers of bn_fold.inc add the partial rows themselves.
// DH_T2_FOLD=0: the round-3 path (partial sums -> finalize launch -> elementwise pass) everywhere, for A/B.
// (read when the engine is created, like DH_T2_JOIN: t->fold).  The channel-sliced REDUCTIONS run on small maps either way, so the two
// modes see the same partial rows and give the same bits (tests/test_gpu_train_bf16.py::test_bn_fold_is_bit_identical).
bool t2_small_map(int64_t rows, int C) {
  static const int fold_rows = dh::env_int("DH_T2_FOLD_ROWS");
  return C % CS_CH == 0 && C <= 2048 && rows >= 1 && rows <= fold_rows;
}
bool t2_fold_ok(const dh_train2* t, int64_t rows, int C) { return t->fold && t2_small_map(rows, C); }
// row groups of a channel-sliced launch: ~512 workgroups in all, at least 64 rows each; `cap` bounds the partial rows of a reduction
int t2_cs_groups(int64_t rows, int C, int cap) {
  const int slices = C / CS_CH;
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(cap, 512 / slices), (rows + 63) / 64));
}

// Z = conv(in).  `stats` (training forward): the batch statistics of Z are wanted; a 1x1 convolution takes the per-tile sums in its
// own epilogue and only the finalize launch follows (*stats_done then tells t2_bn_fwd to skip its pass over Z).
// `fold_rows` (non-null: the BN that follows is a plain apply pass that may add the partial rows itself): where the map is small, the
// finalize launch is left out and *fold_rows = the number of partial rows waiting in t->partial.
int t2_conv_fwd(dh_train2* t, T2Conv& c, const bf16_t* in, hipStream_t st, bool stats = false, bool* stats_done = nullptr, int* fold_rows = nullptr) {
  if (stats_done) *stats_done = false;
  if (fold_rows) *fold_rows = 0;
  if (c.ks == 3) return t2_conv3(t, c.cin, c.cout, c.stride, c.wp_f, in, nullptr, c.Z, t->B, c.Hi, c.Wi, st);
  const int64_t M = (int64_t)t->B * c.Ho * c.Wo, MB = (M + G2_BM - 1) / G2_BM;
  GemmFuse fu;
  if (stats && MB * 2 * c.cout <= T2_PARTIAL_FLOATS) fu.partial = t->partial;
  int rc = t2_gemm(in, c.wp_f, c.Z, M, c.cout, c.cin, c.stride, c.Ho, c.Wo, c.Hi, c.Wi, fu, st);
  if (rc || !fu.partial) return rc;
  if (fold_rows && MB <= CS_MAX_ROWS && t2_fold_ok(t, M, c.cout)) {   // the consumer finalizes (bn_fold.inc)
    *fold_rows = (int)MB;
    if (stats_done) *stats_done = true;
    return DH_OK;
  }
  const BnFinal f = t2_bn_final(t, c);
  if (!(g_t2_abl & 2)) hipLaunchKernelGGL(bn_stat_finalize_onepass_kernel, dim3((c.cout + FIN_CH - 1) / FIN_CH), dim3(256), 0, st, t->partial, (int)MB, c.cout, f.n_rows, f.mean,
                     f.invstd, f.gamma, f.beta, f.scale, f.shift, f.run_mean, f.run_var);
  DH_LAUNCH_CHECK();
  if (stats_done) *stats_done = true;
  return DH_OK;
}

// dX = dgrad(conv, dZ) [+ res]; `scratch` holds the zero-upsampled gradient (3x3 stride 2) or the low-resolution product (1x1 stride 2,
// which is then ADDED into dx: the caller has already written the other branch's gradient there)
// `mask` (1x1 stride 1 only): dx is zeroed where that tensor is <= 0 (the ReLU of the block output dx belongs to)
// `reduce_for` (1x1 stride 1 only): dx is the dY of that BN: the GEMM's epilogue also writes the per-tile sums of its backward pass
// into t->partial (relu mode `reduce_relu`: 0 dx as stored, 2 the BN's own ReLU from its Z); *reduce_rows = rows written
int t2_conv_dgrad(dh_train2* t, const T2Conv& c, const bf16_t* dz, const bf16_t* res, bf16_t* dx, bf16_t* scratch, bool accumulate,
                  hipStream_t st, const uint8_t* mask = nullptr, const T2Conv* reduce_for = nullptr, int reduce_relu = 0,
                  int* reduce_rows = nullptr) {
  if (reduce_rows) *reduce_rows = 0;
  const int B = t->B;
  DH_REQUIRE(!mask || (c.ks == 1 && c.stride == 1), "dgrad: the fused ReLU mask rides on the stride-1 1x1 GEMM");
  if (c.ks == 3) {
    DH_REQUIRE(!accumulate, "dgrad: 3x3 accumulate is not used");
    if (c.stride == 1) return t2_conv3(t, c.cout, c.cin, 1, c.wp_d, dz, res, dx, B, c.Ho, c.Wo, st);
    // The four parity classes of the dX pixel over dZ itself, side by side in one launch (launch_dgrad_s2: a quarter of the MFMA work of
    // the stride-1 conv over a zero-upsampled copy, no 4x-sized tensor written and read).  As four launches this was SLOWER than the
    // upsampled path at bf16 rate (ResNet-18 3.04 -> 3.11 ms per step: each launch fills a fraction of the chip); merged it wins
    // (2.665 -> 2.640 ms, ResNet-50 7.45 -> 7.43; the upsampled path left the engine in round 5).
    ConvLayer L{{"t2", "t2", c.cout, c.cin, 3, 1}};
    L.w_dev = c.wp_d; L.scale_dev = t->ones; L.shift_dev = t->zeros;
    return launch_dgrad_s2<__bf16>(L, dz, res, dx, B, c.Ho, c.Wo, c.Hi, c.Wi, st);
  }
  const int64_t M = (int64_t)B * c.Ho * c.Wo;
  GemmFuse fu;
  fu.mask_bits = mask;
  if (c.stride == 1 && reduce_for && ((M + G2_BM - 1) / G2_BM) * 2 * c.cin <= T2_PARTIAL_FLOATS) {
    fu.partial = t->partial; fu.bwd_of = reduce_for; fu.bwd_relu = reduce_relu;
    if (reduce_rows) *reduce_rows = (int)((M + G2_BM - 1) / G2_BM);
  }
  if (c.stride == 1) { fu.res = accumulate ? dx : res; return t2_gemm(dz, c.wp_d, dx, M, c.cin, c.cout, 1, c.Ho, c.Wo, c.Hi, c.Wi, fu, st); }
  DH_REQUIRE(accumulate && !res, "dgrad: a strided 1x1 conv is a downsample branch (accumulates into dx)");
  fu.mask_bits = nullptr;
  int rc = t2_gemm(dz, c.wp_d, scratch, M, c.cin, c.cout, 1, c.Ho, c.Wo, c.Hi, c.Wi, fu, st);
  if (rc) return rc;
  const int64_t n8 = M * c.cin / 8;
  hipLaunchKernelGGL(upsample2_add_bf16_kernel, dim3(grid_for(n8)), dim3(256), 0, st, scratch, dx, B, c.Ho, c.Wo, c.Hi, c.Wi, c.cin);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

struct Wg2Plan { int R, XR, XC, rb_per_img, total_steps, steps_per_slab, n_slabs, win_bytes, buf_bytes, t128, mp, np, ring; size_t lds; };
bool t2_side_default() { static const bool on = dh::env_int("DH_T2_SIDE") != 0; return on; }   // the engine's side stream is on unless switched off
int t2_wgrad_plan(const T2Conv& c, int B, Wg2Plan* q) {
  DH_REQUIRE(c.Wo <= 64, "wgrad: output rows of %d pixels exceed the 64-pixel step (patch too large for the bf16 engine)", c.Wo);
  const int KS = c.ks, s = c.stride;
  // 1x1 layers: four-quadrant workgroup tiles (wgrad1x1_quad_kernel): 128 x 128 when both channel counts are multiples of 128,
  // 64 couts x 256 cins / 256 x 64 for the 64-channel layers of stage 1; mp / np = 64-channel planes of dZ / X per workgroup
  int mp = 1, np = 1;
  if (KS == 1 && c.cin % 128 == 0 && c.cout % 128 == 0) mp = np = 2;
  else if (KS == 1 && c.cout == 64 && c.cin % 256 == 0) np = 4;
  else if (KS == 1 && c.cin == 64 && c.cout % 256 == 0) mp = 4;
  const int t128 = mp * np == 4 ? 1 : 0;
  // round 4: the quadrant configurations run on the LDS-DMA ring kernel (wgrad_ring.inc): flat 64-pixel steps, D stages in flight
  static const bool use_ring = dh::env_int("DH_WGRAD_RING") != 0;
  q->ring = (t128 && use_ring) ? 1 : 0;
  if (q->ring) {
    const int64_t M = (int64_t)B * c.Ho * c.Wo;
    DH_REQUIRE(M < ((int64_t)1 << 31), "wgrad: too many pixels");
    q->t128 = 1; q->mp = mp; q->np = np; q->R = q->XR = q->XC = q->rb_per_img = q->win_bytes = q->buf_bytes = 0;
    const int depth = (mp + np) == 4 ? 4 : 3;
    q->lds = (size_t)depth * (mp + np) * 8192;
    q->total_steps = (int)((M + 63) / 64);
    const int combos_r = (c.cout / (64 * mp)) * (c.cin / (64 * np));
    // 128 workgroups on the side stream (round 4 sweep, ResNet-50 step: 224: 7.02 ms, 192: 7.00, 160: 6.96, 128: 6.94, 96: 6.97): the ring kernel needs
    // fewer CUs than the round-3 kernel to move the same bytes, and every CU it leaves alone serves the main stream
    static const int WG_RING = dh::env_int("DH_WGRAD_RING_WGS") ? std::max(16, dh::env_int("DH_WGRAD_RING_WGS")) : (t2_side_default() ? 128 : 256);
    const int want = std::max(1, std::min(WG_RING / combos_r, q->total_steps));
    q->steps_per_slab = (q->total_steps + want - 1) / want;
    q->n_slabs = (q->total_steps + q->steps_per_slab - 1) / q->steps_per_slab;
    return DH_OK;
  }
  const int planes = np;
  const int maxpieces = t128 ? 96 : WG2_MAXX * 512 / 8;   // window pixels the staging plan can hold
  auto xr = [&](int R) { return KS == 3 ? (R - 1) * s + 3 : R; };
  const int XC = KS == 3 ? (((c.Wo - 1) * s + 3 + 3) & ~3) : ((c.Wo + 3) & ~3);
  int R = std::max(1, std::min(c.Ho, 64 / c.Wo));
  auto win = [&](int R_) { return planes * ((xr(R_) * XC * 128 + 511) & ~511); };
  while (R > 1 && (xr(R) * XC > maxpieces || 2 * (win(R) + mp * 64 * 128) > 150 * 1024)) --R;
  DH_REQUIRE(xr(R) * XC <= maxpieces, "wgrad: window %dx%d does not fit the staging plan", xr(R), XC);
  q->R = R; q->XR = xr(R); q->XC = XC; q->t128 = t128; q->mp = mp; q->np = np;
  q->win_bytes = win(R); q->buf_bytes = q->win_bytes + mp * 64 * 128;
  q->lds = std::max<size_t>((size_t)2 * q->buf_bytes, t128 ? (size_t)4 * 64 * 64 * 4 : (size_t)4 * 16 * 64 * 4);
  q->rb_per_img = (c.Ho + R - 1) / R;
  q->total_steps = B * q->rb_per_img;
  const int combos = (c.cout / (64 * mp)) * (c.cin / (64 * np));
  // one workgroup per CU: every workgroup writes its whole 64 x 64 (x taps) f32 tile as a slab (147 KB for a 3x3 conv), so the slab
  // traffic -- written here, read by the reduce kernel -- grows with the workgroup count whatever the layer: 512 workgroups moved
  // 75 MB per 3x3 conv each way.  Measured per ResNet-18 / ResNet-50 step: 768 -> 3.76 / 10.33 ms, 512 -> 3.53 / 9.86,
  // 384 -> 3.56 / 10.08, 256 -> 3.29 / 9.58, 192 -> 3.36 / 9.94, 128 -> 3.52 / 10.61.
  // On the side stream (round 3, late) 224: the weight-gradient workgroups hold a CU's LDS for their whole life, and with all 256 CUs
  // taken the main stream's next LDS-heavy launch waits for them to drain; 32 free CUs keep it moving (ResNet-50 7.25 -> 7.18 ms,
  // ResNet-18 2.505 -> 2.461; 240 / 192: 7.23 / 7.22, 2.48 / 2.47).  DH_WGRAD2_WGS overrides.
  static const int WG_TARGET = dh::env_int("DH_WGRAD2_WGS") ? std::max(16, dh::env_int("DH_WGRAD2_WGS")) : (t2_side_default() ? 224 : 256);
  int n_slabs = std::max(1, std::min(WG_TARGET / combos, q->total_steps));
  q->steps_per_slab = (q->total_steps + n_slabs - 1) / n_slabs;
  q->n_slabs = (q->total_steps + q->steps_per_slab - 1) / q->steps_per_slab;
  return DH_OK;
}

int t2_wgrad(dh_train2* t, const T2Conv& c, const bf16_t* x, const bf16_t* dz, hipStream_t st) {
  if (g_t2_abl & 1) return DH_OK;
  Wg2Plan q;
  int rc = t2_wgrad_plan(c, t->B, &q);
  if (rc) return rc;
  const int taps = c.ks * c.ks;
  const int64_t nw = (int64_t)c.cout * c.cin * taps;
  float* dw = t->G + t->slot[c.name + ".weight"].first;
  Wgrad2Params p;
  p.dz = dz; p.x = x;
  p.slabs = q.n_slabs == 1 ? dw : t->wgrad_slabs;   // a single slab IS the gradient
  DH_REQUIRE(q.n_slabs == 1 || (int64_t)q.n_slabs * nw <= t->wgrad_slab_floats, "wgrad: slab buffer too small");
  p.B = t->B; p.Hi = c.Hi; p.Wi = c.Wi; p.Cin = c.cin; p.Ho = c.Ho; p.Wo = c.Wo; p.Cout = c.cout; p.STRIDE = c.stride;
  p.R = q.R; p.XR = q.XR; p.XC = q.XC; p.rb_per_img = q.rb_per_img; p.total_steps = q.total_steps; p.steps_per_slab = q.steps_per_slab;
  p.win_bytes = q.win_bytes; p.buf_bytes = q.buf_bytes;
  p.tap_major = (c.ks == 3 && q.n_slabs > 1) ? 1 : 0;
  const int grid = q.n_slabs * (c.cout / (64 * q.mp)) * (c.cin / (64 * q.np));
  if (q.ring) {
    WgradRingParams r{};
    r.dz = dz; r.x = x; r.slabs = p.slabs;
    if ((rc = zero_page(&r.zero_page))) return rc;
    r.M = (int64_t)t->B * c.Ho * c.Wo; r.Cin = c.cin; r.Cout = c.cout; r.stride = c.stride; r.Ho = c.Ho; r.Wo = c.Wo; r.Hi = c.Hi; r.Wi = c.Wi;
    r.total_steps = q.total_steps; r.steps_per_slab = q.steps_per_slab;
    DH_REQUIRE(c.stride == 1 || c.stride == 2, "wgrad: stride %d", c.stride);
#define DH_WR_LAUNCH(MP_, NP_, D_)                                                                                                  \
    {                                                                                                                                \
      if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(&wgrad1x1_ring_kernel<MP_, NP_, D_>), 160 * 1024))) return rc;          \
      hipLaunchKernelGGL((wgrad1x1_ring_kernel<MP_, NP_, D_>), dim3(grid), dim3(512), q.lds, st, r);                                 \
    }
    if (q.mp == 2) DH_WR_LAUNCH(2, 2, 4)
    else if (q.mp == 1) DH_WR_LAUNCH(1, 4, 3)
    else DH_WR_LAUNCH(4, 1, 3)
#undef DH_WR_LAUNCH
  } else if (q.t128 && q.mp == 2) {
    if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(&wgrad1x1_quad_kernel<2, 2>), 160 * 1024))) return rc;
    hipLaunchKernelGGL((wgrad1x1_quad_kernel<2, 2>), dim3(grid), dim3(512), q.lds, st, p);
  } else if (q.t128 && q.mp == 1) {
    if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(&wgrad1x1_quad_kernel<1, 4>), 160 * 1024))) return rc;
    hipLaunchKernelGGL((wgrad1x1_quad_kernel<1, 4>), dim3(grid), dim3(512), q.lds, st, p);
  } else if (q.t128) {
    if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(&wgrad1x1_quad_kernel<4, 1>), 160 * 1024))) return rc;
    hipLaunchKernelGGL((wgrad1x1_quad_kernel<4, 1>), dim3(grid), dim3(512), q.lds, st, p);
  } else if (c.ks == 3) {
    if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(&wgrad_bf16_kernel<9>), 160 * 1024))) return rc;
    hipLaunchKernelGGL((wgrad_bf16_kernel<9>), dim3(grid), dim3(512), q.lds, st, p);
  } else {
    if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(&wgrad_bf16_kernel<1>), 160 * 1024))) return rc;
    hipLaunchKernelGGL((wgrad_bf16_kernel<1>), dim3(grid), dim3(512), q.lds, st, p);
  }
  DH_LAUNCH_CHECK();
  if (g_t2_abl & 16) return DH_OK;
  if (q.n_slabs > 1 && c.ks == 3) {
    const int64_t npairs = (int64_t)c.cout * c.cin;
    hipLaunchKernelGGL(wgrad_reduce_taps_kernel, dim3((unsigned)((npairs / 4 + 31) / 32), 9), dim3(256), 0, st, t->wgrad_slabs, q.n_slabs, npairs, dw);
    DH_LAUNCH_CHECK();
  } else if (q.n_slabs > 1) {
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((nw / 4 + 31) / 32)), dim3(256), 0, st, t->wgrad_slabs, q.n_slabs, nw, dw);
    DH_LAUNCH_CHECK();
  }
  return DH_OK;
}

// ---- batch norm ---------------------------------------------------------------------------------------------
// pool_out / pool_idx (the stem): the normalised map goes straight through ReLU and the 3x3/2 maxpool (bn2_apply_pool_kernel); c.Y stays unwritten
// join_bn (a block's top BN whose identity comes out of a downsample branch): the branch's BN is applied inside this BN's elementwise pass
// (bn2_apply_join_kernel); the branch itself runs with apply = false (statistics and coefficients only, its Y stays unwritten)
// fold_rows > 0: the producing GEMM left that many partial rows and NO finalize launch has run (t2_conv_fwd): this call must fold
// bits (a block's top BN, training): the ReLU pattern of Y is also written as one byte per 8 channels (st8_bits)
int t2_bn_fwd(dh_train2* t, T2Conv& c, const bf16_t* res, bool relu, bool training, hipStream_t st, bool have_stats = false,
              bf16_t* pool_out = nullptr, uint8_t* pool_idx = nullptr, bool apply = true, const T2Conv* join_bn = nullptr, int fold_rows = 0,
              uint8_t* bits = nullptr) {
  const int C = c.cout;
  const int64_t rows = (int64_t)t->B * c.Ho * c.Wo;
  const BnFinal f = t2_bn_final(t, c);
  const bool plain = apply && !join_bn && !pool_out;
  DH_REQUIRE(fold_rows <= 0 || (training && have_stats && plain), "bn forward: folded statistics need a plain apply pass");
  int nb = fold_rows;            // partial rows waiting for a finalize (0: none)
  if (training && !have_stats && DH_ABL_SKIP_STATS(c) && !pool_out) {
    nb = t2_small_map(rows, C) ? t2_cs_groups(rows, C, 32) : t2_red_blocks(rows, C);
  } else if (training && !have_stats) {
    if (t2_small_map(rows, C) && !pool_out) {   // small map: the channel-sliced reduction, one partial row per row group
      nb = t2_cs_groups(rows, C, 32);
      hipLaunchKernelGGL((bn2_cs_reduce_kernel<0>), dim3((C / CS_CH) * nb), dim3(256), 0, st, c.Z, static_cast<const bf16_t*>(nullptr),
                         static_cast<const bf16_t*>(nullptr), static_cast<const float*>(nullptr), static_cast<const float*>(nullptr),
                         static_cast<const float*>(nullptr), static_cast<const float*>(nullptr), rows, C, 0, t->partial);
    } else {
      nb = t2_red_blocks(rows, C);
      hipLaunchKernelGGL(bn2_stats_kernel, dim3(nb), dim3(256), 0, st, c.Z, rows, C, t->partial);
    }
  }
  if (training && nb > 0 && plain && nb <= CS_MAX_ROWS && t2_fold_ok(t, rows, C)) {   // the apply pass adds the rows itself (bn_fold.inc)
    const int nrg = t2_cs_groups(rows, C, 256);
    if (!DH_ABL_SKIP_APPLY()) hipLaunchKernelGGL(bn2_fold_apply_kernel, dim3((C / CS_CH) * nrg), dim3(256), 0, st, c.Z, t->partial, nb, f.n_rows, f.gamma, f.beta, f.mean, f.invstd,
                       f.scale, f.shift, f.run_mean, f.run_var, res, c.Y, rows, C, relu ? 1 : 0, bits);
    DH_LAUNCH_CHECK();
    return DH_OK;
  }
  if (training && nb > 0) {
    if (!(g_t2_abl & 2)) hipLaunchKernelGGL(bn_stat_finalize_onepass_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(256), 0, st, t->partial, nb, C, (double)rows, f.mean,
                       f.invstd, f.gamma, f.beta, f.scale, f.shift, f.run_mean, f.run_var);
  } else if (!training) {
    hipLaunchKernelGGL(bn2_eval_coef_kernel, dim3((C + 255) / 256), dim3(256), 0, st, f.gamma, f.beta, f.run_mean, f.run_var, c.bnb.scale, c.bnb.shift, C);
  }
  const int64_t n8 = rows * C / 8;
  if (!apply) return DH_OK;
  if (join_bn) {
    DH_REQUIRE(relu && !res && !pool_out && join_bn->cout == C && 256 % (C / 8) == 0, "bn join: ReLU'd top BN of a downsample block");
    if (!(g_t2_abl & 4)) hipLaunchKernelGGL(bn2_apply_join_kernel, dim3(grid_for(n8)), dim3(256), 0, st, c.Z, c.bnb.scale, c.bnb.shift, join_bn->Z, join_bn->bnb.scale,
                       join_bn->bnb.shift, c.Y, n8, C, bits);
    DH_LAUNCH_CHECK();
    return DH_OK;
  }
  if (pool_out) {
    DH_REQUIRE(relu && !res && pool_idx && 256 % (C / 8) == 0, "bn + pool: ReLU'd BN without a residual, C <= 2048");
    const int Hp = (c.Ho + 2 - 3) / 2 + 1, Wp = (c.Wo + 2 - 3) / 2 + 1;
    hipLaunchKernelGGL(bn2_apply_pool_kernel, dim3(grid_for((int64_t)t->B * Hp * Wp * (C / 8))), dim3(256), 0, st, c.Z, c.bnb.scale, c.bnb.shift,
                       pool_out, pool_idx, t->B, c.Ho, c.Wo, C, Hp, Wp);
  } else {
    if (!(g_t2_abl & 4) && !DH_ABL_SKIP_APPLY()) hipLaunchKernelGGL(bn2_apply_kernel, dim3(grid_for(n8)), dim3(256), 0, st, c.Z, c.bnb.scale, c.bnb.shift, res, c.Y, n8, C, relu ? 1 : 0, bits);
  }
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// The route record of one BN's backward pass (the backward tap of train_hooks.inc; the values: include/deephisto_hip_debug.h): plain host values.
enum { T2R_RELU = 0, T2R_PREMASKED, T2R_IN_MASK, T2R_HAVE_ROWS, T2R_REDUCE, T2R_APPLY, T2R_BRANCH, T2R_ROWS, T2R_N };
enum { T2R_REDUCE_EPILOGUE = 0, T2R_REDUCE_SLICED = 1, T2R_REDUCE_BLOCKS = 2, T2R_REDUCE_POOL = 3 };
enum { T2R_APPLY_FOLD = 1, T2R_APPLY_FINALIZE = 2 };
enum { T2R_BRANCH_NONE = 0, T2R_BRANCH_BLOCK_HAS_DOWNSAMPLE = 1, T2R_BRANCH_IS_DOWNSAMPLE = 2 };
struct T2BwdTap {   // one BN, named by its conv: device float32 copies of what its backward read and wrote, and the route on the host
  const T2Conv* c;
  float* grad_in;   // the tensor the BN's backward read as dy
  float* g_out;     // the masked gradient it wrote (null where it writes none)
  int32_t* route;   // host, T2R_N values
};

// relu: 0 none (no ReLU, or dy arrives masked), 1 pattern from y_mask (the BN output was joined with an identity before the ReLU),
// 2 pattern recomputed from Z
// have_rows > 0: the GEMM that produced dy already left that many rows of per-tile sums in t->partial (no reduction pass)
// route (the backward tap of train_hooks.inc; null in every step): receives which launches ran, route[T2R_REDUCE .. T2R_ROWS]
int t2_bn_bwd(dh_train2* t, T2Conv& c, const bf16_t* dy, const bf16_t* y_mask, int relu, bf16_t* dz, bf16_t* g_out, hipStream_t st,
              int have_rows = 0, int32_t* route = nullptr) {
  const int C = c.cout;
  const int64_t rows = (int64_t)t->B * c.Ho * c.Wo;
  const float* gamma = t->Pm + t->slot[c.bn + ".weight"].first;
  float* dgamma = t->G + t->slot[c.bn + ".weight"].first;
  float* dbeta = t->G + t->slot[c.bn + ".bias"].first;
  int nb = have_rows;
  if (route) route[T2R_REDUCE] = T2R_REDUCE_EPILOGUE;
  if (nb <= 0 && t2_small_map(rows, C)) {   // small map: the channel-sliced reduction, one partial row per row group
    nb = t2_cs_groups(rows, C, 32);
    if (route) route[T2R_REDUCE] = T2R_REDUCE_SLICED;
    if (!(g_t2_abl & 64)) hipLaunchKernelGGL((bn2_cs_reduce_kernel<1>), dim3((C / CS_CH) * nb), dim3(256), 0, st, c.Z, dy, y_mask, c.bnb.mean, c.bnb.invstd, c.bnb.scale,
                       c.bnb.shift, rows, C, relu, t->partial);
    have_rows = nb;
  }
  if (nb > 0 && nb <= CS_MAX_ROWS && t2_fold_ok(t, rows, C)) {   // no finalize launch: the apply pass adds the rows itself (bn_fold.inc)
    const int nrg = t2_cs_groups(rows, C, 256);
    if (route) { route[T2R_APPLY] = T2R_APPLY_FOLD; route[T2R_ROWS] = nb; }
    if (!(g_t2_abl & 32)) hipLaunchKernelGGL(bn2_fold_bwd_apply_kernel, dim3((C / CS_CH) * nrg), dim3(256), 0, st, dy, y_mask, c.Z, t->partial, nb, (double)rows, gamma,
                       c.bnb.mean, c.bnb.invstd, c.bnb.scale, c.bnb.shift, dgamma, dbeta, dz, g_out, rows, C, relu);
    DH_LAUNCH_CHECK();
    return DH_OK;
  }
  if (nb <= 0) nb = t2_red_blocks(rows, C);
  if (route) { route[T2R_APPLY] = T2R_APPLY_FINALIZE; route[T2R_ROWS] = nb; if (have_rows <= 0) route[T2R_REDUCE] = T2R_REDUCE_BLOCKS; }
  if (have_rows <= 0)
    if (!(g_t2_abl & 64)) hipLaunchKernelGGL(bn2_bwd_reduce_kernel, dim3(nb), dim3(256), 0, st, c.Z, dy, y_mask, c.bnb.mean, c.bnb.invstd, c.bnb.scale, c.bnb.shift, rows, C,
                       relu, t->partial);
  if (!(g_t2_abl & 2)) hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(256), 0, st, t->partial, nb, C, (double)rows, gamma, c.bnb.mean,
                     c.bnb.invstd, dgamma, dbeta, c.bnb.k0, c.bnb.k1, c.bnb.k2);
  const int64_t n8 = rows * C / 8;
  if (!(g_t2_abl & 32)) hipLaunchKernelGGL(bn2_bwd_apply_kernel, dim3(grid_for(n8)), dim3(256), 0, st, dy, y_mask, c.Z, c.bnb.k0, c.bnb.k1, c.bnb.k2, c.bnb.scale,
                     c.bnb.shift, dz, g_out, n8, C, relu);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// BN(+ReLU, pattern from Z) backward of a map that went through the 3x3/2 maxpool (the stem): dy is gathered from the pooled gradient
// and the recorded positions inside both passes (no maxpool-backward launch, no 112 x 112 gradient tensor in HBM)
int t2_bn_pool_bwd(dh_train2* t, T2Conv& c, const bf16_t* dpool, const uint8_t* pool_idx, bf16_t* dz, hipStream_t st) {
  const int C = c.cout;
  DH_REQUIRE(256 % (C / 8) == 0, "bn + pool backward: C <= 2048");
  const int64_t rows = (int64_t)t->B * c.Ho * c.Wo;
  const int64_t blocks4 = (int64_t)t->B * ((c.Ho + 1) / 2) * ((c.Wo + 1) / 2);   // 2 x 2 pixel blocks: the unit of both passes
  const int nb = t2_red_blocks(blocks4, 4 * C);
  const int Hp = (c.Ho + 2 - 3) / 2 + 1, Wp = (c.Wo + 2 - 3) / 2 + 1;
  const float* gamma = t->Pm + t->slot[c.bn + ".weight"].first;
  float* dgamma = t->G + t->slot[c.bn + ".weight"].first;
  float* dbeta = t->G + t->slot[c.bn + ".bias"].first;
  hipLaunchKernelGGL(bn2_pool_bwd_reduce_kernel, dim3(nb), dim3(256), 0, st, c.Z, dpool, pool_idx, c.bnb.mean, c.bnb.invstd, c.bnb.scale,
                     c.bnb.shift, t->B, c.Ho, c.Wo, C, Hp, Wp, t->partial);
  if (!(g_t2_abl & 2)) hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(256), 0, st, t->partial, nb, C, (double)rows, gamma, c.bnb.mean,
                     c.bnb.invstd, dgamma, dbeta, c.bnb.k0, c.bnb.k1, c.bnb.k2);
  hipLaunchKernelGGL(bn2_pool_bwd_apply_kernel, dim3(grid_for(blocks4 * C / 8)), dim3(256), 0, st, c.Z, dpool, pool_idx, c.bnb.k0, c.bnb.k1, c.bnb.k2,
                     c.bnb.scale, c.bnb.shift, dz, t->B, c.Ho, c.Wo, C, Hp, Wp);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// The stem's dW [64][3][7][7] (`dw`, float32) from bf16 dz [B][Ho][Wo][64] and the float32 NCHW image x: per-slab partial sums over at
// most STEM_WGRAD_SLABS runs of output rows on bf16 MFMA (stem_wgrad_bf16_kernel; `slabs`: STEM_WGRAD_SLABS * 64 * 160 floats), then
// their fixed-order reduction.
int t2_stem_wgrad(const bf16_t* dz, const float* x, float* slabs, float* dw, int B, int P, int Ho, int Wo, hipStream_t st) {
  const StemSlabs sl = stem_wgrad_split(B, Ho);
  DH_REQUIRE(Wo * 8 <= 2 * SWG_T && P + 6 <= SWG_T, "stem wgrad: patch %d too wide for the row staging", P);
  DH_REQUIRE(Wo % 16 == 0, "stem wgrad (bf16 MFMA): the output width %d is not a multiple of 16 pixels", Wo);
  const size_t lds = std::max<size_t>(((size_t)((21 * (P + 6) + 7) & ~7) + (size_t)Wo * 64) * 2, (size_t)64 * 160 * sizeof(float));
  hipLaunchKernelGGL(stem_wgrad_bf16_kernel, dim3(sl.n_slabs), dim3(SWG_T), lds, st, dz, x, slabs, B, P, Ho, Wo, sl.rows_per_slab);
  DH_LAUNCH_CHECK();
  return stem_wgrad_reduce(slabs, sl.n_slabs, dw, st);
}

void t2_free_shape(dh_train2* t) {
  store_free_shape(*t);
  t->B = t->P = 0;
}

// activations / workspaces of a batch shape (the arenas and packed weights are shape-independent)
int t2_shape(dh_train2* t, int B, int P) {
  if (t->B == B && t->P == P) return DH_OK;
  t2_free_shape(t);
  t->shape_phase = true;
  auto done = [&](int r) { t->shape_phase = false; if (r) t2_free_shape(t); return r; };
  const int H1 = (P + 6 - 7) / 2 + 1, H2 = (H1 + 2 - 3) / 2 + 1;
  int64_t maxact = (int64_t)B * H1 * H1 * 64;
  int rc;
  if ((rc = conv_shapes(t->convs, t->blocks, P, [&](T2Conv& c, int i, bool top) -> int {
        const int64_t nout = (int64_t)B * c.Ho * c.Wo * c.cout;
        maxact = std::max(maxact, std::max(nout, (int64_t)B * c.Hi * c.Hi * std::max(c.cin, 8)));
        maxact = std::max(maxact, (int64_t)B * c.Hi * c.Hi * c.cout);   // zero-upsampled gradient of a stride-2 conv
        int r;
        if ((r = store_alloc(*t, &c.Z, nout)) || (r = store_alloc(*t, &c.Y, nout))) return r;
        if (top && (r = store_alloc(*t, &c.Ybits, nout / 8))) return r;
        if (t->side_wgrad && i > 0 && (r = store_alloc(*t, &c.dZ, nout))) return r;
        return DH_OK;
      }))) return done(rc);
  const int64_t S1 = (int64_t)B * H2 * H2 * 64;
  if ((rc = store_alloc(*t, &t->X1, S1)) || (rc = store_alloc(*t, &t->pool_idx, S1)) || (rc = store_alloc(*t, &t->pooled, (int64_t)B * t->feat)))
    return done(rc);
  for (int i = 0; i < 6; ++i) if ((rc = store_alloc(*t, &t->GB[i], maxact))) return done(rc);
  // slab buffer of the weight gradients: the largest n_slabs * weights over the layers (a single slab goes straight to G)
  t->B = B; t->P = P;
  int64_t need = 0;
  for (size_t i = 1; i < t->convs.size(); ++i) {
    Wg2Plan q;
    if ((rc = t2_wgrad_plan(t->convs[i], B, &q))) return done(rc);
    if (q.n_slabs > 1) need = std::max(need, (int64_t)q.n_slabs * t->convs[i].cout * t->convs[i].cin * t->convs[i].ks * t->convs[i].ks);
  }
  t->wgrad_slab_floats = need;
  if ((rc = store_alloc(*t, &t->wgrad_slabs, need))) return done(rc);
  return done(DH_OK);
}

}  // namespace

extern "C" int dh_train2_create(dh_train2** out, const char* arch, int32_t n_classes) {
  DH_REQUIRE(out && arch, "train2 create: null argument");
  const NetDesc* desc = net_desc(arch);
  DH_REQUIRE(desc != nullptr, "train2 create: unknown architecture '%s'", arch);
  DH_REQUIRE(n_classes > 0 && n_classes <= 1024, "train2 create: n_classes=%d", n_classes);
  if (int erc = dh::env_check()) return erc;   // a mistyped DH_* switch stops here, named by dh_last_error()
  auto* t = new dh_train2();
  t->n_classes = n_classes; t->feat = desc->feat; t->blocks = desc->blocks;
  convs_from_desc(t->convs, *desc);
  t2_layout(t);
  int rc;
  auto fail = [&](int r) { store_free_all(*t); delete t; return r; };
  if ((rc = store_alloc_arenas(*t, nullptr)) || (rc = store_alloc(*t, &t->ones, 2048)) ||
      (rc = store_alloc(*t, &t->zeros, 2048)) || (rc = store_alloc(*t, &t->partial, T2_PARTIAL_FLOATS)) ||
      (rc = store_alloc(*t, &t->stem_slabs, (int64_t)STEM_WGRAD_SLABS * 64 * 160))) return fail(rc);
  hipLaunchKernelGGL(fill_kernel, dim3(8), dim3(256), 0, nullptr, t->ones, (int64_t)2048, 1.0f);
  if (hipMemsetAsync(t->zeros, 0, 2048 * 4, nullptr) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) return fail(DH_EHIP);   // the caller's streams need not be ordered behind the null stream
  for (T2Conv& c : t->convs) {
    const int64_t nw = (int64_t)c.cout * c.cin * c.ks * c.ks;   // operands in bf16
    if (c.ks == 7) { if ((rc = store_alloc(*t, reinterpret_cast<bf16_t**>(&c.wp_f), 7 * 2 * 2 * FRAG_BYTES / 2))) return fail(rc); }
    else if ((rc = store_alloc(*t, reinterpret_cast<bf16_t**>(&c.wp_f), nw)) || (rc = store_alloc(*t, reinterpret_cast<bf16_t**>(&c.wp_d), nw))) return fail(rc);
    if ((rc = store_alloc_bn(*t, c.bnb, c.cout))) return fail(rc);
  }
  store_set_buckets(*t, 0, nullptr, nullptr, nullptr);   // one bucket until the caller cuts its own
  // The weight-gradient kernels (one workgroup per CU, bound by their operand ingest) run on a side stream next to the HBM-bound
  // BN backward and the dgrad of the following layers.  Round 2 handed every convolution over by itself (two events per
  // convolution: ResNet-50 8.84 -> 8.56 ms per step, ResNet-18 slower); with one hand-off per block and a dZ buffer per
  // convolution (round 3) both gain: ResNet-50 8.19 -> 7.60 ms, ResNet-18 2.96 -> 2.81 ms.  DH_T2_SIDE=0/1 overrides.
  t->side_wgrad = dh::env_int("DH_T2_SIDE") != 0;
  t->join_fused = dh::env_int("DH_T2_JOIN") != 0;
  t->fold = dh::env_int("DH_T2_FOLD") != 0;
  if (t->side_wgrad && (rc = store_open_side(*t))) return fail(rc);
  *out = t;
  return DH_OK;
}

extern "C" void dh_train2_destroy(dh_train2* t) {
  if (!t) return;
  (void)hipDeviceSynchronize();
  store_free_all(*t);
  delete t;
}

// store_tensor on the engine's arenas; a pushed parameter makes the packed bf16 operands stale
extern "C" int dh_train2_tensor(dh_train2* t, const char* name, int32_t kind, void* ptr, int64_t n_elem, int32_t to_lib, void* stream) {
  DH_REQUIRE(t && name && ptr && kind >= 0 && kind <= 2, "train2 tensor: bad arguments");
  const int rc = store_tensor(*t, "train2 tensor", name, kind, ptr, n_elem, to_lib, dh::as_stream(stream));
  if (rc == DH_OK && to_lib && kind == 0 && !strstr(name, "num_batches_tracked")) t->packed = false;
  return rc;
}

extern "C" int dh_train2_flat(dh_train2* t, int32_t kind, void** ptr_out, int64_t* n_out) {
  DH_REQUIRE(t && ptr_out && n_out && kind >= 0 && kind <= 2, "train2 flat: bad arguments");
  store_flat(*t, kind, ptr_out, n_out);
  return DH_OK;
}

// Gradient buckets for the data-parallel all-reduce (store_set_buckets has the contract): prefixes of the backward-ordered arena
extern "C" int dh_train2_set_buckets(dh_train2* t, int64_t bucket_bytes, dh_bucket_cb cb, void* user, int32_t* n_buckets_out) {
  DH_REQUIRE(t && bucket_bytes >= 0, "train2 buckets: bad arguments");
  store_set_buckets(*t, bucket_bytes, cb, user, n_buckets_out);
  return DH_OK;
}
extern "C" int dh_train2_bucket(dh_train2* t, int32_t i, int64_t* offset, int64_t* count) {
  DH_REQUIRE(t, "train2 bucket: index out of range");
  return store_bucket(*t, "train2 bucket", i, offset, count);
}

// bf16 wire format for gradient buckets (both engines' arenas: offsets and counts are multiples of 4 elements, 16-byte aligned):
// pack = float32 -> bf16 (RNE) before the all-reduce, unpack = bf16 sum -> float32 * scale (1 / world) after it.
extern "C" int dh_grad_pack_bf16(const float* src_dev, uint16_t* dst_dev, int64_t n, void* stream) {
  DH_REQUIRE(src_dev && dst_dev, "grad pack: null src_dev or dst_dev");
  DH_REQUIRE(n >= 0 && n % 4 == 0, "grad pack: n=%lld is not a whole number of 4-element granules", (long long)n);
  DH_REQUIRE((reinterpret_cast<uintptr_t>(src_dev) & 15) == 0, "grad pack: src_dev is not 16-byte aligned");
  DH_REQUIRE((reinterpret_cast<uintptr_t>(dst_dev) & 7) == 0, "grad pack: dst_dev is not 8-byte aligned");
  if (n == 0) return DH_OK;
  hipLaunchKernelGGL(grad_pack_bf16_kernel, dim3(grid_for(n / 4)), dim3(256), 0, dh::as_stream(stream), src_dev, dst_dev, n / 4);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
extern "C" int dh_grad_unpack_bf16(const uint16_t* src_dev, float* dst_dev, int64_t n, float scale, void* stream) {
  DH_REQUIRE(src_dev && dst_dev, "grad unpack: null src_dev or dst_dev");
  DH_REQUIRE(n >= 0 && n % 4 == 0, "grad unpack: n=%lld is not a whole number of 4-element granules", (long long)n);
  DH_REQUIRE((reinterpret_cast<uintptr_t>(src_dev) & 7) == 0, "grad unpack: src_dev is not 8-byte aligned");
  DH_REQUIRE((reinterpret_cast<uintptr_t>(dst_dev) & 15) == 0, "grad unpack: dst_dev is not 16-byte aligned");
  if (n == 0) return DH_OK;
  hipLaunchKernelGGL(grad_unpack_bf16_kernel, dim3(grid_for(n / 4)), dim3(256), 0, dh::as_stream(stream), src_dev, dst_dev, n / 4, scale);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// x_dev: float32[n][3][P][P] NCHW (kept alive by the caller until backward when training) -> logits float32[n][n_classes]
extern "C" int dh_train2_forward(dh_train2* t, const float* x, int64_t n, int32_t P, float* logits, int32_t training, void* stream) {
  DH_REQUIRE(t && x && logits, "train2 forward: null argument");
  DH_REQUIRE(n >= 1 && n <= 1024 && P >= 64 && P <= 256 && P % 32 == 0, "train2 forward: need 1 <= n <= 1024, 64 <= P <= 256, P %% 32 == 0 (got %lld, %d)",
             (long long)n, P);
  hipStream_t st = dh::as_stream(stream);
  int rc;
  if ((rc = t2_shape(t, (int)n, P))) return rc;
  if (!t->packed && (rc = t2_pack_all(t, st))) return rc;
  const int B = (int)n;
  const bool tr = training != 0;
  t->x_in = x; t->last_training = tr; t->bwd_done = false;
  {   // stem: raw conv -> BN + ReLU -> maxpool
    T2Conv& c = t->convs[0];
    StemParams sp;
    sp.x_nchw = x; sp.slide = nullptr; sp.yx = nullptr; sp.row_bytes = 0;
    sp.w = c.wp_f; sp.scale = t->ones; sp.shift = t->zeros; sp.out = c.Z;
    sp.B = B; sp.P = P; sp.Ho = c.Ho; sp.Wo = c.Wo; sp.relu = 0;
    sp.tiles_y = (c.Ho + STEM_TH - 1) / STEM_TH; sp.tiles_x = (c.Wo + STEM_TW - 1) / STEM_TW;
    const size_t lds = (size_t)7 * 2 * 2 * FRAG_BYTES + (size_t)STEM_ROWS * STEM_ROWE * 2;
    if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(&stem_kernel<__bf16, false>), 96 * 1024))) return rc;
    hipLaunchKernelGGL((stem_kernel<__bf16, false>), dim3(B * sp.tiles_y * sp.tiles_x), dim3(256), lds, st, sp);
    DH_LAUNCH_CHECK();
    if ((rc = t2_bn_fwd(t, c, nullptr, true, tr, st, false, t->X1, t->pool_idx))) return rc;   // + ReLU + maxpool in the same pass
  }
  const bf16_t* X = t->X1;
  for (const BlockDesc& b : t->blocks) {
    const bf16_t* in = X;
    for (int i = 0; i < b.nconv; ++i) {
      T2Conv& c = t->convs[b.conv[i]];
      bool have = false, dhave = false;
      // a plain apply pass follows (not the join of a downsample block, whose GEMM would overwrite the partial rows first): it may fold
      int frows = 0;
      const bool may_fold = tr && (i + 1 < b.nconv || b.ds < 0);
      if ((rc = t2_conv_fwd(t, c, in, st, tr, &have, may_fold ? &frows : nullptr))) return rc;
      if (i + 1 < b.nconv) {
#if DH_T2_ABL
        g_abl_consumer_ks = t->convs[b.conv[i + 1]].ks;
#endif
        if ((rc = t2_bn_fwd(t, c, nullptr, true, tr, st, have, nullptr, nullptr, true, nullptr, frows))) return rc;
#if DH_T2_ABL
        g_abl_consumer_ks = 0;
#endif
      } else {
        const bf16_t* idt = X;
        const T2Conv* jb = nullptr;
        if (b.ds >= 0) {
          T2Conv& d = t->convs[b.ds];
          const bool fuse = t->join_fused && 256 % (d.cout / 8) == 0;
          if ((rc = t2_conv_fwd(t, d, X, st, tr, &dhave)) || (rc = t2_bn_fwd(t, d, nullptr, false, tr, st, dhave, nullptr, nullptr, !fuse))) return rc;
          if (fuse) { jb = &d; idt = nullptr; } else idt = d.Y;
        }
        if ((rc = t2_bn_fwd(t, c, idt, true, tr, st, have, nullptr, nullptr, true, jb, frows, tr ? c.Ybits : nullptr))) return rc;
      }
      in = c.Y;
    }
    X = in;
  }
  const T2Conv& last = t->convs[t->blocks.back().conv[t->blocks.back().nconv - 1]];
  hipLaunchKernelGGL(avgpool2_kernel, dim3(B), dim3(256), 0, st, X, last.Ho * last.Wo, t->feat, t->pooled);
  hipLaunchKernelGGL(fc_fwd_kernel, dim3((B * t->n_classes + 3) / 4), dim3(256), 0, st, t->pooled, t->Pm + t->slot["fc.weight"].first,
                     t->Pm + t->slot["fc.bias"].first, B, t->feat, t->n_classes, logits);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

namespace {
// A block whose successor's first convolution is a stride-1 1x1 GEMM without a downsample branch receives its gradient ALREADY
// masked by its own join-ReLU (t2_backward)
bool t2_premasked(const dh_train2* t, int bi) {
  if (bi + 1 >= (int)t->blocks.size()) return false;
  const BlockDesc& nx = t->blocks[bi + 1];
  const T2Conv& c0 = t->convs[nx.conv[0]];
  return nx.ds < 0 && c0.ks == 1 && c0.stride == 1;
}

// `fused` (single-rank training): the Adam update and the bf16 repack of a block's tensors follow that block's weight gradients on
// the side stream, instead of one update of the whole arena after the pass (same arithmetic per element: identical parameters).
// `tap` (the backward tap of train_hooks.inc only, null in every step): copies of one BN's operands, enqueued between the launches below; no
// launch of the pass, no argument of one and no buffer it uses depends on it.
int t2_backward(dh_train2* t, const float* dlogits, hipStream_t st, const AdamArgs* fused, const T2BwdTap* tap = nullptr) {
  const int B = t->B, ncls = t->n_classes;
  int rc;
  // the tapped BN: a float32 copy of its incoming gradient (right before its first reader, after its only writer) and the route's host
  // values; returns where t2_bn_bwd records its launches
  auto tap_in = [&](const T2Conv& c, const bf16_t* g, int64_t n, int relu, bool pm, bool masked, int have_rows, int branch) -> int32_t* {
    if (!tap || tap->c != &c) return nullptr;
    hipLaunchKernelGGL(bf16_to_f32_kernel, dim3(grid_for(n)), dim3(256), 0, st, g, tap->grad_in, n);
    int32_t* r = tap->route;
    r[T2R_RELU] = relu; r[T2R_PREMASKED] = pm; r[T2R_IN_MASK] = masked; r[T2R_HAVE_ROWS] = have_rows; r[T2R_BRANCH] = branch;
    r[T2R_REDUCE] = r[T2R_APPLY] = r[T2R_ROWS] = 0;
    return r;
  };
  store_begin_backward(*t);
  auto mark_done = [&]() { store_mark_done(*t); };
  const T2Conv& lastc = t->convs[t->blocks.back().conv[t->blocks.back().nconv - 1]];
  const int HW = lastc.Ho * lastc.Wo;
  hipLaunchKernelGGL(fc_wgrad_kernel, dim3((ncls * t->feat + 255) / 256), dim3(256), 0, st, dlogits, t->pooled, B, t->feat, ncls,
                     t->G + t->slot["fc.weight"].first, t->G + t->slot["fc.bias"].first);
  bf16_t *dOut = t->GB[0], *Gm = t->GB[1], *dZ = t->GB[2], *dY = t->GB[3], *dX = t->GB[4], *scr = t->GB[5];
  // Which stream a weight gradient runs on, the hand-offs, the joins and the fused optimiser are BwdSched's (train_core.inc): this pass
  // hands a block's weight gradients over behind the block and joins only where a bucket is due -- and in front of the stem's tail.
  const bool side = t->side_wgrad;
  auto sched = bwd_sched<bf16_t>(*t, st, fused, (int)t->convs.size(),
      [&](int i, const bf16_t* xin, const bf16_t* dz, hipStream_t q) { return t2_wgrad(t, t->convs[i], xin, dz, q); },
      [&](int lo, int hi, hipStream_t q) { return t2_pack(t, q, lo, hi + 1); }, (g_t2_abl & 8) != 0, (g_t2_abl & 8) != 0);
  auto next_dz = [&](T2Conv& c) { if (side && c.dZ) dZ = c.dZ; };
  auto wgrad_of = [&](int i, const bf16_t* xin) { return sched.queue(i, xin, dZ); };
  auto bucket_due = [&]() { return store_bucket_due(*t); };
  int top_rows = 0;   // rows of BN-backward sums the last dgrad GEMM left for the NEXT block's join BN (0: none)
  hipLaunchKernelGGL(avgpool_fc_dgrad2_kernel, dim3(B), dim3(256), 0, st, dlogits, t->Pm + t->slot["fc.weight"].first, HW, t->feat, ncls, dOut);
  DH_LAUNCH_CHECK();
  mark_done();   // fc
  // A block whose successor's first convolution is a stride-1 1x1 GEMM without a downsample branch receives its gradient ALREADY
  // masked by its own join-ReLU: that GEMM's dgrad epilogue computes (W^T dZ + identity gradient) * (block output > 0).  Its top
  // BN backward then reads neither the block output nor writes the masked copy: the incoming tensor IS the identity gradient.
  auto premasked = [&](int bi) { return t2_premasked(t, bi); };
  for (int bi = (int)t->blocks.size() - 1; bi >= 0; --bi) {
    const BlockDesc& b = t->blocks[bi];
    const bf16_t* Xin = bi == 0 ? t->X1 : t->convs[t->blocks[bi - 1].conv[t->blocks[bi - 1].nconv - 1]].Y;
    const bf16_t* grad = dOut;
    const bool pm = premasked(bi);
    const bf16_t* gm = pm ? dOut : Gm;             // the gradient that flows down the identity branch
    // this block's dX is the predecessor's masked gradient: the ReLU pattern of the predecessor's output, one byte per 8 channels
    const uint8_t* in_mask = bi > 0 && premasked(bi - 1) ? t->convs[t->blocks[bi - 1].conv[t->blocks[bi - 1].nconv - 1]].Ybits : nullptr;
    // Where a BN's dY comes out of a 1x1 dgrad GEMM, that GEMM's epilogue also leaves the per-tile sums of the BN's backward pass
    // in t->partial (`rows` of them): the 3x3 conv's BN (dY = dgrad of conv3, its own ReLU recomputed from Z) and the join BN of a
    // pre-masked block (dY = the successor's masked dX).  The BN backward then starts at its finalize launch.
    int rows = top_rows;
    top_rows = 0;
    for (int i = b.nconv - 1; i >= 0; --i) {
      T2Conv& c = t->convs[b.conv[i]];
      const bool top = i == b.nconv - 1;
      // top conv of the block: its BN output was joined with the identity and ReLU'd; the masked gradient also feeds the identity branch
      next_dz(c);
      const int64_t n_c = (int64_t)B * c.Ho * c.Wo * c.cout;
      const int bn_rows = top && !pm ? 0 : rows;
      int32_t* route = tap_in(c, grad, n_c, top ? (pm ? 0 : 1) : 2, pm, in_mask && b.ds < 0, bn_rows,
                              b.ds >= 0 ? T2R_BRANCH_BLOCK_HAS_DOWNSAMPLE : T2R_BRANCH_NONE);
      if (top && pm) { if ((rc = t2_bn_bwd(t, c, grad, nullptr, 0, dZ, nullptr, st, rows, route))) return rc; }
      else if ((rc = t2_bn_bwd(t, c, grad, c.Y, top ? 1 : 2, dZ, top ? Gm : nullptr, st, top ? 0 : rows, route))) return rc;
      if (route && top && !pm && tap->g_out) hipLaunchKernelGGL(bf16_to_f32_kernel, dim3(grid_for(n_c)), dim3(256), 0, st, Gm, tap->g_out, n_c);
      rows = 0;
      const bf16_t* xin = i == 0 ? Xin : t->convs[b.conv[i - 1]].Y;
      if ((rc = wgrad_of(b.conv[i], xin))) return rc;
      if (i > 0) {
        const T2Conv* below = &t->convs[b.conv[i - 1]];   // its BN output feeds a ReLU directly: mode 2
        if ((rc = t2_conv_dgrad(t, c, dZ, nullptr, dY, scr, false, st, nullptr, below, 2, &rows))) return rc;
        grad = dY;
      } else {
        const T2Conv* prev_top = (in_mask && b.ds < 0) ? &t->convs[t->blocks[bi - 1].conv[t->blocks[bi - 1].nconv - 1]] : nullptr;
        if ((rc = t2_conv_dgrad(t, c, dZ, b.ds < 0 ? gm : nullptr, dX, scr, false, st, b.ds < 0 ? in_mask : nullptr, prev_top, 0, &top_rows))) return rc;
      }
      if (bucket_due() && (rc = sched.join(0))) return rc;
      mark_done();
    }
    if (b.ds >= 0) {
      T2Conv& d = t->convs[b.ds];
      next_dz(d);
      int32_t* route = tap_in(d, gm, (int64_t)B * d.Ho * d.Wo * d.cout, 0, pm, false, 0, T2R_BRANCH_IS_DOWNSAMPLE);
      if ((rc = t2_bn_bwd(t, d, gm, nullptr, 0, dZ, nullptr, st, 0, route))) return rc;
      if ((rc = wgrad_of(b.ds, Xin))) return rc;
      if ((rc = t2_conv_dgrad(t, d, dZ, nullptr, dX, scr, true, st))) return rc;
      if (bucket_due() && (rc = sched.join(0))) return rc;
      mark_done();
    }
    if ((rc = sched.flush(0))) return rc;   // behind the block: its items are marked done
    std::swap(dOut, dX);
  }
  {   // stem: maxpool backward, BN + ReLU backward, weight gradient (f32 MFMA on the f32 input image)
    T2Conv& c = t->convs[0];
    dZ = t->GB[2];
    const int Hp = (c.Ho + 2 - 3) / 2 + 1, Wp = (c.Wo + 2 - 3) / 2 + 1;
    if (int32_t* route = tap_in(c, dOut, (int64_t)B * Hp * Wp * c.cout, 2, false, false, 0, T2R_BRANCH_NONE)) {
      route[T2R_REDUCE] = T2R_REDUCE_POOL; route[T2R_APPLY] = T2R_APPLY_FINALIZE;
      route[T2R_ROWS] = t2_red_blocks((int64_t)B * ((c.Ho + 1) / 2) * ((c.Wo + 1) / 2), 4 * c.cout);
    }
    // The stem's tail runs ALONE: next to the side stream's weight gradients of layer 1 the column sums of bn2_pool_bwd_reduce_kernel were
    // not reproducible (ResNet-50, P = 96, B = 32: 8 to 39 of 39 identical steps differed in one to six channels of dgamma / dbeta by up to
    // 3 % of the largest, operands bit-identical; none without the side stream: tests/test_gpu_step_bwd.py, FOUND).  Nothing is handed to
    // the side stream after this point, so the join that the optimiser needs anyway moves in front of the tail.
    if ((rc = sched.join(0))) return rc;
    if ((rc = t2_bn_pool_bwd(t, c, dOut, t->pool_idx, dZ, st))) return rc;   // maxpool + ReLU + BN backward, dY never materialised
    if ((rc = t2_stem_wgrad(dZ, t->x_in, t->stem_slabs, t->G + t->slot["conv1.weight"].first, B, t->P, c.Ho, c.Wo, st))) return rc;
    mark_done();   // the optimiser (and the last bucket) follow on the main stream, behind the join above
    if ((rc = sched.tail())) return rc;   // fused: what the side stream has not updated -- the stem (all of the arena without a side stream)
  }
  t->bwd_done = true;
  return DH_OK;
}
}  // namespace

extern "C" int dh_train2_backward(dh_train2* t, const float* dlogits, void* stream) {
  DH_REQUIRE(t && dlogits && t->B > 0 && t->last_training, "train2 backward: no training forward has run");
  return t2_backward(t, dlogits, dh::as_stream(stream), nullptr);
}

// Backward pass and Adam step of a single-rank training step in one call (no gradient exchange in between): the update and the bf16
// repack of each residual block's tensors run on the side stream behind that block's weight gradients.  Same result as
// dh_train2_backward followed by dh_train2_adam_step, bit for bit.
extern "C" int dh_train2_backward_adam(dh_train2* t, const float* dlogits, float lr, float beta1, float beta2, float eps, int64_t step,
                                       void* stream) {
  DH_REQUIRE(t && dlogits && t->B > 0 && t->last_training, "train2 backward: no training forward has run");
  DH_REQUIRE(t->bucket_cb == nullptr, "train2 backward_adam: gradient buckets are armed (data-parallel steps call backward and adam_step)");
  const AdamArgs a = adam_args(*t, lr, beta1, beta2, eps, step);
  int rc = t2_backward(t, dlogits, dh::as_stream(stream), &a);
  if (rc == DH_OK) t->packed = true;
  return rc;
}

extern "C" int dh_train2_adam_step(dh_train2* t, float lr, float beta1, float beta2, float eps, int64_t step, void* stream) {
  DH_REQUIRE(t, "train2 adam: null handle");
  hipStream_t st = dh::as_stream(stream);
  adam_range(*t, adam_args(*t, lr, beta1, beta2, eps, step), 0, t->n_params, st);
  DH_LAUNCH_CHECK();
  return t2_pack_all(t, st);
}
