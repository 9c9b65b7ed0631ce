// train.inc -- training step of the ResNet-18 patch classifier (SURVEY row a7), float32.
// HOST side only: the engine's kernels are train_kernels.inc's, the kernels it shares with the bf16 engine train_core_kernels.inc's.
// Included at the end of resnet_kernels.hip (same translation unit: reuses the conv kernels), behind train_core.inc (the parameter
// store, buckets, Adam launch, conv record and backward scheduler shared with the bf16 engine).  The file ends with its last product entry
// point: the test hooks over this code are train_hooks.inc's, declared in include/deephisto_hip_debug.h.
//
// Replaces, for the network of models/patch_cls_simple/model.py:5-11, the work of
//   outputs = model(inputs); loss = criterion(outputs, labels); loss.backward(); optimizer.step()
// (models/patch_cls_simple/train.py:168-172; CrossEntropyLoss mean, Adam betas (0.9, 0.999),
// eps 1e-8, BN momentum 0.1 / eps 1e-5 -- PyTorch defaults).
//
// Layout: activations and their gradients are NHWC float32.  Master parameters, gradients and
// Adam moments live in HBM in torch's own layouts ([cout][cin][kh][kw], ...), so they are
// exchanged with the caller by plain device copies; MFMA-fragment-ordered copies of the conv
// weights (forward order, and transposed+flipped for dgrad) are re-packed on the device after
// every update.
//   forward  : conv (the inference kernels with unit scale / zero shift) -> batch statistics
//              -> normalise (+residual) (+ReLU)
//   backward : ReLU mask + BN backward (two per-channel sums, then one elementwise pass),
//              dgrad = the same 3x3 conv kernel on the flipped weights (stride 2: the four
//              parity classes of dX over dZ itself), wgrad = pixel-reduction GEMM on v_mfma_f32_32x32x2_f32
//              (K = output pixels); per-workgroup partial tiles go to slab buffers with plain stores and are summed
//              in a fixed order: no float atomics anywhere in the step, so gradients and updates are bit-reproducible.
#include <array>
// Timing-only ablations of the float32 step: a COMPILE-TIME macro of diagnostic builds (tools/build_variant.sh -DDH_T1_ABL=<bits>; results are
// garbage), absent from the shipped library like DH_T2_ABL.  1 no 3x3 weight-gradient launches, 2 no tap-slab reduces, 4 no re-pack, 8 no Adam
#ifndef DH_T1_ABL
#define DH_T1_ABL 0
#endif

// =====================================================================================
// host side: training state of a dh_resnet18 handle
// =====================================================================================
struct dh_train : TrainStore {   // the arena is in FORWARD order: the backward pass completes it from the end
  int B = 0, P = 0;
  std::vector<TrainConv> convs;   // index 0 = stem; copies of the architecture's NetDesc (net_desc.inc) plus this engine's buffers (train_core.inc)
  std::vector<BlockDesc> blocks;  // forward order
  float *ones = nullptr, *zeros = nullptr, *partial = nullptr;
  float *X1 = nullptr, *pooled = nullptr;
  float *BIG1 = nullptr, *SM[4] = {nullptr, nullptr, nullptr, nullptr};
  float* stem_slabs = nullptr;
  uint8_t* pool_idx = nullptr;    // first-maximum position (0..8) of every maxpool output element
  float* wgrad_slabs = nullptr;   // [n_slabs][Cout][Cin][9] partial gradients of the 3x3 wgrad
  PackTable<PackDescF> pack;      // table of pack_all_f32_kernel; descriptor j = conv j + 1 (the stem has its own kernel)
  const float* x_in = nullptr;  // input of the last forward (caller memory; must stay alive until backward)
  bool bwd_done = false;        // a backward pass has run since the last forward: every dZ buffer holds THIS step's gradient (debug tap)
  // TrainStore::side: the weight gradients are handed over once per residual block: they fill the CUs the persistent
  // convolution launches leave idle in their last round of tiles.  DH_T1_SIDE=0: everything on the caller's stream.
};

namespace {

constexpr int WGRAD3_WGS = 256;       // workgroups of the 3x3 wgrad (one per CU: ~135-147 KiB of LDS each)

// Diagnostics of a DIAGNOSTIC BUILD only (tools/build_variant.sh dump -DDH_TRAIN_DUMP_BUILD=1; tools/grad_trace.py): with the macro,
// the environment variable DH_TRAIN_DUMP=<dir> makes dh_resnet18_backward write named intermediate gradients as raw float32 files
// (synchronous).  The shipped library compiles tr_dump to nothing and does not know the variable.
#ifndef DH_TRAIN_DUMP_BUILD
inline void tr_dump(const char*, int, const float*, int64_t, hipStream_t) {}
#else
void tr_dump(const char* name, int blk, const float* dev, int64_t n, hipStream_t st) {
  static const char* dir = getenv("DH_TRAIN_DUMP");
  if (!dir) return;
  std::vector<float> h((size_t)n);
  if (hipStreamSynchronize(st) != hipSuccess) return;
  if (hipMemcpy(h.data(), dev, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) return;
  char path[512];
  snprintf(path, sizeof path, "%s/b%d_%s.bin", dir, blk, name);
  if (FILE* f = fopen(path, "wb")) { fwrite(h.data(), 4, (size_t)n, f); fclose(f); }
}
#endif

// packs the weights of convs [i0, i1), 1 <= i0 (the stem has its own kernel: tr_pack_all)
int tr_pack(dh_train* t, hipStream_t st, int i0, int i1) {
  if (!t->pack.dev) {
    for (size_t i = 1; i < t->convs.size(); ++i) {
      const TrainConv& c = t->convs[i];
      DH_REQUIRE(c.ks != 3 || (c.cout % 64 == 0 && c.cin % 64 == 0), "pack: 3x3 convolution %s with %d -> %d channels (multiples of 64)", c.name.c_str(), c.cin, c.cout);
      t->pack.add({t->Pm + t->slot[c.name + ".weight"].first, static_cast<float*>(c.wp_f), static_cast<float*>(c.wp_d), c.cout, c.cin, c.ks, 0},
                  packf_blocks(c.cout, c.cin, c.ks));
    }
    if (int rc = t->pack.upload(*t)) return rc;
  }
  if (i1 <= i0) return DH_OK;
  const auto l = t->pack.range(i0 - 1, i1 - 1);
  if (!(DH_T1_ABL & 4)) hipLaunchKernelGGL(pack_all_f32_kernel, dim3(l.grid), dim3(256), PACKF_LDS, st, l.first, l.count, l.blk_base);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
int tr_pack_stem(dh_train* t, hipStream_t st) {
  hipLaunchKernelGGL(pack_stem_dev_kernel, dim3(40), dim3(256), 0, st, t->Pm + t->slot[t->convs[0].name + ".weight"].first, static_cast<float*>(t->convs[0].wp_f));
  DH_LAUNCH_CHECK();
  return DH_OK;
}
int tr_pack_all(dh_train* t, hipStream_t st) {
  int rc = tr_pack_stem(t, st);
  return rc ? rc : tr_pack(t, st, 1, (int)t->convs.size());
}

// The launch helpers below take what they use (no engine handle), so the test hooks (train_hooks.inc) run the very code of a step.
// `ones` / `zeros`: per-channel unit scale and zero shift (at least `cout` floats) of the inference kernels' epilogue.
struct UnitAffine { const float *ones, *zeros; };

// conv through the inference kernels with unit scale / zero shift (raw conv output).  1x1 (the downsample branches; round 5): the
// float32 GEMM of gemm1x1_f32.inc -- `wp` is then W[cout][cin] K-contiguous: the master tensor (forward) or the transposed copy of the
// data gradient's operator (pack_all_f32_kernel).
int tr_conv(UnitAffine u, int cin, int cout, int ks, int stride, const void* wp, const float* in,
            const float* res, float* out, int B, int Hi, int Wi, hipStream_t st) {
  if (ks == 1) {
    const int Ho = (Hi - 1) / stride + 1, Wo = (Wi - 1) / stride + 1;
    return gemm1x1_f32(in, static_cast<const float*>(wp), res, out, (int64_t)B * Ho * Wo, cout, cin, stride, Ho, Wo, Hi, Wi, st);
  }
  ConvLayer L{{"train", "train", cin, cout, ks, stride}};
  L.w_dev = const_cast<void*>(wp);
  L.scale_dev = const_cast<float*>(u.ones);
  L.shift_dev = const_cast<float*>(u.zeros);
  int ho, wo;
  return run_conv<float>(L, in, res, out, B, Hi, Wi, false, st, &ho, &wo);
}

// dX = data gradient of a 3x3 / stride-2 conv (cz channels of dZ -> cx channels of dX) from the packed dgrad operator `wp`
int tr_dgrad_s2(UnitAffine u, int cz, int cx, const void* wp, const float* dz, const float* res, float* dx, int B, int Ho, int Wo,
                int Hi, int Wi, hipStream_t st) {
  ConvLayer L{{"train", "train", cz, cx, 3, 1}};
  L.w_dev = const_cast<void*>(wp);
  L.scale_dev = const_cast<float*>(u.ones);
  L.shift_dev = const_cast<float*>(u.zeros);
  return launch_dgrad_s2<float>(L, dz, res, dx, B, Ho, Wo, Hi, Wi, st);
}

// One BN layer as its launches see it: pre-activation map Z [rows][C], affine parameters and their gradients, running statistics,
// the per-channel buffers and the reduction workspace `partial` (RED_NB * 2 * C floats).  B, Ho, Wo: only the pooled (stem) paths.
struct BnView {
  const float* Z;
  const float *gamma, *beta;
  float *run_mean, *run_var, *dgamma, *dbeta;
  BnBufs bn;
  int64_t rows;
  int C, B, Ho, Wo;
  float* partial;
  int red_blocks(int64_t units) const { const int rpi = 256 / (C / 4); return (int)std::min<int64_t>(RED_NB, (units + rpi - 1) / rpi); }
};
BnView tr_bn_view(dh_train* t, const TrainConv& c) {
  const int64_t w = t->slot[c.bn + ".weight"].first, b = t->slot[c.bn + ".bias"].first;
  return {c.Z, t->Pm + w, t->Pm + b, t->R + t->rslot[c.bn + ".running_mean"].first, t->R + t->rslot[c.bn + ".running_var"].first,
          t->G + w, t->G + b, c.bnb, (int64_t)t->B * c.Ho * c.Wo, c.cout, t->B, c.Ho, c.Wo, t->partial};
}

// y = [relu](bn(Z) [+ res]) with batch statistics.  pool_out / pool_idx (the stem): normalise + ReLU + 3x3/2 maxpool in one pass
// (bn_apply_pool_kernel); y stays unwritten
int tr_bn_forward(const BnView& v, const float* res, bool relu, float* y, hipStream_t st, float* pool_out = nullptr, uint8_t* pool_idx = nullptr) {
  const int C = v.C;
  const int nb = v.red_blocks(v.rows);
  // one pass: {sum z, sum z^2} per workgroup in float32, column sums and E[z^2] - mean^2 in double
  hipLaunchKernelGGL((col_reduce_kernel<3>), dim3(nb), dim3(256), 0, st, v.Z, nullptr, nullptr, nullptr, nullptr, v.rows, C, 0, v.partial);
  hipLaunchKernelGGL(bn_stat_finalize_onepass_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(256), 0, st, v.partial, nb, C, (double)v.rows,
                     v.bn.mean, v.bn.invstd, v.gamma, v.beta, v.bn.scale, v.bn.shift, v.run_mean, v.run_var);
  const int64_t n4 = v.rows * C / 4;
  if (pool_out) {
    DH_REQUIRE(relu && !res && pool_idx, "bn + pool: ReLU'd BN without a residual");
    const int Hp = (v.Ho + 2 - 3) / 2 + 1, Wp = (v.Wo + 2 - 3) / 2 + 1;
    hipLaunchKernelGGL(bn_apply_pool_kernel, dim3(grid_for((int64_t)v.B * Hp * Wp * (C / 4))), dim3(256), 0, st, v.Z, v.bn.scale, v.bn.shift,
                       pool_out, pool_idx, v.B, v.Ho, v.Wo, C, Hp, Wp);
  } else {
    hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_for(n4)), dim3(256), 0, st, v.Z, v.bn.scale, v.bn.shift, res, y, n4, C, relu ? 1 : 0);
  }
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// dZ (and optionally the masked gradient g) from dY for one BN(+ReLU); fills dgamma / dbeta
// relu with y_for_mask == nullptr: the BN output went straight into a ReLU (no identity term): the pattern is recomputed from Z
int tr_bn_backward(const BnView& v, const float* dy, const float* y_for_mask, bool relu, float* dz, float* g_out, hipStream_t st) {
  const int rmode = !relu ? 0 : y_for_mask ? 1 : 2;
  const int C = v.C;
  const int nb = v.red_blocks(v.rows);
  hipLaunchKernelGGL((col_reduce_kernel<2>), dim3(nb), dim3(256), 0, st, v.Z, dy, y_for_mask, v.bn.mean, v.bn.invstd, v.rows, C,
                     rmode, v.partial, v.bn.scale, v.bn.shift);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(256), 0, st, v.partial, nb, C, (double)v.rows, v.gamma,
                     v.bn.mean, v.bn.invstd, v.dgamma, v.dbeta, v.bn.k0, v.bn.k1, v.bn.k2);
  const int64_t n4 = v.rows * C / 4;
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_for(n4)), dim3(256), 0, st, dy, y_for_mask, v.Z, v.bn.k0, v.bn.k1, v.bn.k2,
                     dz, g_out, n4, C, rmode, v.bn.scale, v.bn.shift);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// BN(+ReLU, pattern from Z) backward of a map that went through the 3x3/2 maxpool (the stem): dy is gathered from the pooled gradient and
// the recorded positions inside both passes (no maxpool-backward launch, no 112 x 112 gradient tensor in HBM)
int tr_bn_pool_backward(const BnView& v, const float* dpool, const uint8_t* pool_idx, float* dz, hipStream_t st) {
  const int C = v.C;
  const int64_t blocks4 = (int64_t)v.B * ((v.Ho + 1) / 2) * ((v.Wo + 1) / 2);
  const int nb = v.red_blocks(blocks4);
  const int Hp = (v.Ho + 2 - 3) / 2 + 1, Wp = (v.Wo + 2 - 3) / 2 + 1;
  hipLaunchKernelGGL(bn_pool_bwd_reduce_kernel, dim3(nb), dim3(256), 0, st, v.Z, dpool, pool_idx, v.bn.mean, v.bn.invstd, v.bn.scale,
                     v.bn.shift, v.B, v.Ho, v.Wo, C, Hp, Wp, v.partial);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(256), 0, st, v.partial, nb, C, (double)v.rows, v.gamma,
                     v.bn.mean, v.bn.invstd, v.dgamma, v.dbeta, v.bn.k0, v.bn.k1, v.bn.k2);
  hipLaunchKernelGGL(bn_pool_bwd_apply_kernel, dim3(grid_for(blocks4 * C / 4)), dim3(256), 0, st, v.Z, dpool, pool_idx, v.bn.k0, v.bn.k1,
                     v.bn.k2, v.bn.scale, v.bn.shift, dz, v.B, v.Ho, v.Wo, C, Hp, Wp);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// The stem's dW [64][3][7][7] (`dw`) from dz [B][Ho][Wo][64] and the NCHW image x [B][3][P][P]: per-slab partial sums over at most
// STEM_WGRAD_SLABS runs of output rows (`slabs`: STEM_WGRAD_SLABS * 64 * 160 floats), then their fixed-order reduction.
int tr_stem_wgrad(const float* dz, const float* x, float* slabs, float* dw, int B, int P, int Ho, int Wo, hipStream_t st) {
  const StemSlabs sl = stem_wgrad_split(B, Ho);
  const size_t lds = std::max<size_t>((size_t)21 * (P + 6) + (size_t)Wo * 64, (size_t)64 * 160) * sizeof(float);
  DH_REQUIRE(lds <= 64 * 1024 && Wo * 16 <= 4 * SWG_T && P + 6 <= SWG_T, "stem wgrad: patch %d too wide for the row staging", P);
  hipLaunchKernelGGL(stem_wgrad_kernel, dim3(sl.n_slabs), dim3(SWG_T), lds, st, dz, x, slabs, B, P, Ho, Wo, sl.rows_per_slab);
  return stem_wgrad_reduce(slabs, sl.n_slabs, dw, st);
}

// dW (`dw_out`) of one conv from its input x and output gradient dz; `wgrad_slabs` holds WGRAD3_WGS * 64*64*9 floats.  `force_pertap`
// routes a 3x3 layer through the per-tap kernel (the path of layers whose rows do not fit the fused kernel; test hook).
int tr_wgrad(float* wgrad_slabs, float* dw_out, const TrainConv& c, const float* x, const float* dz, int B,
             hipStream_t st, bool force_pertap = false) {
  WgradParams p;
  p.dz = dz; p.x = x; p.slabs = nullptr;
  p.B = B; p.Hi = c.Hi; p.Wi = c.Wi; p.Cin = c.cin; p.Ho = c.Ho; p.Wo = c.Wo; p.Cout = c.cout;
  p.KS = c.ks; p.STRIDE = c.stride; p.PAD = c.ks / 2;
  p.npx = (int64_t)B * c.Ho * c.Wo;
  // fused 9-tap kernel when one output row's window fits its staging plan (else the per-tap kernel below)
  if (!force_pertap && c.ks == 3 && c.Wo <= 64 && 3 * ((c.Wo - 1) * c.stride + 3) * 16 <= WG3_MAXX * 512) {
    Wgrad3Params q;
    q.dz = dz; q.x = x; q.slabs = wgrad_slabs;
    q.B = B; q.Hi = c.Hi; q.Wi = c.Wi; q.Cin = c.cin; q.Ho = c.Ho; q.Wo = c.Wo; q.Cout = c.cout; q.STRIDE = c.stride;
    const int combos3 = (c.cout / 64) * (c.cin / 64);
    const int XC = (c.Wo - 1) * c.stride + 3;   // staged window columns (halo included)
    auto xrows = [&](int R) { return (R - 1) * c.stride + 3; };
    auto buf_floats = [&](int R) { return (xrows(R) * XC + ((R * c.Wo + 1) & ~1)) * 64; };
    int R = std::max(1, std::min(c.Ho, 64 / c.Wo));
    while (R > 1 && (buf_floats(R) * 8 + 256 > 160 * 1024 || xrows(R) * XC * 16 > WG3_MAXX * 512)) --R;
    q.R = R; q.XR = xrows(R); q.XC = XC;
    q.dzpix = (R * c.Wo + 1) & ~1;
    q.buf_floats = buf_floats(R);
    DH_REQUIRE(q.XR * q.XC * 16 <= WG3_MAXX * 512 && q.dzpix * 16 <= WG3_MAXD * 512 && R * c.Wo <= 64,
               "wgrad3: window %dx%d does not fit the staging plan", q.XR, q.XC);
    const size_t lds = std::max<size_t>((size_t)256 + (size_t)q.buf_floats * 8, (size_t)4 * 9 * 16 * 64 * 4);
    DH_REQUIRE(lds <= 160 * 1024, "wgrad3: LDS budget exceeded (%zu B)", lds);
    q.rb_per_img = (c.Ho + R - 1) / R;
    q.total_steps = B * q.rb_per_img;
    // on the side stream 224 of the 256 CUs: wgrad3 workgroups hold a whole CU's LDS for ~180 us, and with every CU taken the main stream's
    // next convolution waits for them to drain (8.72 -> 8.51 ms per step; 248 / 240 / 232 / 216 / 208 / 192: 8.67 / 8.68 / 8.52 / 8.56 / 8.64 / 8.64)
    static const bool side_on = dh::env_int("DH_T1_SIDE") != 0;
    static const int wgs_limit = dh::env_int("DH_WGRAD3_WGS") ? std::max(16, std::min(WGRAD3_WGS, dh::env_int("DH_WGRAD3_WGS"))) : (side_on ? 224 : WGRAD3_WGS);
    int n_slabs = std::max(1, std::min(wgs_limit / combos3, q.total_steps));
    q.steps_per_slab = (q.total_steps + n_slabs - 1) / n_slabs;
    n_slabs = (q.total_steps + q.steps_per_slab - 1) / q.steps_per_slab;
    DH_REQUIRE((int64_t)n_slabs * combos3 <= WGRAD3_WGS, "wgrad3: slab buffer too small");
    if (int arc = ensure_dyn_lds(reinterpret_cast<const void*>(&wgrad3_kernel), 160 * 1024)) return arc;
    if (!(DH_T1_ABL & 1)) hipLaunchKernelGGL(wgrad3_kernel, dim3(n_slabs * combos3), dim3(512), lds, st, q);
    const int64_t npairs = (int64_t)c.cout * c.cin;
    if (!(DH_T1_ABL & 2)) hipLaunchKernelGGL(wgrad_reduce_taps_kernel, dim3((unsigned)((npairs / 4 + 31) / 32), 9), dim3(256), 0, st, wgrad_slabs, n_slabs, npairs, dw_out);
    DH_LAUNCH_CHECK();
    return DH_OK;
  }
  // per-tap kernel (1x1 convs; 3x3 layers whose rows do not fit the fused kernel's staging plan): slabs + fixed-order reduce
  const int64_t pairs = (p.npx + 1) / 2;
  const int combos = c.ks * c.ks * (c.cout / 64) * (c.cin / 64);
  const int max_wgs = WGRAD3_WGS * 9;   // 64x64 tiles that fit the slab buffer
  DH_REQUIRE(combos <= max_wgs, "wgrad: %d weight tiles exceed the slab buffer", combos);
  int n_slabs = (int)std::max<int64_t>(1, std::min<int64_t>(max_wgs / combos, (pairs + 63) / 64));
  p.pairs_per_slab = (int)(((pairs + n_slabs - 1) / n_slabs + 15) / 16 * 16);  // whole 32-pixel chunks
  n_slabs = (int)((pairs + p.pairs_per_slab - 1) / p.pairs_per_slab);
  p.n_slabs = n_slabs;
  p.slabs = wgrad_slabs;
  hipLaunchKernelGGL(wgrad_kernel, dim3(n_slabs * combos), dim3(256), 0, st, p);
  const int64_t nw = (int64_t)c.cout * c.cin * c.ks * c.ks;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((nw / 4 + 31) / 32)), dim3(256), 0, st, wgrad_slabs, n_slabs, nw, dw_out);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// first train_begin: convs and blocks from the network description (net_desc.inc), the arena layout in forward order, and the completion
// items of the backward pass: fc, the blocks last to first, the stem -- each runs from its first tensor down to where the previous item started
void tr_layout(dh_resnet18* net) {
  dh_train* t = net->train;
  convs_from_desc(t->convs, *net->desc);
  t->blocks = net->desc->blocks;
  for (const TrainConv& c : t->convs) store_add_conv(*t, c, true);
  store_add(*t, "fc.weight", (int64_t)net->n_classes * net->desc->feat); store_add(*t, "fc.bias", net->n_classes);
  int64_t end = t->n_params;
  auto item_from = [&](int64_t start) { t->items.push_back({start, end - start}); end = start; };
  item_from(t->slot["fc.weight"].first);
  for (auto b = t->blocks.rbegin(); b != t->blocks.rend(); ++b) item_from(t->slot[t->convs[b->conv[0]].name + ".weight"].first);
  item_from(0);
}

}  // namespace

extern "C" int dh_resnet18_train_begin(dh_resnet18* net, int64_t n, int32_t P, void* stream) {
  DH_REQUIRE(net != nullptr, "train begin: null handle");
  DH_REQUIRE(net->dtype == DH_DTYPE_F32, "train begin: training is float32 only in this build");
  DH_REQUIRE(n >= 1 && n <= 1024 && P >= 64 && P % 32 == 0, "train begin: need 1 <= n <= 1024 and P %% 32 == 0 (got %lld, %d)",
             (long long)n, P);
  if (net->train && net->train->B == (int)n && net->train->P == P) return DH_OK;
  hipStream_t st = dh::as_stream(stream);
  const int B = (int)n;
  int rc;
  dh_train* t = net->train;
  if (!t) {
    // ---- first use: parameter arenas (masters, gradients, Adam moments, running statistics), packed weights,
    // per-channel BN buffers.  These live until train_end: a later change of the batch shape (a short last batch,
    // a train-mode forward at another size) keeps the optimizer state and re-makes only the activations below.
    t = new dh_train();
    net->train = t;
    if (dh::env_int("DH_T1_SIDE") != 0 && (rc = store_open_side(*t))) return rc;
    tr_layout(net);
    if ((rc = store_alloc_arenas(*t, st))) return rc;
    for (const auto& kv : t->slot) {
      auto it = net->params.find(kv.first);
      DH_REQUIRE(it != net->params.end(), "train begin: parameter '%s' was never set", kv.first.c_str());
      DH_HIP(hipMemcpyAsync(t->Pm + kv.second.first, it->second.data(), kv.second.second * 4, hipMemcpyHostToDevice, st));
    }
    for (const auto& kv : t->rslot) {
      auto it = net->params.find(kv.first);
      DH_REQUIRE(it != net->params.end(), "train begin: buffer '%s' was never set", kv.first.c_str());
      DH_HIP(hipMemcpyAsync(t->R + kv.second.first, it->second.data(), kv.second.second * 4, hipMemcpyHostToDevice, st));
    }
    if ((rc = store_alloc(*t, &t->ones, 512)) || (rc = store_alloc(*t, &t->zeros, 512)) ||
        (rc = store_alloc(*t, &t->partial, (int64_t)RED_NB * 2 * 512)) ||
        (rc = store_alloc(*t, &t->stem_slabs, (int64_t)STEM_WGRAD_SLABS * 64 * 160)) ||
        (rc = store_alloc(*t, &t->wgrad_slabs, (int64_t)WGRAD3_WGS * 64 * 64 * 9))) return rc;
    hipLaunchKernelGGL(fill_kernel, dim3(2), dim3(256), 0, st, t->ones, (int64_t)512, 1.0f);
    DH_HIP(hipMemsetAsync(t->zeros, 0, 512 * 4, st));
    for (TrainConv& c : t->convs) {
      const int64_t nw = (int64_t)c.cout * c.cin * c.ks * c.ks;
      if (c.ks == 7) { if ((rc = store_alloc(*t, reinterpret_cast<float**>(&c.wp_f), 7 * 11 * 2 * 64))) return rc; }
      else if ((rc = store_alloc(*t, reinterpret_cast<float**>(&c.wp_f), nw)) || (rc = store_alloc(*t, reinterpret_cast<float**>(&c.wp_d), nw))) return rc;
      if ((rc = store_alloc_bn(*t, c.bnb, c.cout))) return rc;
    }
    if ((rc = tr_pack_all(t, st))) return rc;
  } else {
    store_free_shape(*t);   // batch shape changed: drop the (B, P)-sized buffers only
  }
  t->B = B; t->P = P;
  // ---- activations and workspaces of this batch shape
  t->shape_phase = true;
  auto shape_done = [&](int r) { t->shape_phase = false; return r; };
  if ((rc = conv_shapes(t->convs, t->blocks, P, [&](TrainConv& c, int i, bool) -> int {
        const int64_t nout = (int64_t)B * c.Ho * c.Wo * c.cout;
        int r;
        if ((r = store_alloc(*t, &c.Z, nout)) || (r = store_alloc(*t, &c.Y, nout))) return r;
        if (t->side && i > 0 && (r = store_alloc(*t, &c.dZ, nout))) return r;
        return DH_OK;
      }))) return shape_done(rc);
  const int H2 = t->convs[t->blocks[0].conv[0]].Hi;   // behind the stem's maxpool
  const int64_t S1 = (int64_t)B * H2 * H2 * 64;
  if ((rc = store_alloc(*t, &t->X1, S1)) || (rc = store_alloc(*t, &t->pool_idx, S1)) ||
      (rc = store_alloc(*t, &t->pooled, (int64_t)B * 512)) ||
      (rc = store_alloc(*t, &t->BIG1, 4 * S1))) return shape_done(rc);
  for (int i = 0; i < 4; ++i) if ((rc = store_alloc(*t, &t->SM[i], S1))) return shape_done(rc);
  return shape_done(DH_OK);
}

extern "C" int dh_resnet18_train_end(dh_resnet18* net) {
  DH_REQUIRE(net != nullptr, "train end: null handle");
  dh_train* t = net->train;
  if (!t) return DH_OK;
  DH_HIP(hipDeviceSynchronize());
  // masters and running statistics back into the host parameter table, then re-finalise for eval
  for (const auto& kv : t->slot) {
    auto& v = net->params[kv.first];
    v.resize(kv.second.second);
    DH_HIP(hipMemcpy(v.data(), t->Pm + kv.second.first, kv.second.second * 4, hipMemcpyDeviceToHost));
  }
  for (const auto& kv : t->rslot) {
    auto& v = net->params[kv.first];
    v.resize(kv.second.second);
    DH_HIP(hipMemcpy(v.data(), t->R + kv.second.first, kv.second.second * 4, hipMemcpyDeviceToHost));
  }
  store_free_all(*t);
  delete t;
  net->train = nullptr;
  return dh_resnet18_finalize(net, nullptr);
}

extern "C" int dh_resnet18_forward_train(dh_resnet18* net, const float* x, int64_t n, int32_t P, float* logits, void* stream) {
  DH_REQUIRE(net && x && logits, "forward_train: null argument");
  int rc = dh_resnet18_train_begin(net, n, P, stream);
  if (rc) return rc;
  dh_train* t = net->train;
  hipStream_t st = dh::as_stream(stream);
  const int B = (int)n;
  const UnitAffine u{t->ones, t->zeros};
  t->x_in = x; t->bwd_done = false;
  // stem: raw conv (unit scale, zero shift, no ReLU) -> batch-stat BN + ReLU -> maxpool
  {
    TrainConv& tc = t->convs[0];
    StemParams sp;
    sp.x_nchw = x; sp.slide = nullptr; sp.yx = nullptr; sp.row_bytes = 0;
    sp.w = tc.wp_f; sp.scale = t->ones; sp.shift = t->zeros; sp.out = tc.Z;
    sp.B = B; sp.P = P; sp.Ho = tc.Ho; sp.Wo = tc.Wo; sp.relu = 0;
    sp.tiles_y = (tc.Ho + STEM_TH - 1) / STEM_TH; sp.tiles_x = (tc.Wo + STEM_TW - 1) / STEM_TW;
    const size_t lds = (size_t)7 * 11 * 2 * 256 + (size_t)STEM_ROWS * STEM_ROWE * 4;
    if (int arc = ensure_dyn_lds(reinterpret_cast<const void*>(&stem_kernel<float, false>), 96 * 1024)) return arc;
    hipLaunchKernelGGL((stem_kernel<float, false>), dim3(B * sp.tiles_y * sp.tiles_x), dim3(256), lds, st, sp);
    DH_LAUNCH_CHECK();
    if ((rc = tr_bn_forward(tr_bn_view(t, tc), nullptr, true, nullptr, st, t->X1, t->pool_idx))) return rc;   // + ReLU + maxpool in the same pass
  }
  const float* X = t->X1;
  for (const BlockDesc& b : t->blocks) {
    TrainConv &c1 = t->convs[b.conv[0]], &c2 = t->convs[b.conv[1]];
    if ((rc = tr_conv(u, c1.cin, c1.cout, 3, c1.stride, c1.wp_f, X, nullptr, c1.Z, B, c1.Hi, c1.Wi, st))) return rc;
    if ((rc = tr_bn_forward(tr_bn_view(t, c1), nullptr, true, c1.Y, st))) return rc;
    const float* idt = X;
    if (b.ds >= 0) {
      TrainConv& cd = t->convs[b.ds];
      if ((rc = tr_conv(u, cd.cin, cd.cout, 1, 2, t->Pm + t->slot[cd.name + ".weight"].first, X, nullptr, cd.Z, B, cd.Hi, cd.Wi, st))) return rc;
      if ((rc = tr_bn_forward(tr_bn_view(t, cd), nullptr, false, cd.Y, st))) return rc;
      idt = cd.Y;
    }
    if ((rc = tr_conv(u, c2.cin, c2.cout, 3, 1, c2.wp_f, c1.Y, nullptr, c2.Z, B, c2.Hi, c2.Wi, st))) return rc;
    if ((rc = tr_bn_forward(tr_bn_view(t, c2), idt, true, c2.Y, st))) return rc;
    X = c2.Y;
  }
  const TrainConv& l4 = t->convs[t->blocks.back().conv[1]];
  const int HW = l4.Ho * l4.Wo;
  hipLaunchKernelGGL(avgpool_kernel, dim3(B), dim3(256), 0, st, X, HW, 512, t->pooled);
  const float* fw = t->Pm + t->slot["fc.weight"].first;
  const float* fb = t->Pm + t->slot["fc.bias"].first;
  hipLaunchKernelGGL(fc_fwd_kernel, dim3((B * net->n_classes + 3) / 4), dim3(256), 0, st, t->pooled, fw, fb, B, 512,
                     net->n_classes, logits);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

namespace {
// The block body of the float32 pass; which stream a weight gradient runs on, the hand-offs, the joins and the fused optimiser (`fused`,
// single-rank training) are BwdSched's (train_core.inc): one hand-off per residual block, joined where a gradient bucket may complete.
int tr_backward(dh_resnet18* net, const float* dlogits, hipStream_t st, const AdamArgs* fused) {
  dh_train* t = net->train;
  const int B = t->B, ncls = net->n_classes;
  const UnitAffine u{t->ones, t->zeros};
  int rc;
  store_begin_backward(*t);
  const bool side = t->side != nullptr;
  auto sched = bwd_sched<float>(*t, st, fused, (int)t->convs.size(),
      [&](int i, const float* x, const float* dz, hipStream_t q) {
        const TrainConv& c = t->convs[i];
        return tr_wgrad(t->wgrad_slabs, t->G + t->slot[c.name + ".weight"].first, c, x, dz, B, q);
      },
      [&](int lo, int hi, hipStream_t q) {   // conv 0 (the stem) has its own pack kernel
        if (lo == 0) { if (int r = tr_pack_stem(t, q)) return r; lo = 1; }
        return tr_pack(t, q, lo, hi + 1);
      },
      (DH_T1_ABL & 8) != 0);
  // fc + avgpool
  const TrainConv& l4 = t->convs[t->blocks.back().conv[1]];
  const int HW4 = l4.Ho * l4.Wo;
  hipLaunchKernelGGL(fc_wgrad_kernel, dim3((ncls * 512 + 255) / 256), dim3(256), 0, st, dlogits, t->pooled, B, 512, ncls,
                     t->G + t->slot["fc.weight"].first, t->G + t->slot["fc.bias"].first);
  float* dOut = t->SM[0];
  hipLaunchKernelGGL(avgpool_fc_dgrad_kernel, dim3(B), dim3(256), 0, st, dlogits, t->Pm + t->slot["fc.weight"].first, HW4, 512, ncls, dOut);
  DH_LAUNCH_CHECK();
  store_mark_done(*t);   // fc
  // residual blocks in reverse
  for (int b = (int)t->blocks.size() - 1; b >= 0; --b) {
    const int i1 = t->blocks[b].conv[0], i2 = t->blocks[b].conv[1], id = t->blocks[b].ds;
    TrainConv &c1 = t->convs[i1], &c2 = t->convs[i2];
    const float* Xin = b == 0 ? t->X1 : t->convs[t->blocks[b - 1].conv[1]].Y;
    float* G2 = t->SM[1];   // masked gradient at the block output (flows to both branches)
    float* dZ2 = side ? c2.dZ : t->SM[2];
    const int64_t n2 = (int64_t)B * c2.Ho * c2.Wo * c2.cout;
    tr_dump("dOut", b, dOut, n2, st);
    if ((rc = tr_bn_backward(tr_bn_view(t, c2), dOut, c2.Y, true, dZ2, G2, st))) return rc;   // dOut is dead after this
    tr_dump("dZ2", b, dZ2, n2, st);
    if ((rc = sched.queue(i2, c1.Y, dZ2))) return rc;
    float* dY1 = t->SM[3];
    if ((rc = tr_conv(u, c2.cout, c2.cin, 3, 1, c2.wp_d, dZ2, nullptr, dY1, B, c2.Ho, c2.Wo, st))) return rc;
    tr_dump("dY1", b, dY1, n2, st);
    float* dZ1 = side ? c1.dZ : t->SM[2];  // (single stream: dZ2 is dead now)
    if ((rc = tr_bn_backward(tr_bn_view(t, c1), dY1, nullptr, true, dZ1, nullptr, st))) return rc;   // ReLU pattern from Z
    tr_dump("dZ1", b, dZ1, n2, st);
    if ((rc = sched.queue(i1, Xin, dZ1))) return rc;
    float* dX = t->SM[0];
    if (id < 0) {
      // dX = dgrad(conv1) + G2 (identity branch), fused as the conv's residual input
      if ((rc = tr_conv(u, c1.cout, c1.cin, 3, 1, c1.wp_d, dZ1, G2, dX, B, c1.Ho, c1.Wo, st))) return rc;
    } else {
      TrainConv& cd = t->convs[id];
      // stride-2 data gradient: four parity-class launches over dZ1 itself (round 2 ran a stride-1 conv over a zero-upsampled
      // copy: four times the MFMA work and a 4x-sized tensor written and read)
      if ((rc = tr_dgrad_s2(u, c1.cout, c1.cin, c1.wp_d, dZ1, nullptr, dX, B, c1.Ho, c1.Wo, c1.Hi, c1.Wi, st))) return rc;
      // downsample branch: BN (no ReLU) <- G2 ; 1x1 stride-2 conv
      float* dZd = side ? cd.dZ : t->SM[3];  // (single stream: dY1 is dead)
      if ((rc = tr_bn_backward(tr_bn_view(t, cd), G2, nullptr, false, dZd, nullptr, st))) return rc;
      if ((rc = sched.queue(id, Xin, dZd))) return rc;
      float* tt = side ? t->SM[3] : t->SM[2];   // dY1 (dZ1 on a single stream) is dead: [B, Ho, Wo, cin]
      if ((rc = tr_conv(u, cd.cout, cd.cin, 1, 1, cd.wp_d, dZd, nullptr, tt, B, cd.Ho, cd.Wo, st))) return rc;
      const int64_t m4 = (int64_t)B * cd.Ho * cd.Wo * cd.cin / 4;
      hipLaunchKernelGGL(upsample2_add_kernel, dim3(grid_for(m4)), dim3(256), 0, st, tt, dX, B, cd.Ho, cd.Wo, cd.cin);
      DH_LAUNCH_CHECK();
    }
    dOut = dX;
    // the queued gradients complete this block's item.  Armed buckets: one may complete here, its gradients precede the caller's event
    if ((rc = t->bucket_cb ? sched.join(1) : sched.flush(1))) return rc;
    store_mark_done(*t);   // the block
  }
  // stem: maxpool, BN+ReLU, wgrad
  {
    TrainConv& c = t->convs[0];
    float* dZ0 = t->BIG1;
    if ((rc = tr_bn_pool_backward(tr_bn_view(t, c), dOut, t->pool_idx, dZ0, st))) return rc;   // maxpool + ReLU + BN backward, dY never materialised
    if ((rc = tr_stem_wgrad(dZ0, t->x_in, t->stem_slabs, t->G + t->slot["conv1.weight"].first, B, t->P, c.Ho, c.Wo, st))) return rc;
    if ((rc = sched.join(0))) return rc;   // the optimiser (and the last bucket) follow on the main stream
    store_mark_done(*t);   // the stem
    if ((rc = sched.tail())) return rc;
  }
  t->bwd_done = true;
  return DH_OK;
}
}  // namespace

extern "C" int dh_resnet18_backward(dh_resnet18* net, const float* dlogits, void* stream) {
  DH_REQUIRE(net && net->train && dlogits, "backward: no training forward has run");
  return tr_backward(net, dlogits, dh::as_stream(stream), nullptr);
}

// Backward pass and Adam step of a single-rank training step in one call (see dh_train2_backward_adam): bit-identical to
// dh_resnet18_backward followed by dh_resnet18_adam_step.
extern "C" int dh_resnet18_backward_adam(dh_resnet18* net, const float* dlogits, float lr, float beta1, float beta2, float eps, int64_t step,
                                         void* stream) {
  DH_REQUIRE(net && net->train && dlogits, "backward: no training forward has run");
  DH_REQUIRE(net->train->bucket_cb == nullptr, "backward_adam: gradient buckets are armed (data-parallel steps call backward and adam_step)");
  const AdamArgs a = adam_args(*net->train, lr, beta1, beta2, eps, step);
  return tr_backward(net, dlogits, dh::as_stream(stream), &a);
}

// Gradient buckets of the float32 engine (store_set_buckets has the contract): the arena is in forward order and the backward pass
// completes it from the END, so bucket k is a suffix slice.  Needs a training state (call after a training forward).
extern "C" int dh_resnet18_set_buckets(dh_resnet18* net, int64_t bucket_bytes, void (*cb)(int32_t, int64_t, int64_t, void*), void* user,
                                       int32_t* n_buckets_out) {
  DH_REQUIRE(net && net->train && bucket_bytes >= 0, "set buckets: no training state / bad arguments");
  store_set_buckets(*net->train, bucket_bytes, cb, user, n_buckets_out);
  return DH_OK;
}
extern "C" int dh_resnet18_bucket(dh_resnet18* net, int32_t i, int64_t* offset, int64_t* count) {
  DH_REQUIRE(net && net->train, "bucket: index out of range");
  return store_bucket(*net->train, "bucket", i, offset, count);
}

extern "C" int dh_ce_loss(const float* logits, const int64_t* labels, int64_t n, int32_t n_cls, float* loss_dev,
                          float* dlogits_dev, void* stream) {
  DH_REQUIRE(logits && labels && loss_dev && n > 0 && n_cls > 0, "ce loss: bad arguments");
  hipLaunchKernelGGL(ce_loss_kernel, dim3(1), dim3(256), 0, dh::as_stream(stream), logits, labels, (int)n, n_cls, loss_dev, dlogits_dev);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_resnet18_adam_step(dh_resnet18* net, float lr, float beta1, float beta2, float eps, int64_t step, void* stream) {
  DH_REQUIRE(net && net->train, "adam step: no training state");
  dh_train* t = net->train;
  hipStream_t st = dh::as_stream(stream);
  adam_range(*t, adam_args(*t, lr, beta1, beta2, eps, step), 0, t->n_params, st);
  DH_LAUNCH_CHECK();
  return tr_pack_all(net->train, st);
}

// store_tensor on the training state; the caller re-packs after pushing parameters (dh_resnet18_train_repack)
extern "C" int dh_resnet18_train_tensor(dh_resnet18* net, const char* name, int32_t kind, void* ptr, int64_t n_elem,
                                        int32_t to_lib, void* stream) {
  DH_REQUIRE(net && net->train && name && ptr, "train tensor: no training state / null argument");
  return store_tensor(*net->train, "train tensor", name, kind, ptr, n_elem, to_lib, dh::as_stream(stream));
}

extern "C" int dh_resnet18_train_repack(dh_resnet18* net, void* stream) {
  DH_REQUIRE(net && net->train, "train repack: no training state");
  return tr_pack_all(net->train, dh::as_stream(stream));
}

extern "C" int dh_resnet18_train_flat(dh_resnet18* net, int32_t kind, void** ptr_out, int64_t* n_out) {
  DH_REQUIRE(net && net->train && ptr_out && n_out && kind >= 0 && kind <= 2, "train flat: bad arguments / no training state");
  store_flat(*net->train, kind, ptr_out, n_out);
  return DH_OK;
}
