// train.inc -- training step of the ResNet-18 patch classifier (SURVEY row a7), float32.
// Included at the end of resnet_kernels.hip (same translation unit: reuses the conv kernels), behind train_core.inc (the parameter
// store, buckets, Adam launch and side-stream hand-off shared with the bf16 engine).  The file ends with its last product entry
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
namespace {

constexpr float BN_EPS = 1e-5f, BN_MOMENTUM = 0.1f;

// ---------------- small elementwise / utility kernels (fill_kernel, adam_kernel, grid_for: train_core.inc) ----------------
// pack [cout][cin][ks][ks] f32 master weights into MFMA fragment order (see pack_conv_weights);
// FLIPT: pack the dgrad operator instead: Wd[co'=ci][ci'=co][kh][kw] = W[co][ci][ks-1-kh][ks-1-kw].
template <typename T, bool FLIPT>
__device__ __forceinline__ float pack_conv_elem(const float* __restrict__ w, int cout, int cin, int ks, int64_t o) {   // value of packed element o
  constexpr int ESZ = (int)sizeof(T);
  const int cpc = CHUNK_BYTES / ESZ, epl = 16 / ESZ, taps = ks * ks;
  const int pc_in = FLIPT ? cout : cin;  // packed operator's cin
  const int nch = pc_in / cpc;
  int64_t r = o;
  const int e = (int)(r % epl); r /= epl;
  const int l = (int)(r % 64); r /= 64;
  const int mt = (int)(r % 2); r /= 2;
  const int k2 = (int)(r % 2); r /= 2;
  const int tap = (int)(r % taps); r /= taps;
  const int ch = (int)(r % nch); r /= nch;
  const int cb = (int)r;
  const int co = cb * 64 + mt * 32 + (l & 31);
  const int ci = ch * cpc + k2 * (cpc / 2) + (l >> 5) * epl + e;
  if (FLIPT) return w[((int64_t)ci * cin + co) * taps + (taps - 1 - tap)];   // W[co_src=ci][ci_src=co][flipped]
  return w[((int64_t)co * cin + ci) * taps + tap];
}
template <typename T, bool FLIPT>
__global__ void pack_conv_dev_kernel(const float* __restrict__ w, int cout, int cin, int ks, T* __restrict__ out) {
  const int64_t total = (int64_t)cout * cin * ks * ks;
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
    const float v = pack_conv_elem<T, FLIPT>(w, cout, cin, ks, o);
    if constexpr (sizeof(T) == 4) out[o] = v;
    else reinterpret_cast<uint16_t*>(out)[o] = (uint16_t)f32_to_bf16(v);
  }
}

// Every convolution of the network in ONE launch (after every optimiser step; round 2 launched two kernels per conv: 44 launches
// of ~5.5 us for ResNet-18): a descriptor per conv names the master weights, both packed operators and its first workgroup.
struct PackDescF { const float* w; float* wf; float* wd; int cout, cin, ks, blk0; };
constexpr int PACKF_PER_BLOCK = 256 * 16;   // packed elements per workgroup (1x1 transposes)
// 3x3: one workgroup per SUB-TILE of 16 couts x 64 cins x 9 taps (round 5).  The element-wise form computed eight 64-bit divisions per packed
// element and read the master tensor in 4-byte pieces 36 bytes apart, twice (61 us per launch, 486 us per ResNet-18 step on the side stream).
// Here the sub-tile's 16 rows of 576 contiguous floats are read once as float4 and scattered into LDS as T[tap][co][ci] (pitch 68 floats:
// 16-byte aligned rows, conflict-free columns); both operators are then written as whole 16-byte pieces in runs of 16 / 32 consecutive lanes:
//   forward  piece (co, tap, 4 consecutive ci)            = T[tap][co][ci .. ci+3]
//   dgrad    piece (co' = ci, tap', 4 consecutive ci' = co) = T[8 - tap'][co .. co+3][ci]      (Wd[ci][co][tap'] = W[co][ci][8 - tap'])
// at the addresses of pack_conv_elem<float, false / true> (tests/test_gpu_train_kernels.py::test_pack_f32_tiles_match_the_elementwise_form).
constexpr int PACKF_T_PITCH = 68, PACKF_SUB_CO = 16;
constexpr int PACKF_LDS = 9 * PACKF_SUB_CO * PACKF_T_PITCH * 4;
inline int packf_blocks(int cout, int cin, int ks) {
  return ks == 3 ? (cout / PACKF_SUB_CO) * (cin / 64) : (int)(((int64_t)cout * cin * ks * ks + PACKF_PER_BLOCK - 1) / PACKF_PER_BLOCK);
}
__device__ __forceinline__ void pack3_f32_subtile(const PackDescF& d, int sub, float* T) {
  const int tid = threadIdx.x;
  const int cit = d.cin >> 6;
  const int cs = sub / cit, cik = sub % cit;          // 16-cout strip, 64-cin block
  const int co0 = cs * PACKF_SUB_CO, ci0 = cik * 64;
  for (int i = tid; i < PACKF_SUB_CO * 144; i += 256) {   // float4 pieces: row i / 144, floats (i % 144) * 4 .. of its 576
    const int r = i / 144, j0 = (i % 144) * 4;
    const float4 v = *reinterpret_cast<const float4*>(d.w + ((int64_t)(co0 + r) * d.cin + ci0) * 9 + j0);
    const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = j0 + k, ci_l = j / 9, tap = j - ci_l * 9;
      T[(tap * PACKF_SUB_CO + r) * PACKF_T_PITCH + ci_l] = f[k];
    }
  }
  __syncthreads();
  // packed element index: (((((cb * nch + ch) * 9 + tap) * 2 + k2) * 2 + mt) * 64 + l) * 4 + e, co = cb*64 + mt*32 + (l & 31), ci = ch*16 + k2*8 + (l >> 5)*4 + e
  const int nch_f = d.cin >> 4, nch_d = d.cout >> 4;
  for (int pc = tid; pc < 2 * 2304; pc += 256) {
    if (pc < 2304) {   // forward operator: 16 rows x 16 four-channel groups x 9 taps
      int q = pc;
      const int r = q & 15; q >>= 4;
      const int half = q & 1; q >>= 1;
      const int k2 = q & 1; q >>= 1;
      const int tap = q % 9, chl = q / 9;               // chl: which 16-channel chunk of the block's 64
      const int ci_l = chl * 16 + k2 * 8 + half * 4;
      const float4 v = *reinterpret_cast<const float4*>(T + (tap * PACKF_SUB_CO + r) * PACKF_T_PITCH + ci_l);
      const int co = co0 + r, cb = co >> 6, mt = (co >> 5) & 1, l = (half << 5) | (co & 31), ch = cik * 4 + chl;
      *reinterpret_cast<float4*>(d.wf + ((((((int64_t)cb * nch_f + ch) * 9 + tap) * 2 + k2) * 2 + mt) * 64 + l) * 4) = v;
    } else {           // dgrad operator: 64 rows (= source cins) x 4 four-cout groups x 9 taps
      int q = pc - 2304;
      const int ci_l = q & 63; q >>= 6;
      const int half = q & 1; q >>= 1;
      const int k2 = q & 1; q >>= 1;
      const int tap = q;                                 // 0..8, the packed operator's tap
      const int g = (k2 * 2 + half) * 4;                 // first of the 4 source couts of this piece inside the strip
      const float* src = T + ((8 - tap) * PACKF_SUB_CO + g) * PACKF_T_PITCH + ci_l;
      const float4 v = make_float4(src[0], src[PACKF_T_PITCH], src[2 * PACKF_T_PITCH], src[3 * PACKF_T_PITCH]);
      const int cop = ci0 + ci_l, cb = cop >> 6, mt = (cop >> 5) & 1, l = (half << 5) | (cop & 31), ch = cs;   // ch: the strip IS one 16-channel chunk
      *reinterpret_cast<float4*>(d.wd + ((((((int64_t)cb * nch_d + ch) * 9 + tap) * 2 + k2) * 2 + mt) * 64 + l) * 4) = v;
    }
  }
}
// `desc` .. `desc + nd`: the convolutions this launch packs, `blk_base` = blk0 of the first (a launch over a sub-range of the table)
__global__ __launch_bounds__(256) void pack_all_f32_kernel(const PackDescF* __restrict__ desc, int nd, int blk_base) {
  extern __shared__ __attribute__((aligned(16))) float packf_lds[];
  const int bid = (int)blockIdx.x + blk_base;
  int i = 0;
  while (i + 1 < nd && bid >= desc[i + 1].blk0) ++i;   // workgroup-uniform scan of ~20 descriptors
  const PackDescF d = desc[i];
  if (d.ks == 3) { pack3_f32_subtile(d, bid - d.blk0, packf_lds); return; }
  const int64_t total = (int64_t)d.cout * d.cin * d.ks * d.ks;
  const int64_t o0 = (int64_t)(bid - d.blk0) * PACKF_PER_BLOCK;
  if (d.ks == 1) {   // 1x1 (downsample branches): the GEMM (gemm1x1_f32.inc) reads the master tensor itself forward; its data gradient the transpose
    for (int64_t o = o0 + threadIdx.x; o < o0 + PACKF_PER_BLOCK && o < total; o += 256) {
      const int ci = (int)(o / d.cout), co = (int)(o % d.cout);
      d.wd[o] = d.w[(int64_t)co * d.cin + ci];   // Wt[cin][cout]
    }
    return;
  }
  for (int64_t o = o0 + threadIdx.x; o < o0 + PACKF_PER_BLOCK && o < total; o += 256) {   // any other kernel size: element by element
    d.wf[o] = pack_conv_elem<float, false>(d.w, d.cout, d.cin, d.ks, o);
    d.wd[o] = pack_conv_elem<float, true>(d.w, d.cout, d.cin, d.ks, o);
  }
}

// stem weights [64][3][7][7] -> f32 stem layout [kh][s][mt][lane] (see pack_stem_weights)
__global__ void pack_stem_dev_kernel(const float* __restrict__ w, float* __restrict__ out) {
  const int total = 7 * 11 * 2 * 64;
  for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < total; o += gridDim.x * blockDim.x) {
    int r = o;
    const int l = r % 64; r /= 64;
    const int mt = r % 2; r /= 2;
    const int s = r % 11; r /= 11;
    const int kh = r;
    const int i = 2 * s + (l >> 5), co = mt * 32 + (l & 31);
    float v = 0.f;
    if (i >= 1 && i <= 21) { const int kw = (i - 1) / 3, c = (i - 1) % 3; v = w[((co * 3 + c) * 7 + kh) * 7 + kw]; }
    out[o] = v;
  }
}

// ---------------- per-channel reductions over NHWC rows ----------------
// MODE 0: sum z      MODE 1: sum (z-mean)^2      MODE 2: {sum g, sum g*xhat}, g = dy*(y>0 if relu)      MODE 3: {sum z, sum z^2}
// relu (MODE 2): 0 none, 1 pattern from y, 2 pattern recomputed from z -- y = relu(fma(z, scale, shift)) without an identity term, so
// y > 0 <=> the same fma > 0 (bit-identical to what bn_apply_kernel stored) and y need not be read (a third of the kernel's traffic)
template <int MODE>
__global__ __launch_bounds__(256) void col_reduce_kernel(const float* __restrict__ z, const float* __restrict__ dy,
                                                         const float* __restrict__ y, const float* __restrict__ mean,
                                                         const float* __restrict__ invstd, int64_t rows, int C,
                                                         int relu, float* __restrict__ partial,
                                                         const float* __restrict__ scale = nullptr, const float* __restrict__ shift = nullptr) {
  __shared__ float4 red[2][256];
  const int c4n = C >> 2;                 // float4 lanes per row (16..128)
  const int rpi = 256 / c4n;              // rows per iteration of this workgroup
  const int cl = threadIdx.x % c4n, rl = threadIdx.x / c4n;
  float4 a = make_float4(0, 0, 0, 0), b = make_float4(0, 0, 0, 0);
  float4 mu = make_float4(0, 0, 0, 0), is = make_float4(0, 0, 0, 0);
  if (MODE == 1 || MODE == 2) mu = reinterpret_cast<const float4*>(mean)[cl];
  if (MODE == 2) is = reinterpret_cast<const float4*>(invstd)[cl];
  float4 sc = make_float4(0, 0, 0, 0), sh = make_float4(0, 0, 0, 0);
  if (MODE == 2 && relu == 2) { sc = reinterpret_cast<const float4*>(scale)[cl]; sh = reinterpret_cast<const float4*>(shift)[cl]; }
  for (int64_t r = (int64_t)blockIdx.x * rpi + rl; r < rows; r += (int64_t)gridDim.x * rpi) {
    const float4 v = reinterpret_cast<const float4*>(z + r * C)[cl];
    if (MODE == 0 || MODE == 3) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
    if (MODE == 3) {
      b.x = __builtin_fmaf(v.x, v.x, b.x); b.y = __builtin_fmaf(v.y, v.y, b.y);
      b.z = __builtin_fmaf(v.z, v.z, b.z); b.w = __builtin_fmaf(v.w, v.w, b.w);
    }
    if (MODE == 1) {
      const float dx = v.x - mu.x, dyy = v.y - mu.y, dz = v.z - mu.z, dw = v.w - mu.w;
      a.x += dx * dx; a.y += dyy * dyy; a.z += dz * dz; a.w += dw * dw;
    }
    if (MODE == 2) {
      float4 g = reinterpret_cast<const float4*>(dy + r * C)[cl];
      if (relu == 1) {
        const float4 yy = reinterpret_cast<const float4*>(y + r * C)[cl];
        g.x = yy.x > 0.f ? g.x : 0.f; g.y = yy.y > 0.f ? g.y : 0.f;
        g.z = yy.z > 0.f ? g.z : 0.f; g.w = yy.w > 0.f ? g.w : 0.f;
      } else if (relu == 2) {
        g.x = __builtin_fmaf(v.x, sc.x, sh.x) > 0.f ? g.x : 0.f; g.y = __builtin_fmaf(v.y, sc.y, sh.y) > 0.f ? g.y : 0.f;
        g.z = __builtin_fmaf(v.z, sc.z, sh.z) > 0.f ? g.z : 0.f; g.w = __builtin_fmaf(v.w, sc.w, sh.w) > 0.f ? g.w : 0.f;
      }
      a.x += g.x; a.y += g.y; a.z += g.z; a.w += g.w;
      b.x += g.x * ((v.x - mu.x) * is.x); b.y += g.y * ((v.y - mu.y) * is.y);
      b.z += g.z * ((v.z - mu.z) * is.z); b.w += g.w * ((v.w - mu.w) * is.w);
    }
  }
  red[0][threadIdx.x] = a; red[1][threadIdx.x] = b;
  __syncthreads();
  if (rl == 0) {
    for (int k = 1; k < rpi; ++k) {
      const float4 t = red[0][k * c4n + cl], u = red[1][k * c4n + cl];
      a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
      b.x += u.x; b.y += u.y; b.z += u.z; b.w += u.w;
    }
    reinterpret_cast<float4*>(partial + (int64_t)blockIdx.x * 2 * C)[cl] = a;
    if (MODE >= 2) reinterpret_cast<float4*>(partial + (int64_t)blockIdx.x * 2 * C + C)[cl] = b;
  }
}

// Column sums of the per-workgroup partials [nb][2C] for the 16 consecutive channels of a workgroup: thread = (row phase
// 0..15, channel 0..15), so a row of the partials is read in 64-byte pieces (an earlier version gave every channel a wave that
// walked the rows with a 2C-float stride: one cache line per 4 useful bytes, 6-9 us per call and 100+ calls per training step);
// the 16 phase sums meet in LDS and are added in a fixed order (bit-reproducible).  Returns true in the 16 threads that hold
// the sums of channel c.
constexpr int FIN_CH = 16;
template <int NS>
__device__ __forceinline__ bool partial_colsum(const float* __restrict__ partial, int nb, int C, double (&s)[NS], int& c) {
  __shared__ double sh[16][NS][FIN_CH];
  const int cl = threadIdx.x & (FIN_CH - 1), ph = threadIdx.x >> 4;
  c = blockIdx.x * FIN_CH + cl;
  double a[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) a[k] = 0.0;
  if (c < C)
    for (int b0 = ph; b0 < nb; b0 += 16 * 8) {   // 8 rows in flight per thread: these kernels are load latency, not bandwidth
      float v[8][NS];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int b = b0 + 16 * u, bb = min(b, nb - 1);   // unconditional loads (a row past the end re-reads the last one, weight 0)
#pragma unroll
        for (int k = 0; k < NS; ++k) v[u][k] = partial[(int64_t)bb * 2 * C + k * C + c] * (b < nb ? 1.f : 0.f);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int k = 0; k < NS; ++k) a[k] += (double)v[u][k];
    }
#pragma unroll
  for (int k = 0; k < NS; ++k) sh[ph][k][cl] = a[k];
  __syncthreads();
  if (ph != 0 || c >= C) return false;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    double t = sh[0][k][cl];
    for (int q = 1; q < 16; ++q) t += sh[q][k][cl];
    s[k] = t;
  }
  return true;
}

// which: 0 -> mean = sum/N ; 1 -> var: invstd, scale/shift (training normalisation), running stats
__global__ __launch_bounds__(256) void bn_stat_finalize_kernel(const float* __restrict__ partial, int nb, int C, double n_rows,
                                        int which, float* mean, float* invstd, const float* gamma, const float* beta,
                                        float* scale, float* shift, float* run_mean, float* run_var) {
  double sv[1];
  int c;
  if (!partial_colsum<1>(partial, nb, C, sv, c)) return;
  const double s = sv[0];
  if (which == 0) { mean[c] = (float)(s / n_rows); return; }
  const double var = s / n_rows;  // biased (normalisation)
  const float is = (float)(1.0 / sqrt(var + (double)BN_EPS));
  invstd[c] = is;
  const float sc = gamma[c] * is;
  scale[c] = sc;
  shift[c] = beta[c] - mean[c] * sc;
  const double unbiased = n_rows > 1.0 ? s / (n_rows - 1.0) : var;
  run_mean[c] = (1.f - BN_MOMENTUM) * run_mean[c] + BN_MOMENTUM * mean[c];
  run_var[c] = (1.f - BN_MOMENTUM) * run_var[c] + BN_MOMENTUM * (float)unbiased;
}

// one-pass form: mean and biased variance from {sum z, sum z^2} (double column sums in a fixed order; var clamped at 0),
// normalisation coefficients, running statistics.  Shared by the float32 engine (round 3: one pass over Z and one finalize
// launch per BN instead of two each) and the bf16 engine.
__global__ __launch_bounds__(256) void bn_stat_finalize_onepass_kernel(const float* __restrict__ partial, int nb, int C, double n_rows,
                                                                       float* mean, float* invstd, const float* gamma, const float* beta,
                                                                       float* scale, float* shift, float* run_mean, float* run_var) {
  double sv[2];
  int c;
  if (!partial_colsum<2>(partial, nb, C, sv, c)) return;
  const double s1 = sv[0], s2 = sv[1];
  const double mu = s1 / n_rows;
  double var = s2 / n_rows - mu * mu;
  if (var < 0.0) var = 0.0;
  const float is = (float)(1.0 / sqrt(var + (double)BN_EPS));
  mean[c] = (float)mu;
  invstd[c] = is;
  const float sc = gamma[c] * is;
  scale[c] = sc;
  shift[c] = beta[c] - (float)mu * sc;
  const double unbiased = n_rows > 1.0 ? var * n_rows / (n_rows - 1.0) : var;
  run_mean[c] = (1.f - BN_MOMENTUM) * run_mean[c] + BN_MOMENTUM * (float)mu;
  run_var[c] = (1.f - BN_MOMENTUM) * run_var[c] + BN_MOMENTUM * (float)unbiased;
}

// BN backward coefficients: dgamma = s2, dbeta = s1, and per channel
//   dz = k0 * g + k1 * z + k2   with  k0 = gamma*invstd,
//   k1 = -k0 * invstd * s2 / N,  k2 = -k0 * s1 / N - k1 * mean     (xhat = (z-mean)*invstd)
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ partial, int nb, int C, double n_rows,
                                       const float* gamma, const float* mean, const float* invstd,
                                       float* dgamma, float* dbeta, float* k0, float* k1, float* k2) {
  double sv[2];
  int c;
  if (!partial_colsum<2>(partial, nb, C, sv, c)) return;
  const double s1 = sv[0], s2 = sv[1];
  dgamma[c] = (float)s2;
  dbeta[c] = (float)s1;
  const double a = (double)gamma[c] * (double)invstd[c];
  const double b1 = -a * (double)invstd[c] * s2 / n_rows;
  k0[c] = (float)a;
  k1[c] = (float)b1;
  k2[c] = (float)(-a * s1 / n_rows - b1 * (double)mean[c]);
}

// y = [relu]( z*scale + shift [+ res] )
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ z, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, const float* __restrict__ res,
                                                       float* __restrict__ y, int64_t n4, int C, int relu) {
  // C/4 divides 256 (C = 64 ... 512): a thread meets the same 4 channels in every grid-stride iteration -> coefficients loaded once
  const int c4n = C >> 2;
  const int cl = (int)(threadIdx.x % c4n);
  const float4 sc = reinterpret_cast<const float4*>(scale)[cl], sh = reinterpret_cast<const float4*>(shift)[cl];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(z)[i];
    float4 o = make_float4(__builtin_fmaf(v.x, sc.x, sh.x), __builtin_fmaf(v.y, sc.y, sh.y),
                           __builtin_fmaf(v.z, sc.z, sh.z), __builtin_fmaf(v.w, sc.w, sh.w));
    if (res) { const float4 r = reinterpret_cast<const float4*>(res)[i]; o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w; }
    if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
    reinterpret_cast<float4*>(y)[i] = o;
  }
}

// g = dy*(y>0 if relu);  dz = k0*g + k1*z + k2;  optionally g_out = g (the residual branch's gradient)
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                           const float* __restrict__ z, const float* __restrict__ k0,
                                                           const float* __restrict__ k1, const float* __restrict__ k2,
                                                           float* __restrict__ dz, float* __restrict__ g_out,
                                                           int64_t n4, int C, int relu,
                                                           const float* __restrict__ scale = nullptr, const float* __restrict__ shift = nullptr) {
  const int c4n = C >> 2;
  const int cl = (int)(threadIdx.x % c4n);   // constant over the grid-stride loop (see bn_apply_kernel)
  const float4 a = reinterpret_cast<const float4*>(k0)[cl], b = reinterpret_cast<const float4*>(k1)[cl],
               c = reinterpret_cast<const float4*>(k2)[cl];
  float4 sc = make_float4(0, 0, 0, 0), sh = make_float4(0, 0, 0, 0);
  if (relu == 2) { sc = reinterpret_cast<const float4*>(scale)[cl]; sh = reinterpret_cast<const float4*>(shift)[cl]; }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 g = reinterpret_cast<const float4*>(dy)[i];
    const float4 v = reinterpret_cast<const float4*>(z)[i];
    if (relu == 1) {
      const float4 yy = reinterpret_cast<const float4*>(y)[i];
      g.x = yy.x > 0.f ? g.x : 0.f; g.y = yy.y > 0.f ? g.y : 0.f; g.z = yy.z > 0.f ? g.z : 0.f; g.w = yy.w > 0.f ? g.w : 0.f;
    } else if (relu == 2) {   // pattern from z (col_reduce_kernel)
      g.x = __builtin_fmaf(v.x, sc.x, sh.x) > 0.f ? g.x : 0.f; g.y = __builtin_fmaf(v.y, sc.y, sh.y) > 0.f ? g.y : 0.f;
      g.z = __builtin_fmaf(v.z, sc.z, sh.z) > 0.f ? g.z : 0.f; g.w = __builtin_fmaf(v.w, sc.w, sh.w) > 0.f ? g.w : 0.f;
    }
    float4 o;
    o.x = __builtin_fmaf(a.x, g.x, __builtin_fmaf(b.x, v.x, c.x)); o.y = __builtin_fmaf(a.y, g.y, __builtin_fmaf(b.y, v.y, c.y));
    o.z = __builtin_fmaf(a.z, g.z, __builtin_fmaf(b.z, v.z, c.z)); o.w = __builtin_fmaf(a.w, g.w, __builtin_fmaf(b.w, v.w, c.w));
    reinterpret_cast<float4*>(dz)[i] = o;
    if (g_out) reinterpret_cast<float4*>(g_out)[i] = g;
  }
}

// dx[b][2i][2j][:] += t[b][i][j][:]   (dgrad of the 1x1 stride-2 downsample, step 2)
__global__ __launch_bounds__(256) void upsample2_add_kernel(const float* __restrict__ t, float* __restrict__ dx,
                                                            int B, int Ho, int Wo, int C) {
  const int c4n = C >> 2;
  const int64_t n4 = (int64_t)B * Ho * Wo * c4n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int cl = (int)(i % c4n);
    int64_t r = i / c4n;
    const int x = (int)(r % Wo); r /= Wo;
    const int y = (int)(r % Ho);
    const int b = (int)(r / Ho);
    float4* d = reinterpret_cast<float4*>(dx + (((int64_t)b * 2 * Ho + 2 * y) * 2 * Wo + 2 * x) * C) + cl;
    const float4 v = reinterpret_cast<const float4*>(t)[i];
    float4 o = *d;
    o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
    *d = o;
  }
}

// ---------------- wgrad: dW[co][ci][tap] = sum_px dZ[px][co] * X[px @ tap][ci] ----------------
// One workgroup = one tap x 64 couts x 64 cins x one slab of output pixels; each wave walks
// pixel PAIRS (the K=2 of v_mfma_f32_32x32x2_f32: lane>>5 picks the pixel, lane&31 the channel,
// so both operands are plain coalesced rows of 32 channels); tiles are combined without atomics (below).
struct WgradParams {
  const float* dz; const float* x; float* slabs;   // [n_slabs][Cout][Cin][taps] partial gradients
  int B, Hi, Wi, Cin, Ho, Wo, Cout, KS, STRIDE, PAD;
  int64_t npx; int pairs_per_slab, n_slabs;
};

// One workgroup = one tap x 64 couts x 64 cins x one slab of output pixels.  Per chunk of 32
// pixels the dZ rows and the tap-shifted X rows (256 B each, zero outside the image) are staged
// in LDS with 16-byte loads; wave w then feeds pixel pairs 8w..8w+7 to the MFMA from LDS
// (lanes 0-31 / 32-63 read two rows of 32 consecutive floats: conflict-free).
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradParams p) {
  __shared__ __attribute__((aligned(16))) float lds[2 * 32 * 64];   // [dZ 32x64 | X 32x64]; reused as the 64x64 tile
  float* dzs = lds;
  float* xs = lds + 32 * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int taps = p.KS * p.KS, cot = p.Cout >> 6, cit = p.Cin >> 6;
  int r = blockIdx.x;
  const int ct = r % cit; r /= cit;
  const int ot = r % cot; r /= cot;
  const int tap = r % taps; r /= taps;
  const int slab = r;
  const int kh = tap / p.KS, kw = tap % p.KS;
  const int k = lane >> 5, cl = lane & 31;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
  const int64_t px0 = (int64_t)slab * p.pairs_per_slab * 2;
  const int64_t px1 = min(px0 + (int64_t)p.pairs_per_slab * 2, p.npx);
  const int srow = tid >> 4, scol = (tid & 15) * 4;  // staging: rows srow and srow+16, 4 floats at scol
  for (int64_t base = px0; base < px1; base += 32) {
    float4 dv[2], xv[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t px = base + srow + 16 * u;
      dv[u] = make_float4(0, 0, 0, 0); xv[u] = make_float4(0, 0, 0, 0);
      if (px < px1) {
        dv[u] = *reinterpret_cast<const float4*>(p.dz + px * p.Cout + ot * 64 + scol);
        const int ox = (int)(px % p.Wo);
        const int64_t t = px / p.Wo;
        const int oy = (int)(t % p.Ho), b = (int)(t / p.Ho);
        const int iy = oy * p.STRIDE + kh - p.PAD, ix = ox * p.STRIDE + kw - p.PAD;
        if (iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi)
          xv[u] = *reinterpret_cast<const float4*>(p.x + (((int64_t)b * p.Hi + iy) * p.Wi + ix) * p.Cin + ct * 64 + scol);
      }
    }
    __syncthreads();  // previous chunk consumed
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      *reinterpret_cast<float4*>(dzs + (srow + 16 * u) * 64 + scol) = dv[u];
      *reinterpret_cast<float4*>(xs + (srow + 16 * u) * 64 + scol) = xv[u];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = wave * 8 + 2 * j + k;
      const float a0 = dzs[row * 64 + cl], a1 = dzs[row * 64 + 32 + cl];
      const float b0 = xs[row * 64 + cl], b1 = xs[row * 64 + 32 + cl];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  // The four waves' 64x64 tiles are summed in LDS in a FIXED order (wave 0 stores, waves 1..3 add in turn: every
  // lane owns its own elements, no atomics) and the sum goes to this slab's buffer with plain stores;
  // wgrad_reduce_kernel adds the slabs in a fixed order -> bit-reproducible gradients.
  // D[co][ci]: lane col = ci (lane&31), rows co = (q&3) + 8*(q>>2) + 4*(lane>>5)
  for (int w = 0; w < 4; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            float* e = &lds[(mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * k) * 64 + nt * 32 + cl];
            *e = w == 0 ? acc[mt][nt][q] : *e + acc[mt][nt][q];
          }
    }
  }
  __syncthreads();
  float* out = p.slabs + (int64_t)slab * p.Cout * p.Cin * taps;
  for (int i = tid; i < 64 * 64; i += 256) {
    const int co = ot * 64 + (i >> 6), ci = ct * 64 + (i & 63);
    out[((int64_t)co * p.Cin + ci) * taps + tap] = lds[i];
  }
}

// ---------------- wgrad of the 3x3 convs: all 9 taps from ONE staging of dZ and X ----------------
// One workgroup = 64 couts x 64 cins x a slab of "steps"; a step = R output rows of one image
// (R*Wo <= 64 pixels).  Per step the dZ rows and the X window with halo (((R-1)*s+3) x ((Wo-1)*s+3) pixels,
// zero outside the image) are staged ONCE in LDS (double-buffered; the next step's global loads fly
// under this step's MFMAs) and feed all 9 taps -- the per-tap kernel above re-read both tensors nine times.
// 8 waves: wave = (pair parity g, cout half mt, cin half nt); it owns the nine 32x32 tap tiles of its
// (mt, nt) quadrant (144 accumulator VGPRs) and walks the pixel PAIRS j = g, g+2, ... of the step
// (K = 2 of v_mfma_f32_32x32x2_f32: lane>>5 picks the pixel, lane&31 the channel -> both operands are
// rows of 32 consecutive floats in LDS, conflict-free).  At the end the two parities are summed through
// LDS and the 64x64x9 tile goes to slabs[slab] with plain stores; wgrad_reduce_kernel adds the slabs in
// a fixed order: no atomics, bit-reproducible gradients.
struct Wgrad3Params {
  const float* dz; const float* x; float* slabs;
  int B, Hi, Wi, Cin, Ho, Wo, Cout, STRIDE;
  int R, XR, XC;            // output rows per step; staged window rows / cols (pixels)
  int rb_per_img;           // row blocks per image = ceil(Ho / R)
  int total_steps, steps_per_slab;
  int buf_floats;           // floats per LDS stage buffer (window + dz rows)
  int dzpix;                // dz rows staged per step (R*Wo rounded up to even)
};
constexpr int WG3_MAXX = 7;  // float4 window items per thread (512 threads): 198 px x 16 / 512
constexpr int WG3_MAXD = 2;  // float4 dz items per thread: 64 px x 16 / 512

__global__ __launch_bounds__(512, 2) void wgrad3_kernel(const Wgrad3Params p) {
  extern __shared__ __attribute__((aligned(16))) float wl[];
  int* pixoff = reinterpret_cast<int*>(wl);          // [64] float offset of pixel p inside the window
  float* bufs = wl + 64;                              // 2 stage buffers: [window XR*XC*64 | dz dzpix*64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = wave >> 2, mt = (wave >> 1) & 1, nt = wave & 1;
  const int k = lane >> 5, cl = lane & 31;
  const int cit = p.Cin >> 6, cot = p.Cout >> 6;
  int r = blockIdx.x;
  const int ct = r % cit; r /= cit;
  const int ot = r % cot; r /= cot;
  const int slab = r;
  const int step0 = slab * p.steps_per_slab, step1 = min(step0 + p.steps_per_slab, p.total_steps);
  const int win_floats = p.XR * p.XC * 64;
  if (tid < 64) {
    const int pp = min(tid, p.R * p.Wo - 1);
    pixoff[tid] = ((pp / p.Wo) * p.STRIDE * p.XC + (pp % p.Wo) * p.STRIDE) * 64;
  }
  // staging descriptors (the window geometry is the same for every step)
  const int nx_items = p.XR * p.XC * 16, nd_items = p.dzpix * 16;
  int x_wr[WG3_MAXX], x_ix[WG3_MAXX], x_c4[WG3_MAXX];
#pragma unroll
  for (int u = 0; u < WG3_MAXX; ++u) {
    const int i = tid + 512 * u;
    const int wr = i / (p.XC * 16), rem = i % (p.XC * 16);
    x_wr[u] = i < nx_items ? wr : -4096; x_ix[u] = rem / 16 - 1; x_c4[u] = rem % 16;
  }
  float4 xv[WG3_MAXX], dv[WG3_MAXD];
  auto load_step = [&](int step) __attribute__((always_inline)) {
    const int b = step / p.rb_per_img, oy0 = (step % p.rb_per_img) * p.R;
    const int npix = min(p.R, p.Ho - oy0) * p.Wo;
#pragma unroll
    for (int u = 0; u < WG3_MAXX; ++u) {
      const int iy = oy0 * p.STRIDE - 1 + x_wr[u], ix = x_ix[u];
      xv[u] = make_float4(0, 0, 0, 0);
      if (iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi)
        xv[u] = *reinterpret_cast<const float4*>(p.x + (((int64_t)b * p.Hi + iy) * p.Wi + ix) * p.Cin + ct * 64 + x_c4[u] * 4);
    }
#pragma unroll
    for (int u = 0; u < WG3_MAXD; ++u) {
      const int i = tid + 512 * u, px = i >> 4;
      dv[u] = make_float4(0, 0, 0, 0);
      if (i < nd_items && px < npix)
        dv[u] = *reinterpret_cast<const float4*>(p.dz + (((int64_t)b * p.Ho + oy0) * p.Wo + px) * p.Cout + ot * 64 + (i & 15) * 4);
    }
  };
  auto store_step = [&](int buf) __attribute__((always_inline)) {
    float* xs = bufs + buf * p.buf_floats;
    float* dzs = xs + win_floats;
#pragma unroll
    for (int u = 0; u < WG3_MAXX; ++u)
      if (tid + 512 * u < nx_items) *reinterpret_cast<float4*>(xs + (tid + 512 * u) * 4) = xv[u];
#pragma unroll
    for (int u = 0; u < WG3_MAXD; ++u)
      if (tid + 512 * u < nd_items) *reinterpret_cast<float4*>(dzs + (tid + 512 * u) * 4) = dv[u];
  };
  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
  int tapoff[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) tapoff[t] = ((t / 3) * p.XC + (t % 3)) * 64;

  if (step0 < step1) { load_step(step0); store_step(0); }
  __syncthreads();
  for (int step = step0; step < step1; ++step) {
    const int buf = (step - step0) & 1;
    const bool more = step + 1 < step1;
    if (more) load_step(step + 1);                       // global loads in flight under the MFMAs below
    const float* xs = bufs + buf * p.buf_floats;
    const float* dzs = xs + win_floats;
    const int oy0 = (step % p.rb_per_img) * p.R;
    const int npairs = (min(p.R, p.Ho - oy0) * p.Wo + 1) >> 1;
    for (int j = g; j < npairs; j += 2) {
      const int px = 2 * j + k;                          // this half-wave's pixel (a phantom odd tail has dz = 0)
      const float a = dzs[px * 64 + mt * 32 + cl];
      const float* xb = xs + pixoff[px] + nt * 32 + cl;
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xb[tapoff[t]], acc[t], 0, 0, 0);
    }
    if (more) store_step(buf ^ 1);                       // the other buffer was released by the last barrier
    __syncthreads();
  }
  // parity 1 hands its tiles over through LDS; parity 0 adds them and stores the slab
  float* xch = wl + (wave & 3) * (9 * 16 * 64);
  if (g == 1) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) xch[(t * 16 + q) * 64 + lane] = acc[t][q];
  }
  __syncthreads();
  if (g == 0) {
    float* out = p.slabs + (int64_t)slab * p.Cout * p.Cin * 9;
    const int ci = ct * 64 + nt * 32 + cl;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int co = ot * 64 + mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * k;   // D row of accumulator register q
      // tap-major slab [tap][co][ci]: a half-wave's 32 cins are one 128-byte store (wgrad_reduce_taps_kernel restores [co][ci][tap])
#pragma unroll
      for (int t = 0; t < 9; ++t) out[((int64_t)t * p.Cout + co) * p.Cin + ci] = acc[t][q] + xch[(t * 16 + q) * 64 + lane];
    }
  }
}

// dW = sum over slabs, float4 groups.  32 float4 elements x 8 slab groups per workgroup (one thread per element walking
// up to 256 slabs was a chain of dependent loads on a 36-workgroup grid); the groups are combined in a fixed order.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slabs, int n_slabs, int64_t nw, float* __restrict__ dw) {
  __shared__ float4 part[8][32];
  const int el = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int64_t i = ((int64_t)blockIdx.x * 32 + el) * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < nw)
    for (int b0 = grp; b0 < n_slabs; b0 += 8 * 8) {   // 8 slabs in flight per thread (load latency, not bandwidth)
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int b = b0 + 8 * u, bb = min(b, n_slabs - 1);
        v[u] = *reinterpret_cast<const float4*>(slabs + (int64_t)bb * nw + i);
        const float m = b < n_slabs ? 1.f : 0.f;
        v[u].x *= m; v[u].y *= m; v[u].z *= m; v[u].w *= m;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
    }
  part[grp][el] = s;
  __syncthreads();
  if (grp == 0 && i < nw) {
    float4 t = part[0][el];
#pragma unroll
    for (int g = 1; g < 8; ++g) { const float4 v = part[g][el]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
    *reinterpret_cast<float4*>(dw + i) = t;
  }
}

// dW[co][ci][tap] = sum over tap-major slabs [slab][tap][co][ci].  blockIdx.y = tap; a thread owns 4 consecutive (co, ci) pairs
// of that tap: one float4 per slab, 8 slabs in flight, the 8 slab groups of a workgroup meet in LDS in a fixed order.  The four
// sums go to torch's layout as 4-byte stores 36 bytes apart (the nine tap planes of a pair are written by nine workgroups; the
// gradient is at most 9.4 MB, the slabs it sums 75 MB).
__global__ __launch_bounds__(256) void wgrad_reduce_taps_kernel(const float* __restrict__ slabs, int n_slabs, int64_t npairs, float* __restrict__ dw) {
  __shared__ float4 part[8][32];
  const int el = threadIdx.x & 31, grp = threadIdx.x >> 5, tap = blockIdx.y;
  const int64_t i = ((int64_t)blockIdx.x * 32 + el) * 4;   // first pair
  const int64_t nw = npairs * 9;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < npairs)
    for (int b0 = grp; b0 < n_slabs; b0 += 8 * 8) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int b = b0 + 8 * u, bb = min(b, n_slabs - 1);
        v[u] = *reinterpret_cast<const float4*>(slabs + (int64_t)bb * nw + tap * npairs + i);
        const float m = b < n_slabs ? 1.f : 0.f;
        v[u].x *= m; v[u].y *= m; v[u].z *= m; v[u].w *= m;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
    }
  part[grp][el] = s;
  __syncthreads();
  if (grp == 0 && i < npairs) {
    float4 a = part[0][el];
#pragma unroll
    for (int g = 1; g < 8; ++g) { const float4 v = part[g][el]; a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
    float* d = dw + i * 9 + tap;
    d[0] = a.x; d[9] = a.y; d[18] = a.z; d[27] = a.w;
  }
}

// stem wgrad: dW[co][e] = sum_px dZ[px][co] * x[b, c, 2oy+kh-3, 2ox+kw-3], e = (c*7+kh)*7+kw (147, padded
// to 160 = 5 MFMA column tiles).  A workgroup takes a range of output rows (b, oy).  Per row the 7 x 3 input row
// segments it touches (with the 3-pixel halo, zeros outside the image) are staged in LDS with coalesced loads; each
// wave then walks the row's pixel pairs: A = dZ rows (staged too), B = per-lane gather of the 32 e-values of a column
// tile FROM LDS (the first version gathered them from global memory: 21 short segments per pixel, 408 us).  Per-workgroup
// 64x160 tiles go to a slab buffer (plain stores) and a second kernel sums the slabs (no atomics on the 37 KB gradient).
// 8 waves = 4 pixel-pair groups x 2 cout halves: a wave holds 5 accumulator tiles (80 registers).  With all ten tiles in one
// wave (4 waves per workgroup) the kernel needed 336 registers -- one wave per SIMD, the row staging and the MFMAs strictly one
// after the other: 305 us per step against 125 us of f32 MFMA time.
constexpr int SWG_T = 512;
template <typename DZT>   // float (f32 engine) or uint16_t = raw bf16 bits (bf16 engine, train2.inc)
__global__ __launch_bounds__(SWG_T, sizeof(DZT) == 4 ? 2 : 4) void stem_wgrad_kernel(const DZT* __restrict__ dz, const float* __restrict__ x,
                                                           float* __restrict__ slabs, int B, int P, int Ho, int Wo,
                                                           int rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) float swl[];
  const int Wx = P + 6;                       // staged row: columns -3 .. P+2
  float* xs = swl;                            // [21 = (c, kh)][Wx]
  float* dzs = swl + 21 * Wx;                 // [Wo][64]: the row's dZ (per-pair global loads were a latency chain)
  float* tile = swl;                          // reused at the end: [64][160]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pg = wave & 3, mt = wave >> 2;    // pixel-pair group, cout half
  const int k = lane >> 5, cl = lane & 31;
  int eoff[5];
  bool elive[5];
#pragma unroll
  for (int nt = 0; nt < 5; ++nt) {
    const int e = nt * 32 + cl;
    const int kw = e % 7, kh = (e / 7) % 7, c = e / 49;
    elive[nt] = e < 147;
    eoff[nt] = elive[nt] ? (c * 7 + kh) * Wx + kw : 0;
  }
  f32x16 acc[5];
#pragma unroll
  for (int j = 0; j < 5; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
  const int total_rows = B * Ho;
  const int row0 = blockIdx.x * rows_per_block, row1 = min(row0 + rows_per_block, total_rows);
  // Software pipeline over the output rows: the global loads of row r + 1 (21 input-row values of this thread's column, its pieces of the
  // dZ row) are issued BEFORE the MFMAs of row r and land in registers while they run; they are written to LDS after the barrier that
  // ends row r.  (Round 2 staged a row, waited, computed, staged the next: load latency and matrix work strictly alternated, and with
  // 135 registers only one workgroup fits a CU, so nothing else filled the gaps: 262 us against 105 us of f32 MFMA time.)
  constexpr int ND = sizeof(DZT) == 4 ? 4 : 2;
  float xv[21];
  uint4 dv0 = make_uint4(0, 0, 0, 0), dv1 = dv0, dv2 = dv0, dv3 = dv0;   // named: as an array hipcc parks them in scratch, and the scratch store waits for the loads
  const int xcol = tid;                        // this thread's column of the staged rows (Wx <= SWG_T: checked on the host)
  const int ndz = Wo * (sizeof(DZT) == 4 ? 16 : 8);   // 16-byte pieces of a dZ row
  // the global loads of row `nr` into xv / dv0..3
#define SWG_LOAD(nr)                                                                                                                   \
  {                                                                                                                                    \
    const int b_ = (nr) / Ho, oy_ = (nr) % Ho;                                                                                         \
    _Pragma("unroll") for (int r = 0; r < 21; ++r) { /* r = c*7 + kh */                                                                \
      const int c = r / 7, kh = r % 7;                                                                                                 \
      const int iy = 2 * oy_ + kh - 3;                                                                                                 \
      xv[r] = 0.f;                                                                                                                     \
      if (xcol < Wx && iy >= 0 && iy < P && xcol >= 3 && xcol < P + 3) xv[r] = x[(((int64_t)b_ * 3 + c) * P + iy) * P + xcol - 3];    \
    }                                                                                                                                  \
    /* the row's dZ: unconditional loads (an index past the row re-reads its last piece, which is then not stored) */                  \
    const uint4* dzr = reinterpret_cast<const uint4*>(dz + (int64_t)(nr) * Wo * 64);                                                   \
    dv0 = dzr[min(tid, ndz - 1)]; dv1 = dzr[min(tid + SWG_T, ndz - 1)];                                                                \
    if constexpr (ND == 4) { dv2 = dzr[min(tid + 2 * SWG_T, ndz - 1)]; dv3 = dzr[min(tid + 3 * SWG_T, ndz - 1)]; }                    \
  }
  // PIPE (float32 dZ: 152 registers, one workgroup per CU): software pipeline, the loads of row r + 1 fly during the MFMAs of row r.
  // bf16 dZ (123 registers): two workgroups per CU cover each other's staging; pipelined it needs 141 registers, loses the second
  // workgroup and the step gets 3 % slower (same-box A/B, profiles/r03_exp_stem.txt).
  constexpr bool PIPE = sizeof(DZT) == 4;
  for (int row = PIPE ? row0 - 1 : row0; row < row1; ++row) {        // PIPE: iteration row0 - 1 only loads
    if (!PIPE) SWG_LOAD(row)
    if (!PIPE || row >= row0) {
      __syncthreads();                          // previous row consumed
      if (xcol < Wx) {
#pragma unroll
        for (int r = 0; r < 21; ++r) xs[r * Wx + xcol] = xv[r];
      }
      auto put = [&](const uint4& d, int u) __attribute__((always_inline)) {
        const int i = tid + SWG_T * u;
        if (i < ndz) {
          if constexpr (sizeof(DZT) == 4) reinterpret_cast<uint4*>(dzs)[i] = d;
          else {   // bf16 rows: 16-byte pieces of 8 channels, widened into the float staging image
            reinterpret_cast<float4*>(dzs)[2 * i] = make_float4(bf16_bits_to_f32(d.x & 0xFFFFu), bf16_bits_to_f32(d.x >> 16),
                                                                bf16_bits_to_f32(d.y & 0xFFFFu), bf16_bits_to_f32(d.y >> 16));
            reinterpret_cast<float4*>(dzs)[2 * i + 1] = make_float4(bf16_bits_to_f32(d.z & 0xFFFFu), bf16_bits_to_f32(d.z >> 16),
                                                                    bf16_bits_to_f32(d.w & 0xFFFFu), bf16_bits_to_f32(d.w >> 16));
          }
        }
      };
      put(dv0, 0); put(dv1, 1);
      if constexpr (ND == 4) { put(dv2, 2); put(dv3, 3); }
      __syncthreads();
    }
    if (PIPE && row + 1 < row1) SWG_LOAD(row + 1)   // in flight during the MFMAs below
    if (!PIPE || row >= row0) {
      for (int pp = pg; 2 * pp < Wo; pp += 4) {
        const int ox = 2 * pp + k;
        float a0 = 0.f, bv[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (ox < Wo) {
          a0 = dzs[ox * 64 + mt * 32 + cl];
#pragma unroll
          for (int nt = 0; nt < 5; ++nt) bv[nt] = elive[nt] ? xs[eoff[nt] + 2 * ox] : 0.f;
        }
#pragma unroll
        for (int nt = 0; nt < 5; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv[nt], acc[nt], 0, 0, 0);
      }
    }
  }
#undef SWG_LOAD
  for (int w = 0; w < 4; ++w) {   // fixed-order combine of the four pixel-pair groups (no float atomics: reproducible)
    __syncthreads();
    if (pg == w) {
#pragma unroll
      for (int nt = 0; nt < 5; ++nt)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          float* e = &tile[(mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * k) * 160 + nt * 32 + cl];
          *e = w == 0 ? acc[nt][q] : *e + acc[nt][q];
        }
    }
  }
  __syncthreads();
  for (int i = tid; i < 64 * 160; i += SWG_T) slabs[(int64_t)blockIdx.x * (64 * 160) + i] = tile[i];
}

// dW[co][c][kh][kw] = sum over slabs of tile[co][e]; 32 elements x 8 slab groups per workgroup (a thread per
// element walking all 512 slabs was a 140 us dependency chain), groups combined in a fixed order
__global__ __launch_bounds__(256) void stem_wgrad_reduce_kernel(const float* __restrict__ slabs, int n_slabs, float* __restrict__ dw) {
  __shared__ float part[8][32];
  const int el = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + el;   // over 64*147
  float s = 0.f;
  if (i < 64 * 147) {
    const int co = i / 147, e = i % 147;
    for (int b = grp; b < n_slabs; b += 8) s += slabs[(int64_t)b * (64 * 160) + co * 160 + e];
  }
  part[grp][el] = s;
  __syncthreads();
  if (grp == 0 && i < 64 * 147) {
    float t = part[0][el];
#pragma unroll
    for (int g = 1; g < 8; ++g) t += part[g][el];
    dw[i] = t;   // [co][c][kh][kw] with e = (c*7+kh)*7+kw is exactly torch's layout
  }
}

// maxpool 3x3/2 pad 1 for training: the forward also records, per output element, WHICH window element
// was the first maximum (row-major scan, torch's tie rule) as a byte 0..8; the backward then lets every
// input pixel ask its (at most 4) windows "was it me?" -- 4 byte + 4 float loads instead of re-scanning
// 4 x 8 neighbours.
__global__ __launch_bounds__(256) void maxpool_fwd_idx_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                              uint8_t* __restrict__ idx, int B, int Hi, int Wi, int C,
                                                              int Ho, int Wo) {
  const int c4n = C >> 2;
  const int64_t n4 = (int64_t)B * Ho * Wo * c4n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int cl = (int)(i % c4n);
    int64_t r = i / c4n;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int dyy = 0; dyy < 3; ++dyy) {
      const int yy = 2 * oy + dyy - 1;
      if (yy < 0 || yy >= Hi) continue;
#pragma unroll
      for (int dxx = 0; dxx < 3; ++dxx) {
        const int xx = 2 * ox + dxx - 1;
        if (xx < 0 || xx >= Wi) continue;
        const float4 v = reinterpret_cast<const float4*>(x + (((int64_t)b * Hi + yy) * Wi + xx) * C)[cl];
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (vv[q] > m[q]) { m[q] = vv[q]; w[q] = dyy * 3 + dxx; }   // strict: the earlier element keeps a tie
      }
    }
    reinterpret_cast<float4*>(y)[i] = make_float4(m[0], m[1], m[2], m[3]);
    reinterpret_cast<uchar4*>(idx)[i] = make_uchar4((uint8_t)w[0], (uint8_t)w[1], (uint8_t)w[2], (uint8_t)w[3]);
  }
}

__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const uint8_t* __restrict__ idx, const float* __restrict__ dy,
                                                          float* __restrict__ dx, int B, int Hi, int Wi, int C,
                                                          int Ho, int Wo) {
  const int c4n = C >> 2;
  const int64_t n4 = (int64_t)B * Hi * Wi * c4n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int cl = (int)(i % c4n);
    int64_t r = i / c4n;
    const int ix = (int)(r % Wi); r /= Wi;
    const int iy = (int)(r % Hi);
    const int b = (int)(r / Hi);
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    for (int oy = iy / 2; oy <= (iy + 1) / 2; ++oy) {
      if (oy >= Ho) continue;
      for (int ox = ix / 2; ox <= (ix + 1) / 2; ++ox) {
        if (ox >= Wo) continue;
        const int me = (iy - (2 * oy - 1)) * 3 + (ix - (2 * ox - 1));   // my position in that window
        const int64_t e = (((int64_t)b * Ho + oy) * Wo + ox) * c4n + cl;
        const uchar4 w = reinterpret_cast<const uchar4*>(idx)[e];
        const float4 g = reinterpret_cast<const float4*>(dy)[e];
        if (w.x == me) o[0] += g.x;
        if (w.y == me) o[1] += g.y;
        if (w.z == me) o[2] += g.z;
        if (w.w == me) o[3] += g.w;
      }
    }
    reinterpret_cast<float4*>(dx)[i] = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// ---- the stem's tail in one pass each way (round 3; see bn2_apply_pool_kernel / bn2_pool_bwd_* of the bf16 engine) ----
// forward: pooled = maxpool3x3/2(relu(fma(z, scale, shift))) + first-maximum positions straight from Z: the same float32 values the pair
// bn_apply_kernel + maxpool_fwd_idx_kernel compares, so maxima and positions are identical; the normalised 112 x 112 map is never stored.
__global__ __launch_bounds__(256) void bn_apply_pool_kernel(const float* __restrict__ z, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, float* __restrict__ y, uint8_t* __restrict__ idx,
                                                            int B, int Hi, int Wi, int C, int Ho, int Wo) {
  const int c4n = C >> 2;
  const int cf = (int)(threadIdx.x % c4n);   // 256 % c4n == 0: the same 4 channels in every grid-stride iteration
  const float4 sc = reinterpret_cast<const float4*>(scale)[cf], sh = reinterpret_cast<const float4*>(shift)[cf];
  const int64_t n4 = (int64_t)B * Ho * Wo * c4n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int cl = (int)(i % c4n);
    int64_t r = i / c4n;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int dyy = 0; dyy < 3; ++dyy) {
      const int yy = 2 * oy + dyy - 1;
      if (yy < 0 || yy >= Hi) continue;
#pragma unroll
      for (int dxx = 0; dxx < 3; ++dxx) {
        const int xx = 2 * ox + dxx - 1;
        if (xx < 0 || xx >= Wi) continue;
        const float4 v = reinterpret_cast<const float4*>(z + (((int64_t)b * Hi + yy) * Wi + xx) * C)[cl];
        const float vv[4] = {fmaxf(__builtin_fmaf(v.x, sc.x, sh.x), 0.f), fmaxf(__builtin_fmaf(v.y, sc.y, sh.y), 0.f),
                             fmaxf(__builtin_fmaf(v.z, sc.z, sh.z), 0.f), fmaxf(__builtin_fmaf(v.w, sc.w, sh.w), 0.f)};
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (vv[q] > m[q]) { m[q] = vv[q]; w[q] = dyy * 3 + dxx; }   // strict: the earlier element keeps a tie
      }
    }
    reinterpret_cast<float4*>(y)[i] = make_float4(m[0], m[1], m[2], m[3]);
    reinterpret_cast<uchar4*>(idx)[i] = make_uchar4((uint8_t)w[0], (uint8_t)w[1], (uint8_t)w[2], (uint8_t)w[3]);
  }
}

// maxpool gradient of the 2 x 2 block of input pixels (2a + py, 2q + px), 4 channels each: its four windows (a + wy, q + wx) are loaded once;
// window (wy, wx) reaches pixel (py, px) at its position (py + 1 - 2 wy, px + 1 - 2 wx) when both are >= 0.  g[2 py + px]; the same sums of
// at most four terms, in the same order, as maxpool_bwd_kernel.
struct PoolGrad4F { float g[4][4]; };
__device__ __forceinline__ PoolGrad4F pool_grad_2x2_f32(const uint8_t* __restrict__ idx, const float* __restrict__ dpool, int b, int a, int q,
                                                        int cl, int c4n, int Ho, int Wo) {
  PoolGrad4F o;
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) o.g[k][e] = 0.f;
#pragma unroll
  for (int wy = 0; wy < 2; ++wy)
#pragma unroll
    for (int wx = 0; wx < 2; ++wx) {
      const int oy = a + wy, ox = q + wx;
      if (oy >= Ho || ox >= Wo) continue;
      const int64_t e4 = (((int64_t)b * Ho + oy) * Wo + ox) * c4n + cl;
      const uchar4 w = reinterpret_cast<const uchar4*>(idx)[e4];
      const float4 g = reinterpret_cast<const float4*>(dpool)[e4];
#pragma unroll
      for (int py = wy; py < 2; ++py)
#pragma unroll
        for (int px = wx; px < 2; ++px) {
          const int me = (py + 1 - 2 * wy) * 3 + (px + 1 - 2 * wx);
          if (w.x == me) o.g[2 * py + px][0] += g.x;
          if (w.y == me) o.g[2 * py + px][1] += g.y;
          if (w.z == me) o.g[2 * py + px][2] += g.z;
          if (w.w == me) o.g[2 * py + px][3] += g.w;
        }
    }
  return o;
}

// col_reduce_kernel<2> (relu == 2) with dy = the maxpool's gradient gathered on the fly; a "row" is a 2 x 2 pixel block of Z
__global__ __launch_bounds__(256) void bn_pool_bwd_reduce_kernel(const float* __restrict__ z, const float* __restrict__ dpool,
                                                                 const uint8_t* __restrict__ idx, const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, int B, int Hi, int Wi, int C, int Ho, int Wo,
                                                                 float* __restrict__ partial) {
  __shared__ float4 red[2][256];
  const int c4n = C >> 2;
  const int rpi = 256 / c4n;
  const int cl = threadIdx.x % c4n, rl = threadIdx.x / c4n;
  const int Hb = (Hi + 1) >> 1, Wb = (Wi + 1) >> 1;
  const int64_t rows = (int64_t)B * Hb * Wb;
  const float4 mu4 = reinterpret_cast<const float4*>(mean)[cl], is4 = reinterpret_cast<const float4*>(invstd)[cl];
  const float4 sc4 = reinterpret_cast<const float4*>(scale)[cl], sh4 = reinterpret_cast<const float4*>(shift)[cl];
  const float mu[4] = {mu4.x, mu4.y, mu4.z, mu4.w}, is[4] = {is4.x, is4.y, is4.z, is4.w};
  const float sc[4] = {sc4.x, sc4.y, sc4.z, sc4.w}, sh[4] = {sh4.x, sh4.y, sh4.z, sh4.w};
  float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t r = (int64_t)blockIdx.x * rpi + rl; r < rows; r += (int64_t)gridDim.x * rpi) {
    const int qx = (int)(r % Wb);
    const int64_t t = r / Wb;
    const int ay = (int)(t % Hb), bb = (int)(t / Hb);
    float4 v4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // pixels past an odd map's edge re-read the block's first pixel with weight 0
      const int iy = 2 * ay + (k >> 1), ix = 2 * qx + (k & 1);
      const bool ok = iy < Hi && ix < Wi;
      v4[k] = reinterpret_cast<const float4*>(z + (((int64_t)bb * Hi + (ok ? iy : 2 * ay)) * Wi + (ok ? ix : 2 * qx)) * C)[cl];
    }
    const PoolGrad4F pg = pool_grad_2x2_f32(idx, dpool, bb, ay, qx, cl, c4n, Ho, Wo);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = 2 * ay + (k >> 1) < Hi && 2 * qx + (k & 1) < Wi;
      const float v[4] = {v4[k].x, v4[k].y, v4[k].z, v4[k].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gg = (ok && __builtin_fmaf(v[e], sc[e], sh[e]) > 0.f) ? pg.g[k][e] : 0.f;
        a[e] += gg;
        b[e] += gg * ((v[e] - mu[e]) * is[e]);
      }
    }
  }
  red[0][threadIdx.x] = make_float4(a[0], a[1], a[2], a[3]); red[1][threadIdx.x] = make_float4(b[0], b[1], b[2], b[3]);
  __syncthreads();
  if (rl == 0) {
    float4 sa = red[0][cl], sb = red[1][cl];
    for (int k = 1; k < rpi; ++k) {
      const float4 t = red[0][k * c4n + cl], u = red[1][k * c4n + cl];
      sa.x += t.x; sa.y += t.y; sa.z += t.z; sa.w += t.w;
      sb.x += u.x; sb.y += u.y; sb.z += u.z; sb.w += u.w;
    }
    reinterpret_cast<float4*>(partial + (int64_t)blockIdx.x * 2 * C)[cl] = sa;
    reinterpret_cast<float4*>(partial + (int64_t)blockIdx.x * 2 * C + C)[cl] = sb;
  }
}

// bn_bwd_apply_kernel (relu == 2) with dy gathered as above: dz = k0*g + k1*z + k2, one 2 x 2 pixel block per thread and iteration
__global__ __launch_bounds__(256) void bn_pool_bwd_apply_kernel(const float* __restrict__ z, const float* __restrict__ dpool,
                                                                const uint8_t* __restrict__ idx, const float* __restrict__ k0,
                                                                const float* __restrict__ k1, const float* __restrict__ k2,
                                                                const float* __restrict__ scale, const float* __restrict__ shift,
                                                                float* __restrict__ dz, int B, int Hi, int Wi, int C, int Ho, int Wo) {
  const int c4n = C >> 2;
  const int cf = (int)(threadIdx.x % c4n);
  const float4 a4 = reinterpret_cast<const float4*>(k0)[cf], b4 = reinterpret_cast<const float4*>(k1)[cf], c4 = reinterpret_cast<const float4*>(k2)[cf];
  const float4 sc4 = reinterpret_cast<const float4*>(scale)[cf], sh4 = reinterpret_cast<const float4*>(shift)[cf];
  const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w}, c[4] = {c4.x, c4.y, c4.z, c4.w};
  const float sc[4] = {sc4.x, sc4.y, sc4.z, sc4.w}, sh[4] = {sh4.x, sh4.y, sh4.z, sh4.w};
  const int Hb = (Hi + 1) >> 1, Wb = (Wi + 1) >> 1;
  const int64_t n4 = (int64_t)B * Hb * Wb * c4n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int cl = (int)(i % c4n);
    int64_t r = i / c4n;
    const int qx = (int)(r % Wb); r /= Wb;
    const int ay = (int)(r % Hb);
    const int bb = (int)(r / Hb);
    float4 v4[4];
    int64_t at[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int iy = 2 * ay + (k >> 1), ix = 2 * qx + (k & 1);
      ok[k] = iy < Hi && ix < Wi;
      at[k] = (((int64_t)bb * Hi + (ok[k] ? iy : 2 * ay)) * Wi + (ok[k] ? ix : 2 * qx)) * C;
      v4[k] = reinterpret_cast<const float4*>(z + at[k])[cl];
    }
    const PoolGrad4F pg = pool_grad_2x2_f32(idx, dpool, bb, ay, qx, cl, c4n, Ho, Wo);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float v[4] = {v4[k].x, v4[k].y, v4[k].z, v4[k].w};
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gg = __builtin_fmaf(v[e], sc[e], sh[e]) > 0.f ? pg.g[k][e] : 0.f;
        o[e] = __builtin_fmaf(a[e], gg, __builtin_fmaf(b[e], v[e], c[e]));
      }
      if (ok[k]) reinterpret_cast<float4*>(dz + at[k])[cl] = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

// global average pool (training forward keeps `pooled`), fc forward
__global__ __launch_bounds__(256) void avgpool_kernel(const float* __restrict__ x, int HW, int C, float* __restrict__ pooled) {
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += 256) {
    float s = 0.f;
    for (int q = 0; q < HW; ++q) s += x[((int64_t)b * HW + q) * C + c];
    pooled[(int64_t)b * C + c] = s / (float)HW;
  }
}
// one wave per logit (a single thread walking the 512 products was a 100 us dependency chain)
__global__ __launch_bounds__(256) void fc_fwd_kernel(const float* __restrict__ pooled, const float* __restrict__ w,
                                                     const float* __restrict__ bias, int B, int C, int n_cls,
                                                     float* __restrict__ logits) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= B * n_cls) return;
  const int b = i / n_cls, k = i % n_cls;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s = __builtin_fmaf(pooled[(int64_t)b * C + c], w[k * C + c], s);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if (lane == 0) logits[i] = s + bias[k];
}
// dW_fc[k][c] = sum_b dl[b][k]*pooled[b][c]; db[k] = sum_b dl[b][k]
__global__ void fc_wgrad_kernel(const float* __restrict__ dl, const float* __restrict__ pooled, int B, int C, int n_cls,
                                float* __restrict__ dw, float* __restrict__ db) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_cls * C) {
    const int k = i / C, c = i % C;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s = __builtin_fmaf(dl[b * n_cls + k], pooled[(int64_t)b * C + c], s);
    dw[i] = s;
  }
  if (i < n_cls) { float s = 0.f; for (int b = 0; b < B; ++b) s += dl[b * n_cls + i]; db[i] = s; }
}
// dX[b][q][c] = (sum_k dl[b][k]*w[k][c]) / HW
__global__ __launch_bounds__(256) void avgpool_fc_dgrad_kernel(const float* __restrict__ dl, const float* __restrict__ w,
                                                               int HW, int C, int n_cls, float* __restrict__ dx) {
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += 256) {
    float s = 0.f;
    for (int k = 0; k < n_cls; ++k) s = __builtin_fmaf(dl[b * n_cls + k], w[k * C + c], s);
    s /= (float)HW;
    for (int q = 0; q < HW; ++q) dx[((int64_t)b * HW + q) * C + c] = s;
  }
}

// CrossEntropyLoss(mean): loss = mean_b( logsumexp(l_b) - l_b[y_b] ); dl = (softmax - onehot)/B
__global__ void ce_loss_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, int B, int n_cls,
                               float* __restrict__ loss, float* __restrict__ dl) {
  __shared__ float red[256];
  float local = 0.f;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const float* l = logits + (int64_t)b * n_cls;
    float m = l[0];
    for (int k = 1; k < n_cls; ++k) m = fmaxf(m, l[k]);
    float s = 0.f;
    for (int k = 0; k < n_cls; ++k) s += expf(l[k] - m);
    const float lse = m + logf(s);
    const int64_t y64 = labels[b];
    const bool y_ok = y64 >= 0 && y64 < n_cls;   // torch raises on such a target; a kernel cannot: the loss turns NaN,
    const int y = y_ok ? (int)y64 : 0;           // the sample's dlogits row is zeroed, nothing outside the row is read
    local += y_ok ? lse - l[y] : __builtin_nanf("");
    if (dl)
      for (int k = 0; k < n_cls; ++k)
        dl[(int64_t)b * n_cls + k] = y_ok ? (expf(l[k] - lse) - (k == y ? 1.f : 0.f)) / (float)B : 0.f;
  }
  red[threadIdx.x] = local;
  __syncthreads();
  for (int o = blockDim.x / 2; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) *loss = red[0] / (float)B;
}

}  // namespace

// =====================================================================================
// host side: training state of a dh_resnet18 handle
// =====================================================================================
struct BnBufs { float *mean, *invstd, *scale, *shift, *k0, *k1, *k2; };
struct TrainConv {
  float* wp_f = nullptr;   // packed forward weights (float)
  float* wp_d = nullptr;   // packed dgrad weights (float), not for the stem
  float* Z = nullptr;      // conv output (pre-BN), NHWC
  float* Y = nullptr;      // BN(+residual)(+ReLU) output, NHWC
  float* dZ = nullptr;     // this conv's own dZ (the side stream's weight-gradient kernels read it long after it was written)
  BnBufs bn{};
  int Ho = 0, Wo = 0, Hi = 0, Wi = 0;
};

struct TrBlock { int c1, c2, ds; int hi, ho; };   // a residual block: conv indices (ds: downsample or -1) and its input / output map size

struct dh_train : TrainStore {   // the arena is in FORWARD order: the backward pass completes it from the end
  int B = 0, P = 0;
  std::vector<TrainConv> tc;
  std::vector<TrBlock> blocks;    // forward order; made once at the first train_begin (sizes: per batch shape)
  float *ones = nullptr, *zeros = nullptr, *partial = nullptr;
  float *X1 = nullptr, *pooled = nullptr;
  float *BIG1 = nullptr, *SM[4] = {nullptr, nullptr, nullptr, nullptr};
  float* stem_slabs = nullptr;
  uint8_t* pool_idx = nullptr;    // first-maximum position (0..8) of every maxpool output element
  float* wgrad_slabs = nullptr;   // [n_slabs][Cout][Cin][9] partial gradients of the 3x3 wgrad
  void* pack_desc = nullptr;      // device table of pack_all_f32_kernel (addresses fixed for the life of the training state)
  int pack_blocks = 0, pack_nd = 0;
  std::vector<int> pack_blk0;     // first workgroup of every descriptor (+ the total), host copy; descriptor j = conv j + 1
  const float* x_in = nullptr;  // input of the last forward (caller memory; must stay alive until backward)
  bool bwd_done = false;        // a backward pass has run since the last forward: every dZ buffer holds THIS step's gradient (debug tap)
  // TrainStore::side: the weight gradients are handed over once per residual block: they fill the CUs the persistent
  // convolution launches leave idle in their last round of tiles.  DH_T1_SIDE=0: everything on the caller's stream.
};

namespace {

constexpr int RED_NB = 512;
constexpr int STEM_WGRAD_SLABS = 512;
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
int tr_pack(dh_resnet18* net, hipStream_t st, int i0, int i1) {
  dh_train* t = net->train;
  if (!t->pack_desc) {
    std::vector<PackDescF> d;
    int blk = 0;
    for (size_t i = 1; i < net->convs.size(); ++i) {
      const ConvLayer& c = net->convs[i];
      t->pack_blk0.push_back(blk);
      d.push_back({t->Pm + t->slot[c.name + ".weight"].first, t->tc[i].wp_f, t->tc[i].wp_d, c.cout, c.cin, c.ks, blk});
      DH_REQUIRE(c.ks != 3 || (c.cout % 64 == 0 && c.cin % 64 == 0), "pack: 3x3 convolution %s with %d -> %d channels (multiples of 64)", c.name.c_str(), c.cin, c.cout);
      blk += packf_blocks(c.cout, c.cin, c.ks);
    }
    DH_HIP(hipMalloc(&t->pack_desc, d.size() * sizeof(PackDescF)));
    t->allocs.push_back(t->pack_desc);
    DH_HIP(hipMemcpy(t->pack_desc, d.data(), d.size() * sizeof(PackDescF), hipMemcpyHostToDevice));
    t->pack_blocks = blk; t->pack_nd = (int)d.size();
    t->pack_blk0.push_back(blk);
  }
  if (i1 <= i0) return DH_OK;
  if (!(DH_T1_ABL & 4)) hipLaunchKernelGGL(pack_all_f32_kernel, dim3(t->pack_blk0[i1 - 1] - t->pack_blk0[i0 - 1]), dim3(256), PACKF_LDS, st,
                     static_cast<const PackDescF*>(t->pack_desc) + (i0 - 1), i1 - i0, t->pack_blk0[i0 - 1]);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
int tr_pack_stem(dh_resnet18* net, hipStream_t st) {
  dh_train* t = net->train;
  hipLaunchKernelGGL(pack_stem_dev_kernel, dim3(40), dim3(256), 0, st, t->Pm + t->slot[net->convs[0].name + ".weight"].first, t->tc[0].wp_f);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
int tr_pack_all(dh_resnet18* net, hipStream_t st) {
  int rc = tr_pack_stem(net, st);
  return rc ? rc : tr_pack(net, st, 1, (int)net->convs.size());
}

// The launch helpers below take what they use (no engine handle), so the test hooks (train_hooks.inc) run the very code of a step.
// `ones` / `zeros`: per-channel unit scale and zero shift (at least `cout` floats) of the inference kernels' epilogue.
struct UnitAffine { const float *ones, *zeros; };

// conv through the inference kernels with unit scale / zero shift (raw conv output).  1x1 (the downsample branches; round 5): the
// float32 GEMM of gemm1x1_f32.inc -- `wp` is then W[cout][cin] K-contiguous: the master tensor (forward) or the transposed copy of the
// data gradient's operator (pack_all_f32_kernel).
int tr_conv(UnitAffine u, int cin, int cout, int ks, int stride, const float* wp, const float* in,
            const float* res, float* out, int B, int Hi, int Wi, hipStream_t st) {
  if (ks == 1) {
    const int Ho = (Hi - 1) / stride + 1, Wo = (Wi - 1) / stride + 1;
    return gemm1x1_f32(in, wp, res, out, (int64_t)B * Ho * Wo, cout, cin, stride, Ho, Wo, Hi, Wi, st);
  }
  ConvLayer L{{"train", "train", cin, cout, ks, stride}};
  L.w_dev = const_cast<float*>(wp);
  L.scale_dev = const_cast<float*>(u.ones);
  L.shift_dev = const_cast<float*>(u.zeros);
  int ho, wo;
  return run_conv<float>(L, in, res, out, B, Hi, Wi, false, st, &ho, &wo);
}

// dX = data gradient of a 3x3 / stride-2 conv (cz channels of dZ -> cx channels of dX) from the packed dgrad operator `wp`
int tr_dgrad_s2(UnitAffine u, int cz, int cx, const float* wp, const float* dz, const float* res, float* dx, int B, int Ho, int Wo,
                int Hi, int Wi, hipStream_t st) {
  ConvLayer L{{"train", "train", cz, cx, 3, 1}};
  L.w_dev = const_cast<float*>(wp);
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
BnView tr_bn_view(dh_resnet18* net, int i) {
  dh_train* t = net->train;
  const ConvLayer& c = net->convs[i];
  const TrainConv& tc = t->tc[i];
  const int64_t w = t->slot[c.bn + ".weight"].first, b = t->slot[c.bn + ".bias"].first;
  return {tc.Z, t->Pm + w, t->Pm + b, t->R + t->rslot[c.bn + ".running_mean"].first, t->R + t->rslot[c.bn + ".running_var"].first,
          t->G + w, t->G + b, tc.bn, (int64_t)t->B * tc.Ho * tc.Wo, c.cout, t->B, tc.Ho, tc.Wo, t->partial};
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
  const int total_rows = B * Ho;
  const int rpb = (total_rows + STEM_WGRAD_SLABS - 1) / STEM_WGRAD_SLABS;
  const int n_slabs = (total_rows + rpb - 1) / rpb;
  const size_t lds = std::max<size_t>((size_t)21 * (P + 6) + (size_t)Wo * 64, (size_t)64 * 160) * sizeof(float);
  DH_REQUIRE(lds <= 64 * 1024 && Wo * 16 <= 4 * SWG_T && P + 6 <= SWG_T, "stem wgrad: patch %d too wide for the row staging", P);
  hipLaunchKernelGGL((stem_wgrad_kernel<float>), dim3(n_slabs), dim3(SWG_T), lds, st, dz, x, slabs, B, P, Ho, Wo, rpb);
  hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3((64 * 147 + 31) / 32), dim3(256), 0, st, slabs, n_slabs, dw);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// dW (`dw_out`) of one conv from its input x and output gradient dz; `wgrad_slabs` holds WGRAD3_WGS * 64*64*9 floats.  `force_pertap`
// routes a 3x3 layer through the per-tap kernel (the path of layers whose rows do not fit the fused kernel; test hook).
int tr_wgrad(float* wgrad_slabs, float* dw_out, const ConvLayer& c, const TrainConv& tc, const float* x, const float* dz, int B,
             hipStream_t st, bool force_pertap = false) {
  WgradParams p;
  p.dz = dz; p.x = x; p.slabs = nullptr;
  p.B = B; p.Hi = tc.Hi; p.Wi = tc.Wi; p.Cin = c.cin; p.Ho = tc.Ho; p.Wo = tc.Wo; p.Cout = c.cout;
  p.KS = c.ks; p.STRIDE = c.stride; p.PAD = c.ks / 2;
  p.npx = (int64_t)B * tc.Ho * tc.Wo;
  // fused 9-tap kernel when one output row's window fits its staging plan (else the per-tap kernel below)
  if (!force_pertap && c.ks == 3 && tc.Wo <= 64 && 3 * ((tc.Wo - 1) * c.stride + 3) * 16 <= WG3_MAXX * 512) {
    Wgrad3Params q;
    q.dz = dz; q.x = x; q.slabs = wgrad_slabs;
    q.B = B; q.Hi = tc.Hi; q.Wi = tc.Wi; q.Cin = c.cin; q.Ho = tc.Ho; q.Wo = tc.Wo; q.Cout = c.cout; q.STRIDE = c.stride;
    const int combos3 = (c.cout / 64) * (c.cin / 64);
    const int XC = (tc.Wo - 1) * c.stride + 3;   // staged window columns (halo included)
    auto xrows = [&](int R) { return (R - 1) * c.stride + 3; };
    auto buf_floats = [&](int R) { return (xrows(R) * XC + ((R * tc.Wo + 1) & ~1)) * 64; };
    int R = std::max(1, std::min(tc.Ho, 64 / tc.Wo));
    while (R > 1 && (buf_floats(R) * 8 + 256 > 160 * 1024 || xrows(R) * XC * 16 > WG3_MAXX * 512)) --R;
    q.R = R; q.XR = xrows(R); q.XC = XC;
    q.dzpix = (R * tc.Wo + 1) & ~1;
    q.buf_floats = buf_floats(R);
    DH_REQUIRE(q.XR * q.XC * 16 <= WG3_MAXX * 512 && q.dzpix * 16 <= WG3_MAXD * 512 && R * tc.Wo <= 64,
               "wgrad3: window %dx%d does not fit the staging plan", q.XR, q.XC);
    const size_t lds = std::max<size_t>((size_t)256 + (size_t)q.buf_floats * 8, (size_t)4 * 9 * 16 * 64 * 4);
    DH_REQUIRE(lds <= 160 * 1024, "wgrad3: LDS budget exceeded (%zu B)", lds);
    q.rb_per_img = (tc.Ho + R - 1) / R;
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

// first train_begin: the block table from the network description (net_desc.inc), the arena layout in forward order, and the completion items of the backward pass: fc, the blocks last to first, the stem -- each
// runs from its first tensor down to where the previous item started
void tr_layout(dh_resnet18* net) {
  dh_train* t = net->train;
  for (const BlockDesc& b : net->desc->blocks) t->blocks.push_back({b.conv[0], b.conv[1], b.ds, 0, 0});
  for (const auto& c : net->convs) {
    store_add(*t, c.name + ".weight", (int64_t)c.cout * c.cin * c.ks * c.ks);
    store_add(*t, c.bn + ".weight", c.cout); store_add(*t, c.bn + ".bias", c.cout);
    store_radd(*t, c.bn + ".running_mean", c.cout); store_radd(*t, c.bn + ".running_var", c.cout);
  }
  store_add(*t, "fc.weight", (int64_t)net->n_classes * net->desc->feat); store_add(*t, "fc.bias", net->n_classes);
  int64_t end = t->n_params;
  auto item_from = [&](int64_t start) { t->items.push_back({start, end - start}); end = start; };
  item_from(t->slot["fc.weight"].first);
  for (auto b = t->blocks.rbegin(); b != t->blocks.rend(); ++b) item_from(t->slot[net->convs[b->c1].name + ".weight"].first);
  item_from(0);
}

}  // namespace

extern "C" int dh_resnet18_train_end(dh_resnet18* net);

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
    t->tc.resize(net->convs.size());
    if ((rc = store_alloc(*t, &t->ones, 512)) || (rc = store_alloc(*t, &t->zeros, 512)) ||
        (rc = store_alloc(*t, &t->partial, (int64_t)RED_NB * 2 * 512)) ||
        (rc = store_alloc(*t, &t->stem_slabs, (int64_t)STEM_WGRAD_SLABS * 64 * 160)) ||
        (rc = store_alloc(*t, &t->wgrad_slabs, (int64_t)WGRAD3_WGS * 64 * 64 * 9))) return rc;
    hipLaunchKernelGGL(fill_kernel, dim3(2), dim3(256), 0, st, t->ones, (int64_t)512, 1.0f);
    DH_HIP(hipMemsetAsync(t->zeros, 0, 512 * 4, st));
    for (size_t i = 0; i < net->convs.size(); ++i) {
      const ConvLayer& c = net->convs[i];
      TrainConv& tc = t->tc[i];
      const int64_t nw = (int64_t)c.cout * c.cin * c.ks * c.ks;
      if (i == 0) { if ((rc = store_alloc(*t, &tc.wp_f, 7 * 11 * 2 * 64))) return rc; }
      else { if ((rc = store_alloc(*t, &tc.wp_f, nw)) || (rc = store_alloc(*t, &tc.wp_d, nw))) return rc; }
      float** bb[7] = {&tc.bn.mean, &tc.bn.invstd, &tc.bn.scale, &tc.bn.shift, &tc.bn.k0, &tc.bn.k1, &tc.bn.k2};
      for (auto q : bb) if ((rc = store_alloc(*t, q, c.cout))) return rc;
    }
    if ((rc = tr_pack_all(net, st))) return rc;
  } else {
    store_free_shape(*t);   // batch shape changed: drop the (B, P)-sized buffers only
  }
  t->B = B; t->P = P;
  // ---- activations and workspaces of this batch shape
  t->shape_phase = true;
  const int H1 = (P + 6 - 7) / 2 + 1, H2 = (H1 + 2 - 3) / 2 + 1;
  auto setup = [&](size_t i, int hi, int ho) -> int {
    const ConvLayer& c = net->convs[i];
    TrainConv& tc = t->tc[i];
    tc.Hi = tc.Wi = hi; tc.Ho = tc.Wo = ho;
    const int64_t nout = (int64_t)B * ho * ho * c.cout;
    int r;
    if ((r = store_alloc(*t, &tc.Z, nout)) || (r = store_alloc(*t, &tc.Y, nout))) return r;
    if (t->side && i > 0 && (r = store_alloc(*t, &tc.dZ, nout))) return r;
    return DH_OK;
  };
  auto shape_done = [&](int r) { t->shape_phase = false; return r; };
  if ((rc = setup(0, P, H1))) return shape_done(rc);
  int H = H2;
  for (TrBlock& b : t->blocks) {
    b.hi = H; b.ho = H / net->convs[b.c1].stride;
    if ((rc = setup(b.c1, b.hi, b.ho)) || (rc = setup(b.c2, b.ho, b.ho))) return shape_done(rc);
    if (b.ds >= 0 && (rc = setup(b.ds, b.hi, b.ho))) return shape_done(rc);
    H = b.ho;
  }
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
    TrainConv& tc = t->tc[0];
    StemParams sp;
    sp.x_nchw = x; sp.slide = nullptr; sp.yx = nullptr; sp.row_bytes = 0;
    sp.w = tc.wp_f; sp.scale = t->ones; sp.shift = t->zeros; sp.out = tc.Z;
    sp.B = B; sp.P = P; sp.Ho = tc.Ho; sp.Wo = tc.Wo; sp.relu = 0;
    sp.tiles_y = (tc.Ho + STEM_TH - 1) / STEM_TH; sp.tiles_x = (tc.Wo + STEM_TW - 1) / STEM_TW;
    const size_t lds = (size_t)7 * 11 * 2 * 256 + (size_t)STEM_ROWS * STEM_ROWE * 4;
    if (int arc = ensure_dyn_lds(reinterpret_cast<const void*>(&stem_kernel<float, false>), 96 * 1024)) return arc;
    hipLaunchKernelGGL((stem_kernel<float, false>), dim3(B * sp.tiles_y * sp.tiles_x), dim3(256), lds, st, sp);
    DH_LAUNCH_CHECK();
    if ((rc = tr_bn_forward(tr_bn_view(net, 0), nullptr, true, nullptr, st, t->X1, t->pool_idx))) return rc;   // + ReLU + maxpool in the same pass
  }
  const float* X = t->X1;
  for (const TrBlock& b : t->blocks) {
    const ConvLayer &c1 = net->convs[b.c1], &c2 = net->convs[b.c2];
    TrainConv &t1 = t->tc[b.c1], &t2 = t->tc[b.c2];
    if ((rc = tr_conv(u, c1.cin, c1.cout, 3, c1.stride, t1.wp_f, X, nullptr, t1.Z, B, t1.Hi, t1.Wi, st))) return rc;
    if ((rc = tr_bn_forward(tr_bn_view(net, b.c1), nullptr, true, t1.Y, st))) return rc;
    const float* idt = X;
    if (b.ds >= 0) {
      const ConvLayer& cd = net->convs[b.ds];
      TrainConv& td = t->tc[b.ds];
      if ((rc = tr_conv(u, cd.cin, cd.cout, 1, 2, t->Pm + t->slot[cd.name + ".weight"].first, X, nullptr, td.Z, B, td.Hi, td.Wi, st))) return rc;
      if ((rc = tr_bn_forward(tr_bn_view(net, b.ds), nullptr, false, td.Y, st))) return rc;
      idt = td.Y;
    }
    if ((rc = tr_conv(u, c2.cin, c2.cout, 3, 1, t2.wp_f, t1.Y, nullptr, t2.Z, B, t2.Hi, t2.Wi, st))) return rc;
    if ((rc = tr_bn_forward(tr_bn_view(net, b.c2), idt, true, t2.Y, st))) return rc;
    X = t2.Y;
  }
  const TrainConv& l4 = t->tc[t->blocks.back().c2];
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
// `fused` (single-rank training): the Adam update and the repack of a block's tensors follow that block's weight gradients on the side
// stream, instead of one update of the whole arena after the pass (same arithmetic per element: identical parameters).
int tr_backward(dh_resnet18* net, const float* dlogits, hipStream_t st, const AdamArgs* fused) {
  dh_train* t = net->train;
  const int B = t->B, ncls = net->n_classes;
  const UnitAffine u{t->ones, t->zeros};
  int rc;
  store_begin_backward(*t);
  auto grad_of = [&](const ConvLayer& c) { return t->G + t->slot[c.name + ".weight"].first; };
  // side-stream weight gradients (see t2_backward for the scheme): queued per block behind one event of the main stream
  const bool side = t->side != nullptr;
  struct PendingW { const ConvLayer* c; const TrainConv* tc; const float* x; const float* dz; };
  std::vector<PendingW> pending;
  auto wgrad_of = [&](const ConvLayer& c, const TrainConv& tc, const float* x, const float* dz) -> int {
    if (!side) return tr_wgrad(t->wgrad_slabs, grad_of(c), c, tc, x, dz, B, st);
    pending.push_back({&c, &tc, x, dz});
    return DH_OK;
  };
  int64_t adam_end = t->n_params;   // fused optimiser: the arena from here on has been updated (it completes from the end)
  auto flush_side = [&]() -> int {
    if (pending.empty()) return DH_OK;
    int r = side_handoff(*t, st);
    if (r) return r;
    int lo = (int)net->convs.size(), hi = -1;
    for (const PendingW& w : pending) {
      if ((r = tr_wgrad(t->wgrad_slabs, grad_of(*w.c), *w.c, *w.tc, w.x, w.dz, B, t->side))) return r;
      const int ci = (int)(w.c - net->convs.data());
      lo = std::min(lo, ci); hi = std::max(hi, ci);
    }
    if (fused) {   // the block's tensors start at its first conv (arena = forward order); everything behind them is complete too
      const int64_t from = t->slot[net->convs[lo].name + ".weight"].first;
      DH_REQUIRE(hi - lo + 1 == (int)pending.size() && from < adam_end, "backward: the convolutions of a hand-off are not a contiguous range");
      if (!(DH_T1_ABL & 8)) adam_range(*t, *fused, from, adam_end - from, t->side);
      adam_end = from;
      if ((r = tr_pack(net, t->side, lo, hi + 1))) return r;
    }
    pending.clear();
    return DH_OK;
  };
  auto join_side = [&]() -> int {
    if (!side) return DH_OK;
    int r = flush_side();
    return r ? r : side_join(*t, st);
  };
  // fc + avgpool
  const TrainConv& l4 = t->tc[t->blocks.back().c2];
  const int HW4 = l4.Ho * l4.Wo;
  hipLaunchKernelGGL(fc_wgrad_kernel, dim3((ncls * 512 + 255) / 256), dim3(256), 0, st, dlogits, t->pooled, B, 512, ncls,
                     t->G + t->slot["fc.weight"].first, t->G + t->slot["fc.bias"].first);
  float* dOut = t->SM[0];
  hipLaunchKernelGGL(avgpool_fc_dgrad_kernel, dim3(B), dim3(256), 0, st, dlogits, t->Pm + t->slot["fc.weight"].first, HW4, 512, ncls, dOut);
  DH_LAUNCH_CHECK();
  store_mark_done(*t);   // fc
  // residual blocks in reverse
  for (int b = (int)t->blocks.size() - 1; b >= 0; --b) {
    const int i1 = t->blocks[b].c1, i2 = t->blocks[b].c2, id = t->blocks[b].ds;
    const ConvLayer &c1 = net->convs[i1], &c2 = net->convs[i2];
    TrainConv &t1 = t->tc[i1], &t2 = t->tc[i2];
    const float* Xin = b == 0 ? t->X1 : t->tc[t->blocks[b - 1].c2].Y;
    float* G2 = t->SM[1];   // masked gradient at the block output (flows to both branches)
    float* dZ2 = side ? t2.dZ : t->SM[2];
    const int64_t n2 = (int64_t)B * t2.Ho * t2.Wo * c2.cout;
    tr_dump("dOut", b, dOut, n2, st);
    if ((rc = tr_bn_backward(tr_bn_view(net, i2), dOut, t2.Y, true, dZ2, G2, st))) return rc;   // dOut is dead after this
    tr_dump("dZ2", b, dZ2, n2, st);
    if ((rc = wgrad_of(c2, t2, t1.Y, dZ2))) return rc;
    float* dY1 = t->SM[3];
    if ((rc = tr_conv(u, c2.cout, c2.cin, 3, 1, t2.wp_d, dZ2, nullptr, dY1, B, t2.Ho, t2.Wo, st))) return rc;
    tr_dump("dY1", b, dY1, n2, st);
    float* dZ1 = side ? t1.dZ : t->SM[2];  // (single stream: dZ2 is dead now)
    if ((rc = tr_bn_backward(tr_bn_view(net, i1), dY1, nullptr, true, dZ1, nullptr, st))) return rc;   // ReLU pattern from Z
    tr_dump("dZ1", b, dZ1, n2, st);
    if ((rc = wgrad_of(c1, t1, Xin, dZ1))) return rc;
    float* dX = t->SM[0];
    if (id < 0) {
      // dX = dgrad(conv1) + G2 (identity branch), fused as the conv's residual input
      if ((rc = tr_conv(u, c1.cout, c1.cin, 3, 1, t1.wp_d, dZ1, G2, dX, B, t1.Ho, t1.Wo, st))) return rc;
    } else {
      const ConvLayer& cd = net->convs[id];
      TrainConv& td = t->tc[id];
      // stride-2 data gradient: four parity-class launches over dZ1 itself (round 2 ran a stride-1 conv over a zero-upsampled
      // copy: four times the MFMA work and a 4x-sized tensor written and read)
      if ((rc = tr_dgrad_s2(u, c1.cout, c1.cin, t1.wp_d, dZ1, nullptr, dX, B, t1.Ho, t1.Wo, t1.Hi, t1.Wi, st))) return rc;
      // downsample branch: BN (no ReLU) <- G2 ; 1x1 stride-2 conv
      float* dZd = side ? td.dZ : t->SM[3];  // (single stream: dY1 is dead)
      if ((rc = tr_bn_backward(tr_bn_view(net, id), G2, nullptr, false, dZd, nullptr, st))) return rc;
      if ((rc = wgrad_of(cd, td, Xin, dZd))) return rc;
      float* tt = side ? t->SM[3] : t->SM[2];   // dY1 (dZ1 on a single stream) is dead: [B, Ho, Wo, cin]
      if ((rc = tr_conv(u, cd.cout, cd.cin, 1, 1, td.wp_d, dZd, nullptr, tt, B, td.Ho, td.Wo, st))) return rc;
      const int64_t m4 = (int64_t)B * td.Ho * td.Wo * cd.cin / 4;
      hipLaunchKernelGGL(upsample2_add_kernel, dim3(grid_for(m4)), dim3(256), 0, st, tt, dX, B, td.Ho, td.Wo, cd.cin);
      DH_LAUNCH_CHECK();
    }
    dOut = dX;
    if (t->bucket_cb) { if ((rc = join_side())) return rc; }   // a bucket may complete here: its gradients precede the caller's event
    else if ((rc = flush_side())) return rc;
    store_mark_done(*t);   // the block
  }
  // stem: maxpool, BN+ReLU, wgrad
  {
    TrainConv& tc = t->tc[0];
    float* dZ0 = t->BIG1;
    if ((rc = tr_bn_pool_backward(tr_bn_view(net, 0), dOut, t->pool_idx, dZ0, st))) return rc;   // maxpool + ReLU + BN backward, dY never materialised
    if ((rc = tr_stem_wgrad(dZ0, t->x_in, t->stem_slabs, t->G + t->slot["conv1.weight"].first, B, t->P, tc.Ho, tc.Wo, st))) return rc;
    if ((rc = join_side())) return rc;   // the optimiser (and the last bucket) follow on the main stream
    store_mark_done(*t);   // the stem
    if (fused) {   // what the side stream has not updated: the stem (all of the arena without a side stream)
      if (!(DH_T1_ABL & 8)) adam_range(*t, *fused, 0, adam_end, st);
      if ((rc = tr_pack_stem(net, st))) return rc;
      if (adam_end == t->n_params && (rc = tr_pack(net, st, 1, (int)net->convs.size()))) return rc;
    }
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
  return tr_pack_all(net, st);
}

// store_tensor on the training state; the caller re-packs after pushing parameters (dh_resnet18_train_repack)
extern "C" int dh_resnet18_train_tensor(dh_resnet18* net, const char* name, int32_t kind, void* ptr, int64_t n_elem,
                                        int32_t to_lib, void* stream) {
  DH_REQUIRE(net && net->train && name && ptr, "train tensor: no training state / null argument");
  return store_tensor(*net->train, "train tensor", name, kind, ptr, n_elem, to_lib, dh::as_stream(stream));
}

extern "C" int dh_resnet18_train_repack(dh_resnet18* net, void* stream) {
  DH_REQUIRE(net && net->train, "train repack: no training state");
  return tr_pack_all(net, dh::as_stream(stream));
}

extern "C" int dh_resnet18_train_flat(dh_resnet18* net, int32_t kind, void** ptr_out, int64_t* n_out) {
  DH_REQUIRE(net && net->train && ptr_out && n_out && kind >= 0 && kind <= 2, "train flat: bad arguments / no training state");
  store_flat(*net->train, kind, ptr_out, n_out);
  return DH_OK;
}
