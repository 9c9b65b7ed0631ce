// train_core_kernels.inc -- the device code and the constants that BOTH training engines use.  Included in resnet_kernels.hip in front of
// train_core.inc.  Whatever is here is shared: a change reaches the float32 engine (train.inc), the bf16 engine (train2.inc) and, through the
// finalize arithmetic, the folded prologues of bn_fold.inc.  An engine's own kernels are in train_kernels.inc (float32) and
// train2_kernels.inc / wgrad_ring.inc / bn_fold.inc / gemm1x1.inc (bf16); nothing outside this file is used by both.
//   fill_kernel, adam_kernel, grid_for          train_core.inc (adam_range), both engines' set-up; grid_for sizes every elementwise launch
//   BN_EPS, BN_MOMENTUM, BnBufs, RED_NB         the per-channel buffers of one BN and the most partial rows a reduction leaves
//   FIN_CH, partial_colsum                      the column sums under the three kernels below -- and the order bn_fold.inc re-states
//   bn_stat_finalize_onepass_kernel             tr_bn_forward (train.inc); t2_conv_fwd, t2_bn_fwd (train2.inc)
//   bn_bwd_finalize_kernel                      tr_bn_backward, tr_bn_pool_backward; t2_bn_bwd, t2_bn_pool_bwd
//   wgrad_reduce_kernel, wgrad_reduce_taps_kernel   tr_wgrad; t2_wgrad
//   SWG_T, STEM_WGRAD_SLABS, stem_wgrad_reduce_kernel   stem_wgrad_reduce (train_core.inc) behind either engine's stem weight-gradient kernel
//   fc_fwd_kernel, fc_wgrad_kernel              the head of both forward / backward passes
//   ce_loss_kernel                              dh_ce_loss (train.inc), the loss of both engines' steps
// CONTRACT with bn_fold.inc: its prologues (bn2_fold_apply_kernel, bn2_fold_bwd_apply_kernel) compute, from the same partial rows, the SAME BITS
// as bn_stat_finalize_onepass_kernel / bn_bwd_finalize_kernel: the same 16 phases over the rows, the same fixed-order double sums, the same
// expressions.  Change one side and the other changes with it (tests/test_gpu_train_bf16.py::test_bn_fold_is_bit_identical holds them together).
struct BnBufs { float *mean, *invstd, *scale, *shift, *k0, *k1, *k2; };   // per-channel device arrays of one BN: forward statistics and coefficients, backward coefficients

namespace {

constexpr float BN_EPS = 1e-5f, BN_MOMENTUM = 0.1f;
constexpr int RED_NB = 512;             // most partial rows (workgroups) of a per-channel reduction
constexpr int STEM_WGRAD_SLABS = 512;   // most slabs of a stem weight gradient
constexpr int SWG_T = 512;              // threads of a stem weight-gradient workgroup (either engine's kernel)

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

// one-pass form: mean and biased variance from {sum z, sum z^2} (double column sums in a fixed order; var clamped at 0),
// normalisation coefficients, running statistics.  (Round 3: one pass over Z and one finalize launch per BN instead of
// two each.)
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
