// bn_fold.inc -- batch norm of the bf16 engine on SMALL maps (stages 3-4 of ResNet-50 / ResNet-18: <= 16 384 pixel rows) without the
// finalize launches (round 4; VERDICT r3 item 3).  Included after train2_kernels.inc.
//
// A training-mode BN is three dependent launches each way: per-workgroup partial sums -> a "finalize" launch that adds the partial
// rows and makes the per-channel coefficients -> the elementwise pass.  On the 3-13 MB maps of stages 3-4 every one of them sits at
// the floor of a dependent launch (5-7 us), and the 106 finalize launches of a ResNet-50 step cost 0.56 ms of its 7.15 ms
// (profiles/r04_exp_step_ablation.txt).  Round 3 tried to fold the finalize into the PRODUCER (arrival tickets, integer atomics): both
// put a returning atomic or a fence on every workgroup's lifetime and were slower.  Here it is folded into the CONSUMER, with no
// inter-workgroup communication at all:
//   * the elementwise kernels are CHANNEL-SLICED: a workgroup = 64 channels x a range of pixel rows (one 128-byte line per row:
//     8 threads x 16 B), grid = C / 64 slices x row groups, so a workgroup needs the coefficients of ITS 64 channels only;
//   * its prologue adds the partial rows of those 64 channels itself, in a fixed order in double (every row group of a slice computes
//     the same bits), and makes the coefficients in LDS; row group 0 also writes what later launches need (mean / invstd / scale /
//     shift / running statistics; dgamma / dbeta).  With <= 128 partial rows that is <= 64 KB of L2-resident reads per workgroup;
//   * the partial rows come from the 1x1 GEMM's epilogue (gemm1x1.inc: one row per 128-pixel tile: 25 / 98 rows at 7 x 7 / 14 x 14)
//     or from channel-sliced reduction kernels that leave ONE row per row group (<= 32 rows).
// Arithmetic is that of bn_stat_finalize_onepass_kernel / bn_bwd_finalize_kernel (train_core_kernels.inc) and bn2_apply / bn2_bwd_apply
// (train2_kernels.inc), partial rows added in the finalize kernels' own order: the same bits from the same rows.
namespace {

constexpr int CS_CH = 64;          // channels per slice
constexpr int CS_MAX_ROWS = 128;   // partial rows a consumer prologue accepts

// column sums of partial[nb][2][C] for channels c0 .. c0 + 63 (two sums per channel), left in LDS as doubles s[k][ch].  The ORDER is
// that of partial_colsum (train_core_kernels.inc), so a folded prologue and the finalize launch give the same bits from the same rows: 16 phases,
// phase p adds rows p, p + 16, p + 32, ... in increasing order, the 16 phase sums are added in index order.  Thread = (channel, 4 phases).
__device__ __forceinline__ void cs_colsum(const float* __restrict__ partial, int nb, int C, int c0, double (*s)[CS_CH]) {
  __shared__ double sh[16][2][CS_CH];
  const int ch = threadIdx.x & 63, q4 = threadIdx.x >> 6;
  double a0[4] = {0.0, 0.0, 0.0, 0.0}, a1[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j0 = 0; j0 * 16 < nb; j0 += 2) {   // 2 row blocks x 4 phases = 8 rows (16 loads) in flight per thread
    float v0[2][4], v1[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int b = (j0 + u) * 16 + 4 * q4 + k, bb = min(b, nb - 1);
        const float w = b < nb ? 1.f : 0.f;
        v0[u][k] = partial[((int64_t)bb * 2 + 0) * C + c0 + ch] * w;
        v1[u][k] = partial[((int64_t)bb * 2 + 1) * C + c0 + ch] * w;
      }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k) { a0[k] += (double)v0[u][k]; a1[k] += (double)v1[u][k]; }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) { sh[4 * q4 + k][0][ch] = a0[k]; sh[4 * q4 + k][1][ch] = a1[k]; }
  __syncthreads();
  if (q4 < 2) {   // waves 0 / 1: the first / second sum of the 64 channels
    double t = sh[0][q4][ch];
    for (int p = 1; p < 16; ++p) t += sh[p][q4][ch];
    s[q4][ch] = t;
  }
  __syncthreads();
}

struct CsGeom { int slice, rg, c0; int64_t r0, r1; };
__device__ __forceinline__ CsGeom cs_geom(int64_t rows, int C) {
  CsGeom g;
  const int nsl = C / CS_CH, nrg = gridDim.x / nsl;
  g.slice = blockIdx.x % nsl; g.rg = blockIdx.x / nsl; g.c0 = g.slice * CS_CH;
  const int64_t rpg = (rows + nrg - 1) / nrg;
  g.r0 = g.rg * rpg; g.r1 = min(rows, g.r0 + rpg);
  return g;
}

// ---- forward: statistics finalize + y = [relu]( z*scale + shift [+ res] ) --------------------------------------------------
__global__ __launch_bounds__(256) void bn2_fold_apply_kernel(const bf16_t* __restrict__ z, const float* __restrict__ partial, int nb, double n_rows,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, float* mean, float* invstd,
                                                             float* scale, float* shift, float* run_mean, float* run_var,
                                                             const bf16_t* __restrict__ res, bf16_t* __restrict__ y, int64_t rows, int C, int relu,
                                                             uint8_t* __restrict__ bits = nullptr) {
  __shared__ double s[2][CS_CH];
  __shared__ float coef[2][CS_CH];
  const CsGeom g = cs_geom(rows, C);
  cs_colsum(partial, nb, C, g.c0, s);
  if (threadIdx.x < CS_CH) {
    const int ch = threadIdx.x, c = g.c0 + ch;
    const double mu = s[0][ch] / n_rows;
    double var = s[1][ch] / n_rows - mu * mu;
    if (var < 0.0) var = 0.0;
    const float is = (float)(1.0 / sqrt(var + (double)BN_EPS));
    const float sc = gamma[c] * is, sh = beta[c] - (float)mu * sc;
    coef[0][ch] = sc; coef[1][ch] = sh;
    if (g.rg == 0) {
      mean[c] = (float)mu; invstd[c] = is; scale[c] = sc; shift[c] = sh;
      const double unbiased = n_rows > 1.0 ? var * n_rows / (n_rows - 1.0) : var;
      run_mean[c] = (1.f - BN_MOMENTUM) * run_mean[c] + BN_MOMENTUM * (float)mu;
      run_var[c] = (1.f - BN_MOMENTUM) * run_var[c] + BN_MOMENTUM * (float)unbiased;
    }
  }
  __syncthreads();
  const int o = threadIdx.x & 7, rl = threadIdx.x >> 3;
  float sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { sc[e] = coef[0][o * 8 + e]; sh[e] = coef[1][o * 8 + e]; }
  const int64_t col = g.c0 + o * 8;
  for (int64_t rb = g.r0 + rl; rb < g.r1; rb += 32 * 4) {   // 4 rows in flight per thread
    F8 v[4], rr[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = min(rb + 32 * u, g.r1 - 1);
      v[u] = ld8(z + r * C + col);
      if (res) rr[u] = ld8(res + r * C + col);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = rb + 32 * u;
      if (r >= g.r1) break;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[u].v[e] = __builtin_fmaf(v[u].v[e], sc[e], sh[e]);
      if (res) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[u].v[e] += rr[u].v[e];
      }
      if (relu) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[u].v[e] = fmaxf(v[u].v[e], 0.f);
      }
      st8_bits(y + r * C + col, v[u], bits ? bits + (r * C + col) / 8 : nullptr);
    }
  }
}

// ---- backward: sums finalize + g = dy * mask; dz = k0 g + k1 z + k2 [; g_out = g] ------------------------------------------
// relu: 0 none / pre-masked dy, 1 pattern from y, 2 pattern recomputed from z with the FORWARD's scale / shift (bn2_bwd_apply_kernel)
__global__ __launch_bounds__(256) void bn2_fold_bwd_apply_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ y, const bf16_t* __restrict__ z,
                                                                 const float* __restrict__ partial, int nb, double n_rows, const float* __restrict__ gamma,
                                                                 const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                 const float* __restrict__ scale, const float* __restrict__ shift, float* dgamma,
                                                                 float* dbeta, bf16_t* __restrict__ dz, bf16_t* __restrict__ g_out, int64_t rows, int C,
                                                                 int relu) {
  __shared__ double s[2][CS_CH];
  __shared__ float coef[5][CS_CH];
  const CsGeom g = cs_geom(rows, C);
  cs_colsum(partial, nb, C, g.c0, s);
  if (threadIdx.x < CS_CH) {
    const int ch = threadIdx.x, c = g.c0 + ch;
    const double s1 = s[0][ch], s2 = s[1][ch];
    const double a = (double)gamma[c] * (double)invstd[c];
    const double b1 = -a * (double)invstd[c] * s2 / n_rows;
    coef[0][ch] = (float)a; coef[1][ch] = (float)b1; coef[2][ch] = (float)(-a * s1 / n_rows - b1 * (double)mean[c]);
    coef[3][ch] = scale[c]; coef[4][ch] = shift[c];
    if (g.rg == 0) { dgamma[c] = (float)s2; dbeta[c] = (float)s1; }
  }
  __syncthreads();
  const int o = threadIdx.x & 7, rl = threadIdx.x >> 3;
  float k0[8], k1[8], k2[8], sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    k0[e] = coef[0][o * 8 + e]; k1[e] = coef[1][o * 8 + e]; k2[e] = coef[2][o * 8 + e]; sc[e] = coef[3][o * 8 + e]; sh[e] = coef[4][o * 8 + e];
  }
  const int64_t col = g.c0 + o * 8;
  for (int64_t rb = g.r0 + rl; rb < g.r1; rb += 32 * 4) {
    F8 gg[4], v[4], yy[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = min(rb + 32 * u, g.r1 - 1);
      gg[u] = ld8(dy + r * C + col);
      v[u] = ld8(z + r * C + col);
      if (relu == 1) yy[u] = ld8(y + r * C + col);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = rb + 32 * u;
      if (r >= g.r1) break;
      if (relu == 1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) gg[u].v[e] = yy[u].v[e] > 0.f ? gg[u].v[e] : 0.f;
      } else if (relu == 2) {
#pragma unroll
        for (int e = 0; e < 8; ++e) gg[u].v[e] = __builtin_fmaf(v[u].v[e], sc[e], sh[e]) > 0.f ? gg[u].v[e] : 0.f;
      }
      F8 ov;
#pragma unroll
      for (int e = 0; e < 8; ++e) ov.v[e] = __builtin_fmaf(k0[e], gg[u].v[e], __builtin_fmaf(k1[e], v[u].v[e], k2[e]));
      st8(dz + r * C + col, ov);
      if (g_out) st8(g_out + r * C + col, gg[u]);
    }
  }
}

// ---- channel-sliced reductions: ONE partial row per row group (grid = C / 64 slices x row groups) -------------------------------
// MODE 0: {sum z, sum z^2} (bn2_stats_kernel); MODE 1: {sum g, sum g xhat} (bn2_bwd_reduce_kernel, relu as there)
template <int MODE>
__global__ __launch_bounds__(256) void bn2_cs_reduce_kernel(const bf16_t* __restrict__ z, const bf16_t* __restrict__ dy, const bf16_t* __restrict__ y,
                                                            const float* __restrict__ mean, const float* __restrict__ invstd,
                                                            const float* __restrict__ scale, const float* __restrict__ shift, int64_t rows, int C,
                                                            int relu, float* __restrict__ partial) {
  __shared__ float red[2][32][CS_CH];
  const CsGeom g = cs_geom(rows, C);
  const int o = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int64_t col = g.c0 + o * 8;
  float a[8], b[8], mu[8], is[8], sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { a[e] = 0.f; b[e] = 0.f; mu[e] = 0.f; is[e] = 0.f; sc[e] = 0.f; sh[e] = 0.f; }
  if (MODE == 1) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { mu[e] = mean[col + e]; is[e] = invstd[col + e]; sc[e] = scale[col + e]; sh[e] = shift[col + e]; }
  }
  for (int64_t rb = g.r0 + rl; rb < g.r1; rb += 32 * 4) {
    F8 v[4], gg[4], yy[4];
    float m[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = rb + 32 * u, rr = min(r, g.r1 - 1);
      m[u] = r < g.r1 ? 1.f : 0.f;
      v[u] = ld8(z + rr * C + col);
      if (MODE == 1) {
        gg[u] = ld8(dy + rr * C + col);
        if (relu == 1) yy[u] = ld8(y + rr * C + col);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (MODE == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float x = v[u].v[e] * m[u]; a[e] += x; b[e] = __builtin_fmaf(x, x, b[e]); }
      } else {
        if (relu == 1) {
#pragma unroll
          for (int e = 0; e < 8; ++e) gg[u].v[e] = yy[u].v[e] > 0.f ? gg[u].v[e] : 0.f;
        } else if (relu == 2) {
#pragma unroll
          for (int e = 0; e < 8; ++e) gg[u].v[e] = __builtin_fmaf(v[u].v[e], sc[e], sh[e]) > 0.f ? gg[u].v[e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float q = gg[u].v[e] * m[u]; a[e] += q; b[e] = __builtin_fmaf(q, (v[u].v[e] - mu[e]) * is[e], b[e]); }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) { red[0][rl][o * 8 + e] = a[e]; red[1][rl][o * 8 + e] = b[e]; }
  __syncthreads();
  if (threadIdx.x < 2 * CS_CH) {   // the 32 row lanes of a channel, added in index order
    const int k = threadIdx.x >> 6, ch = threadIdx.x & 63;
    if (MODE == 0) {
      // The statistics' lanes are added in DOUBLE and rounded once: the consumer forms var = E z^2 - mean^2, which multiplies the relative
      // error of sum z^2 by 1 + (mean / std)^2.  A lane holds at most 16 rows and its float32 sum of bf16 squares is exact or nearly so;
      // the 31 float32 additions of the lanes were not: at 512 rows a group they left sum z^2 of a channel whose mean is 8 standard
      // deviations 1.2e-7 off, 3.7e-6 in invstd (tests/test_gpu_bn_bf16_parity.py, 16384 x 128).  The backward sums have no such
      // amplification and keep their float32 order.  What remains is the ONE rounding of each partial row to float32 (<= 2^-25 of the
      // row): on such a channel up to 64 * 2^-25 = 1.9e-6 of var when a map has one or two row groups (64 - 128 rows); with 32 rows the
      // roundings average out (2.6e-7 of invstd measured at 16384 x 128).  So the 1e-6 of the tests holds for the data and shapes
      // tested, not by construction: a structural bound needs partial rows that lose nothing (a hi / lo float pair).
      double t = (double)red[k][0][ch];
#pragma unroll
      for (int q = 1; q < 32; ++q) t += (double)red[k][q][ch];
      partial[((int64_t)g.rg * 2 + k) * C + g.c0 + ch] = (float)t;
    } else {
      float t = red[k][0][ch];
#pragma unroll
      for (int q = 1; q < 32; ++q) t += red[k][q][ch];
      partial[((int64_t)g.rg * 2 + k) * C + g.c0 + ch] = t;
    }
  }
}

}  // namespace
