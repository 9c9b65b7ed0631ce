// train2_kernels.inc -- device kernels of the bf16 training engine (train2.inc): ResNet-18 / ResNet-50 patch
// classifiers with bf16 activations and bf16 MFMA (f32 accumulation), f32 master weights / gradients / Adam.
// Included inside resnet_kernels.hip (same translation unit: the 3x3 forward / dgrad convolutions are the
// conv3x3_kernel<bf16> of conv3x3.inc on NHWC data).
//
// Everything here is NHWC ("pixel-major") bf16: a pixel's channels are contiguous, 8 channels = one 16-byte access.
//   * 1x1 convolutions (51.9 % of the ResNet-50 MACs) = NT GEMM  D[px][n] = sum_k A[px][k] * W[n][k], both operands
//     K-contiguous: gemm1x1_ring_kernel (gemm1x1.inc; stride-2 row gather for the downsample branch);
//   * weight gradients = pixel-reduction GEMMs  dW[co][ci][tap] = sum_px dZ[px][co] * X[px @ tap][ci]: both operands are
//     K-STRIDED in a pixel-major layout, so fragments come out of LDS through the hardware transpose read
//     ds_read_b64_tr_b16 (wgrad_bf16_kernel);
//   * batch-norm statistics / apply / backward, max-pool, average-pool: HBM-bound elementwise kernels, f32 arithmetic.
namespace {

typedef uint16_t bf16_t;   // raw bfloat16 bits in HBM
typedef short v4s_t __attribute__((ext_vector_type(4)));

struct F8 { float v[8]; };
__device__ __forceinline__ F8 ld8(const bf16_t* p) {   // 16-byte load -> 8 floats
  const uint4 u = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
  F8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) { r.v[2 * i] = bf16_bits_to_f32(w[i] & 0xFFFFu); r.v[2 * i + 1] = bf16_bits_to_f32(w[i] >> 16); }
  return r;
}
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {   // v_cvt_pk_bf16_f32 (RNE; keeps NaN a NaN)
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, bf16x2_t{(__bf16)a, (__bf16)b});
}
__device__ __forceinline__ void st8(bf16_t* p, const F8& r) {
  *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf16x2(r.v[0], r.v[1]), pack_bf16x2(r.v[2], r.v[3]),
                                            pack_bf16x2(r.v[4], r.v[5]), pack_bf16x2(r.v[6], r.v[7]));
}

// st8 plus the ReLU pattern of the 8 stored values as ONE byte (bit e: the bf16 value e is non-zero; the values are ReLU outputs, never
// negative).  Round 5: the dgrad GEMM that applies a block's join-ReLU to the gradient flowing into it (gemm1x1.inc, `mbits`) reads this
// byte instead of the 16-byte activation -- the 4w-channel block outputs are the largest tensors of a ResNet-50 step and that GEMM is
// bandwidth-bound (dZ in, dX out, identity gradient, BN-backward Z: the mask was a quarter of its traffic).  bits = [rows][C / 8] bytes.
__device__ __forceinline__ void st8_bits(bf16_t* p, const F8& r, uint8_t* bits_byte) {
  const uint32_t w[4] = {pack_bf16x2(r.v[0], r.v[1]), pack_bf16x2(r.v[2], r.v[3]), pack_bf16x2(r.v[4], r.v[5]), pack_bf16x2(r.v[6], r.v[7])};
  *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  if (bits_byte) {
    uint32_t b = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) b |= ((w[i] & 0x7FFFu) ? 1u << (2 * i) : 0u) | ((w[i] & 0x7FFF0000u) ? 2u << (2 * i) : 0u);
    *bits_byte = (uint8_t)b;
  }
}
// the same byte per 8 values of an existing activation (test hooks: the fused-GEMM tests hand over a bf16 mask tensor)
__global__ __launch_bounds__(256) void relu_bits_pack_kernel(const bf16_t* __restrict__ y, uint8_t* __restrict__ bits, int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const uint4 u = *reinterpret_cast<const uint4*>(y + i * 8);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
    uint32_t b = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) b |= ((w[k] & 0x7FFFu) ? 1u << (2 * k) : 0u) | ((w[k] & 0x7FFF0000u) ? 2u << (2 * k) : 0u);
    bits[i] = (uint8_t)b;
  }
}

// ---------------- weight packing (f32 masters -> bf16 operand copies) ----------------
// All convolutions of the network in ONE launch (after every optimiser step: ResNet-50 has 53 of them, and ~5 us is the floor
// of a launch): a descriptor per conv names the master weights, the operand copies and the workgroups that pack them.
//   1x1: W[cout][cin] -> bf16 in the same layout (forward operand) and its transpose Wt[cin][cout] (dgrad operand);
//   3x3: MFMA fragment order of pack_conv_weights, forward operator and the flipped / transposed dgrad operator;
//   7x7 stem: [kh][t][mt][lane][8] (pack_stem_weights, esz 2).
struct PackDesc { const float* w; bf16_t* wf; bf16_t* wd; int cout, cin, ks, blk0; };
__device__ __forceinline__ float pack_stem_elem(const float* __restrict__ w, int o) {
  int r = o;
  const int j = r % 8; r /= 8;
  const int l = r % 64; r /= 64;
  const int mt = r % 2; r /= 2;
  const int t = r % 2; r /= 2;
  const int kh = r;
  const int i = 16 * t + 8 * (l >> 5) + j, co = mt * 32 + (l & 31);
  if (i < 1 || i > 21) return 0.f;
  const int kw = (i - 1) / 3, c = (i - 1) % 3;
  return w[((co * 3 + c) * 7 + kh) * 7 + kw];
}
// 3x3: one workgroup per 64-cout x 64-cin tile.  The tile's 64 rows of 576 consecutive floats are read once (coalesced), rounded to
// bf16 and kept twice in LDS -- [tap][co][ci] for the forward fragments, [tap][ci][co] for the flipped / transposed dgrad operator --
// so that every 16-byte fragment piece of either packed operand is one ds_read_b128 and one coalesced store (a thread per packed
// element with nine div/mods and a 36-byte-strided read made this kernel 136 us for ResNet-18's 11 M weights).  16-byte slots of a
// 64-element row are XOR-swizzled with the row (conflict-free when 8 consecutive lanes read 8 consecutive rows).
constexpr int PACK3_LDS = 2 * 9 * 64 * 64 * 2;
__device__ __forceinline__ int pack3_idx(int tap, int row, int col) {   // bf16 element index in one LDS copy
  return (tap * 64 + row) * 64 + ((((col >> 3) ^ (row & 7)) << 3) | (col & 7));
}
__device__ __forceinline__ void pack3_tile(const PackDesc& d, int tile, bf16_t* lds) {
  const int cit = d.cin >> 6, cbk = tile / cit, cik = tile % cit, tid = threadIdx.x;
  bf16_t* A = lds;                      // [tap][co][ci]
  bf16_t* Bt = lds + 9 * 64 * 64;       // [tap][ci][co]
  for (int i = tid; i < 64 * 144; i += 256) {   // float4 pieces: row co_l, 144 per row
    const int co_l = i / 144, j0 = (i % 144) * 4;
    const float4 v = *reinterpret_cast<const float4*>(d.w + ((int64_t)(cbk * 64 + co_l) * d.cin + cik * 64) * 9 + j0);
    const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = j0 + k, ci_l = j / 9, tap = j % 9;
      const bf16_t b = (bf16_t)f32_to_bf16(f[k]);
      A[pack3_idx(tap, co_l, ci_l)] = b;
      Bt[pack3_idx(tap, ci_l, co_l)] = b;
    }
  }
  __syncthreads();
  const int nch_f = d.cin >> 5, nch_d = d.cout >> 5;
  for (int pc = tid; pc < 2 * 4608; pc += 256) {   // 16-byte pieces: 4608 of the forward operand, then 4608 of the dgrad operand
    const bool dg = pc >= 4608;
    int r = dg ? pc - 4608 : pc;
    const int l = r & 63; r >>= 6;
    const int mt = r & 1; r >>= 1;
    const int k2 = r & 1; r >>= 1;
    const int tap = r % 9, chl = r / 9;              // chl: which 32-channel chunk of the tile's 64
    const int row = 32 * mt + (l & 31), col0 = 32 * chl + 16 * k2 + 8 * (l >> 5);
    const bf16_t* src = (dg ? Bt : A) + pack3_idx(dg ? 8 - tap : tap, row, col0);
    const uint4 v = *reinterpret_cast<const uint4*>(src);
    const int cb = dg ? cik : cbk, ch = 2 * (dg ? cbk : cik) + chl, nch = dg ? nch_d : nch_f;
    bf16_t* dst = (dg ? d.wd : d.wf) + ((((int64_t)(cb * nch + ch) * 9 + tap) * 2 + k2) * 2 + mt) * 512 + l * 8;
    *reinterpret_cast<uint4*>(dst) = v;
  }
}
// `desc` .. `desc + nd`: the convolutions this launch packs; `blk_base` = blk0 of the first of them (a launch over a sub-range of the
// table: the weights one residual block's Adam update has just changed)
__global__ __launch_bounds__(256) void pack_all_kernel(const PackDesc* __restrict__ desc, int nd, int blk_base) {
  extern __shared__ __attribute__((aligned(16))) char pack_lds[];
  const int bid = (int)blockIdx.x + blk_base;
  int i = 0;
  while (i + 1 < nd && bid >= desc[i + 1].blk0) ++i;   // workgroup-uniform scan of <= 64 descriptors
  const PackDesc d = desc[i];
  const int nblk = (i + 1 < nd ? desc[i + 1].blk0 : (int)gridDim.x + blk_base) - d.blk0;
  const int64_t first = (int64_t)(bid - d.blk0) * 256 + threadIdx.x, step = (int64_t)nblk * 256;
  if (d.ks == 7) {
    for (int64_t o = first; o < 7 * 2 * 2 * 64 * 8; o += step) d.wf[o] = (bf16_t)f32_to_bf16(pack_stem_elem(d.w, (int)o));
  } else if (d.ks == 3) {
    pack3_tile(d, bid - d.blk0, reinterpret_cast<bf16_t*>(pack_lds));   // nblk == (cout / 64) * (cin / 64)
  } else {
    // 1x1: 64 x 64 tiles through LDS so that both the copy and its transpose are written in 128-byte rows (the transpose used to
    // be 2-byte stores cout*2 bytes apart)
    bf16_t (*tl)[66] = reinterpret_cast<bf16_t (*)[66]>(pack_lds);   // [co][ci], odd dword pitch
    const int cit = d.cin >> 6, ntile = (d.cout >> 6) * cit, tid = threadIdx.x;
    for (int tile = bid - d.blk0; tile < ntile; tile += nblk) {
      const int co0 = (tile / cit) * 64, ci0 = (tile % cit) * 64;
      __syncthreads();
      for (int i = tid; i < 64 * 16; i += 256) {          // float4 pieces: row i / 16, 4 cins at (i % 16) * 4
        const int r = i >> 4, c4 = (i & 15) * 4;
        const float4 v = *reinterpret_cast<const float4*>(d.w + (int64_t)(co0 + r) * d.cin + ci0 + c4);
        const bf16_t b0 = (bf16_t)f32_to_bf16(v.x), b1 = (bf16_t)f32_to_bf16(v.y), b2 = (bf16_t)f32_to_bf16(v.z), b3 = (bf16_t)f32_to_bf16(v.w);
        tl[r][c4] = b0; tl[r][c4 + 1] = b1; tl[r][c4 + 2] = b2; tl[r][c4 + 3] = b3;
        *reinterpret_cast<uint2*>(d.wf + (int64_t)(co0 + r) * d.cin + ci0 + c4) =
            make_uint2((uint32_t)b0 | ((uint32_t)b1 << 16), (uint32_t)b2 | ((uint32_t)b3 << 16));
      }
      __syncthreads();
      for (int i = tid; i < 64 * 16; i += 256) {          // transposed rows: ci = i / 16, 4 couts at (i % 16) * 4
        const int r = i >> 4, c4 = (i & 15) * 4;
        *reinterpret_cast<uint2*>(d.wd + (int64_t)(ci0 + r) * d.cout + co0 + c4) =
            make_uint2((uint32_t)tl[c4][r] | ((uint32_t)tl[c4 + 1][r] << 16), (uint32_t)tl[c4 + 2][r] | ((uint32_t)tl[c4 + 3][r] << 16));
      }
    }
  }
}

// ---------------- batch norm ----------------
// Statistics travel as rows of per-workgroup partial sums [producers][2][C] (float32) that a finalize launch adds up in index
// order in double: bit-reproducible whatever the arrival order.  Producers: bn2_stats_kernel / bn2_bwd_reduce_kernel (one pass
// over the tensors) and, for 1x1 convolutions, the GEMM's own epilogue (gemm1x1.inc: one row per 128-pixel tile).
// Measured and dropped in round 3 (profiles/r03_exp_bn_accumulators.txt): per-layer fixed-point INTEGER accumulators fed by
// 64-bit atomics (order-independent, so still bit-reproducible) with the coefficients made in the consumer's prologue -- no
// finalize launches.  Device-scope atomics execute at the memory side: ~80 ns per add to one address, so 128 producers per
// replica added 10-19 us to every reduction, and the consumers' prologue (64 dependent 8-byte loads per thread) 40-90 us.
#ifndef RED_U
#define RED_U 4
#endif
// per-workgroup partial sums over rows: partial[block][0][c] = sum z, partial[block][1][c] = sum z^2   (one pass)
__global__ __launch_bounds__(256) void bn2_stats_kernel(const bf16_t* __restrict__ z, int64_t rows, int C, float* __restrict__ partial) {
  __shared__ float red[2][256][8];
  const int c8n = C >> 3;                                   // 16-byte lanes per row
  const int tpr = c8n < 256 ? c8n : 256;                    // threads working on one row
  const int rpi = 256 / tpr;                                // rows per iteration
  const int cl = threadIdx.x % tpr, rl = threadIdx.x / tpr;
  for (int c0 = cl; c0 < c8n; c0 += tpr) {                  // C > 2048 would loop; ResNet-50 tops out at 2048 = 256 lanes
    float a[8], b[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { a[e] = 0.f; b[e] = 0.f; }
    // RED_U rows in flight per thread (these reductions are load latency x memory-level parallelism: one 16-byte load per iteration
    // read 2.7 TB/s); rows past the end re-read the last row with weight 0; the order of the additions is unchanged
    const int64_t rstride = (int64_t)gridDim.x * rpi;
    for (int64_t r0 = (int64_t)blockIdx.x * rpi + rl; r0 < rows; r0 += RED_U * rstride) {
      F8 v[RED_U];
      float m[RED_U];
#pragma unroll
      for (int u = 0; u < RED_U; ++u) {
        const int64_t r = r0 + u * rstride;
        v[u] = ld8(z + (r < rows ? r : rows - 1) * C + c0 * 8);
        m[u] = r < rows ? 1.f : 0.f;
      }
#pragma unroll
      for (int u = 0; u < RED_U; ++u)
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float x = v[u].v[e] * m[u]; a[e] += x; b[e] = __builtin_fmaf(x, x, b[e]); }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { red[0][threadIdx.x][e] = a[e]; red[1][threadIdx.x][e] = b[e]; }
    __syncthreads();
    if (rl == 0) {
      for (int k = 1; k < rpi; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) { a[e] += red[0][k * tpr + cl][e]; b[e] += red[1][k * tpr + cl][e]; }
      float* p0 = partial + (int64_t)blockIdx.x * 2 * C + c0 * 8;
#pragma unroll
      for (int e = 0; e < 8; ++e) { p0[e] = a[e]; p0[C + e] = b[e]; }
    }
    __syncthreads();
  }
}

// (mean / variance / coefficients from the partial rows: bn_stat_finalize_onepass_kernel, train_core_kernels.inc)
// eval mode: scale / shift from the running statistics
__global__ void bn2_eval_coef_kernel(const float* gamma, const float* beta, const float* rm, const float* rv, float* scale,
                                     float* shift, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double s = (double)gamma[c] / sqrt((double)rv[c] + (double)BN_EPS);
  scale[c] = (float)s;
  shift[c] = (float)((double)beta[c] - (double)rm[c] * s);
}

// y = [relu]( z*scale + shift [+ res] ).  C/8 divides 256 (C = 64 ... 2048), so a thread meets the SAME 8 channels in every
// grid-stride iteration: the coefficients are loaded once, the loop moves only the payload.
__global__ __launch_bounds__(256) void bn2_apply_kernel(const bf16_t* __restrict__ z, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, const bf16_t* __restrict__ res,
                                                        bf16_t* __restrict__ y, int64_t n8, int C, int relu, uint8_t* __restrict__ bits = nullptr) {
  const int c8n = C >> 3;
  const int c0 = (int)(threadIdx.x % c8n) * 8;
  const float4 s0 = *reinterpret_cast<const float4*>(scale + c0), s1 = *reinterpret_cast<const float4*>(scale + c0 + 4);
  const float4 h0 = *reinterpret_cast<const float4*>(shift + c0), h1 = *reinterpret_cast<const float4*>(shift + c0 + 4);
  const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w}, sh[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    F8 v = ld8(z + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) v.v[e] = __builtin_fmaf(v.v[e], sc[e], sh[e]);
    if (res) {
      const F8 r = ld8(res + i * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) v.v[e] += r.v[e];
    }
    if (relu) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v.v[e] = fmaxf(v.v[e], 0.f);
    }
    st8_bits(y + i * 8, v, bits ? bits + i : nullptr);
  }
}

// The join of a block with a downsample branch: y = relu( bn(z) + bf16( bn_ds(z2) ) ) in one pass -- the branch's normalised map (rounded to
// bf16 exactly where bn2_apply_kernel would have stored it) is made on the fly instead of written by one launch and read back by this one.
__global__ __launch_bounds__(256) void bn2_apply_join_kernel(const bf16_t* __restrict__ z, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, const bf16_t* __restrict__ z2,
                                                             const float* __restrict__ scale2, const float* __restrict__ shift2,
                                                             bf16_t* __restrict__ y, int64_t n8, int C, uint8_t* __restrict__ bits = nullptr) {
  const int c8n = C >> 3;
  const int c0 = (int)(threadIdx.x % c8n) * 8;
  float sc[8], sh[8], s2[8], h2[8];
  {
    const float4* q[4] = {reinterpret_cast<const float4*>(scale + c0), reinterpret_cast<const float4*>(shift + c0),
                          reinterpret_cast<const float4*>(scale2 + c0), reinterpret_cast<const float4*>(shift2 + c0)};
    float* d[4] = {sc, sh, s2, h2};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 lo = q[i][0], hi = q[i][1];
      d[i][0] = lo.x; d[i][1] = lo.y; d[i][2] = lo.z; d[i][3] = lo.w; d[i][4] = hi.x; d[i][5] = hi.y; d[i][6] = hi.z; d[i][7] = hi.w;
    }
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const F8 v = ld8(z + i * 8), w = ld8(z2 + i * 8);
    F8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float r = bf16_bits_to_f32(f32_to_bf16(__builtin_fmaf(w.v[e], s2[e], h2[e])));
      o.v[e] = fmaxf(__builtin_fmaf(v.v[e], sc[e], sh[e]) + r, 0.f);
    }
    st8_bits(y + i * 8, o, bits ? bits + i : nullptr);
  }
}

// partial[block][0][c] = sum g, partial[block][1][c] = sum g*xhat;  g = dy * (y > 0 if relu), xhat = (z - mean)*invstd.
// relu == 2: the ReLU pattern is recomputed from z (y = relu(fma(z, scale, shift)) without an identity term: y > 0 <=> the same fma > 0),
// which saves reading y -- a quarter of this kernel's traffic -- for two BNs out of three.  relu == 0: the BN has no ReLU (downsample
// branch), or dy arrives already masked: the dgrad GEMM that produced it applied this block's ReLU in its epilogue (gemm1x1.inc).
__global__ __launch_bounds__(256) void bn2_bwd_reduce_kernel(const bf16_t* __restrict__ z, const bf16_t* __restrict__ dy,
                                                             const bf16_t* __restrict__ y, const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, int64_t rows, int C, int relu,
                                                             float* __restrict__ partial) {
  __shared__ float red[2][256][8];
  const int c8n = C >> 3;
  const int tpr = c8n < 256 ? c8n : 256;
  const int rpi = 256 / tpr;
  const int cl = threadIdx.x % tpr, rl = threadIdx.x / tpr;
  for (int c0 = cl; c0 < c8n; c0 += tpr) {
    float a[8], b[8], mu[8], is[8], sc[8], sh[8];
    {
      const float4* q[4] = {reinterpret_cast<const float4*>(mean + c0 * 8), reinterpret_cast<const float4*>(invstd + c0 * 8),
                            reinterpret_cast<const float4*>(scale + c0 * 8), reinterpret_cast<const float4*>(shift + c0 * 8)};
      float* d[4] = {mu, is, sc, sh};
#pragma unroll
      for (int i = 0; i < 4; ++i) {   // unconditional 16-byte loads (see bn2_bwd_apply_kernel)
        const float4 lo = q[i][0], hi = q[i][1];
        d[i][0] = lo.x; d[i][1] = lo.y; d[i][2] = lo.z; d[i][3] = lo.w; d[i][4] = hi.x; d[i][5] = hi.y; d[i][6] = hi.z; d[i][7] = hi.w;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) { a[e] = 0.f; b[e] = 0.f; }
    }
    const int64_t rstride = (int64_t)gridDim.x * rpi;
    for (int64_t r0 = (int64_t)blockIdx.x * rpi + rl; r0 < rows; r0 += RED_U * rstride) {   // RED_U rows in flight (bn2_stats_kernel)
      F8 v[RED_U], g[RED_U], yy[RED_U];
      float m[RED_U];
#pragma unroll
      for (int u = 0; u < RED_U; ++u) {
        const int64_t r = r0 + u * rstride, rr = r < rows ? r : rows - 1;
        v[u] = ld8(z + rr * C + c0 * 8);
        g[u] = ld8(dy + rr * C + c0 * 8);
        if (relu == 1) yy[u] = ld8(y + rr * C + c0 * 8);   // kernel-uniform
        m[u] = r < rows ? 1.f : 0.f;
      }
#pragma unroll
      for (int u = 0; u < RED_U; ++u) {
        if (relu == 1) {
#pragma unroll
          for (int e = 0; e < 8; ++e) g[u].v[e] = yy[u].v[e] > 0.f ? g[u].v[e] : 0.f;
        } else if (relu == 2) {
#pragma unroll
          for (int e = 0; e < 8; ++e) g[u].v[e] = __builtin_fmaf(v[u].v[e], sc[e], sh[e]) > 0.f ? g[u].v[e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float gg = g[u].v[e] * m[u]; a[e] += gg; b[e] = __builtin_fmaf(gg, (v[u].v[e] - mu[e]) * is[e], b[e]); }
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { red[0][threadIdx.x][e] = a[e]; red[1][threadIdx.x][e] = b[e]; }
    __syncthreads();
    if (rl == 0) {
      for (int k = 1; k < rpi; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) { a[e] += red[0][k * tpr + cl][e]; b[e] += red[1][k * tpr + cl][e]; }
      float* p0 = partial + (int64_t)blockIdx.x * 2 * C + c0 * 8;
#pragma unroll
      for (int e = 0; e < 8; ++e) { p0[e] = a[e]; p0[C + e] = b[e]; }
    }
    __syncthreads();
  }
}

// g = dy*(y>0 if relu);  dz = k0*g + k1*z + k2;  optionally g_out = g (the gradient that also flows down the identity branch).
// Coefficients hoisted as in bn2_apply_kernel (24 scalar loads per 8 elements otherwise: the vector-memory pipe, not HBM, set the pace).
__global__ __launch_bounds__(256) void bn2_bwd_apply_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ y,
                                                            const bf16_t* __restrict__ z, const float* __restrict__ k0,
                                                            const float* __restrict__ k1, const float* __restrict__ k2,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            bf16_t* __restrict__ dz, bf16_t* __restrict__ g_out, int64_t n8, int C,
                                                            int relu) {
  const int c8n = C >> 3;
  const int c0 = (int)(threadIdx.x % c8n) * 8;
  // unconditional 16-byte loads: a per-element "load only if relu == 2" makes hipcc branch around every load and wait for each
  float a[8], b[8], c[8], sc[8], sh[8];
  {
    const float4* q[5] = {reinterpret_cast<const float4*>(k0 + c0), reinterpret_cast<const float4*>(k1 + c0), reinterpret_cast<const float4*>(k2 + c0),
                          reinterpret_cast<const float4*>(scale + c0), reinterpret_cast<const float4*>(shift + c0)};
    float* d[5] = {a, b, c, sc, sh};
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const float4 lo = q[i][0], hi = q[i][1];
      d[i][0] = lo.x; d[i][1] = lo.y; d[i][2] = lo.z; d[i][3] = lo.w; d[i][4] = hi.x; d[i][5] = hi.y; d[i][6] = hi.z; d[i][7] = hi.w;
    }
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    F8 g = ld8(dy + i * 8);
    const F8 v = ld8(z + i * 8);
    if (relu == 1) {
      const F8 yy = ld8(y + i * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) g.v[e] = yy.v[e] > 0.f ? g.v[e] : 0.f;
    } else if (relu == 2) {   // pattern from z (see bn2_bwd_reduce_kernel)
#pragma unroll
      for (int e = 0; e < 8; ++e) g.v[e] = __builtin_fmaf(v.v[e], sc[e], sh[e]) > 0.f ? g.v[e] : 0.f;
    }
    F8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o.v[e] = __builtin_fmaf(a[e], g.v[e], __builtin_fmaf(b[e], v.v[e], c[e]));
    st8(dz + i * 8, o);
    if (g_out) st8(g_out + i * 8, g);
  }
}

// dx[b][2i][2j][:] += t[b][i][j][:]
__global__ __launch_bounds__(256) void upsample2_add_bf16_kernel(const bf16_t* __restrict__ t, bf16_t* __restrict__ dx, int B, int Ho,
                                                                 int Wo, int Hi, int Wi, int C) {
  const int c8n = C >> 3;
  const int64_t n8 = (int64_t)B * Ho * Wo * c8n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const int cl = (int)(i % c8n);
    int64_t r = i / c8n;
    const int x = (int)(r % Wo); r /= Wo;
    const int y = (int)(r % Ho);
    const int b = (int)(r / Ho);
    bf16_t* d = dx + ((((int64_t)b * Hi + 2 * y) * Wi + 2 * x) * C + cl * 8);
    F8 o = ld8(d);
    const F8 v = ld8(t + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) o.v[e] += v.v[e];
    st8(d, o);
  }
}

// ---------------- max pool 3x3/2 pad 1 (forward records the first-maximum position), average pool, fc ----------------
// (the engine runs the stem's pool fused with its BN -- bn2_apply_pool_kernel / bn2_pool_bwd_* below; the stand-alone pair stays as the
//  reference point of the per-kernel tests: dh_debug_maxpool2_bf16)
__global__ __launch_bounds__(256) void maxpool2_fwd_idx_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                                               uint8_t* __restrict__ idx, int B, int Hi, int Wi, int C, int Ho, int Wo) {
  const int c8n = C >> 3;
  const int64_t n8 = (int64_t)B * Ho * Wo * c8n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const int cl = (int)(i % c8n);
    int64_t r = i / c8n;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    F8 m;
    int w[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { m.v[e] = -INFINITY; w[e] = 0; }
#pragma unroll
    for (int dyy = 0; dyy < 3; ++dyy) {
      const int yy = 2 * oy + dyy - 1;
      if (yy < 0 || yy >= Hi) continue;
#pragma unroll
      for (int dxx = 0; dxx < 3; ++dxx) {
        const int xx = 2 * ox + dxx - 1;
        if (xx < 0 || xx >= Wi) continue;
        const F8 v = ld8(x + ((((int64_t)b * Hi + yy) * Wi + xx) * C + cl * 8));
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (v.v[e] > m.v[e]) { m.v[e] = v.v[e]; w[e] = dyy * 3 + dxx; }   // strict: the earlier element keeps a tie (torch)
      }
    }
    st8(y + i * 8, m);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) { lo |= (uint32_t)w[e] << (8 * e); hi |= (uint32_t)w[4 + e] << (8 * e); }
    *reinterpret_cast<uint2*>(idx + i * 8) = make_uint2(lo, hi);
  }
}
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const uint8_t* __restrict__ idx, const bf16_t* __restrict__ dy,
                                                           bf16_t* __restrict__ dx, int B, int Hi, int Wi, int C, int Ho, int Wo) {
  const int c8n = C >> 3;
  const int64_t n8 = (int64_t)B * Hi * Wi * c8n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const int cl = (int)(i % c8n);
    int64_t r = i / c8n;
    const int ix = (int)(r % Wi); r /= Wi;
    const int iy = (int)(r % Hi);
    const int b = (int)(r / Hi);
    F8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o.v[e] = 0.f;
    for (int oy = iy / 2; oy <= (iy + 1) / 2; ++oy) {
      if (oy >= Ho) continue;
      for (int ox = ix / 2; ox <= (ix + 1) / 2; ++ox) {
        if (ox >= Wo) continue;
        const int me = (iy - (2 * oy - 1)) * 3 + (ix - (2 * ox - 1));
        const int64_t e8 = (((int64_t)b * Ho + oy) * Wo + ox) * c8n + cl;
        const uint2 w = *reinterpret_cast<const uint2*>(idx + e8 * 8);
        const F8 g = ld8(dy + e8 * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if ((int)((w.x >> (8 * e)) & 0xFF) == me) o.v[e] += g.v[e];
          if ((int)((w.y >> (8 * e)) & 0xFF) == me) o.v[4 + e] += g.v[4 + e];
        }
      }
    }
    st8(dx + i * 8, o);
  }
}
// ---- the stem's tail in one pass each way (round 3): BN + ReLU + maxpool forward, maxpool + ReLU + BN backward ----
// Forward: pooled = maxpool3x3/2( bf16( relu( fma(z, scale, shift) ) ) ) and the first-maximum positions, straight from the raw conv output
// Z: the normalised 112 x 112 map is never written (103 MB written and read back per 64 x 224^2 step).  Every value is rounded to bf16
// before the comparison, so maxima and positions are those of the unfused pair bn2_apply_kernel + maxpool2_fwd_idx_kernel.
__global__ __launch_bounds__(256) void bn2_apply_pool_kernel(const bf16_t* __restrict__ z, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, bf16_t* __restrict__ y,
                                                             uint8_t* __restrict__ idx, int B, int Hi, int Wi, int C, int Ho, int Wo) {
  const int c8n = C >> 3;
  const int c0 = (int)(threadIdx.x % c8n) * 8;   // 256 % c8n == 0: a thread keeps its 8 channels through the grid-stride loop
  const float4 s0 = *reinterpret_cast<const float4*>(scale + c0), s1 = *reinterpret_cast<const float4*>(scale + c0 + 4);
  const float4 h0 = *reinterpret_cast<const float4*>(shift + c0), h1 = *reinterpret_cast<const float4*>(shift + c0 + 4);
  const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w}, sh[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
  const int64_t n8 = (int64_t)B * Ho * Wo * c8n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const int cl = (int)(i % c8n);
    int64_t r = i / c8n;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    F8 m;
    int w[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { m.v[e] = -INFINITY; w[e] = 0; }
#pragma unroll
    for (int dyy = 0; dyy < 3; ++dyy) {
      const int yy = 2 * oy + dyy - 1;
      if (yy < 0 || yy >= Hi) continue;
#pragma unroll
      for (int dxx = 0; dxx < 3; ++dxx) {
        const int xx = 2 * ox + dxx - 1;
        if (xx < 0 || xx >= Wi) continue;
        const F8 v = ld8(z + ((((int64_t)b * Hi + yy) * Wi + xx) * C + cl * 8));
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float a = bf16_bits_to_f32(f32_to_bf16(fmaxf(__builtin_fmaf(v.v[e], sc[e], sh[e]), 0.f)));
          if (a > m.v[e]) { m.v[e] = a; w[e] = dyy * 3 + dxx; }   // strict: the earlier element keeps a tie (torch)
        }
      }
    }
    st8(y + i * 8, m);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) { lo |= (uint32_t)w[e] << (8 * e); hi |= (uint32_t)w[4 + e] << (8 * e); }
    *reinterpret_cast<uint2*>(idx + i * 8) = make_uint2(lo, hi);
  }
}

// Gradient of the 3x3/2 (pad 1) maxpool at the 2 x 2 block of input pixels (2a + py, 2q + px), 8 channels each: the block lies under the four
// windows (a + wy, q + wx) and every window is loaded ONCE for the block (positions + pooled gradient: 24 bytes), 2.25x fewer gather loads
// than pixel by pixel.  Window (wy, wx) reaches pixel (py, px) at its position (py + 1 - 2 wy, px + 1 - 2 wx) when both are >= 0.  float32
// sums of at most four terms (maxpool2_bwd_kernel rounds the same sums to bf16 on their way to HBM).  g[2 * py + px].
struct PoolGrad4 { F8 g[4]; };
__device__ __forceinline__ PoolGrad4 pool_grad_2x2(const uint8_t* __restrict__ idx, const bf16_t* __restrict__ dpool, int b, int a, int q, int cl,
                                                   int c8n, int Ho, int Wo) {
  PoolGrad4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) o.g[k].v[e] = 0.f;
#pragma unroll
  for (int wy = 0; wy < 2; ++wy)
#pragma unroll
    for (int wx = 0; wx < 2; ++wx) {
      const int oy = a + wy, ox = q + wx;
      if (oy >= Ho || ox >= Wo) continue;
      const int64_t e8 = (((int64_t)b * Ho + oy) * Wo + ox) * c8n + cl;
      const uint2 w = *reinterpret_cast<const uint2*>(idx + e8 * 8);
      const F8 g = ld8(dpool + e8 * 8);
#pragma unroll
      for (int py = wy; py < 2; ++py)
#pragma unroll
        for (int px = wx; px < 2; ++px) {
          const int me = (py + 1 - 2 * wy) * 3 + (px + 1 - 2 * wx);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if ((int)((w.x >> (8 * e)) & 0xFF) == me) o.g[2 * py + px].v[e] += g.v[e];
            if ((int)((w.y >> (8 * e)) & 0xFF) == me) o.g[2 * py + px].v[4 + e] += g.v[4 + e];
          }
        }
    }
  return o;
}

// bn2_bwd_reduce_kernel (relu == 2) with dy = the maxpool's gradient gathered on the fly; a "row" is a 2 x 2 pixel block of Z
__global__ __launch_bounds__(256) void bn2_pool_bwd_reduce_kernel(const bf16_t* __restrict__ z, const bf16_t* __restrict__ dpool,
                                                                  const uint8_t* __restrict__ idx, const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd, const float* __restrict__ scale,
                                                                  const float* __restrict__ shift, int B, int Hi, int Wi, int C, int Ho, int Wo,
                                                                  float* __restrict__ partial) {
  __shared__ float red[2][256][8];
  const int c8n = C >> 3;          // <= 256 (the stem has 64 channels)
  const int rpi = 256 / c8n;
  const int cl = threadIdx.x % c8n, rl = threadIdx.x / c8n;
  const int Hb = (Hi + 1) >> 1, Wb = (Wi + 1) >> 1;
  const int64_t rows = (int64_t)B * Hb * Wb;
  float a[8], b[8], mu[8], is[8], sc[8], sh[8];
  {
    const float4* q[4] = {reinterpret_cast<const float4*>(mean + cl * 8), reinterpret_cast<const float4*>(invstd + cl * 8),
                          reinterpret_cast<const float4*>(scale + cl * 8), reinterpret_cast<const float4*>(shift + cl * 8)};
    float* d[4] = {mu, is, sc, sh};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 lo = q[i][0], hi = q[i][1];
      d[i][0] = lo.x; d[i][1] = lo.y; d[i][2] = lo.z; d[i][3] = lo.w; d[i][4] = hi.x; d[i][5] = hi.y; d[i][6] = hi.z; d[i][7] = hi.w;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { a[e] = 0.f; b[e] = 0.f; }
  }
  const int64_t rstride = (int64_t)gridDim.x * rpi;
  for (int64_t r = (int64_t)blockIdx.x * rpi + rl; r < rows; r += rstride) {
    const int qx = (int)(r % Wb);
    const int64_t t = r / Wb;
    const int ay = (int)(t % Hb), bb = (int)(t / Hb);
    F8 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // pixels past an odd map's edge re-read the block's first pixel with weight 0
      const int iy = 2 * ay + (k >> 1), ix = 2 * qx + (k & 1);
      const bool ok = iy < Hi && ix < Wi;
      v[k] = ld8(z + ((((int64_t)bb * Hi + (ok ? iy : 2 * ay)) * Wi + (ok ? ix : 2 * qx)) * C + cl * 8));
    }
    const PoolGrad4 pg = pool_grad_2x2(idx, dpool, bb, ay, qx, cl, c8n, Ho, Wo);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = 2 * ay + (k >> 1) < Hi && 2 * qx + (k & 1) < Wi;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float gg = (ok && __builtin_fmaf(v[k].v[e], sc[e], sh[e]) > 0.f) ? pg.g[k].v[e] : 0.f;
        a[e] += gg;
        b[e] = __builtin_fmaf(gg, (v[k].v[e] - mu[e]) * is[e], b[e]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) { red[0][threadIdx.x][e] = a[e]; red[1][threadIdx.x][e] = b[e]; }
  __syncthreads();
  if (rl == 0) {
    for (int k = 1; k < rpi; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) { a[e] += red[0][k * c8n + cl][e]; b[e] += red[1][k * c8n + cl][e]; }
    float* p0 = partial + (int64_t)blockIdx.x * 2 * C + cl * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) { p0[e] = a[e]; p0[C + e] = b[e]; }
  }
}

// bn2_bwd_apply_kernel (relu == 2) with dy gathered as above: dz = k0*g + k1*z + k2, one 2 x 2 pixel block per thread and iteration
__global__ __launch_bounds__(256) void bn2_pool_bwd_apply_kernel(const bf16_t* __restrict__ z, const bf16_t* __restrict__ dpool,
                                                                 const uint8_t* __restrict__ idx, const float* __restrict__ k0,
                                                                 const float* __restrict__ k1, const float* __restrict__ k2,
                                                                 const float* __restrict__ scale, const float* __restrict__ shift,
                                                                 bf16_t* __restrict__ dz, int B, int Hi, int Wi, int C, int Ho, int Wo) {
  const int c8n = C >> 3;
  const int c0 = (int)(threadIdx.x % c8n) * 8;
  float a[8], b[8], c[8], sc[8], sh[8];
  {
    const float4* q[5] = {reinterpret_cast<const float4*>(k0 + c0), reinterpret_cast<const float4*>(k1 + c0), reinterpret_cast<const float4*>(k2 + c0),
                          reinterpret_cast<const float4*>(scale + c0), reinterpret_cast<const float4*>(shift + c0)};
    float* d[5] = {a, b, c, sc, sh};
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const float4 lo = q[i][0], hi = q[i][1];
      d[i][0] = lo.x; d[i][1] = lo.y; d[i][2] = lo.z; d[i][3] = lo.w; d[i][4] = hi.x; d[i][5] = hi.y; d[i][6] = hi.z; d[i][7] = hi.w;
    }
  }
  const int Hb = (Hi + 1) >> 1, Wb = (Wi + 1) >> 1;
  const int64_t n8 = (int64_t)B * Hb * Wb * c8n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const int cl = (int)(i % c8n);
    int64_t r = i / c8n;
    const int qx = (int)(r % Wb); r /= Wb;
    const int ay = (int)(r % Hb);
    const int bb = (int)(r / Hb);
    F8 v[4];
    int64_t at[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int iy = 2 * ay + (k >> 1), ix = 2 * qx + (k & 1);
      ok[k] = iy < Hi && ix < Wi;
      at[k] = (((int64_t)bb * Hi + (ok[k] ? iy : 2 * ay)) * Wi + (ok[k] ? ix : 2 * qx)) * C + cl * 8;
      v[k] = ld8(z + at[k]);
    }
    const PoolGrad4 pg = pool_grad_2x2(idx, dpool, bb, ay, qx, cl, c8n, Ho, Wo);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      F8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float gg = __builtin_fmaf(v[k].v[e], sc[e], sh[e]) > 0.f ? pg.g[k].v[e] : 0.f;
        o.v[e] = __builtin_fmaf(a[e], gg, __builtin_fmaf(b[e], v[k].v[e], c[e]));
      }
      if (ok[k]) st8(dz + at[k], o);
    }
  }
}

__global__ __launch_bounds__(256) void avgpool2_kernel(const bf16_t* __restrict__ x, int HW, int C, float* __restrict__ pooled) {
  const int b = blockIdx.x;
  for (int c0 = threadIdx.x; c0 < (C >> 3); c0 += 256) {
    float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int q = 0; q < HW; ++q) {
      const F8 v = ld8(x + (((int64_t)b * HW + q) * C + c0 * 8));
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += v.v[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) pooled[(int64_t)b * C + c0 * 8 + e] = s[e] / (float)HW;
  }
}
// dX[b][q][c] = (sum_k dl[b][k]*w[k][c]) / HW
__global__ __launch_bounds__(256) void avgpool_fc_dgrad2_kernel(const float* __restrict__ dl, const float* __restrict__ w, int HW, int C,
                                                                int n_cls, bf16_t* __restrict__ dx) {
  const int b = blockIdx.x;
  for (int c0 = threadIdx.x; c0 < (C >> 3); c0 += 256) {
    F8 s;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = 0.f;
      for (int k = 0; k < n_cls; ++k) t = __builtin_fmaf(dl[b * n_cls + k], w[k * C + c0 * 8 + e], t);
      s.v[e] = t / (float)HW;
    }
    for (int q = 0; q < HW; ++q) st8(dx + (((int64_t)b * HW + q) * C + c0 * 8), s);
  }
}
// ---- stem weight gradient on the bf16 matrix pipe (round 3) ----
// dW[co][e] = sum_px dZ[px][co] * x[b, c, 2oy+kh-3, 2ox+kw-3], e = (c*7+kh)*7+kw (147, padded to 160 = 5 column tiles), as stem_wgrad_kernel
// (train_kernels.inc) does it on the float32 MFMA: K = output pixels, 2 per `32x32x2_f32` there, 16 per `v_mfma_f32_32x32x16_bf16` here (the
// matrix work of a 64 x 224^2 step drops from 105 us to 7 us; what remains is the row staging).  Per output row the 21 input-row
// segments (bf16, the rounding the forward stem applies to x as well) and the dZ row sit in LDS in their natural order; a lane's
// fragment is 8 consecutive pixels of ONE dZ channel (stride 128 B) or of ONE (c, kh, kw) column of x (stride 4 B): eight 2-byte LDS
// reads each, packed in registers -- cheaper than transposed or parity-split staging images, and the LDS has the cycles.
// 8 waves = 4 k-step groups x 2 cout halves; slabs and the fixed-order reduce as in the float32 kernel (bit-reproducible).
__global__ __launch_bounds__(SWG_T, 4) void stem_wgrad_bf16_kernel(const bf16_t* __restrict__ dz, const float* __restrict__ x,
                                                                   float* __restrict__ slabs, int B, int P, int Ho, int Wo,
                                                                   int rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) char swb[];
  const int Wx = P + 6;                                        // staged row: columns -3 .. P+2
  const int xs_elems = (21 * Wx + 7) & ~7;
  uint16_t* xs = reinterpret_cast<uint16_t*>(swb);             // [21 = (c, kh)][Wx] bf16
  uint16_t* dzs = xs + xs_elems;                               // [Wo][64] bf16 (+ one zero pixel block for the tail k-step)
  float* tile = reinterpret_cast<float*>(swb);                 // reused at the end: [64][160]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pg = wave & 3, mt = wave >> 2;                     // k-step group, cout half
  const int kg = lane >> 5, cl = lane & 31;
  int eoff[5];
  bool elive[5];
#pragma unroll
  for (int nt = 0; nt < 5; ++nt) {
    const int e = nt * 32 + cl;
    const int kw = e % 7, kh = (e / 7) % 7, c = e / 49;
    elive[nt] = e < 147;
    eoff[nt] = elive[nt] ? (c * 7 + kh) * Wx + kw : 0;
  }
  (void)elive;
  f32x16 acc[5];
#pragma unroll
  for (int j = 0; j < 5; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
  const int total_rows = B * Ho;
  const int row0 = blockIdx.x * rows_per_block, row1 = min(row0 + rows_per_block, total_rows);
  const int ndz = Wo * 8;                                      // 16-byte pieces of a dZ row
  const int nks = (Wo + 15) >> 4;
  for (int row = row0; row < row1; ++row) {
    const int b = row / Ho, oy = row % Ho;
    __syncthreads();                                           // previous row consumed
    if (tid < Wx) {                                            // one staged column per thread: 21 loads in flight, then 21 stores
      float v[21];
#pragma unroll
      for (int r = 0; r < 21; ++r) {
        const int c = r / 7, kh = r % 7;
        const int iy = 2 * oy + kh - 3;
        v[r] = 0.f;
        if (iy >= 0 && iy < P && tid >= 3 && tid < P + 3) v[r] = x[(((int64_t)b * 3 + c) * P + iy) * P + tid - 3];
      }
#pragma unroll
      for (int r = 0; r < 21; ++r) xs[r * Wx + tid] = (uint16_t)f32_to_bf16(v[r]);
    }
    {
      const uint4* dzr = reinterpret_cast<const uint4*>(dz + (int64_t)row * Wo * 64);
      uint4 d[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) d[u] = dzr[min(tid + SWG_T * u, ndz - 1)];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int i = tid + SWG_T * u;
        if (i < ndz) reinterpret_cast<uint4*>(dzs)[i] = d[u];
      }
    }
    __syncthreads();
    for (int ks = pg; ks < nks; ks += 4) {
      const int ox0 = 16 * ks + 8 * kg;                        // this lane's 8 pixels
      // unconditional reads (Wo % 16 == 0: no pixel tail; the dead columns e >= 147 of the last tile read column 0 and are never
      // looked at by the reduce): a branch around every 2-byte read had serialised 96 LDS round trips per k-step
      const uint16_t* ap = dzs + ox0 * 64 + mt * 32 + cl;
      uint32_t aw[4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) aw[jj] = (uint32_t)ap[(2 * jj) * 64] | ((uint32_t)ap[(2 * jj + 1) * 64] << 16);
      const uint4 a = make_uint4(aw[0], aw[1], aw[2], aw[3]);
#pragma unroll
      for (int nt = 0; nt < 5; ++nt) {   // one column tile at a time: 4 operand registers live, not 20
        const uint16_t* bp = xs + eoff[nt] + 2 * ox0;
        uint32_t bw[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) bw[jj] = (uint32_t)bp[4 * jj] | ((uint32_t)bp[4 * jj + 2] << 16);
        mma_frag<__bf16>(acc[nt], a, make_uint4(bw[0], bw[1], bw[2], bw[3]));
      }
    }
  }
  for (int w = 0; w < 4; ++w) {   // fixed-order combine of the four k-step groups (no float atomics: reproducible)
    __syncthreads();
    if (pg == w) {
#pragma unroll
      for (int nt = 0; nt < 5; ++nt)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          float* e = &tile[(mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * kg) * 160 + nt * 32 + cl];
          *e = w == 0 ? acc[nt][q] : *e + acc[nt][q];
        }
    }
  }
  __syncthreads();
  for (int i = tid; i < 64 * 160; i += SWG_T) slabs[(int64_t)blockIdx.x * (64 * 160) + i] = tile[i];
}

// gradient wire format of the data-parallel exchange (optional): float32 arena slice -> bf16 (round to nearest even) and back with the
// 1 / world factor; 4 elements per thread (arena offsets and counts are multiples of 4)
// A NaN gradient must reach every rank as a NaN: the rounding add of f32_to_bf16 carries out of a NaN's mantissa (0x7F80xxxx with a small
// payload came out as infinity, 0x7FFF8000 and above as a signed zero), so NaNs are truncated and made quiet here.  Finite values and
// infinities round as everywhere else (to nearest even; past the largest bf16 to infinity).
__device__ __forceinline__ uint32_t f32_to_bf16_wire(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x7FFFFFFFu) > 0x7F800000u ? ((u >> 16) | 0x0040u) : f32_to_bf16(f);
}
__global__ __launch_bounds__(256) void grad_pack_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(src)[i];
    reinterpret_cast<uint2*>(dst)[i] = make_uint2(f32_to_bf16_wire(v.x) | (f32_to_bf16_wire(v.y) << 16),
                                                  f32_to_bf16_wire(v.z) | (f32_to_bf16_wire(v.w) << 16));
  }
}
__global__ __launch_bounds__(256) void grad_unpack_bf16_kernel(const bf16_t* __restrict__ src, float* __restrict__ dst, int64_t n4, float scale) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const uint2 u = reinterpret_cast<const uint2*>(src)[i];
    reinterpret_cast<float4*>(dst)[i] = make_float4(bf16_bits_to_f32(u.x & 0xFFFFu) * scale, bf16_bits_to_f32(u.x >> 16) * scale,
                                                    bf16_bits_to_f32(u.y & 0xFFFFu) * scale, bf16_bits_to_f32(u.y >> 16) * scale);
  }
}
__global__ __launch_bounds__(256) void bf16_to_f32_kernel(const bf16_t* __restrict__ in, float* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = bf16_bits_to_f32(in[i]);
}

// (the 1x1 convolutions' NT GEMM lives in gemm1x1.inc)

// ---------------- weight gradient on bf16 MFMA: dW[co][ci][tap] = sum_px dZ[px][co] * X[px @ tap][ci] ----------------
// One workgroup = 64 couts x 64 cins x a slab of "steps"; a step = R output rows of one image (R*Wo <= 64 pixels =
// 4 k-steps of 16).  Per step the dZ rows and the X window (3x3: with halo, zero outside the image; 1x1: exactly the
// strided pixels) are staged once in LDS (double-buffered, the next step's global loads in flight under the MFMAs).
// Both MFMA operands are indexed [k = pixel][m = channel] in LDS, i.e. k-strided: fragments are read with
// ds_read_b64_tr_b16 (4 pixels x 16 channels per 16-lane group, delivered channel-per-lane): lane l of a 32x32x16
// operand needs channel l & 31 and pixels 8 (l >> 5) .. +7 -> two transposed reads whose row addresses are supplied by
// lanes 4q + p of each group (q = pixel within the block of 4).  LDS rows are 128 B (64 channels); the two 64-byte halves
// of a row are swapped on rows with bit 1 set, so the four rows of a block hit four different bank groups.  The window's
// row pitch is a multiple of 4 pixels: a tap's row shift kh never changes that swap, so every (pixel, kw) address is
// computed ONCE per kernel and taps differ by an immediate offset.
// TAPS == 9: wave = (cout half, cin half, tap group {0-4 | 5-8}), every wave walks all k-steps, no exchange.
// TAPS == 1: wave = (cout half, cin half, k parity); the two parities are summed through LDS at the end.
// Partial 64x64xTAPS tiles go to slabs[slab] with plain stores; wgrad_reduce_kernel sums the slabs in a fixed order.
struct Wgrad2Params {
  const bf16_t* dz; const bf16_t* x; float* slabs;
  int B, Hi, Wi, Cin, Ho, Wo, Cout, STRIDE;
  int R, XR, XC;             // output rows per step; staged window rows / columns (XC a multiple of 4)
  int rb_per_img, total_steps, steps_per_slab;
  int win_bytes, buf_bytes;  // window bytes / stage buffer bytes (window + 64 dz rows)
  int tap_major;             // 3x3 slabs as [tap][cout][cin] (a lane's 32 cins are contiguous: 128-byte stores; wgrad_reduce_taps_kernel
                             // restores torch's [cout][cin][tap]); 0: write [cout][cin][tap] directly (single slab = the gradient)
};
constexpr int WG2_MAXX = 6;   // 16-byte window pieces per thread (512 threads): <= 384 window pixels

template <int TAPS>
__global__ __launch_bounds__(512, 2) void wgrad_bf16_kernel(const Wgrad2Params p) {
  extern __shared__ __attribute__((aligned(16))) char wl2[];
  constexpr int KS = TAPS == 9 ? 3 : 1, PAD = KS / 2;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mt = (wave >> 1) & 1, nt = wave & 1, sel = wave >> 2;   // sel: tap group (TAPS 9) / k parity (TAPS 1)
  const int cit = p.Cin >> 6, cot = p.Cout >> 6;
  int r_ = blockIdx.x;
  const int ct = r_ % cit; r_ /= cit;
  const int ot = r_ % cot; r_ /= cot;
  const int slab = r_;
  const int step0 = slab * p.steps_per_slab, step1 = min(step0 + p.steps_per_slab, p.total_steps);
  const int wst = KS == 3 ? 1 : p.STRIDE;   // window pixel -> source pixel stride (1x1: the window holds only the strided pixels)
  // ---- staging plan (window geometry is the same for every step)
  const int nx_items = p.XR * p.XC * 8;
  int x_wr[WG2_MAXX], x_wc[WG2_MAXX], x_dst[WG2_MAXX];
#pragma unroll
  for (int u = 0; u < WG2_MAXX; ++u) {
    const int i = tid + 512 * u, px = i >> 3, j = i & 7;
    x_wr[u] = i < nx_items ? px / p.XC : -(1 << 20);
    x_wc[u] = px % p.XC;
    x_dst[u] = px * 128 + ((((j >> 2) ^ ((px >> 1) & 1))) << 6) + (j & 3) * 16;
  }
  const int d_px = tid >> 3, d_j = tid & 7;   // dz: 64 pixels x 8 pieces = 512 threads exactly
  const int d_dst = p.win_bytes + d_px * 128 + ((((d_j >> 2) ^ ((d_px >> 1) & 1))) << 6) + (d_j & 3) * 16;
  uint4 xv[WG2_MAXX], dv;
  auto load_step = [&](int step) __attribute__((always_inline)) {
    const int b = step / p.rb_per_img, oy0 = (step % p.rb_per_img) * p.R;
    const int npix = min(p.R, p.Ho - oy0) * p.Wo;
#pragma unroll
    for (int u = 0; u < WG2_MAXX; ++u) {
      const int iy = oy0 * p.STRIDE - PAD + x_wr[u] * wst, ix = x_wc[u] * wst - PAD;
      xv[u] = make_uint4(0, 0, 0, 0);
      if (iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi)
        xv[u] = *reinterpret_cast<const uint4*>(p.x + ((((int64_t)b * p.Hi + iy) * p.Wi + ix) * p.Cin + ct * 64 + (tid & 7) * 8));
    }
    dv = make_uint4(0, 0, 0, 0);
    if (d_px < npix)
      dv = *reinterpret_cast<const uint4*>(p.dz + ((((int64_t)b * p.Ho + oy0) * p.Wo + d_px) * p.Cout + ot * 64 + d_j * 8));
  };
  auto store_step = [&](int buf) __attribute__((always_inline)) {
    char* base = wl2 + buf * p.buf_bytes;
#pragma unroll
    for (int u = 0; u < WG2_MAXX; ++u)
      if (tid + 512 * u < nx_items) *reinterpret_cast<uint4*>(base + x_dst[u]) = xv[u];
    *reinterpret_cast<uint4*>(base + d_dst) = dv;
  };
  // ---- fragment addresses: this lane supplies, in each transposed read, the address of pixel row q of its group's block
  const int q = (lane & 15) >> 2, pp = lane & 3, cb = (lane >> 4) & 1, hh = lane >> 5;
  const int col_bytes = 32 * cb + 8 * pp;
  constexpr int NKS = TAPS == 9 ? 4 : 2;             // k-steps this wave walks per step
  int a_addr[NKS][2];                                // dz rows      [k-step][first | second block of 4 pixels]
  int b_addr[NKS][2][KS];                            // window rows  [k-step][block][kw]
  const int maxpx = p.R * p.Wo - 1;
#pragma unroll
  for (int s = 0; s < NKS; ++s) {
    const int ks = TAPS == 9 ? s : 2 * s + sel;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const int px = 16 * ks + 8 * hh + 4 * blk + q;
      a_addr[s][blk] = p.win_bytes + px * 128 + ((mt ^ ((px >> 1) & 1)) << 6) + col_bytes;
      const int pc = min(px, maxpx);                // pixels past the step: dz row is zero, any valid window row will do
      const int wpx = KS == 3 ? (pc / p.Wo) * p.STRIDE * p.XC + (pc % p.Wo) * p.STRIDE : (pc / p.Wo) * p.XC + (pc % p.Wo);
#pragma unroll
      for (int kw = 0; kw < KS; ++kw) {
        const int row = wpx + kw;
        b_addr[s][blk][kw] = row * 128 + ((nt ^ ((row >> 1) & 1)) << 6) + col_bytes;
      }
    }
  }
  const int khoff = p.XC * 128;                      // byte shift of one tap row (XC % 4 == 0: preserves the half swap)
  typedef __attribute__((address_space(3))) v4s_t* lds_v4s;
  auto tr_read = [&](const char* base, int off) __attribute__((always_inline)) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(base + off));
  };
  auto frag_of = [&](v4s_t lo, v4s_t hi) __attribute__((always_inline)) {
    typedef short v8s_t __attribute__((ext_vector_type(8)));
    const v8s_t f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, f);
  };
  float* out = p.slabs + (int64_t)slab * p.Cout * p.Cin * TAPS;
  const int ci = ct * 64 + nt * 32 + (lane & 31);

  // the wave's role (tap group / k parity) as a compile-time constant: taps and their (kh, kw) fold into immediates
  auto body = [&](auto sel_c) __attribute__((always_inline)) {
    constexpr int SEL = decltype(sel_c)::value;
    constexpr int NT_ = TAPS == 9 ? (SEL ? 4 : 5) : 1;   // accumulator tiles of this wave
    constexpr int TAP0 = TAPS == 9 ? 5 * SEL : 0;
    f32x16 acc[NT_];
#pragma unroll
    for (int t = 0; t < NT_; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    if (step0 < step1) { load_step(step0); store_step(0); }
    __syncthreads();
    for (int step = step0; step < step1; ++step) {
      const int buf = (step - step0) & 1;
      const bool more = step + 1 < step1;
      if (more) load_step(step + 1);
      const char* base = wl2 + buf * p.buf_bytes;
      const int oy0 = (step % p.rb_per_img) * p.R;
      const int nks = (min(p.R, p.Ho - oy0) * p.Wo + 15) >> 4;   // live k-steps of this step (<= 4)
#pragma unroll
      for (int s = 0; s < NKS; ++s) {
        const int ks = TAPS == 9 ? s : 2 * s + SEL;
        if (ks < nks) {                                          // wave-uniform
          const bf16x8 a = frag_of(tr_read(base, a_addr[s][0]), tr_read(base, a_addr[s][1]));
#pragma unroll
          for (int t = 0; t < NT_; ++t) {
            constexpr int dummy = 0; (void)dummy;
            const int tap = TAP0 + t, kh = tap / 3, kw = tap % 3;   // compile-time after unrolling
            const bf16x8 b = frag_of(tr_read(base, b_addr[s][0][kw] + kh * khoff), tr_read(base, b_addr[s][1][kw] + kh * khoff));
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[t], 0, 0, 0);
          }
        }
      }
      if (more) store_step(buf ^ 1);
      __syncthreads();
    }
    // ---- output: D[co][ci] tiles; lane col = ci (lane & 31), register r -> co = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    if constexpr (TAPS == 9) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = ot * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        if (p.tap_major) {
#pragma unroll
          for (int t = 0; t < NT_; ++t) out[((int64_t)(TAP0 + t) * p.Cout + co) * p.Cin + ci] = acc[t][r];
        } else {
          float* o = out + ((int64_t)co * p.Cin + ci) * 9 + TAP0;
#pragma unroll
          for (int t = 0; t < NT_; ++t) o[t] = acc[t][r];
        }
      }
    } else {
      float* xch = reinterpret_cast<float*>(wl2) + (wave & 3) * (16 * 64);
      if constexpr (SEL == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) xch[r * 64 + lane] = acc[0][r];
      }
      __syncthreads();
      if constexpr (SEL == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = ot * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
          out[(int64_t)co * p.Cin + ci] = acc[0][r] + xch[r * 64 + lane];
        }
      }
    }
  };
  if (sel == 0) body(std::integral_constant<int, 0>{});
  else body(std::integral_constant<int, 1>{});
}


// ---------------- 1x1 weight gradient with four-quadrant workgroup tiles ----------------
// wgrad_bf16_kernel<1> re-reads X once per 64-cout tile and dZ once per 64-cin tile: at 32 FLOP per staged byte the 1x1 weight
// gradients of ResNet-50 move ~7.8 GB per step (4.6 TB/s: bandwidth-bound).  Here a workgroup owns FOUR 64 x 64 quadrants,
// MP x NP planes of 64 channels (cout x cin): 128 x 128 (MP = NP = 2) for the layers whose channel counts are multiples of 128,
// 64 x 256 (1, 4) / 256 x 64 (4, 1) for the 64-channel layers of stage 1 (round 3: their X / dZ re-reads fall from 4 to 1).
// 8 waves = 4 quadrants (MT = NT = 2: 8 transposed reads per 4 MFMAs) x 2 k-groups (k-steps kg, kg + 2 of the step's four);
// the two k-groups of a quadrant are summed through LDS at the end.  LDS image: per operand PLANES of 64 channels
// ([pixel][64 ch] rows of 128 B with the half swap of wgrad_bf16_kernel), so every address formula carries over.
template <int MP, int NP>
__global__ __launch_bounds__(512, 2) void wgrad1x1_quad_kernel(const Wgrad2Params p) {
  static_assert(MP * NP == 4, "four 64 x 64 quadrants per workgroup");
  extern __shared__ __attribute__((aligned(16))) char wl4[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = wave & 3, kg = wave >> 2;
  const int mq = NP == 1 ? quad : NP == 2 ? quad >> 1 : 0, nq = NP == 1 ? 0 : NP == 2 ? quad & 1 : quad;
  const int cit = p.Cin / (64 * NP), cot = p.Cout / (64 * MP);
  int r_ = blockIdx.x;
  const int ct = r_ % cit; r_ /= cit;
  const int ot = r_ % cot; r_ /= cot;
  const int slab = r_;
  const int step0 = slab * p.steps_per_slab, step1 = min(step0 + p.steps_per_slab, p.total_steps);
  const int xplane = p.win_bytes / NP;            // bytes of one 64-channel window plane (win_bytes covers all NP)
  const int dz_base = p.win_bytes;                // then MP dz planes of 64 px x 128 B
  // staging: a piece = 16 bytes = 8 channels; X: window pixel i / (8 NP), piece i % (8 NP) (plane = piece >> 3); dz likewise with MP
  constexpr int XU = (96 * NP * 8 + 511) / 512;   // window pieces per thread (<= 96 window pixels)
  const int nx_items = p.XR * p.XC * NP * 8;
  int x_wr[XU], x_wc[XU], x_dst[XU], x_ch[XU];
#pragma unroll
  for (int u = 0; u < XU; ++u) {
    const int i = tid + 512 * u, px = i / (8 * NP), j = i % (8 * NP), jj = j & 7;
    x_wr[u] = i < nx_items ? px / p.XC : -(1 << 20);
    x_wc[u] = px % p.XC;
    x_ch[u] = j * 8;
    x_dst[u] = (j >> 3) * xplane + px * 128 + ((((jj >> 2) ^ ((px >> 1) & 1))) << 6) + (jj & 3) * 16;
  }
  int d_dst[MP], d_px[MP], d_ch[MP];
#pragma unroll
  for (int u = 0; u < MP; ++u) {
    const int i = tid + 512 * u, px = i / (8 * MP), j = i % (8 * MP), jj = j & 7;
    d_px[u] = px;
    d_ch[u] = j * 8;
    d_dst[u] = dz_base + (j >> 3) * (64 * 128) + px * 128 + ((((jj >> 2) ^ ((px >> 1) & 1))) << 6) + (jj & 3) * 16;
  }
  uint4 xv[XU], dv[MP];
#define W4_LOAD(step_)                                                                                                  \
  {                                                                                                                     \
    const int b_ = (step_) / p.rb_per_img, oy0_ = ((step_) % p.rb_per_img) * p.R;                                       \
    const int npix_ = min(p.R, p.Ho - oy0_) * p.Wo;                                                                     \
    _Pragma("unroll") for (int u = 0; u < XU; ++u) {                                                                    \
      const int iy = (oy0_ + x_wr[u]) * p.STRIDE, ix = x_wc[u] * p.STRIDE;                                              \
      xv[u] = make_uint4(0, 0, 0, 0);                                                                                   \
      if (iy >= 0 && iy < p.Hi && ix < p.Wi && x_wc[u] < p.Wo)                                                          \
        xv[u] = *reinterpret_cast<const uint4*>(p.x + ((((int64_t)b_ * p.Hi + iy) * p.Wi + ix) * p.Cin + ct * (64 * NP) + x_ch[u])); \
    }                                                                                                                   \
    _Pragma("unroll") for (int u = 0; u < MP; ++u) {                                                                    \
      dv[u] = make_uint4(0, 0, 0, 0);                                                                                   \
      if (d_px[u] < npix_)                                                                                              \
        dv[u] = *reinterpret_cast<const uint4*>(p.dz + ((((int64_t)b_ * p.Ho + oy0_) * p.Wo + d_px[u]) * p.Cout + ot * (64 * MP) + d_ch[u])); \
    }                                                                                                                   \
  }
#define W4_STORE(buf_)                                                                                                  \
  {                                                                                                                     \
    char* base_ = wl4 + (buf_) * p.buf_bytes;                                                                           \
    _Pragma("unroll") for (int u = 0; u < XU; ++u)                                                                      \
      if (tid + 512 * u < nx_items) *reinterpret_cast<uint4*>(base_ + x_dst[u]) = xv[u];                                \
    _Pragma("unroll") for (int u = 0; u < MP; ++u) *reinterpret_cast<uint4*>(base_ + d_dst[u]) = dv[u];                 \
  }
  // fragment addresses of this wave's two k-steps (kg, kg + 2): [k-step][first | second block of 4 pixels], half 0; half 1 = ^ 64
  const int q = (lane & 15) >> 2, pp = lane & 3, cb = (lane >> 4) & 1, hh = lane >> 5;
  const int col_bytes = 32 * cb + 8 * pp;
  const int maxpx = p.R * p.Wo - 1;
  int a_addr[2][2], b_addr[2][2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const int px = 16 * (kg + 2 * s) + 8 * hh + 4 * blk + q;
      a_addr[s][blk] = dz_base + mq * (64 * 128) + px * 128 + (((px >> 1) & 1) << 6) + col_bytes;
      const int pc = min(px, maxpx);
      const int row = (pc / p.Wo) * p.XC + (pc % p.Wo);
      b_addr[s][blk] = nq * xplane + row * 128 + (((row >> 1) & 1) << 6) + col_bytes;
    }
  typedef __attribute__((address_space(3))) v4s_t* lds_v4s;
  typedef short v8s_t __attribute__((ext_vector_type(8)));
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  if (step0 < step1) { W4_LOAD(step0) W4_STORE(0) }
  __syncthreads();
  for (int step = step0; step < step1; ++step) {
    const int buf = (step - step0) & 1;
    const bool more = step + 1 < step1;
    if (more) { W4_LOAD(step + 1) }
    const char* base = wl4 + buf * p.buf_bytes;
    const int oy0 = (step % p.rb_per_img) * p.R;
    const int nks = (min(p.R, p.Ho - oy0) * p.Wo + 15) >> 4;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (kg + 2 * s < nks) {
        bf16x8 a[2], b[2];
#pragma unroll
        for (int hsel = 0; hsel < 2; ++hsel) {
          const v4s_t a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(base + (a_addr[s][0] ^ (hsel << 6))));
          const v4s_t a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(base + (a_addr[s][1] ^ (hsel << 6))));
          const v4s_t b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(base + (b_addr[s][0] ^ (hsel << 6))));
          const v4s_t b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(base + (b_addr[s][1] ^ (hsel << 6))));
          a[hsel] = __builtin_bit_cast(bf16x8, (v8s_t){a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]});
          b[hsel] = __builtin_bit_cast(bf16x8, (v8s_t){b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]});
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
      }
    }
    if (more) { W4_STORE(buf ^ 1) }
    __syncthreads();
  }
#undef W4_LOAD
#undef W4_STORE
  // k-group 1 hands its quadrant to k-group 0 through LDS; k-group 0 adds (fixed order) and writes the slab
  float* xch = reinterpret_cast<float*>(wl4) + (wave & 3) * (64 * 64);
  if (kg == 1) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) xch[((mt * 2 + nt) * 16 + r) * 64 + lane] = acc[mt][nt][r];
  }
  __syncthreads();
  if (kg == 0) {
    float* out = p.slabs + (int64_t)slab * p.Cout * p.Cin;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int ci = ct * (64 * NP) + nq * 64 + nt * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = ot * (64 * MP) + mq * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
          out[(int64_t)co * p.Cin + ci] = acc[mt][nt][r] + xch[((mt * 2 + nt) * 16 + r) * 64 + lane];
        }
      }
  }
}

}  // namespace
