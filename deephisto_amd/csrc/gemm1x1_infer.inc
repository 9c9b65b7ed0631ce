// gemm1x1_infer.inc -- 1x1 convolutions of the ResNet-50 INFERENCE engine (resnet50_infer.inc) as an NT GEMM on bf16 MFMA, with the
// eval-mode epilogue fused in.  Included after gemm1x1.inc (same translation unit; it reuses lds_dma, mma_frag, pack_bf16x2).
//
//   out[m][n] = relu( sum_k A[m][k] * W'[n][k] + b'[n]  (+ res[m][n]) ),    W' = W * gamma / sqrt(var + eps) (BN folded at finalize)
//
// One pass per convolution writes its final activation: no Z / Y pair, no BN apply pass.  A bottleneck's conv3 takes the block's join
// in the same epilogue (+ identity or + the downsample's output, then ReLU); the downsample itself runs here with relu = 0.
//
// Structure: the LDS-DMA ring of gemm1x1.inc (workgroup tile 128 pixels x 32 NMT channels, K-tile 64, 4 waves, `global_load_lds_dwordx4`
// with the XOR swizzle carried by the per-lane source address), but the activations are in the channel-blocked bf16 inference layout
// [image][C/32][H][W][32] that the fused stem (stem_pool.inc) writes and the 3x3 kernel (conv3x3.inc, `blocked`) reads and writes:
// channel c of pixel (b, q) lives at element  b*C*HW + (c >> 5)*HW*32 + q*32 + (c & 31).
//   * A operand: a K-tile (64 channels) is two 32-channel planes; a lane's 16-byte slot ls (8 channels) sits in plane ls >> 2 at
//     (ls & 3) * 16 bytes of the pixel's 64-byte row, and the next K-tile is 2 planes further (a_kstep bytes).  8 consecutive pixels of
//     a DMA piece read two 512-byte runs.
//   * stride 2 (downsample): output pixel (b, oy, ox) reads input pixel (b, 2 oy, 2 ox) directly -- no staging copy.
//   * the epilogue stores (and reads the residual in) 16-byte pieces of 8 channels at the same blocked address.
// Every output element is one dot product over K in a fixed order: the result of a pixel does not depend on the launch's batch.
namespace {

struct GemmInferParams {
  const bf16_t* a; const bf16_t* w; const float* bias; const bf16_t* res; bf16_t* out;
  int M, N, K;
  int HWo;                      // output pixels per image
  int stride, Ho, Wo, Hi, Wi;   // input map (stride 1: Hi = Ho, Wi = Wo)
  int MB, NB, nstage, relu;
};

template <int NMT>
__global__ __launch_bounds__(256, NMT == 2 ? 4 : 2) void gemm1x1_infer_kernel(const GemmInferParams p) {
  constexpr int BN = G2Cfg<NMT>::BN, STAGE = G2Cfg<NMT>::STAGE;
  extern __shared__ __attribute__((aligned(1024))) char gil[];
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // XCD-aware tile map (as gemm1x1.inc): workgroups bid = x (mod 8) share an XCD and walk the NB channel tiles of one pixel tile
  const int bid = blockIdx.x;
  const int mb = (bid / (8 * p.NB)) * 8 + (bid & 7), nb = (bid >> 3) % p.NB;
  if (mb >= p.MB) return;
  const int m0 = mb * G2_BM, n0 = nb * BN;
  const int HWi = p.Hi * p.Wi;
  const int64_t a_kstep = (int64_t)2 * HWi * 64;   // bytes from one K-tile (two 32-channel planes) to the next
  // ---- DMA plan: a 1 KiB piece = 8 rows of 128 B.  A: pieces 4 wave + j (j < 4); W: pieces NMT wave + j (j < NMT)
  const char* a_src[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = (wave * 4 + j) * 8 + (lane >> 3), ls = (lane & 7) ^ ((row >> 1) & 7);
    int m = m0 + row;
    if (m >= p.M) m = p.M - 1;   // clamped rows are computed and never stored
    const int b = m / p.HWo, q = m - b * p.HWo;
    int qi = q;
    if (p.stride == 2) { const int oy = q / p.Wo, ox = q - oy * p.Wo; qi = 2 * oy * p.Wi + 2 * ox; }
    const int64_t e = (int64_t)b * p.K * HWi + (int64_t)(ls >> 2) * HWi * 32 + (int64_t)qi * 32 + (ls & 3) * 8;
    a_src[j] = reinterpret_cast<const char*>(p.a + e);
  }
  const char* w_src[NMT];
#pragma unroll
  for (int j = 0; j < NMT; ++j) {
    const int row = (wave * NMT + j) * 8 + (lane >> 3), ls = (lane & 7) ^ ((row >> 1) & 7);
    w_src[j] = reinterpret_cast<const char*>(p.w + (int64_t)(n0 + row) * p.K + ls * 8);
  }
  const unsigned lds0 = lds_addr_of(gil);
  const unsigned a_dst = lds0 + wave * 4096, w_dst = lds0 + G2_BM * 128 + wave * (NMT * 1024);
#define GI_ISSUE(kt_, slot_)                                                                                  \
  {                                                                                                           \
    const unsigned so_ = (unsigned)(slot_) * STAGE;                                                           \
    const int64_t ka_ = (int64_t)(kt_) * a_kstep;                                                             \
    const int kw_ = (kt_) * 128;                                                                              \
    lds_dma<16>(a_src[0] + ka_, a_dst + so_);        lds_dma<16>(a_src[1] + ka_, a_dst + so_ + 1024);         \
    lds_dma<16>(a_src[2] + ka_, a_dst + so_ + 2048); lds_dma<16>(a_src[3] + ka_, a_dst + so_ + 3072);         \
    _Pragma("unroll") for (int j_ = 0; j_ < NMT; ++j_) lds_dma<16>(w_src[j_] + kw_, w_dst + so_ + j_ * 1024); \
  }
  // output pixel of this lane and the element offset of its 32-channel plane 0 (blocked layout); the residual is requested NOW,
  // in the 16-byte pieces the lane will store
  const int m = m0 + wave * 32 + (lane & 31);
  const bool ok = m < p.M;
  const int mc = ok ? m : p.M - 1;
  const int ob = mc / p.HWo, oq = mc - ob * p.HWo;
  const int64_t obase = (int64_t)ob * p.N * p.HWo + (int64_t)oq * 32;
  auto piece = [&](int mt, int pr) -> int64_t {   // element offset of channels n0 + 32 mt + 8 (2 pr + h) .. + 7 of this pixel
    const int c = n0 + mt * 32 + (2 * pr + h) * 8;
    return obase + (int64_t)(c >> 5) * p.HWo * 32 + (c & 31);
  };
  uint4 rres[NMT][2];
#pragma unroll
  for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) rres[mt][pr] = make_uint4(0, 0, 0, 0);
  if (p.res) {
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) rres[mt][pr] = *reinterpret_cast<const uint4*>(p.res + piece(mt, pr));
  }
  const int KT = p.K / G2_BK;
  const int NS = p.nstage;   // K-tiles kt + 1 .. kt + NS - 1 are in flight while K-tile kt is multiplied
  GI_ISSUE(0, 0)
  if (NS > 2 && KT > 1) GI_ISSUE(1, 1)
  f32x16 acc[NMT];
#pragma unroll
  for (int i = 0; i < NMT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  const int prow = wave * 32 + (lane & 31), wrow = lane & 31;
  const int b_off = prow * 128, b_sw = (prow >> 1) & 7;
  int slot = 0;
  for (int kt = 0; kt < KT; ++kt) {
    if (NS > 2 && kt + 1 < KT) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 + NMT) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (NS > 1 && kt + NS - 1 < KT) {
      const int s2 = slot == 0 ? NS - 1 : slot - 1;   // (kt + NS - 1) % NS: the slot K-tile kt - 1 has just left
      GI_ISSUE(kt + NS - 1, s2)
    }
    const char* As = gil + slot * STAGE;
    const char* Ws = As + G2_BM * 128;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int sl = 2 * ks + h;
      const uint4 b = *reinterpret_cast<const uint4*>(As + b_off + ((sl ^ b_sw) << 4));
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt) {
        const int r = mt * 32 + wrow;
        const uint4 a = *reinterpret_cast<const uint4*>(Ws + r * 128 + ((sl ^ ((r >> 1) & 7)) << 4));
        mma_frag<__bf16>(acc[mt], a, b);
      }
    }
    slot = slot + 1 == NS ? 0 : slot + 1;
    if (NS == 1 && kt + 1 < KT) {   // single slot: reload in place
      __builtin_amdgcn_s_barrier();
      GI_ISSUE(kt + 1, 0)
    }
  }
#undef GI_ISSUE
  // epilogue: lane = pixel (lane & 31), register r of acc[mt] = channel 32 mt + (r & 3) + 8 (r >> 2) + 4 h
#pragma unroll
  for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      uint32_t pk[2][2];
      uint32_t rx[2] = {rres[mt][pr].x, rres[mt][pr].z}, ry[2] = {rres[mt][pr].y, rres[mt][pr].w};
      if (p.res) {   // back to per-lane ownership (the swap below is its own inverse): [gg] = this lane's 4 channels of group 2 pr + gg
        { const auto s = __builtin_amdgcn_permlane32_swap(rx[0], rx[1], false, false); rx[0] = s[0]; rx[1] = s[1]; }
        { const auto s = __builtin_amdgcn_permlane32_swap(ry[0], ry[1], false, false); ry[0] = s[0]; ry[1] = s[1]; }
      }
#pragma unroll
      for (int gg = 0; gg < 2; ++gg) {
        const int g = 2 * pr + gg;
        const float4 bb = *reinterpret_cast<const float4*>(p.bias + n0 + mt * 32 + 8 * g + 4 * h);
        float v[4] = {acc[mt][4 * g + 0] + bb.x, acc[mt][4 * g + 1] + bb.y, acc[mt][4 * g + 2] + bb.z, acc[mt][4 * g + 3] + bb.w};
        if (p.res) {
          v[0] += bf16_bits_to_f32(rx[gg] & 0xFFFFu); v[1] += bf16_bits_to_f32(rx[gg] >> 16);
          v[2] += bf16_bits_to_f32(ry[gg] & 0xFFFFu); v[3] += bf16_bits_to_f32(ry[gg] >> 16);
        }
        if (p.relu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        pk[gg][0] = pack_bf16x2(v[0], v[1]);
        pk[gg][1] = pack_bf16x2(v[2], v[3]);
      }
      // half-waves trade halves: lane h = 0 keeps all 8 channels of group 2 pr, lane h = 1 those of group 2 pr + 1
      { const auto s = __builtin_amdgcn_permlane32_swap(pk[0][0], pk[1][0], false, false); pk[0][0] = s[0]; pk[1][0] = s[1]; }
      { const auto s = __builtin_amdgcn_permlane32_swap(pk[0][1], pk[1][1], false, false); pk[0][1] = s[0]; pk[1][1] = s[1]; }
      if (ok) *reinterpret_cast<uint4*>(p.out + piece(mt, pr)) = make_uint4(pk[0][0], pk[0][1], pk[1][0], pk[1][1]);
    }
}

// Global average pool over the 2048 channels of the last block (blocked layout) + fc, one workgroup per image: thread t owns channels
// 8t .. 8t+7 and adds the pixels in index order; the fc dot products are summed per thread (8 channels), per wave (shuffle tree) and over
// the 4 waves in a fixed order.  No atomics: the logits of an image do not depend on the launch.
// FEAT: the pooled vector also goes to feat[image][2048] (dh_resnet50_features_tiles), and a null `logits` skips the fc; pooled values
// and logits are those of the FEAT = false instantiation, which forward / forward_tiles launch.
template <bool FEAT = false>
__global__ __launch_bounds__(256) void r50_head_kernel(const bf16_t* __restrict__ in, int HW, const float* __restrict__ fc_w,
                                                       const float* __restrict__ fc_b, int n_cls, float* __restrict__ logits,
                                                       float* __restrict__ feat = nullptr) {
  constexpr int C = 2048;
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x, c0 = tid * 8;
  const bf16_t* src = in + (int64_t)b * C * HW + (int64_t)(c0 >> 5) * HW * 32 + (c0 & 31);
  float s[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = 0.f;
  for (int q = 0; q < HW; ++q) {
    const uint4 v = *reinterpret_cast<const uint4*>(src + q * 32);
    const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) { s[2 * e] += bf16_bits_to_f32(u[e] & 0xFFFFu); s[2 * e + 1] += bf16_bits_to_f32(u[e] >> 16); }
  }
  const float inv = 1.0f / (float)HW;
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] *= inv;
  if constexpr (FEAT) {
    float4* dst = reinterpret_cast<float4*>(feat + (int64_t)b * C + c0);
    dst[0] = make_float4(s[0], s[1], s[2], s[3]);
    dst[1] = make_float4(s[4], s[5], s[6], s[7]);
    if (!logits) return;   // uniform for the launch
  }
  for (int k = 0; k < n_cls; ++k) {
    const float* wk = fc_w + (int64_t)k * C + c0;
    const float4 w0 = *reinterpret_cast<const float4*>(wk), w1 = *reinterpret_cast<const float4*>(wk + 4);
    float t = s[0] * w0.x;
    t = __builtin_fmaf(s[1], w0.y, t); t = __builtin_fmaf(s[2], w0.z, t); t = __builtin_fmaf(s[3], w0.w, t);
    t = __builtin_fmaf(s[4], w1.x, t); t = __builtin_fmaf(s[5], w1.y, t); t = __builtin_fmaf(s[6], w1.z, t); t = __builtin_fmaf(s[7], w1.w, t);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = t;
    __syncthreads();
    if (tid == 0) logits[(int64_t)b * n_cls + k] = ((red[0] + red[1]) + (red[2] + red[3])) + fc_b[k];
    __syncthreads();
  }
}

}  // namespace
