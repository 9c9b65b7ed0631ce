// gemm1x1_f32.inc -- the 1x1 convolutions of the FLOAT32 training engine (train.inc) as an NT GEMM on v_mfma_f32_32x32x2_f32 (round 5).
// Included before train_core_kernels.inc / train.inc (same translation unit).
//
//   out[m][n] = sum_k A[row(m)][k] * W[n][k]  (+ res[m][n]),   m = output pixel, n = channel; both operands K-contiguous.
//
// What it replaces: the downsample branches of ResNet-18 (models/patch_cls_simple/model.py:5-11; step train.py:166-172) -- forward
// 1x1 / stride 2 and the data gradient 1x1 / stride 1 -- ran on the round-1 generic convolution (conv_kernel<float, 1, *>): per 64-byte
// channel chunk (16 floats) a weight copy and an activation copy global -> registers -> LDS behind three workgroup barriers, nothing in
// flight under the MFMAs, and 64-256 workgroups on 256 CUs.  Round-5 timeline of a 64 x 224^2 step: three data gradients at 76 / 87 / 101
// us (0.8 GFLOP each: 5 us of matrix time, 10 us of HBM time) and three forward convolutions at 23 / 25 / 42 us.
//
// Structure = the bf16 engine's gemm1x1_ring_kernel (gemm1x1.inc) with float32 fragments: workgroup tile 128 pixels x 64 channels, K-tile
// 32 floats = the same 128-byte LDS rows, operands global -> LDS by LDS-DMA into a ring of two 24 KB stages (the per-lane SOURCE
// address carries the XOR swizzle of the 16-byte slots), one barrier per K-tile, 4 waves (wave w = pixels 32 w .. 32 w + 31 x 64
// channels).  A 16-byte fragment is 4 k-values; the two half-waves hold the two k of a 32x32x2 instruction, so slot 2 ks + h, component
// j of A and of W meet in MFMA j of k-step ks: any consistent k order sums the same products.  The channel is the MFMA row: a lane ends
// with 4 consecutive channels of one pixel per register group = one 16-byte store (+ one 16-byte residual load).
// Weights: forward W[cout][cin] is the float32 master tensor itself (torch layout, no packed copy); the data gradient reads the
// transposed copy Wt[cin][cout] that pack_all_f32_kernel keeps for 1x1 convolutions.
namespace {

struct GemmF32Params {
  const float* a; const float* w; const float* res; float* out;
  int M, N, K;
  int stride, Ho, Wo, Hi, Wi;   // stride 2: output pixel (b, oy, ox) reads input pixel (b, 2 oy, 2 ox)
  int MB, NB, nstage;
};
constexpr int GF_BM = 128, GF_BN = 64, GF_BK = 32;
constexpr int GF_STAGE = (GF_BM + GF_BN) * 128;   // 24 KB

__global__ __launch_bounds__(256, 4) void gemm1x1_f32_kernel(const GemmF32Params p) {
  extern __shared__ __attribute__((aligned(1024))) char gfl[];
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // XCD-aware tile map: workgroups bid = x (mod 8) share an XCD; they walk the NB channel tiles of one pixel tile
  const int bid = blockIdx.x;
  const int mb = (bid / (8 * p.NB)) * 8 + (bid & 7), nb = (bid >> 3) % p.NB;
  if (mb >= p.MB) return;
  const int m0 = mb * GF_BM, n0 = nb * GF_BN;
  // DMA plan: a 1 KiB piece = 8 rows of 128 B.  A: pieces 4 wave + j (j < 4); W: pieces 2 wave + j (j < 2)
  const char* a_src[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = (wave * 4 + j) * 8 + (lane >> 3), ls = (lane & 7) ^ ((row >> 1) & 7);
    int m = m0 + row;
    if (m >= p.M) m = p.M - 1;   // clamped rows are computed and never stored
    int64_t src_row = m;
    if (p.stride == 2) {
      const int ox = m % p.Wo, t = m / p.Wo, oy = t % p.Ho, b = t / p.Ho;
      src_row = ((int64_t)b * p.Hi + 2 * oy) * p.Wi + 2 * ox;
    }
    a_src[j] = reinterpret_cast<const char*>(p.a + src_row * p.K + ls * 4);
  }
  const char* w_src[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = (wave * 2 + j) * 8 + (lane >> 3), ls = (lane & 7) ^ ((row >> 1) & 7);
    w_src[j] = reinterpret_cast<const char*>(p.w + (int64_t)(n0 + row) * p.K + ls * 4);
  }
  const unsigned lds0 = lds_addr_of(gfl);
  const unsigned a_dst = lds0 + wave * 4096, w_dst = lds0 + GF_BM * 128 + wave * 2048;
#define GF_ISSUE(kt_, slot_)                                                                                  \
  {                                                                                                           \
    const unsigned so_ = (unsigned)(slot_) * GF_STAGE;                                                        \
    const int ko_ = (kt_) * 128;                                                                              \
    lds_dma<16>(a_src[0] + ko_, a_dst + so_);        lds_dma<16>(a_src[1] + ko_, a_dst + so_ + 1024);         \
    lds_dma<16>(a_src[2] + ko_, a_dst + so_ + 2048); lds_dma<16>(a_src[3] + ko_, a_dst + so_ + 3072);         \
    lds_dma<16>(w_src[0] + ko_, w_dst + so_);        lds_dma<16>(w_src[1] + ko_, w_dst + so_ + 1024);         \
  }
  const int m = m0 + wave * 32 + (lane & 31);
  const bool ok = m < p.M;
  const int64_t orow = (int64_t)(ok ? m : p.M - 1) * p.N + n0;
  const int KT = p.K / GF_BK, NS = p.nstage;
  GF_ISSUE(0, 0)
  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  const int prow = wave * 32 + (lane & 31), wrow = lane & 31;
  const int b_off = prow * 128, b_sw = (prow >> 1) & 7;
  int slot = 0;
  for (int kt = 0; kt < KT; ++kt) {
    // my DMAs of K-tile kt have landed; the barrier says the same of every wave's, and that every wave is done reading K-tile kt - 1,
    // whose slot the next issue overwrites
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (NS > 1 && kt + 1 < KT) GF_ISSUE(kt + 1, slot ^ 1)
    const char* As = gfl + slot * GF_STAGE;
    const char* Ws = As + GF_BM * 128;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int sl = 2 * ks + h;
      const uint4 b = *reinterpret_cast<const uint4*>(As + b_off + ((sl ^ b_sw) << 4));
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const int r = mt * 32 + wrow;
        const uint4 a = *reinterpret_cast<const uint4*>(Ws + r * 128 + ((sl ^ ((r >> 1) & 7)) << 4));
        mma_frag<float>(acc[mt], a, b);
      }
    }
    if (NS > 1) slot ^= 1;
    else if (kt + 1 < KT) {   // single slot: reload in place
      __builtin_amdgcn_s_barrier();
      GF_ISSUE(kt + 1, 0)
    }
  }
#undef GF_ISSUE
  if (!ok) return;
  // epilogue: lane = pixel (lane & 31), register r of acc[mt] = channel 32 mt + (r & 3) + 8 (r >> 2) + 4 h
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t o = orow + mt * 32 + g * 8 + 4 * h;
      float4 v = make_float4(acc[mt][4 * g + 0], acc[mt][4 * g + 1], acc[mt][4 * g + 2], acc[mt][4 * g + 3]);
      if (p.res) { const float4 r = *reinterpret_cast<const float4*>(p.res + o); v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w; }
      *reinterpret_cast<float4*>(p.out + o) = v;
    }
}

// out[M][N] = A . W^T (+ res);  stride 2: A rows gathered from [B][Hi][Wi][K] at (b, 2 oy, 2 ox), M = B Ho Wo
int gemm1x1_f32(const float* a, const float* w, const float* res, float* out, int64_t M, int N, int K, int stride, int Ho, int Wo, int Hi, int Wi,
                hipStream_t st) {
  DH_REQUIRE(N % GF_BN == 0 && K % GF_BK == 0 && M > 0 && M < ((int64_t)1 << 31) && (stride == 1 || stride == 2),
             "gemm1x1 f32: M=%lld N=%d K=%d stride=%d unsupported", (long long)M, N, K, stride);
  GemmF32Params p{};
  p.a = a; p.w = w; p.res = res; p.out = out;
  p.M = (int)M; p.N = N; p.K = K; p.stride = stride; p.Ho = Ho; p.Wo = Wo; p.Hi = Hi; p.Wi = Wi;
  p.MB = (int)((M + GF_BM - 1) / GF_BM); p.NB = N / GF_BN;
  p.nstage = std::min(K / GF_BK, 2);
  const int grid = ((p.MB + 7) / 8) * 8 * p.NB;
  hipLaunchKernelGGL(gemm1x1_f32_kernel, dim3(grid), dim3(256), (size_t)p.nstage * GF_STAGE, st, p);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

}  // namespace
