// cam.inc -- the CAM head of both inference engines (DESIGN.md section 4.20): fc applied at every position of the last activation
// instead of to its mean,  cam[t][p][k] = fc_b[k] + sum_c fc_w[k][c] * a[t][p][c],  float32 [n][HW][n_cls].
// Included in resnet_kernels.hip behind infer_core.inc; launched by forward_impl / r50_forward_impl behind the unchanged head.
//
// Memory-bound: one read of the last activation per chunk of CAM_KC classes.  A wave takes 16 consecutive positions of one image: lane
// l owns position l / 4 and, of every step's 4 * 16 bytes of channels, the 16-byte piece l % 4 -- in the channel-blocked bf16 layout
// [image][C/32][HW][32] a step is one 32-channel block and the wave's load is 1 KiB contiguous; in float32 NHWC a step is 16 channels.
// fc_w of the chunk sits in LDS (CAM_KC x C floats: 16 KiB at C = 512, 64 KiB at C = 2048); the four lanes of a position read four
// distinct 16 / 32-byte pieces of a row, every other lane the same ones (broadcast).
// Order of one output, fixed by (C, n_cls) alone: lane piece e adds its channels in ascending order into one accumulator starting
// from 0 (one fused multiply-add per channel), the four pieces join as (s0 + s1) + (s2 + s3), the bias is added last.  Nothing
// depends on HW, on the tile's index or on the launch size; no atomics.
namespace {

constexpr int CAM_KC = 8;         // classes per pass over the activation
constexpr int CAM_MAX_CLS = 64;   // accumulate.hip's MAX_CLS: the maps built from these rows take no more
constexpr int CAM_MAX_HW = 1024;

template <typename T, bool BLOCKED>
__global__ __launch_bounds__(256) void cam_head_kernel(const T* __restrict__ in, int B, int HW, int C, const float* __restrict__ fc_w,
                                                       const float* __restrict__ fc_b, int n_cls, float* __restrict__ cam) {
  extern __shared__ __attribute__((aligned(16))) float s_w[];   // [min(CAM_KC, n_cls)][C]
  constexpr int EPV = 16 / (int)sizeof(T);   // channels per lane and step
  constexpr int CPS = 4 * EPV;               // channels per step
  static_assert(!BLOCKED || CPS == 32, "a step of the channel-blocked layout is one 32-channel block");
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 2, e = lane & 3;
  const int groups = (HW + 15) >> 4, units = B * groups, nstep = C / CPS;
  const int64_t step_stride = BLOCKED ? (int64_t)HW * 32 : CPS;
  for (int k0 = 0; k0 < n_cls; k0 += CAM_KC) {
    const int kn = min(CAM_KC, n_cls - k0);
    __syncthreads();   // the previous chunk's readers are done
    for (int i = tid; i < kn * C / 4; i += 256)
      reinterpret_cast<float4*>(s_w)[i] = reinterpret_cast<const float4*>(fc_w + (int64_t)k0 * C)[i];
    __syncthreads();
    for (int u = blockIdx.x * 4 + wave; u < units; u += gridDim.x * 4) {   // wave-uniform
      const int b = u / groups, p = ((u - b * groups) << 4) + q;
      const bool ok = p < HW;
      const T* src = in + (BLOCKED ? ((int64_t)b * (C / 32) * HW + p) * 32 : ((int64_t)b * HW + p) * C) + e * EPV;
      float acc[CAM_KC];
#pragma unroll
      for (int kk = 0; kk < CAM_KC; ++kk) acc[kk] = 0.f;
#pragma unroll 4
      for (int s = 0; s < nstep; ++s) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (ok) v = *reinterpret_cast<const uint4*>(src + s * step_stride);
        const uint32_t uw[4] = {v.x, v.y, v.z, v.w};
        float a[EPV];
        if constexpr (sizeof(T) == 2) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { a[2 * j] = bf16_bits_to_f32(uw[j] & 0xFFFFu); a[2 * j + 1] = bf16_bits_to_f32(uw[j] >> 16); }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] = __uint_as_float(uw[j]);
        }
        const float* wrow = s_w + s * CPS + e * EPV;
#pragma unroll
        for (int kk = 0; kk < CAM_KC; ++kk) {
          if (kk < kn) {   // uniform
            float t = acc[kk];
#pragma unroll
            for (int j4 = 0; j4 < EPV / 4; ++j4) {
              const float4 w4 = *reinterpret_cast<const float4*>(wrow + kk * C + 4 * j4);
              t = __builtin_fmaf(a[4 * j4], w4.x, t); t = __builtin_fmaf(a[4 * j4 + 1], w4.y, t);
              t = __builtin_fmaf(a[4 * j4 + 2], w4.z, t); t = __builtin_fmaf(a[4 * j4 + 3], w4.w, t);
            }
            acc[kk] = t;
          }
        }
      }
#pragma unroll
      for (int kk = 0; kk < CAM_KC; ++kk) {
        if (kk < kn) {   // uniform: every lane of the wave takes part in the exchanges
          float t = acc[kk];
          t = t + __shfl_xor(t, 1, 64);   // (s0 + s1), (s2 + s3): float addition commutes, so the four lanes hold the same bits
          t = t + __shfl_xor(t, 2, 64);
          if (ok && (kk & 3) == e) cam[((int64_t)b * HW + p) * n_cls + k0 + kk] = t + fc_b[k0 + kk];
        }
      }
    }
  }
}

// the launch behind an engine's head: `act` is the last activation of B tiles, [image][C/32][HW][32] bf16 or float32 NHWC
template <typename T>
int launch_cam_head(const InferNet* net, const void* act, int B, int HW, float* cam, hipStream_t st) {
  constexpr bool BLOCKED = sizeof(T) == 2;
  const int C = net->desc->feat, n_cls = net->n_classes;
  DH_REQUIRE(C % 64 == 0 && HW >= 1 && HW <= CAM_MAX_HW && n_cls >= 1 && n_cls <= CAM_MAX_CLS,
             "cam head: C=%d, HW=%d, n_cls=%d unsupported (C %% 64 == 0, 1 <= HW <= %d, 1 <= n_cls <= %d)", C, HW, n_cls, CAM_MAX_HW,
             CAM_MAX_CLS);
  const int lds = std::min(CAM_KC, n_cls) * C * 4;
  const int units = B * ((HW + 15) / 16);
  const int grid = std::min((units + 3) / 4, 1024);   // four workgroups per CU at most: fc_w is staged once per workgroup and chunk
  if (int rc = ensure_dyn_lds(reinterpret_cast<const void*>(&cam_head_kernel<T, BLOCKED>), CAM_KC * 2048 * 4)) return rc;
  hipLaunchKernelGGL((cam_head_kernel<T, BLOCKED>), dim3(grid), dim3(256), (size_t)lds, st, static_cast<const T*>(act), B, HW, C,
                     net->fc_w_dev, net->fc_b_dev, n_cls, cam);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// what the cam_tiles entries refuse on top of their forward_tiles sibling's checks, before any launch
int cam_check(const InferEngine& e, const InferNet* net, int32_t P, const char* what) {
  DH_REQUIRE(net != nullptr, "%s: null handle", what);
  DH_REQUIRE(P % 32 == 0, "%s: patch %d is not a multiple of 32 (a position is a 32 x 32-pixel block of the tile)", what, P);
  DH_REQUIRE(net->n_classes <= CAM_MAX_CLS, "%s: %d classes, the %s class activation map takes at most %d", what, net->n_classes, e.name,
             CAM_MAX_CLS);
  return DH_OK;
}

}  // namespace
