// ResNet-18 patch-classifier forward for MI355X (gfx950), hand-written HIP.
//
// Replaces `model(features)` of the network built by
// models/patch_cls_simple/model.py:5-11 (torchvision resnet18 + fc[n_cls,512]) as
// called from examples/predict_full_patched.py:77 (eval mode).
//
// Design:
//  * activations live in HBM pixel-major: NHWC for float32, channel-blocked [image][C/32][H][W][32] for bf16
//    inference, so the reduction index of every convolution, (tap, cin), is contiguous in cin: a 64-byte channel
//    chunk of one pixel is one LDS row, and a lane's MFMA B-fragment is one 16-byte read;
//  * each conv is an implicit GEMM  D[cout][pixel] = sum_k W[cout][k] * X[k][pixel]
//    on v_mfma_f32_32x32x16_bf16 (bf16 mode) or v_mfma_f32_32x32x2_f32 (f32 mode, exact f32 products, used for
//    the 1e-4 parity runs).  cout is the MFMA row index so every lane ends up with 4 consecutive couts of one
//    pixel -> 8/16-byte stores with BN scale/shift, residual add and ReLU fused in the epilogue;
//  * 3x3 convs (stride 1 and 2; the 1x1 stride-2 downsample rides on the stride-2 kernel): conv3x3.inc --
//    persistent 8-wave workgroups, one per CU, 64 couts x 128..512 pixels per tile, LDS-DMA ring of
//    [weight slab | input window] stages, all 9 taps read shifted views of the staged window;
//  * bf16 stem: stem_pool.inc (conv 7x7/2 + BN + ReLU + maxpool fused, persistent); the generic conv_kernel
//    below serves the f32 1x1 convs of training and the debug hook;
//  * weights are pre-packed on the host in MFMA fragment order, so staging them is a linear copy and reading them
//    is conflict-free `base + lane*16`;
//  * host-side caches (lookup tables, zero page, function attributes) are keyed by HIP device and guarded by one
//    mutex: one process may drive several devices / call from several threads (one handle per thread).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "dh_common.h"
#include "conv3_plan_host.h"   // (includes conv3_tables_host.h)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

namespace {

constexpr int CHUNK_BYTES = 64;   // channel bytes of one pixel staged per pass
constexpr int PIX_PITCH = 80;     // LDS bytes per staged pixel (64 + 16 pad: bank spread)
constexpr int FRAG_BYTES = 1024;  // one MFMA operand fragment: 64 lanes x 16 B
constexpr int SLAB_TAP = 4 * FRAG_BYTES;  // per tap: 2 k-steps x 2 cout-tiles

template <typename T> struct ElemTraits;
template <> struct ElemTraits<float> { static constexpr int ESZ = 4; };
template <> struct ElemTraits<__bf16> { static constexpr int ESZ = 2; };

__device__ __forceinline__ float bf16_bits_to_f32(uint32_t b) { return __uint_as_float(b << 16); }
__device__ __forceinline__ uint32_t f32_to_bf16(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ float div255f(uint32_t k) {
  const float r = 1.0f / 255.0f;
  const float kf = (float)k;
  const float q = kf * r;
  return __builtin_fmaf(__builtin_fmaf(-q, 255.0f, kf), r, q);
}

template <typename T>
__device__ __forceinline__ void mma_frag(f32x16& acc, const uint4& a, const uint4& b) {
  if constexpr (sizeof(T) == 2) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                  __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
  } else {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
  }
}

// Epilogue shared by stem and conv kernels.  acc[mt][nt] holds D[cout][pixel]:
// lane: pixel = lane&31 of n-tile nt; register r: cout = 32*mt + (r&3) + 8*(r>>2) + 4*(lane>>5).
// y = acc*scale + shift (+ residual) (ReLU) -> 4 consecutive couts per store.
template <typename T>
__device__ __forceinline__ void store_group(const f32x16& acc, int g, const float* __restrict__ scale,
                                            const float* __restrict__ shift, const T* __restrict__ res,
                                            T* __restrict__ out, int64_t off, int co, bool relu) {
  const float4 sc = *reinterpret_cast<const float4*>(scale + co);
  const float4 sh = *reinterpret_cast<const float4*>(shift + co);
  float v[4] = {__builtin_fmaf(acc[4 * g + 0], sc.x, sh.x), __builtin_fmaf(acc[4 * g + 1], sc.y, sh.y),
                __builtin_fmaf(acc[4 * g + 2], sc.z, sh.z), __builtin_fmaf(acc[4 * g + 3], sc.w, sh.w)};
  if (res) {
    if constexpr (sizeof(T) == 2) {
      const uint2 r = *reinterpret_cast<const uint2*>(res + off);
      v[0] += bf16_bits_to_f32(r.x & 0xFFFFu); v[1] += bf16_bits_to_f32(r.x >> 16);
      v[2] += bf16_bits_to_f32(r.y & 0xFFFFu); v[3] += bf16_bits_to_f32(r.y >> 16);
    } else {
      const float4 r = *reinterpret_cast<const float4*>(res + off);
      v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
    }
  }
  if (relu) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = v[i] > 0.f ? v[i] : 0.f;
  }
  if constexpr (sizeof(T) == 2) {
    uint2 w;
    w.x = f32_to_bf16(v[0]) | (f32_to_bf16(v[1]) << 16);
    w.y = f32_to_bf16(v[2]) | (f32_to_bf16(v[3]) << 16);
    *reinterpret_cast<uint2*>(out + off) = w;
  } else {
    *reinterpret_cast<float4*>(out + off) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// ---------------------------------------------------------------------------
// Generic conv (KS x KS, stride STRIDE, pad KS/2), NHWC, Cin % (64/ESZ) == 0,
// Cout % 64 == 0.  HALO (3x3, stride 1 only): stage patch+halo once per chunk.
// ---------------------------------------------------------------------------
struct ConvParams {
  const void* in; const void* w; const float* scale; const float* shift; const void* res; void* out;
  int B, Hi, Wi, Cin, Ho, Wo, Cout;
  int TH, TW, IMGS;       // output patch per workgroup: IMGS images x TH x TW = 256 pixels
  int tiles_y, tiles_x;   // patches per image
  int relu;
};

constexpr int MAX_HALO_PIECES = 7;  // ceil(4 * IMGS*(TH+2)*(TW+2) / 256), worst case 4*400/256

template <typename T, int KS, int STRIDE, bool HALO>
__global__ __launch_bounds__(256, 2) void conv_kernel(const ConvParams p) {
  static_assert(!HALO || (KS == 3 && STRIDE == 1), "halo staging is for 3x3 stride 1");
  constexpr int ESZ = ElemTraits<T>::ESZ;
  constexpr int CPC = CHUNK_BYTES / ESZ;  // channels per chunk
  constexpr int TAPS = KS * KS, PAD = KS / 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* w_lds = smem;
  char* a_lds = smem + TAPS * SLAB_TAP;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ncb = p.Cout >> 6;
  const int cb = blockIdx.x % ncb, pt = blockIdx.x / ncb;
  const int tiles_per_img = p.tiles_y * p.tiles_x;
  const int img0 = (pt / tiles_per_img) * p.IMGS;
  const int tile = pt % tiles_per_img;
  const int oy0 = (tile / p.tiles_x) * p.TH, ox0 = (tile % p.tiles_x) * p.TW;
  const int nchunks = p.Cin / CPC;
  const int HW2 = p.TW + 2, HH2 = p.TH + 2;
  const char* in = static_cast<const char*>(p.in);

  // this lane's two pixels (one per n-tile)
  int pimg[2], poy[2], pox[2], b_off[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int pidx = wave * 64 + nt * 32 + (lane & 31);
    const int img = pidx / (p.TH * p.TW), rem = pidx % (p.TH * p.TW);
    const int ty = rem / p.TW, tx = rem % p.TW;
    pimg[nt] = img0 + img; poy[nt] = oy0 + ty; pox[nt] = ox0 + tx;
    b_off[nt] = (HALO ? ((img * HH2 + ty) * HW2 + tx) : pidx) * PIX_PITCH + 16 * (lane >> 5);
  }

  // staging descriptors (global byte offset at chunk 0, LDS byte offset); -1 = zero fill
  uint32_t g_off[MAX_HALO_PIECES];
  int l_off[MAX_HALO_PIECES];
  bool g_ok[MAX_HALO_PIECES];
  const int n_pieces = HALO ? p.IMGS * HH2 * HW2 * 4 : 0;
  if constexpr (HALO) {
#pragma unroll
    for (int j = 0; j < MAX_HALO_PIECES; ++j) {
      const int i = tid + j * 256;
      const int hp = i >> 2, q = i & 3;
      const int img = hp / (HH2 * HW2), r = hp % (HH2 * HW2);
      const int iy = oy0 + r / HW2 - 1, ix = ox0 + r % HW2 - 1, b = img0 + img;
      g_ok[j] = i < n_pieces && b < p.B && iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
      g_off[j] = (uint32_t)((((int64_t)b * p.Hi + iy) * p.Wi + ix) * p.Cin * ESZ + q * 16);
      l_off[j] = i < n_pieces ? hp * PIX_PITCH + q * 16 : -1;
    }
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const char* wsrc = static_cast<const char*>(p.w) + (int64_t)cb * nchunks * TAPS * SLAB_TAP;

  for (int ch = 0; ch < nchunks; ++ch) {
    __syncthreads();  // previous chunk's LDS reads are done
    // weights: linear copy of the fragment-ordered slab
    for (int i = tid * 16; i < TAPS * SLAB_TAP; i += 256 * 16)
      *reinterpret_cast<uint4*>(w_lds + i) =
          *reinterpret_cast<const uint4*>(wsrc + (int64_t)ch * TAPS * SLAB_TAP + i);
    if constexpr (HALO) {
#pragma unroll
      for (int j = 0; j < MAX_HALO_PIECES; ++j) {
        if (l_off[j] >= 0) {
          uint4 v = make_uint4(0, 0, 0, 0);
          if (g_ok[j]) v = *reinterpret_cast<const uint4*>(in + g_off[j] + ch * CHUNK_BYTES);
          *reinterpret_cast<uint4*>(a_lds + l_off[j]) = v;
        }
      }
    }
#pragma unroll 1
    for (int tap = 0; tap < TAPS; ++tap) {
      const int kh = tap / KS, kw = tap % KS;
      if constexpr (!HALO) {
        if (tap > 0) __syncthreads();  // previous tap's reads done before overwrite
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = tid + j * 256;
          const int pidx = i >> 2, q = i & 3;
          const int img = pidx / (p.TH * p.TW), rem = pidx % (p.TH * p.TW);
          const int oy = oy0 + rem / p.TW, ox = ox0 + rem % p.TW, b = img0 + img;
          const int iy = oy * STRIDE + kh - PAD, ix = ox * STRIDE + kw - PAD;
          uint4 v = make_uint4(0, 0, 0, 0);
          if (b < p.B && iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi)
            v = *reinterpret_cast<const uint4*>(
                in + (((int64_t)b * p.Hi + iy) * p.Wi + ix) * p.Cin * ESZ + ch * CHUNK_BYTES + q * 16);
          *reinterpret_cast<uint4*>(a_lds + pidx * PIX_PITCH + q * 16) = v;
        }
      }
      if (!HALO || tap == 0) __syncthreads();
      const int tap_off = HALO ? (kh * HW2 + kw) * PIX_PITCH : 0;
      const char* wt = w_lds + tap * SLAB_TAP + lane * 16;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const uint4 a0 = *reinterpret_cast<const uint4*>(wt + (ks * 2 + 0) * FRAG_BYTES);
        const uint4 a1 = *reinterpret_cast<const uint4*>(wt + (ks * 2 + 1) * FRAG_BYTES);
        const uint4 b0 = *reinterpret_cast<const uint4*>(a_lds + b_off[0] + tap_off + ks * 32);
        const uint4 b1 = *reinterpret_cast<const uint4*>(a_lds + b_off[1] + tap_off + ks * 32);
        mma_frag<T>(acc[0][0], a0, b0);
        mma_frag<T>(acc[0][1], a0, b1);
        mma_frag<T>(acc[1][0], a1, b0);
        mma_frag<T>(acc[1][1], a1, b1);
      }
    }
  }

  // epilogue
  const T* res = static_cast<const T*>(p.res);
  T* out = static_cast<T*>(p.out);
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    if (pimg[nt] < p.B && poy[nt] < p.Ho && pox[nt] < p.Wo) {
      const int64_t pix = ((int64_t)pimg[nt] * p.Ho + poy[nt]) * p.Wo + pox[nt];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int co = cb * 64 + mt * 32 + g * 8 + 4 * (lane >> 5);
          store_group<T>(acc[mt][nt], g, p.scale, p.shift, res, out, pix * p.Cout + co, co, p.relu != 0);
        }
    }
  }
}

#include "conv3x3.inc"
#include "stem_pool.inc"

// ---------------------------------------------------------------------------
// Stem: conv 7x7 / stride 2 / pad 3, 3 -> 64, + BN + ReLU, output NHWC.
// Source is either the model input float32 NCHW [n,3,P,P] (SRC_NCHW) or the uint8
// HWC slide plus tile origins (SRC_U8: gather and /255 fused, a2+a5+a6).
// Workgroup = 64 couts x (8 x 32 output pixels).  The 21 x 69 input window is
// staged in LDS in HWC element order, normalised; a tap row kh contributes a
// 32-wide (bf16) / 22-wide (f32) k-slice: slot 0 and the slots past 21 carry zero
// weights, which keeps every fragment read 4-byte aligned (element 6*tx + i).
// ---------------------------------------------------------------------------
constexpr int STEM_TH = 8, STEM_TW = 32;
constexpr int STEM_ROWS = 2 * STEM_TH + 5;   // 21 input rows
constexpr int STEM_ROWE = 224;               // elements per staged row (>= 6*31 + 32)
constexpr int STEM_REAL = 1 + 3 * (2 * STEM_TW + 5);  // 208 meaningful elements (slot 0 = dummy)

struct StemParams {
  const float* x_nchw; const uint8_t* slide; const int32_t* yx; int64_t row_bytes;
  const void* w; const float* scale; const float* shift; void* out;
  int B, P, Ho, Wo, tiles_y, tiles_x;
  int relu;
};

template <typename T, bool SRC_U8>
__global__ __launch_bounds__(256, 2) void stem_kernel(const StemParams p) {
  constexpr int ESZ = ElemTraits<T>::ESZ;
  constexpr int W_BYTES = (ESZ == 2) ? 7 * 2 * 2 * FRAG_BYTES : 7 * 11 * 2 * 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* w_lds = smem;
  T* e_lds = reinterpret_cast<T*>(smem + W_BYTES);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_per_img = p.tiles_y * p.tiles_x;
  const int b = blockIdx.x / tiles_per_img, tile = blockIdx.x % tiles_per_img;
  const int oy0 = (tile / p.tiles_x) * STEM_TH, ox0 = (tile % p.tiles_x) * STEM_TW;
  const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;

  for (int i = tid * 16; i < W_BYTES; i += 256 * 16)
    *reinterpret_cast<uint4*>(w_lds + i) = *reinterpret_cast<const uint4*>(static_cast<const char*>(p.w) + i);

  int ty0 = 0, tx0 = 0;
  if constexpr (SRC_U8) { ty0 = p.yx[2 * b]; tx0 = p.yx[2 * b + 1]; }
  // window staging in two phases: every load of the thread's 19 elements is issued before the first LDS store (a load + store per
  // iteration of a rolled loop serialised on the load latency: 18 round trips per tile, ~90 % of the bf16 kernel's time in training)
  constexpr int NE = STEM_ROWS * STEM_ROWE;
  auto fetch = [&](int i) __attribute__((always_inline)) -> float {   // element i of the window image (raw value; 0 outside the image)
    const int r = i / STEM_ROWE, e = i % STEM_ROWE;
    const int q = e - 1, ix = ix0 + q / 3, c = q % 3, iy = iy0 + r;
    float x = 0.f;
    if (i < NE && e >= 1 && e < STEM_REAL && iy >= 0 && iy < p.P && ix >= 0 && ix < p.P) {
      if constexpr (SRC_U8) x = (float)p.slide[(int64_t)(ty0 + iy) * p.row_bytes + (int64_t)(tx0 + ix) * 3 + c];
      else x = p.x_nchw[(((int64_t)b * 3 + c) * p.P + iy) * p.P + ix];
    }
    return x;
  };
  if constexpr (ESZ == 2) {   // element pairs: one 4-byte LDS store per two elements
    constexpr int NP = NE / 2, NIT = (NP + 255) / 256;
    float v0[NIT], v1[NIT];
#pragma unroll
    for (int k = 0; k < NIT; ++k) { const int j = tid + 256 * k; v0[k] = fetch(j < NP ? 2 * j : NE); v1[k] = fetch(j < NP ? 2 * j + 1 : NE); }
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
      const int j = tid + 256 * k;
      const float x0 = SRC_U8 ? div255f((uint32_t)v0[k]) : v0[k], x1 = SRC_U8 ? div255f((uint32_t)v1[k]) : v1[k];
      if (j < NP) reinterpret_cast<uint32_t*>(e_lds)[j] = f32_to_bf16(x0) | (f32_to_bf16(x1) << 16);
    }
  } else {
    constexpr int NIT = (NE + 255) / 256;
    float v[NIT];
#pragma unroll
    for (int k = 0; k < NIT; ++k) v[k] = fetch(tid + 256 * k);
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
      const int i = tid + 256 * k;
      if (i < NE) reinterpret_cast<float*>(e_lds)[i] = SRC_U8 ? div255f((uint32_t)v[k]) : v[k];
    }
  }
  __syncthreads();

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int tx = lane & 31, h = lane >> 5;
  // n-tile nt = output row ty = 2*wave + nt; input row for tap row kh: 2*ty + kh
#pragma unroll 1
  for (int kh = 0; kh < 7; ++kh) {
    if constexpr (ESZ == 2) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const char* wt = w_lds + ((kh * 2 + t) * 2) * FRAG_BYTES + lane * 16;
        const uint4 a0 = *reinterpret_cast<const uint4*>(wt);
        const uint4 a1 = *reinterpret_cast<const uint4*>(wt + FRAG_BYTES);
        uint4 bb[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          const int row = 2 * (2 * wave + nt) + kh;
          const uint32_t* src = reinterpret_cast<const uint32_t*>(
              reinterpret_cast<const char*>(e_lds) + (row * STEM_ROWE + 6 * tx + 16 * t + 8 * h) * 2);
          bb[nt] = make_uint4(src[0], src[1], src[2], src[3]);
        }
        mma_frag<T>(acc[0][0], a0, bb[0]);
        mma_frag<T>(acc[0][1], a0, bb[1]);
        mma_frag<T>(acc[1][0], a1, bb[0]);
        mma_frag<T>(acc[1][1], a1, bb[1]);
      }
    } else {
#pragma unroll
      for (int s = 0; s < 11; ++s) {
        const float* wt = reinterpret_cast<const float*>(w_lds) + ((kh * 11 + s) * 2) * 64 + lane;
        const float a0 = wt[0], a1 = wt[64];
        float bv[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          const int row = 2 * (2 * wave + nt) + kh;
          bv[nt] = reinterpret_cast<const float*>(e_lds)[row * STEM_ROWE + 6 * tx + 2 * s + h];
        }
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv[0], acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv[1], acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv[0], acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv[1], acc[1][1], 0, 0, 0);
      }
    }
  }

  T* out = static_cast<T*>(p.out);
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int oy = oy0 + 2 * wave + nt, ox = ox0 + tx;
    if (oy < p.Ho && ox < p.Wo) {
      const int64_t pix = ((int64_t)b * p.Ho + oy) * p.Wo + ox;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int co = mt * 32 + g * 8 + 4 * h;
          store_group<T>(acc[mt][nt], g, p.scale, p.shift, (const T*)nullptr, out, pix * 64 + co, co, p.relu != 0);
        }
    }
  }
}

// ---------------------------------------------------------------------------
// maxpool 3x3 / stride 2 / pad 1, NHWC; one thread = 16 bytes of channels.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void maxpool_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                      int B, int Hi, int Wi, int C, int Ho, int Wo) {
  constexpr int EPV = 16 / (int)sizeof(T);
  const int cv = C / EPV;
  const int64_t total = (int64_t)B * Ho * Wo * cv;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % cv);
    int64_t r = i / cv;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    float m[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) m[e] = -INFINITY;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int iy = 2 * oy + dy - 1;
      if (iy < 0 || iy >= Hi) continue;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int ix = 2 * ox + dx - 1;
        if (ix < 0 || ix >= Wi) continue;
        const uint4 v = *reinterpret_cast<const uint4*>(in + (((int64_t)b * Hi + iy) * Wi + ix) * C + c * EPV);
        const uint32_t u[4] = {v.x, v.y, v.z, v.w};
        if constexpr (sizeof(T) == 2) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            m[2 * e] = fmaxf(m[2 * e], bf16_bits_to_f32(u[e] & 0xFFFFu));
            m[2 * e + 1] = fmaxf(m[2 * e + 1], bf16_bits_to_f32(u[e] >> 16));
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], __uint_as_float(u[e]));
        }
      }
    }
    uint4 o;
    if constexpr (sizeof(T) == 2) {
      o.x = f32_to_bf16(m[0]) | (f32_to_bf16(m[1]) << 16); o.y = f32_to_bf16(m[2]) | (f32_to_bf16(m[3]) << 16);
      o.z = f32_to_bf16(m[4]) | (f32_to_bf16(m[5]) << 16); o.w = f32_to_bf16(m[6]) | (f32_to_bf16(m[7]) << 16);
    } else {
      o = make_uint4(__float_as_uint(m[0]), __float_as_uint(m[1]), __float_as_uint(m[2]), __float_as_uint(m[3]));
    }
    *reinterpret_cast<uint4*>(out + i * EPV) = o;
  }
}

// ---------------------------------------------------------------------------
// global average pool + fc: one workgroup per image; f32 arithmetic.
// FEAT: the pooled vector also goes to feat[image][C] (dh_resnet18_features_tiles), and a null `logits` skips the fc; the pooled
// values and the logits are those of the FEAT = false instantiation, which forward / forward_tiles launch.
// ---------------------------------------------------------------------------
template <typename T, bool FEAT = false>
__global__ __launch_bounds__(256) void avgpool_fc_kernel(const T* __restrict__ in, int HW, int C, int blocked,
                                                         const float* __restrict__ fc_w,
                                                         const float* __restrict__ fc_b, int n_cls,
                                                         float* __restrict__ logits, float* __restrict__ feat = nullptr) {
  // one workgroup per image; lane = 16 bytes of channels, waves split the pixels (C == 512:
  // bf16 -> 64 lanes x 8 channels per pixel; f32 -> 128 lanes x 4 channels, 2 pixel groups)
  constexpr int EPV = 16 / (int)sizeof(T);
  __shared__ float part[4][512];
  __shared__ float pooled[512];
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int lanes_per_px = C / EPV;               // 64 or 128
  const int groups = 256 / lanes_per_px;          // 4 or 2 pixel groups
  const int grp = tid / lanes_per_px, cl = tid % lanes_per_px;
  float s[EPV];
#pragma unroll
  for (int e = 0; e < EPV; ++e) s[e] = 0.f;
  for (int q = grp; q < HW; q += groups) {
    // NHWC, or channel-blocked [image][C/32][HW][32] (a lane's 16 bytes never straddle a 32-channel chunk)
    const int64_t off = blocked ? (int64_t)b * HW * C + (int64_t)((cl * EPV) >> 5) * HW * 32 + q * 32 + ((cl * EPV) & 31)
                                : ((int64_t)b * HW + q) * C + cl * EPV;
    const uint4 v = *reinterpret_cast<const uint4*>(in + off);
    const uint32_t u[4] = {v.x, v.y, v.z, v.w};
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { s[2 * e] += bf16_bits_to_f32(u[e] & 0xFFFFu); s[2 * e + 1] += bf16_bits_to_f32(u[e] >> 16); }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] += __uint_as_float(u[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < EPV; ++e) part[grp][cl * EPV + e] = s[e];
  __syncthreads();
  const float inv = 1.0f / (float)HW;
  for (int c = tid; c < C; c += 256) {
    float t = 0.f;
    for (int g = 0; g < groups; ++g) t += part[g][c];
    pooled[c] = t * inv;
    if constexpr (FEAT) feat[(int64_t)b * C + c] = t * inv;
  }
  if constexpr (FEAT) {
    if (!logits) return;   // uniform for the launch
  }
  __syncthreads();
  for (int k = 0; k < n_cls; ++k) {
    float t = 0.f;
    for (int c = tid; c < C; c += 256) t = __builtin_fmaf(pooled[c], fc_w[k * C + c], t);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = t;
    __syncthreads();
    if (tid == 0) logits[(int64_t)b * n_cls + k] = red[0] + red[1] + red[2] + red[3] + fc_b[k];
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
}  // namespace

#include "net_desc.inc"

namespace {

inline uint16_t host_bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7F800000u) == 0x7F800000u && (u & 0x7FFFFFu)) return (uint16_t)((u >> 16) | 0x40);
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// Pack [cout][cin][ks][ks] f32 into fragment order:
//   [cb = cout/64][chunk][tap][ks2][mt][lane][16 B];  element e of lane l:
//   co = 64cb + 32mt + (l&31); ci = chunk*CPC + ks2*(CPC/2) + (l>>5)*EPL + e.
void pack_conv_weights(const float* w, int cout, int cin, int ks, int esz, std::vector<uint8_t>& out) {
  const int cpc = CHUNK_BYTES / esz, epl = 16 / esz, taps = ks * ks;
  const int ncb = cout / 64, nch = cin / cpc;
  out.assign((size_t)ncb * nch * taps * SLAB_TAP, 0);
  size_t o = 0;
  for (int cb = 0; cb < ncb; ++cb)
    for (int ch = 0; ch < nch; ++ch)
      for (int tap = 0; tap < taps; ++tap)
        for (int k2 = 0; k2 < 2; ++k2)
          for (int mt = 0; mt < 2; ++mt)
            for (int l = 0; l < 64; ++l)
              for (int e = 0; e < epl; ++e) {
                const int co = cb * 64 + mt * 32 + (l & 31);
                const int ci = ch * cpc + k2 * (cpc / 2) + (l >> 5) * epl + e;
                const float v = w[((size_t)co * cin + ci) * taps + tap];
                if (esz == 4) { memcpy(&out[o], &v, 4); o += 4; }
                else { const uint16_t hb = host_bf16(v); memcpy(&out[o], &hb, 2); o += 2; }
              }
}

// The wide stride-2 variant's packing (conv3x3.inc, HALF): [cb = cout/128][hc = cin/16][tap][mt (4)][lane][8 bf16]; element e of lane l:
//   co = 128 cb + 32 mt + (l & 31); ci = 16 hc + 8 (l >> 5) + e.   (ks = 1: one "tap" per (cb, hc): 4 KiB)
void pack_conv_weights_wide(const float* w, int cout, int cin, int ks, std::vector<uint8_t>& out) {
  const int taps = ks * ks, ncb = cout / 128, nhc = cin / 16;
  out.assign((size_t)ncb * nhc * taps * SLAB_TAP, 0);
  size_t o = 0;
  for (int cb = 0; cb < ncb; ++cb)
    for (int hc = 0; hc < nhc; ++hc)
      for (int tap = 0; tap < taps; ++tap)
        for (int mt = 0; mt < 4; ++mt)
          for (int l = 0; l < 64; ++l)
            for (int e = 0; e < 8; ++e) {
              const int co = cb * 128 + mt * 32 + (l & 31), ci = hc * 16 + (l >> 5) * 8 + e;
              const uint16_t hb = host_bf16(w[((size_t)co * cin + ci) * taps + tap]);
              memcpy(&out[o], &hb, 2); o += 2;
            }
}

// Stem weights [64][3][7][7].  bf16: [kh][t][mt][lane][8], slot i = 16t + 8h + j,
// value W[co][c][kh][kw] for i-1 = 3kw + c in [0,21), else 0.
// f32: [kh][s][mt][lane], slot i = 2s + h.
void pack_stem_weights(const float* w, int esz, std::vector<uint8_t>& out) {
  auto slot = [&](int co, int kh, int i) -> float {
    if (i < 1 || i > 21) return 0.f;
    const int kw = (i - 1) / 3, c = (i - 1) % 3;
    return w[((size_t)(co * 3 + c) * 7 + kh) * 7 + kw];
  };
  if (esz == 2) {
    out.assign((size_t)7 * 2 * 2 * FRAG_BYTES, 0);
    size_t o = 0;
    for (int kh = 0; kh < 7; ++kh)
      for (int t = 0; t < 2; ++t)
        for (int mt = 0; mt < 2; ++mt)
          for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 8; ++j) {
              const uint16_t hb = host_bf16(slot(mt * 32 + (l & 31), kh, 16 * t + 8 * (l >> 5) + j));
              memcpy(&out[o], &hb, 2); o += 2;
            }
  } else {
    out.assign((size_t)7 * 11 * 2 * 256, 0);
    size_t o = 0;
    for (int kh = 0; kh < 7; ++kh)
      for (int s = 0; s < 11; ++s)
        for (int mt = 0; mt < 2; ++mt)
          for (int l = 0; l < 64; ++l) {
            const float v = slot(mt * 32 + (l & 31), kh, 2 * s + (l >> 5));
            memcpy(&out[o], &v, 4); o += 4;
          }
  }
}

// Stem weights for the fused bf16 stem (stem_pool.inc): [k-step (11)][cout half][lane][8], two kernel rows per three k-steps
// (sp_kslot maps a k-slot to its kernel row and 24-slot row image; slot s carries W[co][c][kh][kw] for s-1 = 3kw + c in [0,21)).
void pack_stem_pool_weights(const float* w, std::vector<uint8_t>& out) {
  out.assign((size_t)SP_WBYTES, 0);
  size_t o = 0;
  for (int ks = 0; ks < SP_KS; ++ks)
    for (int mt = 0; mt < 2; ++mt)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) {
          int kh, sl;
          sp_kslot(ks, l >> 5, j, &kh, &sl);
          float v = 0.f;
          if (kh >= 0 && sl >= 1 && sl <= 21) {
            const int co = mt * 32 + (l & 31), kw = (sl - 1) / 3, c = (sl - 1) % 3;
            v = w[((size_t)(co * 3 + c) * 7 + kh) * 7 + kw];
          }
          const uint16_t hb = host_bf16(v);
          memcpy(&out[o], &hb, 2); o += 2;
        }
}

// Inverses of the three packers (test hooks: the operand the kernels read, back as float32 [cout][cin][ks][ks]).  Slots that carry no
// weight are skipped; an element no slot carries stays as the caller left it.
inline float packed_value(const std::vector<uint8_t>& in, size_t o, int esz) {
  float v;
  if (esz == 4) { memcpy(&v, &in[o], 4); return v; }
  uint16_t hb; memcpy(&hb, &in[o], 2);
  const uint32_t u = (uint32_t)hb << 16;
  memcpy(&v, &u, 4);
  return v;
}

void unpack_conv_weights(const std::vector<uint8_t>& in, int cout, int cin, int ks, int esz, float* w) {
  const int cpc = CHUNK_BYTES / esz, epl = 16 / esz, taps = ks * ks;
  const int ncb = cout / 64, nch = cin / cpc;
  size_t o = 0;
  for (int cb = 0; cb < ncb; ++cb)
    for (int ch = 0; ch < nch; ++ch)
      for (int tap = 0; tap < taps; ++tap)
        for (int k2 = 0; k2 < 2; ++k2)
          for (int mt = 0; mt < 2; ++mt)
            for (int l = 0; l < 64; ++l)
              for (int e = 0; e < epl; ++e, o += esz) {
                const int co = cb * 64 + mt * 32 + (l & 31);
                const int ci = ch * cpc + k2 * (cpc / 2) + (l >> 5) * epl + e;
                w[((size_t)co * cin + ci) * taps + tap] = packed_value(in, o, esz);
              }
}

void unpack_stem_weights_f32(const std::vector<uint8_t>& in, float* w) {
  size_t o = 0;
  for (int kh = 0; kh < 7; ++kh)
    for (int s = 0; s < 11; ++s)
      for (int mt = 0; mt < 2; ++mt)
        for (int l = 0; l < 64; ++l, o += 4) {
          const int i = 2 * s + (l >> 5), co = mt * 32 + (l & 31);
          if (i < 1 || i > 21) continue;
          const int kw = (i - 1) / 3, c = (i - 1) % 3;
          w[((size_t)(co * 3 + c) * 7 + kh) * 7 + kw] = packed_value(in, o, 4);
        }
}

void unpack_stem_pool_weights(const std::vector<uint8_t>& in, float* w) {
  size_t o = 0;
  for (int ks = 0; ks < SP_KS; ++ks)
    for (int mt = 0; mt < 2; ++mt)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j, o += 2) {
          int kh, sl;
          sp_kslot(ks, l >> 5, j, &kh, &sl);
          if (kh < 0 || sl < 1 || sl > 21) continue;
          const int co = mt * 32 + (l & 31), kw = (sl - 1) / 3, c = (sl - 1) % 3;
          w[((size_t)(co * 3 + c) * 7 + kh) * 7 + kw] = packed_value(in, o, 2);
        }
}

// Optional in-library timing of the dominant kernel (3x3 stride-1 conv): HIP events on
// the launch stream around sampled launches, summed by dh_profile_stop (bench.py's
// `roofline.achieved`).  Off by default; costs nothing when off.
bool g_stamps_on = false;
unsigned long long* g_stamps_dev = nullptr;

struct Profiler {
  bool on = false;
  int every = 1, counter = 0;
  std::vector<hipEvent_t> ev;  // pairs
  size_t used = 0;
  double flops = 0.0;
} g_prof;

// ---- per-device host state ---------------------------------------------------------------------------------
std::mutex g_host_mu;   // guards every cache below (ctypes releases the GIL: two threads may be in here)
inline int current_device() { int d = 0; (void)hipGetDevice(&d); return d; }

// hipFuncSetAttribute is per device: remember which (kernel, device) pairs are done
int ensure_dyn_lds(const void* fn, int bytes) {
  static std::set<std::pair<const void*, int>> done;
  const std::pair<const void*, int> key(fn, current_device());
  std::lock_guard<std::mutex> lk(g_host_mu);
  if (done.count(key)) return DH_OK;
  DH_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  done.insert(key);
  return DH_OK;
}

template <typename T, int KS, int STRIDE, bool HALO>
int launch_conv(const ConvParams& p, hipStream_t st) {
  const int npx_lds = HALO ? p.IMGS * (p.TH + 2) * (p.TW + 2) : 256;
  const size_t lds = (size_t)KS * KS * SLAB_TAP + (size_t)npx_lds * PIX_PITCH;
  const int blocks_per_img = p.tiles_y * p.tiles_x;
  const int groups = ((p.B + p.IMGS - 1) / p.IMGS) * blocks_per_img;
  const int grid = groups * (p.Cout / 64);
  if (int rc = ensure_dyn_lds(reinterpret_cast<const void*>(&conv_kernel<T, KS, STRIDE, HALO>), 96 * 1024)) return rc;
  hipLaunchKernelGGL((conv_kernel<T, KS, STRIDE, HALO>), dim3(grid), dim3(256), lds, st, p);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

std::map<int, void*> g_zero_page;  // per device: 1 KiB of zeros, the DMA source of padding pixels
int zero_page(const void** out) {
  const int dev = current_device();
  std::lock_guard<std::mutex> lk(g_host_mu);
  auto it = g_zero_page.find(dev);
  if (it == g_zero_page.end()) {
    void* z = nullptr;
    DH_HIP(hipMalloc(&z, 1024));
    DH_HIP(hipMemset(z, 0, 1024));
    it = g_zero_page.emplace(dev, z).first;
  }
  *out = it->second;
  return DH_OK;
}

#include "conv3x3_launch.inc"   // plan, tables, launch of the 3x3 kernels: launch_conv3x3, launch_dgrad_s2, stamp_row

template <typename T>
int run_conv(const ConvLayer& L, const void* in, const void* res, void* out, int B, int Hi, int Wi,
             bool relu, hipStream_t st, int* Ho_out, int* Wo_out, bool blocked = false, bool out16 = false) {
  const int pad = L.ks / 2;
  const int Ho = (Hi + 2 * pad - L.ks) / L.stride + 1, Wo = (Wi + 2 * pad - L.ks) / L.stride + 1;
  *Ho_out = Ho; *Wo_out = Wo;
  DH_REQUIRE((int64_t)B * Hi * Wi * L.cin * (int64_t)sizeof(T) < ((int64_t)1 << 32),
             "conv %s: input larger than 4 GiB, reduce the batch", L.name.c_str());
  DH_REQUIRE(!out16 || (L.ks == 3 && L.stride == 1), "conv %s: only the stride-1 3x3 kernel writes 16-channel planes", L.name.c_str());
  if (L.ks == 3 && (L.stride == 1 || L.stride == 2)) return launch_conv3x3<T>(L.stride, L, in, res, out, B, Hi, Wi, relu, st, Ho, Wo, nullptr, nullptr, blocked, false, out16);
  DH_REQUIRE(!blocked, "conv %s: only the 3x3 kernels read the channel-blocked layout", L.name.c_str());
  ConvParams p;
  p.in = in; p.w = L.w_dev; p.scale = L.scale_dev; p.shift = L.shift_dev; p.res = res; p.out = out;
  p.B = B; p.Hi = Hi; p.Wi = Wi; p.Cin = L.cin; p.Cout = L.cout; p.Ho = Ho; p.Wo = Wo;
  if (p.Ho > 8 || p.Wo > 8) { p.TH = 16; p.TW = 16; p.IMGS = 1; }
  else { p.TH = 8; p.TW = 8; p.IMGS = 4; }
  p.tiles_y = (p.Ho + p.TH - 1) / p.TH; p.tiles_x = (p.Wo + p.TW - 1) / p.TW;
  p.relu = relu ? 1 : 0;
  if (L.ks == 1 && L.stride == 2) return launch_conv<T, 1, 2, false>(p, st);
  dh::set_error("conv %s: unsupported shape", L.name.c_str());
  return DH_EINVAL;
}

int g_stem_pc_force = 0;   // dh_debug_stem_strip_width: 0 = by geometry, 15 / 16 = that strip width

// pooled columns per strip of the fused stem: 16 (strips joined by the seam pass) only where that saves a strip
int stem_pool_pc(int P) {
  const int H1 = (P + 6 - 7) / 2 + 1, H2 = (H1 + 2 - 3) / 2 + 1;
  if (g_stem_pc_force) return g_stem_pc_force;
  return (H2 + 15) / 16 < (H2 + 14) / 15 ? 16 : 15;
}

// bytes of the seam scratch of launch_stem_pool (0: the geometry has no seams)
size_t stem_seam_bytes(int B, int P) {
  const int H1 = (P + 6 - 7) / 2 + 1, H2 = (H1 + 2 - 3) / 2 + 1;
  return stem_pool_pc(P) == 16 ? (size_t)B * ((H2 + 15) / 16 - 1) * H2 * 64 * 2 : 0;
}

template <int PC>
int launch_stem_pool_pc(const StemPoolParams& sp, int grid, hipStream_t st) {
  int arc;
  if ((arc = ensure_dyn_lds(reinterpret_cast<const void*>(&stem_pool_kernel<true, false, PC>), SP_LDS)) ||
      (arc = ensure_dyn_lds(reinterpret_cast<const void*>(&stem_pool_kernel<true, true, PC>), SP_LDS)) ||
      (arc = ensure_dyn_lds(reinterpret_cast<const void*>(&stem_pool_kernel<false, false, PC>), SP_LDS))) return arc;
  if (sp.slide && sp.stamps) hipLaunchKernelGGL((stem_pool_kernel<true, true, PC>), dim3(grid), dim3(SP_T), SP_LDS, st, sp);
  else if (sp.slide) hipLaunchKernelGGL((stem_pool_kernel<true, false, PC>), dim3(grid), dim3(SP_T), SP_LDS, st, sp);
  else hipLaunchKernelGGL((stem_pool_kernel<false, false, PC>), dim3(grid), dim3(SP_T), SP_LDS, st, sp);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// fused bf16 stem (conv1 + bn1 + relu + maxpool) of `B` tiles -> channel-blocked [image][2][H2][W2][32] bf16.  `seam`: scratch of
// stem_seam_bytes(B, P) bytes, dead once the call's launches have run (may be null when that is 0)
int launch_stem_pool(const ConvLayer& stem, const float* x, const uint8_t* slide, int64_t slide_h, int64_t slide_w,
                     const int32_t* yx, int B, int P, void* out, void* seam, hipStream_t st) {
  const int H1 = (P + 6 - 7) / 2 + 1, H2 = (H1 + 2 - 3) / 2 + 1;
  const int pc = stem_pool_pc(P);
  StemPoolParams sp;
  DH_REQUIRE(!slide || slide_w < (1 << 24), "stem: slide rows of %lld pixels are not supported (< 2^24)", (long long)slide_w);
  sp.x_nchw = x; sp.slide = slide; sp.yx = yx; sp.row_bytes = slide_w * 3; sp.slide_bytes = slide_h * slide_w * 3;
  sp.w = stem.w_dev; sp.scale = stem.scale_dev; sp.shift = stem.shift_dev; sp.out = out;
  sp.B = B; sp.P = P; sp.Hc = H1; sp.Wc = H1; sp.Hp = H2; sp.Wp = H2;
  sp.tiles_y = (H2 + SP_PR - 1) / SP_PR; sp.tiles_x = (H2 + pc - 1) / pc;
  sp.seam = seam;
  const int nseam = pc == 16 ? sp.tiles_x - 1 : 0;
  DH_REQUIRE(!nseam || seam, "stem: %d strips of 16 pooled columns need a seam scratch", sp.tiles_x);
  sp.nstrips = B * sp.tiles_x;                 // a strip = one image x pc pooled columns, swept top to bottom
  const int grid = std::min(768, sp.nstrips);  // persistent: three 4-wave workgroups per CU
  sp.iters = ((sp.nstrips + grid - 1) / grid) * sp.tiles_y;
  sp.stamps = nullptr;
  if (g_stamps_on && slide)
    if (int rc = stamp_row(7, &sp.stamps)) return rc;
  if (int rc = pc == 16 ? launch_stem_pool_pc<16>(sp, grid, st) : launch_stem_pool_pc<15>(sp, grid, st)) return rc;
  if (nseam) {   // first pooled column of every strip but an image's first: fold in the neighbour's last conv column
    const int64_t total = (int64_t)B * nseam * H2 * 8;
    hipLaunchKernelGGL(stem_seam_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, static_cast<const void*>(seam),
                       static_cast<__bf16*>(out), total, nseam, H2, H2);
    DH_LAUNCH_CHECK();
  }
  return DH_OK;
}

}  // namespace

#include "infer_core.inc"
#include "cam.inc"

struct dh_train;
struct dh_resnet18 : InferNet {
  dh_train* train = nullptr;  // training state (train.inc), owned
  int dtype = DH_DTYPE_F32;
  int esz() const { return dtype == DH_DTYPE_F32 ? 4 : 2; }
};

namespace {

template <typename T>
int forward_impl(dh_resnet18* net, const float* x, const uint8_t* slide, int64_t slide_h, int64_t slide_w,
                 const int32_t* yx, int64_t n64, int P, float* logits, hipStream_t st, Tap* tap = nullptr, float* feat = nullptr,
                 float* cam = nullptr) {
  const int B = (int)n64;
  const int esz = (int)sizeof(T);
  const int H1 = (P + 6 - 7) / 2 + 1;       // stem out
  const int H2 = (H1 + 2 - 3) / 2 + 1;      // pool out
  const size_t stem_bytes = (size_t)B * H1 * H1 * 64 * esz;
  const size_t act_bytes = (size_t)B * H2 * H2 * 64 * esz;  // largest post-pool activation
  // BEFORE any launch: the conv schedule tables carry window byte offsets as 32-bit words (the stem and pool kernels index with
  // 64 bits) -- a launch whose largest conv input does not fit is refused here, not half-way through the network
  DH_REQUIRE(act_bytes < ((size_t)1 << 32),
             "resnet18 forward: %d tiles of %d x %d in %s make an activation larger than 4 GiB: use fewer tiles per launch", B, P, P,
             sizeof(T) == 2 ? "bf16" : "float32");
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t need = al(stem_bytes) + 3 * al(act_bytes);
  if (int rc = infer_workspace(net, need)) return rc;
  char* base = static_cast<char*>(net->ws);
  void* S = base;
  void* bufA = base + al(stem_bytes);
  void* bufB = base + al(stem_bytes) + al(act_bytes);
  void* bufC = base + al(stem_bytes) + 2 * al(act_bytes);

  if constexpr (sizeof(T) == 2) {
    // bf16: fused stem + BN + ReLU + maxpool (persistent, weights resident in LDS), straight into bufA.  The unfused stem's slot S
    // of the workspace is free in this path and holds the seam scratch ((tiles_x - 1) * H2 <= H1 * H1 pixels per image)
    DH_REQUIRE(stem_seam_bytes(B, P) <= al(stem_bytes), "resnet18 forward: seam scratch larger than the stem slot");
    if (int rc = launch_stem_pool(net->convs[0], x, slide, slide_h, slide_w, yx, B, P, bufA, S, st)) return rc;
    for (const char* nm : {"conv1", "maxpool"})   // the fused stem stores only the pooled map
      if (int rc = tap_after<T>(tap, nm, bufA, 64, H2, H2, 32, st)) return rc;
  } else {
  // stem
  {
    StemParams sp;
    sp.x_nchw = x; sp.slide = slide; sp.yx = yx; sp.row_bytes = slide_w * 3;
    sp.w = net->convs[0].w_dev; sp.scale = net->convs[0].scale_dev; sp.shift = net->convs[0].shift_dev;
    sp.out = S; sp.B = B; sp.P = P; sp.Ho = H1; sp.Wo = H1; sp.relu = 1;
    sp.tiles_y = (H1 + STEM_TH - 1) / STEM_TH; sp.tiles_x = (H1 + STEM_TW - 1) / STEM_TW;
    const size_t wb = esz == 2 ? (size_t)7 * 2 * 2 * FRAG_BYTES : (size_t)7 * 11 * 2 * 256;
    const size_t lds = wb + (size_t)STEM_ROWS * STEM_ROWE * esz;
    const int grid = B * sp.tiles_y * sp.tiles_x;
    if (slide) {
      if (int arc = ensure_dyn_lds(reinterpret_cast<const void*>(&stem_kernel<T, true>), 96 * 1024)) return arc;
      hipLaunchKernelGGL((stem_kernel<T, true>), dim3(grid), dim3(256), lds, st, sp);
    } else {
      if (int arc = ensure_dyn_lds(reinterpret_cast<const void*>(&stem_kernel<T, false>), 96 * 1024)) return arc;
      hipLaunchKernelGGL((stem_kernel<T, false>), dim3(grid), dim3(256), lds, st, sp);
    }
    DH_LAUNCH_CHECK();
    if (int rc = tap_after<T>(tap, "conv1", S, 64, H1, H1, 64, st)) return rc;
  }
  // maxpool
  {
    const int64_t total = (int64_t)B * H2 * H2 * (64 / (16 / esz));
    const int grid = (int)std::min<int64_t>((total + 255) / 256, 256 * 32);
    hipLaunchKernelGGL((maxpool_kernel<T>), dim3(grid), dim3(256), 0, st, static_cast<const T*>(S),
                       static_cast<T*>(bufA), B, H1, H1, 64, H2, H2);
    DH_LAUNCH_CHECK();
    if (int rc = tap_after<T>(tap, "maxpool", bufA, 64, H2, H2, 64, st)) return rc;
  }
  }
  // residual stages: X lives in bufA; T in bufB; downsample in bufC.  bf16 activations are channel-blocked
  // ([image][C/32][H][W][32], written that way by the fused stem), f32 activations NHWC.
  constexpr bool BLK = sizeof(T) == 2;
  int H = H2, W = H2;
  bool x16 = false;   // X holds the block input in 16-channel planes (written that way for the wide stride-2 kernel)
  void* X = bufA;     // block input / output; bufB: the block's intermediate; `other`: the third buffer
  const std::vector<BlockDesc>& blocks = net->desc->blocks;
  for (size_t bi = 0; bi < blocks.size(); ++bi) {
    const BlockDesc& b = blocks[bi];
    const bool has_ds = b.ds >= 0;
    const ConvLayer& c1 = net->convs[b.conv[0]];
    const ConvLayer& c2 = net->convs[b.conv[1]];
    void* other = X == bufA ? bufC : bufA;
    int Ho, Wo, h2, w2;
    int rc;
    const void* resid = X;
    if (has_ds) {
      // conv1 (3x3/2 + BN + ReLU) and the 1x1/2 downsample (+ BN) of the block in ONE launch
      Ho = (H + 2 - 3) / 2 + 1; Wo = (W + 2 - 3) / 2 + 1;
      rc = launch_conv3x3<T>(2, c1, X, nullptr, bufB, B, H, W, true, st, Ho, Wo, &net->convs[b.ds], other, BLK, x16, false);
      if (rc) return rc;
      if ((rc = tap_after<T>(tap, net->convs[b.ds].name, other, c1.cout, Ho, Wo, BLK ? 32 : c1.cout, st))) return rc;
      resid = other;
    } else {
      DH_REQUIRE(!x16, "resnet18 forward: only a downsample block reads 16-channel planes");
      rc = run_conv<T>(c1, X, nullptr, bufB, B, H, W, true, st, &Ho, &Wo, BLK);
      if (rc) return rc;
    }
    if ((rc = tap_after<T>(tap, c1.name, bufB, c1.cout, Ho, Wo, BLK ? 32 : c1.cout, st))) return rc;
    // the block that follows starts with a stride-2 conv on the wide kernel: this block's output goes out in 16-channel planes
    x16 = false;
    if (bi + 1 < blocks.size() && blocks[bi + 1].stride == 2) {
      const BlockDesc& nb = blocks[bi + 1];
      x16 = BLK && s2_wide_eligible(net->convs[nb.conv[0]], net->convs[nb.ds], esz, (Wo + 2 - 3) / 2 + 1);
    }
    // conv2 + residual.  Same layout: in place over the residual (every lane reads the elements it then writes).  16-channel planes out,
    // 32-channel planes in: the two layouts put different pixels at the same address -- the output goes to the third buffer
    void* O = X;
    if (has_ds) O = X;                 // the block input is dead once conv1 and the downsample have run (stream order)
    else if (x16) O = other;
    rc = run_conv<T>(c2, bufB, resid, O, B, Ho, Wo, true, st, &h2, &w2, BLK, x16);
    if (rc) return rc;
    if ((rc = tap_after<T>(tap, c2.name, O, c2.cout, Ho, Wo, x16 ? 16 : BLK ? 32 : c2.cout, st))) return rc;
    X = O;
    H = Ho; W = Wo;
  }
  if (feat)   // dh_resnet18_features_tiles: the same head, the pooled vector stored as well
    hipLaunchKernelGGL((avgpool_fc_kernel<T, true>), dim3(B), dim3(256), 0, st, static_cast<const T*>(X), H * W,
                       net->desc->feat, BLK ? 1 : 0, net->fc_w_dev, net->fc_b_dev, net->n_classes, logits, feat);
  else if (logits)   // null only in dh_resnet18_cam_tiles without logits
    hipLaunchKernelGGL((avgpool_fc_kernel<T, false>), dim3(B), dim3(256), 0, st, static_cast<const T*>(X), H * W,
                       net->desc->feat, BLK ? 1 : 0, net->fc_w_dev, net->fc_b_dev, net->n_classes, logits, nullptr);
  DH_LAUNCH_CHECK();
  if (cam) return launch_cam_head<T>(net, X, B, H * W, cam, st);   // dh_resnet18_cam_tiles: fc per position of the same activation
  return DH_OK;
}

// the forward in the handle's dtype
int r18_forward(dh_resnet18* net, const float* x, const uint8_t* slide, int64_t slide_h, int64_t slide_w, const int32_t* yx, int64_t n,
                int P, float* logits, hipStream_t st, Tap* tap = nullptr, float* feat = nullptr, float* cam = nullptr) {
  return net->dtype == DH_DTYPE_F32 ? forward_impl<float>(net, x, slide, slide_h, slide_w, yx, n, P, logits, st, tap, feat, cam)
                                    : forward_impl<__bf16>(net, x, slide, slide_h, slide_w, yx, n, P, logits, st, tap, feat, cam);
}

int r18_check_forward(const InferNet* net, int64_t n, int32_t P, const void* logits, const char*) {
  DH_REQUIRE(net && (logits || n == 0), "resnet18 forward: null argument");
  DH_REQUIRE(net->finalized, "resnet18 forward: call dh_resnet18_finalize after setting parameters");
  DH_REQUIRE(n >= 0 && n <= 4096, "resnet18 forward: batch %lld out of range [0, 4096]", (long long)n);
  DH_REQUIRE(P >= 32 && P <= 1024, "resnet18 forward: patch %d out of range [32, 1024]", P);
  return DH_OK;
}

const InferEngine R18_ENGINE = {"resnet18", r18_check_forward, 1, false};

}  // namespace

extern "C" int dh_resnet18_create(dh_resnet18** out, int32_t n_classes, int32_t dtype) {
  DH_REQUIRE(out != nullptr, "resnet18 create: null output");
  DH_REQUIRE(n_classes > 0 && n_classes <= 1024, "resnet18 create: n_classes=%d", n_classes);
  DH_REQUIRE(dtype == DH_DTYPE_F32 || dtype == DH_DTYPE_BF16, "resnet18 create: bad dtype %d", dtype);
  if (int erc = dh::env_check()) return erc;   // a mistyped DH_* switch stops here, named by dh_last_error()
  auto* net = new dh_resnet18();
  infer_init(net, "resnet18", n_classes);
  net->dtype = dtype;
  *out = net;
  return DH_OK;
}

extern "C" int dh_resnet18_train_end(dh_resnet18* net);
extern "C" void dh_resnet18_destroy(dh_resnet18* net) {
  if (!net) return;
  if (net->train) (void)dh_resnet18_train_end(net);
  infer_free(net);
  delete net;
}

extern "C" int dh_resnet18_set_param(dh_resnet18* net, const char* name, const float* data,
                                     int64_t n_elem) {
  return infer_set_param(R18_ENGINE, net, name, data, n_elem);
}

extern "C" int dh_resnet18_finalize(dh_resnet18* net, void* stream) {
  (void)stream;
  int rc = infer_finalize_begin(R18_ENGINE, net);   // every parameter is checked before any upload
  if (rc) return rc;
  const int esz = net->esz();
  std::vector<double> scale, shift;
  for (size_t i = 0; i < net->convs.size(); ++i) {
    ConvLayer& c = net->convs[i];
    const std::vector<float>& w = *infer_param(net, c.name + ".weight");
    std::vector<uint8_t> packed;
    if (i == 0 && esz == 2) pack_stem_pool_weights(w.data(), packed);   // bf16 inference runs the fused stem only
    else if (i == 0) pack_stem_weights(w.data(), esz, packed);
    else pack_conv_weights(w.data(), c.cout, c.cin, c.ks, esz, packed);
    if ((rc = upload(packed, &c.w_dev))) return rc;
    // the wide stride-2 variant's packing: a 3x3 / stride-2 conv of a downsample block and that block's 1x1 / stride-2 conv (bf16 inference)
    const bool wide3 = esz == 2 && c.ks == 3 && c.stride == 2 && c.cout % 128 == 0 && c.cin % 16 == 0;
    const bool wide1 = esz == 2 && c.ks == 1 && c.stride == 2 && c.cout % 128 == 0 && c.cin % 16 == 0;
    if (wide3 || wide1) {
      std::vector<uint8_t> packed2;
      pack_conv_weights_wide(w.data(), c.cout, c.cin, c.ks, packed2);
      if ((rc = upload(packed2, &c.w2_dev))) return rc;
    }
    infer_bn_affine(net, c, scale, shift);
    const std::vector<float> sc(scale.begin(), scale.end()), sh(shift.begin(), shift.end());
    if ((rc = upload(sc, reinterpret_cast<void**>(&c.scale_dev))) || (rc = upload(sh, reinterpret_cast<void**>(&c.shift_dev)))) return rc;
  }
  return infer_finalize_end(net);
}

extern "C" int dh_resnet18_forward(dh_resnet18* net, const float* x, int64_t n, int32_t P,
                                   float* logits, void* stream) {
  int rc = r18_check_forward(net, n, P, logits, nullptr);
  if (rc) return rc;
  if (n == 0) return DH_OK;
  DH_REQUIRE(x != nullptr, "resnet18 forward: null input");
  return r18_forward(net, x, nullptr, 0, 0, nullptr, n, P, logits, dh::as_stream(stream));
}

extern "C" int dh_resnet18_forward_tiles(dh_resnet18* net, const uint8_t* slide, int64_t h, int64_t w,
                                         const int32_t* yx, int64_t n, int32_t P, float* logits, void* stream) {
  return infer_tiles(R18_ENGINE, net, slide, h, w, yx, n, P, nullptr, logits, "resnet18 forward_tiles", [&](Tap* tap) {
    return r18_forward(net, nullptr, slide, h, w, yx, n, P, logits, dh::as_stream(stream), tap);
  });
}

extern "C" int dh_resnet18_features_tiles(dh_resnet18* net, const uint8_t* slide, int64_t h, int64_t w,
                                          const int32_t* yx, int64_t n, int32_t P, float* feat, float* logits, void* stream) {
  return infer_tiles(R18_ENGINE, net, slide, h, w, yx, n, P, feat, feat, "resnet18 features_tiles", [&](Tap* tap) {
    return r18_forward(net, nullptr, slide, h, w, yx, n, P, logits, dh::as_stream(stream), tap, feat);
  });
}

extern "C" int dh_resnet18_cam_tiles(dh_resnet18* net, const uint8_t* slide, int64_t h, int64_t w, const int32_t* yx, int64_t n,
                                     int32_t P, float* cam, float* logits, void* stream) {
  if (int rc = cam_check(R18_ENGINE, net, P, "resnet18 cam_tiles")) return rc;
  return infer_tiles(R18_ENGINE, net, slide, h, w, yx, n, P, nullptr, cam, "resnet18 cam_tiles", [&](Tap* tap) {
    return r18_forward(net, nullptr, slide, h, w, yx, n, P, logits, dh::as_stream(stream), tap, nullptr, cam);
  });
}

// ---------------------------------------------------------------------------
// Test hooks (declared in include/deephisto_hip_debug.h): run one conv
// layer on caller-provided NHWC data, and read back the stem activation of the
// last forward.  They exist so the GPU parity tests can localise an error to a
// kernel; the product path never calls them.
// ---------------------------------------------------------------------------
namespace {
template <typename T>
__global__ void to_f32_kernel(const T* __restrict__ in, float* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (sizeof(T) == 2) out[i] = bf16_bits_to_f32(reinterpret_cast<const uint16_t*>(in)[i]);
    else out[i] = in[i];
  }
}
}  // namespace

extern "C" int dh_debug_conv_bn_act(const void* in_dev, const float* w_host, const float* scale_host,
                                    const float* shift_host, const void* res_dev, void* out_dev,
                                    int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout,
                                    int32_t ks, int32_t stride, int32_t relu, int32_t dtype,
                                    void* stream) {
  DH_REQUIRE(in_dev && w_host && scale_host && shift_host && out_dev, "debug conv: null pointer");
  DH_REQUIRE(dtype == DH_DTYPE_F32 || dtype == DH_DTYPE_BF16, "debug conv: bad dtype");
  const int esz = dtype == DH_DTYPE_F32 ? 4 : 2;
  DH_REQUIRE(cout % 64 == 0 && cin % (CHUNK_BYTES / esz) == 0, "debug conv: channel counts");
  ConvLayer L{{"debug", "debug", cin, cout, ks, stride}};
  std::vector<uint8_t> packed;
  pack_conv_weights(w_host, cout, cin, ks, esz, packed);
  int rc = upload(packed, &L.w_dev);
  if (rc) return rc;
  std::vector<float> sc(scale_host, scale_host + cout), sh(shift_host, shift_host + cout);
  rc = upload(sc, reinterpret_cast<void**>(&L.scale_dev));
  if (!rc) rc = upload(sh, reinterpret_cast<void**>(&L.shift_dev));
  int ho, wo;
  hipStream_t st = dh::as_stream(stream);
  if (!rc)
    rc = dtype == DH_DTYPE_F32 ? run_conv<float>(L, in_dev, res_dev, out_dev, B, H, W, relu != 0, st, &ho, &wo)
                               : run_conv<__bf16>(L, in_dev, res_dev, out_dev, B, H, W, relu != 0, st, &ho, &wo);
  hipError_t e = hipStreamSynchronize(st);
  if (L.w_dev) (void)hipFree(L.w_dev);
  if (L.scale_dev) (void)hipFree(L.scale_dev);
  if (L.shift_dev) (void)hipFree(L.shift_dev);
  if (!rc && e != hipSuccess) { dh::set_error("debug conv: %s", hipGetErrorString(e)); rc = DH_EHIP; }
  return rc;
}

extern "C" int dh_debug_stem_out(dh_resnet18* net, int64_t n, int32_t P, float* out_dev, void* stream) {
  DH_REQUIRE(net && out_dev && net->ws, "debug stem out: no forward has run");
  const int H1 = (P + 6 - 7) / 2 + 1;
  const int64_t elems = n * H1 * H1 * 64;
  DH_REQUIRE((size_t)elems * net->esz() <= net->ws_bytes, "debug stem out: workspace smaller than request");
  hipStream_t st = dh::as_stream(stream);
  if (net->dtype == DH_DTYPE_F32)
    hipLaunchKernelGGL((to_f32_kernel<float>), dim3(1024), dim3(256), 0, st, static_cast<const float*>(net->ws), out_dev, elems);
  else
    hipLaunchKernelGGL((to_f32_kernel<__bf16>), dim3(1024), dim3(256), 0, st, static_cast<const __bf16*>(net->ws), out_dev, elems);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

namespace {
__global__ void blocked_to_nhwc_f32_kernel(const __bf16* in, float* out, int64_t n, int hw) {   // [n][2][hw][32] -> [n][hw][64]
  const int64_t total = n * hw * 64;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % 64);
    const int64_t px = (i / 64) % hw, b = i / 64 / hw;
    out[i] = (float)in[((b * 2 + c / 32) * hw + px) * 32 + c % 32];
  }
}
}  // namespace

extern "C" int dh_debug_stem_pool_bf16(dh_resnet18* net, const uint8_t* slide_dev, int64_t slide_h, int64_t slide_w,
                                       const int32_t* yx_dev, int64_t n, int32_t P, float* out_dev, void* stream) {
  DH_REQUIRE(net && net->finalized && net->dtype == DH_DTYPE_BF16, "debug stem pool: needs a finalized bf16 network");
  DH_REQUIRE(slide_dev && yx_dev && out_dev && n > 0 && n <= (1 << 20) && P >= 32 && P <= 1024, "debug stem pool: bad arguments");
  hipStream_t st = dh::as_stream(stream);
  const int H1 = (P + 6 - 7) / 2 + 1, H2 = (H1 + 2 - 3) / 2 + 1;
  void* tmp = nullptr;
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t out_bytes = al((size_t)n * H2 * H2 * 64 * 2);
  DH_HIP(hipMalloc(&tmp, out_bytes + stem_seam_bytes((int)n, P) + 256));
  int rc = launch_stem_pool(net->convs[0], nullptr, slide_dev, slide_h, slide_w, yx_dev, (int)n, P, tmp, static_cast<char*>(tmp) + out_bytes, st);
  if (!rc) {
    hipLaunchKernelGGL(blocked_to_nhwc_f32_kernel, dim3(1024), dim3(256), 0, st, static_cast<const __bf16*>(tmp), out_dev, n, H2 * H2);
    if (hipGetLastError() != hipSuccess) rc = DH_EHIP;
    (void)hipStreamSynchronize(st);
  }
  (void)hipFree(tmp);
  return rc;
}

extern "C" int dh_debug_resnet18_forward_tap(dh_resnet18* net, const uint8_t* slide, int64_t h, int64_t w, const int32_t* yx_dev, int64_t n,
                                             int32_t P, const char* conv_name, const int32_t* sel_dev, int32_t k, float* out_dev,
                                             int64_t out_elems, float* logits_dev, void* stream) {
  hipStream_t st = dh::as_stream(stream);
  return infer_tap(R18_ENGINE, net, slide, h, w, yx_dev, n, P, conv_name, sel_dev, k, out_dev, out_elems, logits_dev, st, [&](Tap* tap) {
    return r18_forward(net, nullptr, slide, h, w, yx_dev, n, P, logits_dev, st, tap);
  });
}

extern "C" int dh_debug_resnet18_operands(dh_resnet18* net, const char* conv_name, float* w_host, int64_t w_elems, float* scale_host,
                                          float* shift_host, int64_t c_elems) {
  return infer_operands(R18_ENGINE, net, net ? net->esz() : 0, conv_name, w_host, w_elems, scale_host, shift_host, c_elems);
}

// ---------------------------------------------------------------------------
// dominant-kernel timing (see Profiler above)
// ---------------------------------------------------------------------------
extern "C" int dh_profile_start(int32_t sample_every, int32_t max_samples) {
  DH_REQUIRE(sample_every > 0 && max_samples > 0 && max_samples <= (1 << 20), "profile start: bad arguments");
  for (hipEvent_t e : g_prof.ev) (void)hipEventDestroy(e);
  g_prof.ev.assign((size_t)max_samples * 2, nullptr);
  for (auto& e : g_prof.ev) DH_HIP(hipEventCreate(&e));
  g_prof.every = sample_every; g_prof.counter = 0; g_prof.used = 0; g_prof.flops = 0.0;
  g_prof.on = true;
  return DH_OK;
}

extern "C" int dh_profile_stop(double* total_ms, double* total_flops, int64_t* n_samples) {
  g_prof.on = false;
  double ms = 0.0;
  for (size_t i = 0; i + 1 < g_prof.used; i += 2) {
    DH_HIP(hipEventSynchronize(g_prof.ev[i + 1]));
    float t = 0.f;
    DH_HIP(hipEventElapsedTime(&t, g_prof.ev[i], g_prof.ev[i + 1]));
    ms += t;
  }
  if (total_ms) *total_ms = ms;
  if (total_flops) *total_flops = g_prof.flops;
  if (n_samples) *n_samples = (int64_t)(g_prof.used / 2);
  for (hipEvent_t e : g_prof.ev) (void)hipEventDestroy(e);
  g_prof.ev.clear(); g_prof.used = 0;
  return DH_OK;
}

// Diagnostic phase stamps of the 3x3 conv kernel (DH tests/tools only): enable, then read
// 8 rows x 8 counters {load-issue, mfma, barrier, epilogue, lds-write, barrier, workgroups, -}.
extern "C" int dh_debug_stamps(int32_t enable, unsigned long long* out64_host) {
  g_stamps_on = enable != 0;
  if (out64_host) {
    if (!g_stamps_dev) { memset(out64_host, 0, 64 * sizeof(unsigned long long)); return DH_OK; }
    DH_HIP(hipDeviceSynchronize());
    DH_HIP(hipMemcpy(out64_host, g_stamps_dev, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    DH_HIP(hipMemset(g_stamps_dev, 0, 64 * sizeof(unsigned long long)));
  }
  return DH_OK;
}

// Test hook: tile variant (0 / 1 / 2 = 512 / 256 / 128 pixels; -1: not a plain stride-1 launch) and MFMA shape (16: 16x16x32, 32: 32x32x16) of the
// process's last 3x3 convolution launch.
extern "C" int dh_debug_last_conv3(int32_t* variant, int32_t* mfma_m) {
  DH_REQUIRE(variant && mfma_m, "dh_debug_last_conv3: null argument");
  *variant = g_last_conv3_variant; *mfma_m = g_last_conv3_mfma;
  return DH_OK;
}

// Test hook: strips of the fused bf16 stem of 15 or 16 pooled columns whatever the geometry; 0 = chosen by geometry (the default).
extern "C" int dh_debug_stem_strip_width(int32_t pc) {
  DH_REQUIRE(pc == 0 || pc == 15 || pc == 16, "debug stem strip width: %d is not 0, 15 or 16", pc);
  g_stem_pc_force = pc;
  return DH_OK;
}

#include "gemm1x1_f32.inc"
#include "train_core_kernels.inc"
#include "train_core.inc"
#include "train_kernels.inc"
#include "train.inc"
#include "train2_kernels.inc"
#include "wgrad_ring.inc"
#include "bn_fold.inc"
#include "gemm1x1.inc"
#include "train2.inc"
#include "train_hooks.inc"
#include "gemm1x1_infer.inc"
#include "resnet50_infer.inc"
