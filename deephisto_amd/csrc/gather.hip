// Tile gathers of the deephisto hot path for MI355X (gfx950, wave64):
//   a1  dh_tile_grid            host integer restatement of the dense grid order
//   --  dh_synth_slide          closed-form benchmark slide generated in HBM
//   a2/a4/a5 dh_tile_gather     uint8 HWC slide -> [n,P,P,3] / [n,3,P,P] f32|bf16, exactly k/255
//   --  dh_tile_gather_aug / _stain_aug / _affine_aug   the training batch gather: flips, stain jitter, rotation and scale
//   --  dh_tile_gather_raw, dh_tile_coords_f32          the random-branch sampler's raw tiles and float coordinates
// All of these are HBM-bound byte/integer work: no MFMA, LDS only for the stain tables; the design
// rules are full-width coalesced rows (one wave = one tile row) and 16-byte stores.
#include <algorithm>
#include <type_traits>

#include "dh_common.h"
#include "stain_fixed.h"

// ---------------------------------------------------------------------------
// a1: tile grid (host).  Reference: patch_samplers/full_samplers.py:374-404.
// ---------------------------------------------------------------------------
static inline int64_t range_len(int64_t stop, int64_t step) {  // len(range(0, stop, step))
  return stop <= 0 ? 0 : (stop + step - 1) / step;
}

extern "C" int dh_tile_grid_count(int64_t h, int64_t w, int32_t patch, int32_t stride,
                                  int32_t batch, int64_t* n_unique, int64_t* n_padded) {
  DH_REQUIRE(patch > 0 && stride > 0 && batch > 0, "tile grid: patch, stride, batch must be > 0");
  DH_REQUIRE(h >= patch && w >= patch, "tile grid: slide %lldx%lld smaller than patch %d",
             (long long)h, (long long)w, patch);
  DH_REQUIRE(h <= INT32_MAX && w <= INT32_MAX, "tile grid: slide side exceeds int32");
  const int64_t ny = range_len(h - patch, stride), nx = range_len(w - patch, stride);
  const int64_t n = ny * nx + ny + nx + 1;
  if (n_unique) *n_unique = n;
  if (n_padded) *n_padded = (n + batch - 1) / batch * batch;
  return DH_OK;
}

extern "C" int dh_tile_grid(int64_t h, int64_t w, int32_t patch, int32_t stride, int32_t batch,
                            int32_t* out, int64_t capacity_pairs) {
  int64_t n = 0, np = 0;
  int rc = dh_tile_grid_count(h, w, patch, stride, batch, &n, &np);
  if (rc) return rc;
  DH_REQUIRE(out != nullptr, "tile grid: null output");
  DH_REQUIRE(capacity_pairs >= np, "tile grid: capacity %lld < %lld padded origins",
             (long long)capacity_pairs, (long long)np);
  const int64_t ylim = h - patch, xlim = w - patch;
  int32_t* p = out;
  for (int64_t y = 0; y < ylim; y += stride)
    for (int64_t x = 0; x < xlim; x += stride) { *p++ = (int32_t)y; *p++ = (int32_t)x; }
  for (int64_t y = 0; y < ylim; y += stride) { *p++ = (int32_t)y; *p++ = (int32_t)xlim; }
  for (int64_t x = 0; x < xlim; x += stride) { *p++ = (int32_t)ylim; *p++ = (int32_t)x; }
  for (int64_t i = n - 1; i < np; ++i) {  // the corner, then its padding copies
    *p++ = (int32_t)ylim; *p++ = (int32_t)xlim;
  }
  return DH_OK;
}

// ---------------------------------------------------------------------------
// synthetic slide: pix(y,x,c,seed) = (((y*K_Y)^(x*K_X)^(c*K_C)^(seed*K_S)) >> 7) & 0xFF
// One thread = 16 consecutive bytes of the HWC image (one 16-B store).
// ---------------------------------------------------------------------------
#define DH_KY 73856093u
#define DH_KX 19349663u
#define DH_KC 83492791u
#define DH_KS 2654435761u

__global__ __launch_bounds__(256) void synth_slide_kernel(uint8_t* __restrict__ out, int64_t total,
                                                          uint32_t row_bytes, uint32_t seed_term) {
  const int64_t chunks = (total + 15) >> 4;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < chunks;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = t << 4;
    uint32_t y = (uint32_t)(i0 / row_bytes);
    uint32_t xb = (uint32_t)(i0 - (int64_t)y * row_bytes);
    uint32_t x = xb / 3u, c = xb - 3u * x;
    uint32_t wv[4] = {0, 0, 0, 0};
    const int nb = (total - i0 >= 16) ? 16 : (int)(total - i0);
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const uint32_t v = (((y * DH_KY) ^ (x * DH_KX) ^ (c * DH_KC) ^ seed_term) >> 7) & 0xFFu;
      wv[b >> 2] |= v << (8 * (b & 3));
      if (++c == 3u) { c = 0; ++x; }
      if (++xb == row_bytes) { xb = 0; x = 0; c = 0; ++y; }
    }
    if (nb == 16) {
      *reinterpret_cast<uint4*>(out + i0) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
    } else {
      for (int b = 0; b < nb; ++b) out[i0 + b] = (uint8_t)(wv[b >> 2] >> (8 * (b & 3)));
    }
  }
}

extern "C" int dh_synth_slide(uint8_t* slide, int64_t h, int64_t w, uint32_t seed, void* stream) {
  DH_REQUIRE(slide && h > 0 && w > 0, "synth slide: bad arguments");
  DH_REQUIRE(w * 3 <= (int64_t)UINT32_MAX, "synth slide: row too long");
  DH_REQUIRE((reinterpret_cast<uintptr_t>(slide) & 15) == 0, "synth slide: base must be 16-B aligned");
  const int64_t total = h * w * 3;
  const int64_t chunks = (total + 15) >> 4;
  const int grid = (int)std::min<int64_t>((chunks + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(synth_slide_kernel, dim3(grid), dim3(256), 0, dh::as_stream(stream), slide,
                     total, (uint32_t)(w * 3), seed * DH_KS);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// ---------------------------------------------------------------------------
// a2/a4/a5: gather.  k/255 in float32, correctly rounded, without a divide:
//   q = k*r; e = fma(-q,255,k); q' = fma(e,r,q)   with r = RN(1/255).
// (tests/test_div255.py checks all 256 inputs against IEEE division on the host;
//  tests/test_gpu_tiles.py checks the kernel's outputs bit-for-bit.)
// ---------------------------------------------------------------------------
__device__ __forceinline__ float div255(uint32_t k) {
  const float r = 1.0f / 255.0f;
  const float kf = (float)k;
  const float q = kf * r;
  const float e = __builtin_fmaf(-q, 255.0f, kf);
  return __builtin_fmaf(e, r, q);
}

__device__ __forceinline__ uint32_t f32_to_bf16_bits(float f) {  // RNE; inputs are finite
  const uint32_t u = __float_as_uint(f);
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

struct __attribute__((packed, aligned(1))) Px4 { uint32_t a, b, c; };   // 4 RGB pixels
struct __attribute__((packed, aligned(1))) U32u { uint32_t v; };

constexpr int GATHER_ROWS = 16;  // tile rows per 256-thread block (4 per wave)

// The gathered tiles are written once and read by a later kernel (0.8 GB per 1 024 tiles: far past the 256 MB Infinity Cache), the slide
// bytes are read once: non-temporal accesses keep neither in the caches.  Measured (tools/hbm_mix_peak.hip: the same 1 : 4 byte mix as a
// linear stream reaches 5.1-5.4 TB/s plain, 5.4-5.5 TB/s non-temporal; profiles/r04_exp_tiler.txt for the kernels).
#ifndef DH_TILER_NT
#define DH_TILER_NT 1
#endif
typedef float f4v_t __attribute__((ext_vector_type(4)));
typedef uint32_t u2v_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void st_f4(float* p, float a, float b, float c, float d) {
  if (DH_TILER_NT) __builtin_nontemporal_store(f4v_t{a, b, c, d}, reinterpret_cast<f4v_t*>(p));
  else *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}
__device__ __forceinline__ void st_u2(uint16_t* p, uint32_t x, uint32_t y) {
  if (DH_TILER_NT) __builtin_nontemporal_store(u2v_t{x, y}, reinterpret_cast<u2v_t*>(p));
  else *reinterpret_cast<uint2*>(p) = make_uint2(x, y);
}

// The (layout, dtype) codes of deephisto_hip.h: the one test of what is a code, and the one place that turns a pair of codes into
// the kernels' <BF16, NCHW> template pair -- `launch` is a generic lambda called with the two as std::bool_constant values.
static inline bool known_layout(int32_t layout) { return layout == DH_LAYOUT_NHWC || layout == DH_LAYOUT_NCHW; }
static inline bool known_dtype(int32_t dtype) { return dtype == DH_DTYPE_F32 || dtype == DH_DTYPE_BF16; }

static int require_layout_dtype(const char* who, int32_t layout, int32_t dtype) {
  DH_REQUIRE(known_layout(layout), "%s: bad layout %d", who, layout);
  DH_REQUIRE(known_dtype(dtype), "%s: bad dtype %d", who, dtype);
  return DH_OK;
}

template <class Launch>
static void for_layout_dtype(int32_t layout, int32_t dtype, Launch&& launch) {
  if (layout == DH_LAYOUT_NCHW) {
    if (dtype == DH_DTYPE_F32) launch(std::false_type{}, std::true_type{});
    else launch(std::true_type{}, std::true_type{});
  } else {
    if (dtype == DH_DTYPE_F32) launch(std::false_type{}, std::false_type{});
    else launch(std::true_type{}, std::false_type{});
  }
}

// NCHW: one wave = one tile row; lane j owns pixels 4j..4j+3 (12 contiguous bytes) and
// writes one 16-B (f32) / 8-B (bf16) store into each of the three planes.
template <bool BF16>
__global__ __launch_bounds__(256) void gather_nchw_kernel(const uint8_t* __restrict__ slide,
                                                          int64_t row_bytes,
                                                          const int32_t* __restrict__ yx, int P,
                                                          void* __restrict__ outv) {
  const int t = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y0 = yx[2 * t], x0 = yx[2 * t + 1];
  const int r0 = blockIdx.x * GATHER_ROWS + wave;
  const int64_t plane = (int64_t)P * P;
  for (int pj = lane * 4; pj < P; pj += 256) {
#pragma unroll
    for (int rr = 0; rr < GATHER_ROWS / 4; ++rr) {
      const int r = r0 + rr * 4;
      if (r < P) {
        const uint8_t* src = slide + (int64_t)(y0 + r) * row_bytes + (int64_t)(x0 + pj) * 3;
        const Px4 v = *reinterpret_cast<const Px4*>(src);
        const uint32_t b[3] = {v.a, v.b, v.c};
        float f[3][4];
#pragma unroll
        for (int i = 0; i < 12; ++i) f[i % 3][i / 3] = div255((b[i >> 2] >> (8 * (i & 3))) & 0xFFu);
        const int64_t o = (int64_t)t * 3 * plane + (int64_t)r * P + pj;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if constexpr (BF16) {
            st_u2(static_cast<uint16_t*>(outv) + o + c * plane, f32_to_bf16_bits(f[c][0]) | (f32_to_bf16_bits(f[c][1]) << 16),
                  f32_to_bf16_bits(f[c][2]) | (f32_to_bf16_bits(f[c][3]) << 16));
          } else {
            st_f4(static_cast<float*>(outv) + o + c * plane, f[c][0], f[c][1], f[c][2], f[c][3]);
          }
        }
      }
    }
  }
}

// NHWC: the tile row is 3P contiguous bytes -> 3P contiguous outputs; lane j owns
// bytes 4j..4j+3 of each 256-byte piece (4-B load, 16-B / 8-B store).
template <bool BF16>
__global__ __launch_bounds__(256) void gather_nhwc_kernel(const uint8_t* __restrict__ slide,
                                                          int64_t row_bytes,
                                                          const int32_t* __restrict__ yx, int P,
                                                          void* __restrict__ outv) {
  const int t = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y0 = yx[2 * t], x0 = yx[2 * t + 1];
  const int r0 = blockIdx.x * GATHER_ROWS + wave;
  const int rowlen = 3 * P;  // multiple of 4 (P % 4 == 0)
  for (int bj = lane * 4; bj < rowlen; bj += 256) {
#pragma unroll
    for (int rr = 0; rr < GATHER_ROWS / 4; ++rr) {
      const int r = r0 + rr * 4;
      if (r < P) {
        const uint8_t* src = slide + (int64_t)(y0 + r) * row_bytes + (int64_t)x0 * 3 + bj;
        const uint32_t v = reinterpret_cast<const U32u*>(src)->v;
        const float f0 = div255(v & 0xFFu), f1 = div255((v >> 8) & 0xFFu),
                    f2 = div255((v >> 16) & 0xFFu), f3 = div255(v >> 24);
        const int64_t o = ((int64_t)t * P + r) * rowlen + bj;
        if constexpr (BF16) {
          st_u2(static_cast<uint16_t*>(outv) + o, f32_to_bf16_bits(f0) | (f32_to_bf16_bits(f1) << 16), f32_to_bf16_bits(f2) | (f32_to_bf16_bits(f3) << 16));
        } else {
          st_f4(static_cast<float*>(outv) + o, f0, f1, f2, f3);
        }
      }
    }
  }
}

// Any patch size (P % 4 != 0): one thread per output element.
template <bool BF16, bool NCHW>
__global__ __launch_bounds__(256) void gather_generic_kernel(const uint8_t* __restrict__ slide,
                                                             int64_t row_bytes,
                                                             const int32_t* __restrict__ yx, int P,
                                                             void* __restrict__ outv) {
  const int t = blockIdx.y;
  const int y0 = yx[2 * t], x0 = yx[2 * t + 1];
  const int64_t per_tile = (int64_t)P * P * 3;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_tile;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / (3 * P));
    const int rem = (int)(i - (int64_t)r * 3 * P);
    const int px = rem / 3, c = rem - 3 * px;
    const float f = div255(slide[(int64_t)(y0 + r) * row_bytes + (int64_t)(x0 + px) * 3 + c]);
    const int64_t o = (int64_t)t * per_tile + (NCHW ? ((int64_t)c * P + r) * P + px : i);
    if constexpr (BF16) static_cast<uint16_t*>(outv)[o] = (uint16_t)f32_to_bf16_bits(f);
    else static_cast<float*>(outv)[o] = f;
  }
}

extern "C" int dh_tile_gather(const uint8_t* slide, int64_t h, int64_t w, const int32_t* yx_dev,
                              const int32_t* yx_host_check, int64_t n, int32_t P, int32_t layout,
                              int32_t dtype, void* out, void* stream) {
  DH_REQUIRE(n >= 0 && n <= 65535, "tile gather: n=%lld out of range [0, 65535]", (long long)n);
  if (n == 0) return DH_OK;  // empty batch: nothing to read or write (pointers may be null)
  DH_REQUIRE(slide && yx_dev && out, "tile gather: null pointer");
  DH_REQUIRE(P > 0 && h >= P && w >= P, "tile gather: patch %d does not fit %lldx%lld", P,
             (long long)h, (long long)w);
  if (const int rc = require_layout_dtype("tile gather", layout, dtype)) return rc;
  if (yx_host_check)
    for (int64_t i = 0; i < n; ++i) {
      const int64_t y = yx_host_check[2 * i], x = yx_host_check[2 * i + 1];
      DH_REQUIRE(y >= 0 && x >= 0 && y + P <= h && x + P <= w,
                 "tile gather: origin %lld = (%lld,%lld) outside slide", (long long)i, (long long)y,
                 (long long)x);
    }
  const bool fast = (P % 4 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  hipStream_t st = dh::as_stream(stream);
  const int64_t rb = w * 3;
  const int64_t per_tile = (int64_t)P * P * 3;
  const dim3 block(256);
  const dim3 grid = fast ? dim3((P + GATHER_ROWS - 1) / GATHER_ROWS, (unsigned)n)
                         : dim3((unsigned)std::min<int64_t>((per_tile + 255) / 256, 1024), (unsigned)n);
  for_layout_dtype(layout, dtype, [&](auto bf16, auto nchw) {
    constexpr bool BF = decltype(bf16)::value, NC = decltype(nchw)::value;
    if (!fast) hipLaunchKernelGGL((gather_generic_kernel<BF, NC>), grid, block, 0, st, slide, rb, yx_dev, P, out);
    else if constexpr (NC) hipLaunchKernelGGL(gather_nchw_kernel<BF>, grid, block, 0, st, slide, rb, yx_dev, P, out);
    else hipLaunchKernelGGL(gather_nhwc_kernel<BF>, grid, block, 0, st, slide, rb, yx_dev, P, out);
  });
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// Gather with the batch-level flips of the training pipeline (train.py:71-81 applies
// RandomHorizontalFlip / RandomVerticalFlip to the whole [B,C,H,W] batch: one coin per batch).
template <bool BF16, bool NCHW>
__global__ __launch_bounds__(256) void gather_aug_kernel(const uint8_t* __restrict__ slide, int64_t row_bytes, int h, int w,
                                                         const int32_t* __restrict__ yx, int P, int flip_h, int flip_v,
                                                         void* __restrict__ outv) {
  const int t = blockIdx.y;
  const int y0 = yx[2 * t], x0 = yx[2 * t + 1];
  const int64_t per_tile = (int64_t)P * P * 3;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_tile; i += (int64_t)gridDim.x * blockDim.x) {
    // i enumerates OUTPUT elements in output order
    int r, px, c;
    if (NCHW) { c = (int)(i / ((int64_t)P * P)); const int rem = (int)(i - (int64_t)c * P * P); r = rem / P; px = rem - r * P; }
    else { r = (int)(i / (3 * P)); const int rem = (int)(i - (int64_t)r * 3 * P); px = rem / 3; c = rem - 3 * px; }
    const int sr = flip_v ? P - 1 - r : r, sx = flip_h ? P - 1 - px : px;
    // region samplers keep the reference's origin bounds, which let a patch hang over the image border
    // (region_samplers.py:112-118): pixels outside the slide read as 0, never as memory outside the allocation
    const int yy = y0 + sr, xx = x0 + sx;
    const bool in = yy >= 0 && yy < h && xx >= 0 && xx < w;
    const float f = in ? div255(slide[(int64_t)yy * row_bytes + (int64_t)xx * 3 + c]) : 0.f;
    const int64_t o = (int64_t)t * per_tile + i;
    if constexpr (BF16) static_cast<uint16_t*>(outv)[o] = (uint16_t)f32_to_bf16_bits(f);
    else static_cast<float*>(outv)[o] = f;
  }
}

extern "C" int dh_tile_gather_aug(const uint8_t* slide, int64_t h, int64_t w, const int32_t* yx_dev, int64_t n, int32_t P,
                                  int32_t layout, int32_t dtype, int32_t flip_h, int32_t flip_v, void* out, void* stream) {
  DH_REQUIRE(n >= 0 && n <= 65535, "tile gather aug: n=%lld out of range", (long long)n);
  if (n == 0) return DH_OK;
  DH_REQUIRE(slide && yx_dev && out && P > 0 && h >= P && w >= P && h <= INT32_MAX && w <= INT32_MAX, "tile gather aug: bad arguments");
  DH_REQUIRE(known_layout(layout) && known_dtype(dtype), "tile gather aug: bad layout/dtype");
  hipStream_t st = dh::as_stream(stream);
  const int64_t per_tile = (int64_t)P * P * 3;
  dim3 grid((unsigned)std::min<int64_t>((per_tile + 255) / 256, 1024), (unsigned)n), block(256);
  const int64_t rb = w * 3;
  for_layout_dtype(layout, dtype, [&](auto bf16, auto nchw) {
    hipLaunchKernelGGL((gather_aug_kernel<decltype(bf16)::value, decltype(nchw)::value>), grid, block, 0, st, slide, rb, (int)h, (int)w,
                       yx_dev, P, flip_h, flip_v, out);
  });
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// Gather with the flips above and a per-tile stain jitter, integer-exact: a pixel inside the slide goes
// bytes -> optical densities T (the 256-entry table) -> o_c = A_c . T + b_c in int64 with the tile's fixed-point matrix and bias
// -> v'_c = lut[clamp(o_c >> shift, 0, lut_n - 1)] -> v'_c / 255; a pixel outside the slide is 0 as above, not transformed.
// One thread per output PIXEL (all three channels need all three inputs), in output order, so NCHW is three coalesced plane
// writes and NHWC 3 consecutive elements per lane.  Both tables live in LDS (1 KiB + lut_n bytes); a workgroup covers
// kStainPxPerWg pixels of one tile, which amortises loading them, and reads the tile's 12 parameters once (uniform loads).
constexpr int kStainPxPerWg = 4096;   // 16 pixels per thread: 12 KiB of slide bytes and 24-48 KiB of output per 25 KiB of tables

template <bool BF16>
__device__ __forceinline__ void st_elem(void* outv, int64_t o, float f) {
  if constexpr (BF16) static_cast<uint16_t*>(outv)[o] = (uint16_t)f32_to_bf16_bits(f);
  else static_cast<float*>(outv)[o] = f;
}

template <bool BF16, bool NCHW>
__global__ __launch_bounds__(256) void gather_stain_aug_kernel(const uint8_t* __restrict__ slide, int64_t row_bytes, int h, int w,
                                                               const int32_t* __restrict__ yx, const int32_t* __restrict__ params,
                                                               int P, int flip_h, int flip_v, const int32_t* __restrict__ od,
                                                               int shift, const uint8_t* __restrict__ lut, int lut_n,
                                                               void* __restrict__ outv) {
  __shared__ int32_t s_od[256];
  __shared__ __attribute__((aligned(16))) uint8_t s_lut[dh_stain::kLutMax];
  s_od[threadIdx.x] = od[threadIdx.x];   // 256 threads, 256 entries
  const int lut16 = lut_n >> 4;          // lut is 16-byte aligned (checked by the entry)
  for (int i = threadIdx.x; i < lut16; i += 256) reinterpret_cast<uint4*>(s_lut)[i] = reinterpret_cast<const uint4*>(lut)[i];
  for (int i = (lut16 << 4) + threadIdx.x; i < lut_n; i += 256) s_lut[i] = lut[i];
  const int t = blockIdx.y;
  const int y0 = yx[2 * t], x0 = yx[2 * t + 1];
  int32_t A[3][3], b[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) A[k / 3][k % 3] = params[12 * (int64_t)t + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) b[k] = params[12 * (int64_t)t + 9 + k];
  __syncthreads();
  const int64_t plane = (int64_t)P * P;
  const int64_t p0 = (int64_t)blockIdx.x * kStainPxPerWg;   // first output pixel of this workgroup: row r0, column c0 (uniform)
  const int r0 = (int)(p0 / P), c0 = (int)(p0 - (int64_t)r0 * P);
  const int live = (int)std::min<int64_t>(plane - p0, kStainPxPerWg);
  for (int q = threadIdx.x; q < live; q += 256) {
    const uint32_t lin = (uint32_t)c0 + (uint32_t)q;        // < P + kStainPxPerWg: no overflow (checked by the entry)
    const int dr = (int)(lin / (uint32_t)P);
    const int r = r0 + dr, px = (int)(lin - (uint32_t)dr * (uint32_t)P);
    const int yy = y0 + (flip_v ? P - 1 - r : r), xx = x0 + (flip_h ? P - 1 - px : px);
    float f[3] = {0.f, 0.f, 0.f};
    if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
      const uint8_t* src = slide + (int64_t)yy * row_bytes + (int64_t)xx * 3;
      const int32_t tr = s_od[src[0]], tg = s_od[src[1]], tb = s_od[src[2]];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int64_t o = (int64_t)A[c][0] * tr + (int64_t)A[c][1] * tg + (int64_t)A[c][2] * tb + b[c];
        const int k = (int)std::min<int64_t>(std::max<int64_t>(o >> shift, 0), lut_n - 1);   // arithmetic shift: floor
        f[c] = div255(s_lut[k]);
      }
    }
    const int64_t p = p0 + q;
    if (NCHW) {
      const int64_t o = (int64_t)t * 3 * plane + p;
#pragma unroll
      for (int c = 0; c < 3; ++c) st_elem<BF16>(outv, o + c * plane, f[c]);
    } else {
      const int64_t o = ((int64_t)t * plane + p) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) st_elem<BF16>(outv, o + c, f[c]);
    }
  }
}

// What both stain entries ask of the stain arguments; `who` opens every message.
static int require_stain_args(const char* who, int32_t lut_n, const uint8_t* lut_dev, int32_t shift, const int32_t* od_host,
                              const int32_t* params_host_check, int64_t n) {
  using namespace dh_stain;
  DH_REQUIRE(lut_n > 0 && lut_n <= kLutMax, "%s: lut_n = %d, an output table has 1 to %d entries", who, lut_n, kLutMax);
  DH_REQUIRE(((uintptr_t)lut_dev & 15) == 0, "%s: lut_dev must be 16-byte aligned", who);
  DH_REQUIRE(shift >= 0 && shift < 40, "%s: shift %d outside [0, 40)", who, shift);
  for (int i = 0; i < 256; ++i)
    DH_REQUIRE(od_host[i] >= 0 && od_host[i] <= kOdMax, "%s: od table entry %d = %d outside [0, %d]", who, i, od_host[i], kOdMax);
  if (params_host_check)
    for (int64_t i = 0; i < 12 * n; ++i) {
      const int32_t v = params_host_check[i], lim = i % 12 < 9 ? kCoefMax : kBiasMax;
      DH_REQUIRE(v >= -lim && v <= lim, "%s: params row %lld, %s entry %d = %d outside +-%d", who, (long long)(i / 12),
                 i % 12 < 9 ? "matrix" : "bias", (int)(i % 12 < 9 ? i % 12 : i % 12 - 9), v, lim);
    }
  return DH_OK;
}

extern "C" int dh_tile_gather_stain_aug(const uint8_t* slide, int64_t h, int64_t w, const int32_t* yx_dev, const int32_t* params_dev,
                                        const int32_t* params_host_check, int64_t n, int32_t P, int32_t layout, int32_t dtype,
                                        int32_t flip_h, int32_t flip_v, const int32_t* od_dev, const int32_t* od_host, int32_t shift,
                                        const uint8_t* lut_dev, int32_t lut_n, void* out, void* stream) {
  DH_REQUIRE(n >= 0 && n <= 65535, "tile gather stain aug: n=%lld out of range [0, 65535]", (long long)n);
  if (n == 0) return DH_OK;
  DH_REQUIRE(slide && yx_dev && params_dev && od_dev && od_host && lut_dev && out, "tile gather stain aug: null pointer");
  DH_REQUIRE(h > 0 && w > 0 && h <= INT32_MAX && w <= INT32_MAX, "tile gather stain aug: bad slide size %lld x %lld", (long long)h,
             (long long)w);
  DH_REQUIRE(P > 0 && h >= P && w >= P && P <= INT32_MAX - kStainPxPerWg, "tile gather stain aug: patch %d does not fit %lldx%lld", P,
             (long long)h, (long long)w);
  if (const int rc = require_layout_dtype("tile gather stain aug", layout, dtype)) return rc;
  if (const int rc = require_stain_args("tile gather stain aug", lut_n, lut_dev, shift, od_host, params_host_check, n)) return rc;
  const int64_t blocks = ((int64_t)P * P + kStainPxPerWg - 1) / kStainPxPerWg;
  DH_REQUIRE(blocks <= INT32_MAX, "tile gather stain aug: patch %d too large", P);
  hipStream_t st = dh::as_stream(stream);
  dim3 grid((unsigned)blocks, (unsigned)n), block(256);
  const int64_t rb = w * 3;
  for_layout_dtype(layout, dtype, [&](auto bf16, auto nchw) {
    hipLaunchKernelGGL((gather_stain_aug_kernel<decltype(bf16)::value, decltype(nchw)::value>), grid, block, 0, st, slide, rb, (int)h,
                       (int)w, yx_dev, params_dev, P, flip_h, flip_v, od_dev, (int)shift, lut_dev, (int)lut_n, out);
  });
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// Gather with the flips above, a per-tile rotation and scale about the patch centre, and optionally the stain jitter (DESIGN.md
// section 4.13), integer-exact.  With (sr, sx) the flipped row and column of an output pixel, U2 = 2 sx + 1 - P, V2 = 2 sr + 1 - P and
// the tile's row m = round(2^15 s [[cos, -sin], [sin, cos]]), the source point in Q16 is X = Cx + m00 U2 + m01 V2,
// Y = Cy + m10 U2 + m11 V2 (int64; Cx = ((2 x0 + P) << 15) - 2^15), its taps (xi, yi) = (X >> 16, Y >> 16) and the three
// neighbours, its weights fx = (X >> 8) & 255, fy likewise; a tap outside the slide reads as 0.  Per channel
// v = ((a (256 - fx) + b fx)(256 - fy) + (c (256 - fx) + d fx) fy + 32768) >> 16, and v goes where the slide byte goes in the
// kernels above: div255(v), or od -> matrix + bias -> lut -> div255 when STAIN.  A pixel none of whose taps of non-zero weight
// lies inside the slide is written as 0 and not transformed, which for an identity row is the rule of gather_stain_aug_kernel.
// The tile's 4 (+ 12) parameters are uniform loads; each lane reads two 6-byte row
// pairs straight from the slide (neighbouring lanes walk a rotated line: a wave's taps stay within a few cache lines).
// The table staging, the stain stage, the pixel of a workgroup and the stores are spelled out here as in gather_stain_aug_kernel:
// written over shared device helpers this kernel's bf16 rows measured 0.7-1.1 % slower at the training shape, more than the same
// code's own spread (profiles/tile_split_ab.json).
constexpr int kAffineMaxPatch = 4096;   // |U2|, |V2| <= P - 1 < 2^12 and |m| <= 2^16: products below 2^28
constexpr int kAffineCoefMax = 1 << 16;

struct __attribute__((packed, aligned(1))) Px2 { uint32_t lo; uint16_t hi; };   // 2 RGB pixels

template <bool BF16, bool NCHW, bool STAIN>
__global__ __launch_bounds__(256) void gather_affine_aug_kernel(const uint8_t* __restrict__ slide, int64_t row_bytes, int h, int w,
                                                                const int32_t* __restrict__ yx, const int32_t* __restrict__ affine,
                                                                const int32_t* __restrict__ params, int P, int flip_h, int flip_v,
                                                                const int32_t* __restrict__ od, int shift,
                                                                const uint8_t* __restrict__ lut, int lut_n, void* __restrict__ outv) {
  __shared__ int32_t s_od[STAIN ? 256 : 1];
  __shared__ __attribute__((aligned(16))) uint8_t s_lut[STAIN ? dh_stain::kLutMax : 16];
  const int t = blockIdx.y;
  int32_t A[3][3] = {}, b[3] = {};
  if constexpr (STAIN) {
    s_od[threadIdx.x] = od[threadIdx.x];   // 256 threads, 256 entries
    const int lut16 = lut_n >> 4;          // lut is 16-byte aligned (checked by the entry)
    for (int i = threadIdx.x; i < lut16; i += 256) reinterpret_cast<uint4*>(s_lut)[i] = reinterpret_cast<const uint4*>(lut)[i];
    for (int i = (lut16 << 4) + threadIdx.x; i < lut_n; i += 256) s_lut[i] = lut[i];
#pragma unroll
    for (int k = 0; k < 9; ++k) A[k / 3][k % 3] = params[12 * (int64_t)t + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) b[k] = params[12 * (int64_t)t + 9 + k];
    __syncthreads();
  }
  const int64_t cy = (((int64_t)2 * yx[2 * t] + P) << 15) - (1 << 15), cx = (((int64_t)2 * yx[2 * t + 1] + P) << 15) - (1 << 15);
  const int64_t m00 = affine[4 * (int64_t)t], m01 = affine[4 * (int64_t)t + 1], m10 = affine[4 * (int64_t)t + 2],
                m11 = affine[4 * (int64_t)t + 3];
  const int64_t plane = (int64_t)P * P;
  const int64_t p0 = (int64_t)blockIdx.x * kStainPxPerWg;   // first output pixel of this workgroup: row r0, column c0 (uniform)
  const int r0 = (int)(p0 / P), c0 = (int)(p0 - (int64_t)r0 * P);
  const int live = (int)std::min<int64_t>(plane - p0, kStainPxPerWg);
  for (int q = threadIdx.x; q < live; q += 256) {
    const uint32_t lin = (uint32_t)c0 + (uint32_t)q;        // < P + kStainPxPerWg
    const int dr = (int)(lin / (uint32_t)P);
    const int r = r0 + dr, px = (int)(lin - (uint32_t)dr * (uint32_t)P);
    const int u2 = 2 * (flip_h ? P - 1 - px : px) + 1 - P, v2 = 2 * (flip_v ? P - 1 - r : r) + 1 - P;
    const int64_t X = cx + m00 * u2 + m01 * v2, Y = cy + m10 * u2 + m11 * v2;
    const int64_t xi = X >> 16, yi = Y >> 16;               // arithmetic shifts: floor; compared with h and w as int64
    const uint32_t fx = (uint32_t)(X >> 8) & 255u, fy = (uint32_t)(Y >> 8) & 255u;
    const bool x_in0 = xi >= 0 && xi < w, x_in1 = xi >= -1 && xi < (int64_t)w - 1;
    const bool y_in0 = yi >= 0 && yi < h, y_in1 = yi >= -1 && yi < (int64_t)h - 1;
    float f[3] = {0.f, 0.f, 0.f};
    if ((x_in0 || (fx && x_in1)) && (y_in0 || (fy && y_in1))) {
      uint32_t ta[3] = {0, 0, 0}, tb[3] = {0, 0, 0}, tc[3] = {0, 0, 0}, td[3] = {0, 0, 0};
      if (x_in0 && x_in1 && y_in0 && y_in1) {               // all four taps inside: two 6-byte reads
        const uint8_t* src = slide + yi * row_bytes + xi * 3;
        const Px2 p = *reinterpret_cast<const Px2*>(src), s = *reinterpret_cast<const Px2*>(src + row_bytes);
        ta[0] = p.lo & 0xFFu; ta[1] = (p.lo >> 8) & 0xFFu; ta[2] = (p.lo >> 16) & 0xFFu;
        tb[0] = p.lo >> 24; tb[1] = p.hi & 0xFFu; tb[2] = p.hi >> 8;
        tc[0] = s.lo & 0xFFu; tc[1] = (s.lo >> 8) & 0xFFu; tc[2] = (s.lo >> 16) & 0xFFu;
        td[0] = s.lo >> 24; td[1] = s.hi & 0xFFu; td[2] = s.hi >> 8;
      } else {                                              // at the border: every tap checked on its own, 0 outside
        const uint8_t* src = slide + yi * row_bytes + xi * 3;   // formed, not read, where a tap is outside
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (y_in0 && x_in0) ta[c] = src[c];
          if (y_in0 && x_in1) tb[c] = src[3 + c];
          if (y_in1 && x_in0) tc[c] = src[row_bytes + c];
          if (y_in1 && x_in1) td[c] = src[row_bytes + 3 + c];
        }
      }
      uint32_t v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint32_t top = ta[c] * (256u - fx) + tb[c] * fx, bot = tc[c] * (256u - fx) + td[c] * fx;
        v[c] = (top * (256u - fy) + bot * fy + 32768u) >> 16;   // <= 255 * 2^16 + 2^15: fits 32 bits
      }
      if constexpr (STAIN) {
        const int32_t tr = s_od[v[0]], tg = s_od[v[1]], tbl = s_od[v[2]];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int64_t o = (int64_t)A[c][0] * tr + (int64_t)A[c][1] * tg + (int64_t)A[c][2] * tbl + b[c];
          const int k = (int)std::min<int64_t>(std::max<int64_t>(o >> shift, 0), lut_n - 1);   // arithmetic shift: floor
          f[c] = div255(s_lut[k]);
        }
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c] = div255(v[c]);
      }
    }
    const int64_t p = p0 + q;
    if (NCHW) {
      const int64_t o = (int64_t)t * 3 * plane + p;
#pragma unroll
      for (int c = 0; c < 3; ++c) st_elem<BF16>(outv, o + c * plane, f[c]);
    } else {
      const int64_t o = ((int64_t)t * plane + p) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) st_elem<BF16>(outv, o + c, f[c]);
    }
  }
}

extern "C" int dh_tile_gather_affine_aug(const uint8_t* slide, int64_t h, int64_t w, const int32_t* yx_dev, const int32_t* params_dev,
                                         const int32_t* params_host_check, const int32_t* affine_dev, const int32_t* affine_host_check,
                                         int64_t n, int32_t P, int32_t layout, int32_t dtype, int32_t flip_h, int32_t flip_v,
                                         const int32_t* od_dev, const int32_t* od_host, int32_t shift, const uint8_t* lut_dev,
                                         int32_t lut_n, void* out, void* stream) {
  DH_REQUIRE(n >= 0 && n <= 65535, "tile gather affine aug: n=%lld out of range [0, 65535]", (long long)n);
  if (n == 0) return DH_OK;
  DH_REQUIRE(slide && yx_dev && affine_dev && out, "tile gather affine aug: null pointer");
  const int n_stain = (params_dev != nullptr) + (od_dev != nullptr) + (od_host != nullptr) + (lut_dev != nullptr);
  DH_REQUIRE(n_stain == 0 || n_stain == 4,
             "tile gather affine aug: partial stain arguments: params_dev, od_dev, od_host and lut_dev must be all given or all null");
  const bool stain = n_stain == 4;
  DH_REQUIRE(stain || !params_host_check, "tile gather affine aug: partial stain arguments: params_host_check without params_dev");
  DH_REQUIRE(h > 0 && w > 0 && h <= INT32_MAX && w <= INT32_MAX, "tile gather affine aug: bad slide size %lld x %lld", (long long)h,
             (long long)w);
  DH_REQUIRE(P >= 1 && P <= kAffineMaxPatch, "tile gather affine aug: patch %d outside [1, %d]", P, kAffineMaxPatch);
  DH_REQUIRE(h >= P && w >= P, "tile gather affine aug: patch %d does not fit %lldx%lld", P, (long long)h, (long long)w);
  if (const int rc = require_layout_dtype("tile gather affine aug", layout, dtype)) return rc;
  if (stain)
    if (const int rc = require_stain_args("tile gather affine aug", lut_n, lut_dev, shift, od_host, params_host_check, n)) return rc;
  if (affine_host_check)
    for (int64_t i = 0; i < 4 * n; ++i)
      DH_REQUIRE(affine_host_check[i] >= -kAffineCoefMax && affine_host_check[i] <= kAffineCoefMax,
                 "tile gather affine aug: affine row %lld, entry %d = %d outside +-%d", (long long)(i / 4), (int)(i % 4),
                 affine_host_check[i], kAffineCoefMax);
  const int64_t blocks = ((int64_t)P * P + kStainPxPerWg - 1) / kStainPxPerWg;
  hipStream_t st = dh::as_stream(stream);
  dim3 grid((unsigned)blocks, (unsigned)n), block(256);
  const int64_t rb = w * 3;
  for_layout_dtype(layout, dtype, [&](auto bf16, auto nchw) {
    constexpr bool BF = decltype(bf16)::value, NC = decltype(nchw)::value;
    auto launch = [&](auto with_stain) {
      hipLaunchKernelGGL((gather_affine_aug_kernel<BF, NC, decltype(with_stain)::value>), grid, block, 0, st, slide, rb, (int)h, (int)w,
                         yx_dev, affine_dev, params_dev, P, flip_h, flip_v, od_dev, (int)shift, lut_dev, (int)lut_n, out);
    };
    if (stain) launch(std::true_type{});
    else launch(std::false_type{});
  });
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// NHWC float32 WITHOUT the /255 (FullImageRndSampler.generator_torch, full_samplers.py:286, yields the
// raw 0..255 values as floats -- unlike the dense sampler).
__global__ __launch_bounds__(256) void gather_raw_nhwc_kernel(const uint8_t* __restrict__ slide, int64_t row_bytes, int h, int w,
                                                              const int32_t* __restrict__ yx, int P, float* __restrict__ out) {
  const int t = blockIdx.y;
  const int y0 = yx[2 * t], x0 = yx[2 * t + 1];
  const int64_t per_tile = (int64_t)P * P * 3;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_tile; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / (3 * P)), rem = (int)(i - (int64_t)r * 3 * P);
    const int yy = y0 + r, xx = x0 + rem / 3;
    const bool in = yy >= 0 && yy < h && xx >= 0 && xx < w;   // outside the slide: 0 (see gather_aug_kernel)
    out[(int64_t)t * per_tile + i] = in ? (float)slide[(int64_t)yy * row_bytes + (int64_t)x0 * 3 + rem] : 0.f;
  }
}

extern "C" int dh_tile_gather_raw(const uint8_t* slide, int64_t h, int64_t w, const int32_t* yx_dev, int64_t n, int32_t P,
                                  float* out, void* stream) {
  DH_REQUIRE(n >= 0 && n <= 65535, "tile gather raw: n=%lld out of range", (long long)n);
  if (n == 0) return DH_OK;
  DH_REQUIRE(slide && yx_dev && out && P > 0 && h >= P && w >= P && h <= INT32_MAX && w <= INT32_MAX, "tile gather raw: bad arguments");
  const int64_t per_tile = (int64_t)P * P * 3;
  dim3 grid((unsigned)std::min<int64_t>((per_tile + 255) / 256, 1024), (unsigned)n), block(256);
  hipLaunchKernelGGL(gather_raw_nhwc_kernel, grid, block, 0, dh::as_stream(stream), slide, w * 3, (int)h, (int)w, yx_dev, P, out);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

__global__ void coords_kernel(const int32_t* __restrict__ yx, int64_t n2, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n2) out[i] = (float)yx[i];
}

extern "C" int dh_tile_coords_f32(const int32_t* yx_dev, int64_t n, float* out, void* stream) {
  if (n == 0) return DH_OK;
  DH_REQUIRE(yx_dev && out && n > 0, "tile coords: bad arguments");
  hipLaunchKernelGGL(coords_kernel, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0,
                     dh::as_stream(stream), yx_dev, 2 * n, out);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
