// n1: Macenko stain normalisation of the resident slide, integer-exact.
//
// Everything a pixel contributes is an integer: its optical density per channel is T[v], a 256-entry fixed-point table the host
// builds (kOdBits fractional bits); a pixel is stained when max(R,G,B) <= vmax (the host's float64 restatement of OD >= beta on
// all three channels).  Four streaming passes over the flat byte stream, as in tissue.hip (16-byte loads, 48 bytes = 16 whole
// pixels per lane and iteration, the h*w % 16 trailing pixels by byte loads, 64-bit flat offsets, capped grid):
//
//   stain_moments_kernel   count, 3 sums and 6 product sums of T over the stained pixels (64-bit registers, wave shuffle,
//                          64-bit integer atomics)
//   stain_angle_kernel     p = (E0.T, E1.T) with the fixed-point eigenvectors E; bin = the k with boundary direction d_k at or
//                          clockwise of p and d_k+1 counter-clockwise of it: quadrant by signs, then a binary search on the
//                          signs of 64-bit cross products (no atan2)
//   stain_conc_kernel      c_s = Pinv_s . T in fixed point, bin = clamp(c_s >> shift, 0, NB-1), one histogram per stain
//   stain_apply_kernel     OD'_c = M_c . T in fixed point, v'_c = lut[clamp(OD'_c >> shift, 0, n-1)] (lut in LDS); in place allowed
//
// The histograms live in LDS as 32-bit bins, runs of equal bins among a lane's 16 pixels cost one LDS atomic, and are flushed
// with 64-bit integer atomics.  No float arithmetic and no float atomics anywhere.
#include <algorithm>

#include "dh_common.h"
#include "stain_fixed.h"

namespace {
using namespace dh_stain;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int64_t kMaxGrid = 256 * 8;      // as tissue.hip: 8 workgroups per CU on 256 CUs
constexpr int64_t kMaxPixels = INT64_MAX / ((int64_t)kOdMax * kOdMax);   // a product sum of all-black pixels stays below 2^63
constexpr int kAngleBins = 1024;
constexpr int kConcBins = 2048;
constexpr int kEvecMax = 1 << 14;          // |eigenvector component|: the projections stay inside int32

struct Vec23 { int32_t m[2][3]; };
struct Mat33 { int32_t m[3][3]; };

__device__ __forceinline__ int px_byte(const uint32_t (&v)[12], int k) { return (v[k >> 2] >> (8 * (k & 3))) & 0xFF; }

__device__ __forceinline__ void load_group(const uint4* src, int64_t g, uint32_t (&v)[12]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const uint4 q = src[3 * g + j];
    v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
  }
}

__device__ __forceinline__ void load_table(int32_t* s_od, const int32_t* __restrict__ od) {
  for (int i = threadIdx.x; i < 256; i += kThreads) s_od[i] = od[i];
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
  return v;
}

// ---------------------------------------------------------------------------------------------- moments
struct Moments {
  uint64_t a[10];   // n, Sr, Sg, Sb, Srr, Srg, Srb, Sgg, Sgb, Sbb
  __device__ __forceinline__ void add(int r, int g, int b, int vmax, const int32_t* s_od) {
    if (max(r, max(g, b)) > vmax) return;
    const uint32_t tr = s_od[r], tg = s_od[g], tb = s_od[b];
    a[0] += 1; a[1] += tr; a[2] += tg; a[3] += tb;
    a[4] += (uint64_t)tr * tr; a[5] += (uint64_t)tr * tg; a[6] += (uint64_t)tr * tb;
    a[7] += (uint64_t)tg * tg; a[8] += (uint64_t)tg * tb; a[9] += (uint64_t)tb * tb;
  }
};

__global__ __launch_bounds__(kThreads) void stain_moments_kernel(const uint8_t* __restrict__ slide, int64_t npix,
                                                                 const int32_t* __restrict__ od, int vmax,
                                                                 unsigned long long* __restrict__ out) {
  __shared__ int32_t s_od[256];
  __shared__ uint64_t s_part[kWaves][10];
  load_table(s_od, od);
  __syncthreads();
  Moments m;
#pragma unroll
  for (int k = 0; k < 10; ++k) m.a[k] = 0;
  const uint4* src = reinterpret_cast<const uint4*>(slide);
  const int64_t groups = npix >> 4;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += stride) {
    uint32_t v[12];
    load_group(src, g, v);
#pragma unroll
    for (int i = 0; i < 16; ++i) m.add(px_byte(v, 3 * i), px_byte(v, 3 * i + 1), px_byte(v, 3 * i + 2), vmax, s_od);
  }
  if (blockIdx.x == 0 && threadIdx.x < (npix & 15)) {   // the trailing h*w % 16 pixels
    const int64_t p = (groups << 4) + threadIdx.x;
    m.add(slide[3 * p], slide[3 * p + 1], slide[3 * p + 2], vmax, s_od);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    const uint64_t s = wave_sum(m.a[k]);
    if (lane == 0) s_part[wid][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 10) {
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) s += s_part[k][threadIdx.x];
    if (s) atomicAdd(&out[threadIdx.x], (unsigned long long)s);
  }
}

// ---------------------------------------------------------------------------------------------- angle histogram
// bin of a stained pixel, -1 for an unstained one.  Quadrants in order of the angle from -pi:
//   0: p0 < 0, p1 <= 0    1: p0 >= 0, p1 < 0    2: p0 >= 0, p1 >= 0 (the zero vector too)    3: p0 <= 0, p1 > 0 (what is left)
// inside quadrant q the answer is the largest k in [256 q, 256 q + 255] with cross(d_k, p) = dx*p1 - dy*p0 >= 0; d_256q is the
// axis itself, so k = 256 q always qualifies.
__device__ __forceinline__ int angle_bin(int r, int g, int b, int vmax, const int32_t* s_od, const Vec23& E,
                                         const int2* __restrict__ s_dir) {
  if (max(r, max(g, b)) > vmax) return -1;
  const int32_t tr = s_od[r], tg = s_od[g], tb = s_od[b];
  const int32_t p0 = E.m[0][0] * tr + E.m[0][1] * tg + E.m[0][2] * tb;
  const int32_t p1 = E.m[1][0] * tr + E.m[1][1] * tg + E.m[1][2] * tb;
  int q;
  if (p0 < 0 && p1 <= 0) q = 0;
  else if (p0 >= 0 && p1 < 0) q = 1;
  else if (p0 >= 0 && p1 >= 0) q = 2;
  else q = 3;
  int lo = q * (kAngleBins / 4);
#pragma unroll
  for (int step = kAngleBins / 8; step > 0; step >>= 1) {
    const int2 d = s_dir[lo + step];
    if ((int64_t)d.x * p1 - (int64_t)d.y * p0 >= 0) lo += step;
  }
  return lo;
}

// runs of equal keys among a lane's pixels cost one LDS atomic; key < 0: no bin
struct RunHist {
  int prev = -1;
  uint32_t run = 0;
  __device__ __forceinline__ void push(int key, uint32_t* bins) {
    if (key == prev) {
      ++run;
    } else {
      if (prev >= 0) atomicAdd(&bins[prev], run);
      prev = key;
      run = 1;
    }
  }
  __device__ __forceinline__ void flush(uint32_t* bins) {
    if (prev >= 0) atomicAdd(&bins[prev], run);
    prev = -1;
    run = 0;
  }
};

__global__ __launch_bounds__(kThreads) void stain_angle_kernel(const uint8_t* __restrict__ slide, int64_t npix,
                                                               const int32_t* __restrict__ od, int vmax, Vec23 E,
                                                               const int2* __restrict__ dirs,
                                                               unsigned long long* __restrict__ hist) {
  __shared__ int32_t s_od[256];
  __shared__ int2 s_dir[kAngleBins];
  __shared__ uint32_t s_bins[kWaves][kAngleBins];   // one copy per wave, as the chroma histogram
  load_table(s_od, od);
  for (int i = threadIdx.x; i < kAngleBins; i += kThreads) s_dir[i] = dirs[i];
  for (int i = threadIdx.x; i < kWaves * kAngleBins; i += kThreads) (&s_bins[0][0])[i] = 0;
  __syncthreads();
  uint32_t* bins = s_bins[threadIdx.x >> 6];
  const uint4* src = reinterpret_cast<const uint4*>(slide);
  const int64_t groups = npix >> 4;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += stride) {
    uint32_t v[12];
    load_group(src, g, v);
    RunHist rh;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      rh.push(angle_bin(px_byte(v, 3 * i), px_byte(v, 3 * i + 1), px_byte(v, 3 * i + 2), vmax, s_od, E, s_dir), bins);
    rh.flush(bins);
  }
  if (blockIdx.x == 0 && threadIdx.x < (npix & 15)) {
    const int64_t p = (groups << 4) + threadIdx.x;
    const int k = angle_bin(slide[3 * p], slide[3 * p + 1], slide[3 * p + 2], vmax, s_od, E, s_dir);
    if (k >= 0) atomicAdd(&bins[k], 1u);
  }
  __syncthreads();
  // per-wave counts stay below 2^32: a wave sees at most npix / (kMaxGrid * kWaves) + 16 pixels
  for (int i = threadIdx.x; i < kAngleBins; i += kThreads) {
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) s += s_bins[k][i];
    if (s) atomicAdd(&hist[i], (unsigned long long)s);
  }
}

// ---------------------------------------------------------------------------------------------- concentration histograms
__device__ __forceinline__ void conc_bins(int r, int g, int b, int vmax, const int32_t* s_od, const Vec23& P, int shift,
                                          int& k0, int& k1) {
  if (max(r, max(g, b)) > vmax) { k0 = k1 = -1; return; }
  const int32_t tr = s_od[r], tg = s_od[g], tb = s_od[b];
  const int64_t c0 = (int64_t)P.m[0][0] * tr + (int64_t)P.m[0][1] * tg + (int64_t)P.m[0][2] * tb;
  const int64_t c1 = (int64_t)P.m[1][0] * tr + (int64_t)P.m[1][1] * tg + (int64_t)P.m[1][2] * tb;
  k0 = (int)std::min<int64_t>(std::max<int64_t>(c0 >> shift, 0), kConcBins - 1);   // arithmetic shift: floor
  k1 = (int)std::min<int64_t>(std::max<int64_t>(c1 >> shift, 0), kConcBins - 1);
}

__global__ __launch_bounds__(kThreads) void stain_conc_kernel(const uint8_t* __restrict__ slide, int64_t npix,
                                                              const int32_t* __restrict__ od, int vmax, Vec23 P, int shift,
                                                              unsigned long long* __restrict__ hist) {
  __shared__ int32_t s_od[256];
  __shared__ uint32_t s_bins[2][2][kConcBins];   // [wave pair][stain][bin]: 32 KiB
  load_table(s_od, od);
  for (int i = threadIdx.x; i < 4 * kConcBins; i += kThreads) (&s_bins[0][0][0])[i] = 0;
  __syncthreads();
  uint32_t* b0 = s_bins[(threadIdx.x >> 6) & 1][0];
  uint32_t* b1 = s_bins[(threadIdx.x >> 6) & 1][1];
  const uint4* src = reinterpret_cast<const uint4*>(slide);
  const int64_t groups = npix >> 4;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += stride) {
    uint32_t v[12];
    load_group(src, g, v);
    RunHist r0, r1;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      int k0, k1;
      conc_bins(px_byte(v, 3 * i), px_byte(v, 3 * i + 1), px_byte(v, 3 * i + 2), vmax, s_od, P, shift, k0, k1);
      r0.push(k0, b0);
      r1.push(k1, b1);
    }
    r0.flush(b0);
    r1.flush(b1);
  }
  if (blockIdx.x == 0 && threadIdx.x < (npix & 15)) {
    const int64_t p = (groups << 4) + threadIdx.x;
    int k0, k1;
    conc_bins(slide[3 * p], slide[3 * p + 1], slide[3 * p + 2], vmax, s_od, P, shift, k0, k1);
    if (k0 >= 0) { atomicAdd(&b0[k0], 1u); atomicAdd(&b1[k1], 1u); }
  }
  __syncthreads();
  // a copy's counts stay below 2^32: a workgroup sees at most npix / kMaxGrid + 16 * kThreads pixels
  for (int i = threadIdx.x; i < 2 * kConcBins; i += kThreads) {
    const uint64_t s = (uint64_t)(&s_bins[0][0][0])[i] + (&s_bins[1][0][0])[i];
    if (s) atomicAdd(&hist[i], (unsigned long long)s);
  }
}

// ---------------------------------------------------------------------------------------------- apply
__device__ __forceinline__ uint32_t apply_px(int r, int g, int b, const int32_t* s_od, const Mat33& M, int shift,
                                             const uint8_t* s_lut, int lut_n) {
  const int32_t tr = s_od[r], tg = s_od[g], tb = s_od[b];
  uint32_t out = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int64_t o = (int64_t)M.m[c][0] * tr + (int64_t)M.m[c][1] * tg + (int64_t)M.m[c][2] * tb;
    const int k = (int)std::min<int64_t>(std::max<int64_t>(o >> shift, 0), lut_n - 1);
    out |= (uint32_t)s_lut[k] << (8 * c);
  }
  return out;   // R | G << 8 | B << 16
}

// slide and out may be the same buffer: a lane writes only the bytes it has read
__global__ __launch_bounds__(kThreads) void stain_apply_kernel(const uint8_t* slide, int64_t npix, const int32_t* __restrict__ od,
                                                               Mat33 M, int shift, const uint8_t* __restrict__ lut, int lut_n,
                                                               uint8_t* out) {
  __shared__ int32_t s_od[256];
  __shared__ uint8_t s_lut[kLutMax];
  load_table(s_od, od);
  for (int i = threadIdx.x; i < lut_n; i += kThreads) s_lut[i] = lut[i];
  __syncthreads();
  const uint4* src = reinterpret_cast<const uint4*>(slide);
  uint4* dst = reinterpret_cast<uint4*>(out);
  const int64_t groups = npix >> 4;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += stride) {
    uint32_t v[12];
    load_group(src, g, v);
    uint32_t o[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) o[j] = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t px = apply_px(px_byte(v, 3 * i), px_byte(v, 3 * i + 1), px_byte(v, 3 * i + 2), s_od, M, shift, s_lut, lut_n);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int k = 3 * i + c;
        o[k >> 2] |= ((px >> (8 * c)) & 0xFF) << (8 * (k & 3));
      }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) dst[3 * g + j] = make_uint4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
  }
  if (blockIdx.x == 0 && threadIdx.x < (npix & 15)) {
    const int64_t p = (groups << 4) + threadIdx.x;
    const uint32_t px = apply_px(slide[3 * p], slide[3 * p + 1], slide[3 * p + 2], s_od, M, shift, s_lut, lut_n);
    out[3 * p] = (uint8_t)px; out[3 * p + 1] = (uint8_t)(px >> 8); out[3 * p + 2] = (uint8_t)(px >> 16);
  }
}

int grid_for(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>((items + kThreads - 1) / kThreads, kMaxGrid)); }

// the checks every entry shares; od_host_check: the table on the host, every value in [0, kOdMax]
int check_common(const char* what, const void* slide, int64_t h, int64_t w, const void* od_dev, const int32_t* od_host,
                 int32_t vmax) {
  DH_REQUIRE(slide && od_dev && od_host, "%s: null pointer", what);
  DH_REQUIRE(h > 0 && w > 0, "%s: bad slide size %lld x %lld", what, (long long)h, (long long)w);
  DH_REQUIRE(h <= kMaxPixels / w, "%s: slide of %lld x %lld pixels exceeds max_pixels = %lld (64-bit product sums)", what,
             (long long)h, (long long)w, (long long)kMaxPixels);
  DH_REQUIRE(((uintptr_t)slide & 15) == 0, "%s: slide must be 16-byte aligned", what);
  DH_REQUIRE(vmax >= -1 && vmax <= 255, "%s: vmax %d outside [-1, 255]", what, vmax);
  for (int i = 0; i < 256; ++i)
    DH_REQUIRE(od_host[i] >= 0 && od_host[i] <= kOdMax, "%s: od table entry %d = %d outside [0, %d]", what, i, od_host[i], kOdMax);
  return DH_OK;
}

}  // namespace

extern "C" int64_t dh_stain_max_pixels(void) { return kMaxPixels; }

extern "C" int dh_stain_moments(const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* od_dev, const int32_t* od_host,
                                int32_t vmax, uint64_t* moments_dev, void* stream) {
  if (int rc = check_common("stain_moments", slide_dev, h, w, od_dev, od_host, vmax)) return rc;
  DH_REQUIRE(moments_dev, "stain_moments: null pointer");
  hipStream_t st = dh::as_stream(stream);
  const int64_t npix = h * w;
  DH_HIP(hipMemsetAsync(moments_dev, 0, 10 * sizeof(uint64_t), st));
  hipLaunchKernelGGL(stain_moments_kernel, dim3(grid_for(npix >> 4)), dim3(kThreads), 0, st, slide_dev, npix, od_dev, (int)vmax,
                     reinterpret_cast<unsigned long long*>(moments_dev));
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_stain_angle_hist(const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* od_dev, const int32_t* od_host,
                                   int32_t vmax, const int32_t* evec_host, const int32_t* bounds_dev, int32_t n_bins,
                                   uint64_t* hist_dev, void* stream) {
  if (int rc = check_common("stain_angle_hist", slide_dev, h, w, od_dev, od_host, vmax)) return rc;
  DH_REQUIRE(evec_host && bounds_dev && hist_dev, "stain_angle_hist: null pointer");
  DH_REQUIRE(n_bins == kAngleBins, "stain_angle_hist: %d angle bins, %d expected", n_bins, kAngleBins);
  DH_REQUIRE(((uintptr_t)bounds_dev & 7) == 0, "stain_angle_hist: boundary table must be 8-byte aligned");
  Vec23 E;
  for (int i = 0; i < 6; ++i) {
    DH_REQUIRE(evec_host[i] >= -kEvecMax && evec_host[i] <= kEvecMax, "stain_angle_hist: eigenvector component %d outside +-%d",
               evec_host[i], kEvecMax);
    E.m[i / 3][i % 3] = evec_host[i];
  }
  hipStream_t st = dh::as_stream(stream);
  const int64_t npix = h * w;
  DH_HIP(hipMemsetAsync(hist_dev, 0, kAngleBins * sizeof(uint64_t), st));
  hipLaunchKernelGGL(stain_angle_kernel, dim3(grid_for(npix >> 4)), dim3(kThreads), 0, st, slide_dev, npix, od_dev, (int)vmax, E,
                     reinterpret_cast<const int2*>(bounds_dev), reinterpret_cast<unsigned long long*>(hist_dev));
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_stain_conc_hist(const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* od_dev, const int32_t* od_host,
                                  int32_t vmax, const int32_t* pinv_host, int32_t shift, int32_t n_bins, uint64_t* hist_dev,
                                  void* stream) {
  if (int rc = check_common("stain_conc_hist", slide_dev, h, w, od_dev, od_host, vmax)) return rc;
  DH_REQUIRE(pinv_host && hist_dev, "stain_conc_hist: null pointer");
  DH_REQUIRE(n_bins == kConcBins, "stain_conc_hist: %d concentration bins, %d expected", n_bins, kConcBins);
  DH_REQUIRE(shift >= 0 && shift < 40, "stain_conc_hist: shift %d outside [0, 40)", shift);
  Vec23 P;
  for (int i = 0; i < 6; ++i) {
    DH_REQUIRE(pinv_host[i] >= -kCoefMax && pinv_host[i] <= kCoefMax, "stain_conc_hist: pseudo-inverse entry %d outside +-%d",
               pinv_host[i], kCoefMax);
    P.m[i / 3][i % 3] = pinv_host[i];
  }
  hipStream_t st = dh::as_stream(stream);
  const int64_t npix = h * w;
  DH_HIP(hipMemsetAsync(hist_dev, 0, 2 * kConcBins * sizeof(uint64_t), st));
  hipLaunchKernelGGL(stain_conc_kernel, dim3(grid_for(npix >> 4)), dim3(kThreads), 0, st, slide_dev, npix, od_dev, (int)vmax, P,
                     (int)shift, reinterpret_cast<unsigned long long*>(hist_dev));
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_stain_apply(const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* od_dev, const int32_t* od_host,
                              const int32_t* matrix_host, int32_t shift, const uint8_t* lut_dev, int32_t lut_n, uint8_t* out_dev,
                              void* stream) {
  if (int rc = check_common("stain_apply", slide_dev, h, w, od_dev, od_host, 255)) return rc;
  DH_REQUIRE(matrix_host && lut_dev && out_dev, "stain_apply: null pointer");
  DH_REQUIRE(((uintptr_t)out_dev & 15) == 0, "stain_apply: out must be 16-byte aligned");
  DH_REQUIRE(lut_n > 0 && lut_n <= kLutMax, "stain_apply: output table of %d entries, at most %d", lut_n, kLutMax);
  DH_REQUIRE(shift >= 0 && shift < 40, "stain_apply: shift %d outside [0, 40)", shift);
  const int64_t npix = h * w;
  const uintptr_t a = (uintptr_t)slide_dev, b = (uintptr_t)out_dev;
  DH_REQUIRE(a == b || a + (uintptr_t)(3 * npix) <= b || b + (uintptr_t)(3 * npix) <= a,
             "stain_apply: out must be the slide itself or not overlap it");
  Mat33 M;
  for (int i = 0; i < 9; ++i) {
    DH_REQUIRE(matrix_host[i] >= -kCoefMax && matrix_host[i] <= kCoefMax, "stain_apply: matrix entry %d outside +-%d",
               matrix_host[i], kCoefMax);
    M.m[i / 3][i % 3] = matrix_host[i];
  }
  hipStream_t st = dh::as_stream(stream);
  hipLaunchKernelGGL(stain_apply_kernel, dim3(grid_for(npix >> 4)), dim3(kThreads), 0, st, slide_dev, npix, od_dev, M, (int)shift,
                     lut_dev, (int)lut_n, out_dev);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
