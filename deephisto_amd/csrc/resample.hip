// n2: pyramid layers of the resident slide: integer-exact area average by a rational factor num/den >= 1.
//
// Semantics (every output byte is these bits; the header states the same):
//   oh = (h * den) / num, ow = (w * den) / num            only output pixels whose footprint lies wholly inside the source
//   wy(y, j) = max(0, min((j+1) den, (y+1) num) - max(j den, y num))      wx the same in x; each sums to num over its axis
//   S = sum_j sum_i wy wx src[j][i][c],  D = num^2,  out = (2 S + D) / (2 D)        the exact mean, rounded half up, once
//
// One kernel, one path.  A workgroup owns a strip of `strip` output columns and a band of kBandH output rows.  The strip's source
// footprint is at most kSrcPx pixels = kThreads chunks of 16 bytes, so lane t owns the same 16 source byte columns in every
// source row: it reads them with one 16-byte load per row (neighbouring lanes read neighbouring chunks; the rows of a slide whose
// pitch is no multiple of 16 start at any byte, so the load is by memcpy: one unaligned global_load_dwordx4 on this target) and
// keeps the vertical sums V = sum_j wy * byte in 16 registers.  Per output row the sums go to LDS once (padded so the 16-byte
// stores of neighbouring lanes fall on different banks), each thread reduces its output pixels (t, t + 256, ...: the three bytes
// x*3+c each, with the tap range and edge weight worked out once per strip) horizontally from there, divides, and puts
// the bytes into an LDS row image at the phase of the destination address; the image leaves with 16-byte stores
// where the destination is aligned and byte stores at the two ragged ends.  No float, no atomics; all byte offsets are 64-bit.
//
// The division by 2 D is a multiply-high by M = (2^64 - 1) / (2 D) + 1 (resample.div_magic is its host twin): with
// e = M * 2 D - 2^64 in [0, 2 D], floor(n M / 2^64) = floor(n / (2 D)) while n e < 2^64, and n < 2^32, e < 2^24.
#include <algorithm>
#include <numeric>

#include "dh_common.h"

namespace {

// the tiling constants; deephisto_amd/resample.py repeats them (THREADS, SRC_PX, BAND_H, STORE_GROUP) for the tests
constexpr int kThreads = 256;
constexpr int kChunk = 16;                          // source bytes per lane and row; also the store group
constexpr int kSrcBytes = kThreads * kChunk;        // 4096
constexpr int kSrcPx = kSrcBytes / 3;               // 1365 source pixels under one strip
constexpr int kBandH = 16;                          // output rows per workgroup
constexpr int kMaxNum = 2048;
constexpr int kMaxRatio = 64;
constexpr int64_t kMaxSide = 1 << 20;               // h, w: side * kMaxNum stays inside int32
constexpr int kVWords = kSrcBytes + kSrcBytes / 8;  // V with 4 pad words after every 32
constexpr int kOutBytes = kSrcBytes + 2 * kChunk;   // an output row of the strip (<= 3 * (kSrcPx - 2) bytes) plus its phase
constexpr int kStripMax = kSrcPx - 2;               // output pixels of a strip at most (factor 1)

__device__ __forceinline__ int v_index(int i) { return i + ((i >> 5) << 2); }

__device__ __forceinline__ uint32_t div_magic_apply(uint32_t n, uint32_t mlo, uint32_t mhi) {
  const uint64_t t = ((uint64_t)n * mlo) >> 32;
  return (uint32_t)(((uint64_t)n * mhi + t) >> 32);
}

struct Geom {
  int32_t h, w, oh, ow, num, den, strip, strips;
  uint32_t mlo, mhi;   // the multiply-high constant of 2 num^2
  uint32_t dlo, dhi;   // the multiply-high constant of den (unused for den = 1, whose constant would be 2^64)
};

// floor(n / den) for n < 2^32: the same multiply-high, e <= den < 2^11
__device__ __forceinline__ int div_den(int n, const Geom& g) {
  return g.den == 1 ? n : (int)div_magic_apply((uint32_t)n, g.dlo, g.dhi);
}

__global__ __launch_bounds__(kThreads) void resample_area_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, Geom g) {
  __shared__ __attribute__((aligned(16))) uint32_t s_v[kVWords];
  __shared__ __attribute__((aligned(16))) uint8_t s_out[kOutBytes];
  __shared__ uint32_t s_tap[kStripMax];
  const int t = threadIdx.x;
  const int num = g.num, den = g.den;
  const int strip_i = blockIdx.x, band_i = blockIdx.y;
  const int ox0 = strip_i * g.strip;
  const int nx = min(g.strip, g.ow - ox0);                       // output pixels of this strip
  const int sx0 = div_den(ox0 * num, g);                         // first source pixel under it
  const int sx1 = div_den((ox0 + nx) * num + den - 1, g);        // one past the last; <= w because (ox0 + nx) num <= w den
  const int nsb = 3 * (sx1 - sx0);                               // source bytes under the strip, <= kSrcBytes
  const int lim = 3 * (g.w - sx0);                               // bytes from the strip's start to the end of the source row
  const int cb = kChunk * t;                                     // this lane's chunk
  const bool need = cb < nsb, full = cb + kChunk <= lim;
  const int part = need && !full ? lim - cb : 0;                 // bytes of a chunk cut by the row's end (only the last strip)
  const int64_t pitch = 3 * (int64_t)g.w, opitch = 3 * (int64_t)g.ow;
  const uint8_t* col = src + 3 * (int64_t)sx0 + cb;
  const int nob = 3 * nx;                                        // output bytes per row of this strip
  const uint32_t D = (uint32_t)num * (uint32_t)num;

  // The horizontal taps of an output pixel do not depend on the row: source pixels [i0, i1), the first with weight wf, the last
  // (when there are two or more) with wl = num - wf - (n - 2) den, every one between with den.  Worked out once per strip and
  // kept packed in LDS: (index of V at i0) | n << 12 | wf << 19 (the index below 4096, at most 65 taps, wf <= 2048).
  for (int xr = t; xr < nx; xr += kThreads) {
    const int lo_x = (ox0 + xr) * num, hi_x = lo_x + num;
    const int i0 = div_den(lo_x, g), i1 = div_den(hi_x + den - 1, g);
    const uint32_t wf = (uint32_t)(min((i0 + 1) * den, hi_x) - lo_x);        // i0 den <= lo_x
    s_tap[xr] = (uint32_t)(3 * (i0 - sx0)) | (uint32_t)(i1 - i0) << 12 | wf << 19;
  }
  // (the first __syncthreads() of the row loop orders these stores before their readers)

  const int y0 = band_i * kBandH, y1 = min(y0 + kBandH, g.oh);
  for (int y = y0; y < y1; ++y) {
    const int j0 = div_den(y * num, g);
    const int j1 = div_den((y + 1) * num + den - 1, g);          // <= h because (y + 1) num <= h den
    uint32_t acc[kChunk];
#pragma unroll
    for (int q = 0; q < kChunk; ++q) acc[q] = 0;
    if (need) {
      const int lo_y = y * num, hi_y = lo_y + num;
      int j = j0;
      if (full) {
        for (; j + 4 <= j1; j += 4) {       // four rows in flight
          uint4 v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) __builtin_memcpy(&v[r], col + (int64_t)(j + r) * pitch, 16);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const uint32_t wy = (uint32_t)(min((j + r + 1) * den, hi_y) - max((j + r) * den, lo_y));
            const uint32_t d[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
#pragma unroll
            for (int q = 0; q < kChunk; ++q) acc[q] += wy * ((d[q >> 2] >> (8 * (q & 3))) & 0xFF);
          }
        }
        for (; j < j1; ++j) {
          uint4 v;
          __builtin_memcpy(&v, col + (int64_t)j * pitch, 16);
          const uint32_t wy = (uint32_t)(min((j + 1) * den, hi_y) - max(j * den, lo_y));
          const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int q = 0; q < kChunk; ++q) acc[q] += wy * ((d[q >> 2] >> (8 * (q & 3))) & 0xFF);
        }
      } else {
        for (; j < j1; ++j) {
          const uint8_t* p = col + (int64_t)j * pitch;
          const uint32_t wy = (uint32_t)(min((j + 1) * den, hi_y) - max(j * den, lo_y));
#pragma unroll
          for (int q = 0; q < kChunk; ++q)
            if (q < part) acc[q] += wy * p[q];
        }
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)   // v_index(cb + 4 m) = 16 t + 4 m + 4 (t >> 1): 16-byte aligned, no pad inside the four words
        *reinterpret_cast<uint4*>(&s_v[v_index(cb + 4 * m)]) = make_uint4(acc[4 * m], acc[4 * m + 1], acc[4 * m + 2], acc[4 * m + 3]);
    }
    uint8_t* orow = dst + (int64_t)y * opitch + 3 * (int64_t)ox0;
    const int phase = (int)((uintptr_t)orow & (kChunk - 1));
    __syncthreads();
    for (int xr = t; xr < nx; xr += kThreads) {
      const uint32_t tap = s_tap[xr];
      const int first = (int)(tap & 4095), n = (int)((tap >> 12) & 127);
      const uint32_t wf = tap >> 19;
      uint32_t S[3], mid[3] = {0, 0, 0};
#pragma unroll
      for (int c = 0; c < 3; ++c) S[c] = wf * s_v[v_index(first + c)];
      if (n >= 2) {
        const int last = first + 3 * (n - 1);
        const uint32_t wl = (uint32_t)num - wf - (uint32_t)((n - 2) * den);
#pragma unroll
        for (int c = 0; c < 3; ++c) S[c] += wl * s_v[v_index(last + c)];
        for (int i = first + 3; i < last; i += 3) {
#pragma unroll
          for (int c = 0; c < 3; ++c) mid[c] += s_v[v_index(i + c)];
        }
      }
      uint8_t* o = &s_out[phase + 3 * xr];
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = (uint8_t)div_magic_apply(2 * (S[c] + (uint32_t)den * mid[c]) + D, g.mlo, g.mhi);
    }
    __syncthreads();
    // the image's byte k goes to orow - phase + k; chunks of 16 are aligned in LDS and at the destination alike
    const int end = phase + nob;
    for (int k = kChunk * t; k < end; k += kChunk * kThreads) {
      uint8_t* out = orow - phase + k;
      if (k >= phase && k + kChunk <= end) {
        *reinterpret_cast<uint4*>(out) = *reinterpret_cast<const uint4*>(&s_out[k]);
      } else {
        for (int b = max(k, phase); b < min(k + kChunk, end); ++b) out[b - k] = s_out[b];
      }
    }
    // the next row's stores to s_v come after its loads and the next __syncthreads() after them; its stores to s_out after that one
  }
}

}  // namespace

extern "C" int dh_resample_area(const uint8_t* src_dev, int64_t h, int64_t w, int32_t num, int32_t den, uint8_t* dst_dev, int64_t oh,
                                int64_t ow, void* stream) {
  DH_REQUIRE(src_dev && dst_dev, "resample_area: null pointer");
  DH_REQUIRE(h > 0 && w > 0 && h <= kMaxSide && w <= kMaxSide, "resample_area: bad slide size %lld x %lld (sides in [1, %lld])",
             (long long)h, (long long)w, (long long)kMaxSide);
  DH_REQUIRE(den >= 1 && den <= num && num <= kMaxNum, "resample_area: factor %d/%d outside 1 <= den <= num <= %d", num, den, kMaxNum);
  DH_REQUIRE((int64_t)num <= (int64_t)kMaxRatio * den, "resample_area: factor %d/%d above %d", num, den, kMaxRatio);
  const int32_t gc = std::gcd(num, den);
  num /= gc;
  den /= gc;
  DH_REQUIRE(oh == h * den / num && ow == w * den / num, "resample_area: output of %lld x %lld, %lld x %lld expected", (long long)oh,
             (long long)ow, (long long)(h * den / num), (long long)(w * den / num));
  DH_REQUIRE(oh > 0 && ow > 0, "resample_area: a slide of %lld x %lld has no whole output pixel at factor %d/%d", (long long)h,
             (long long)w, num, den);
  DH_REQUIRE(((uintptr_t)src_dev & 15) == 0 && ((uintptr_t)dst_dev & 15) == 0, "resample_area: src and dst must be 16-byte aligned");
  const uintptr_t a = (uintptr_t)src_dev, b = (uintptr_t)dst_dev;
  DH_REQUIRE(a + (uintptr_t)(3 * h * w) <= b || b + (uintptr_t)(3 * oh * ow) <= a, "resample_area: dst must not overlap src");
  Geom g;
  g.h = (int32_t)h; g.w = (int32_t)w; g.oh = (int32_t)oh; g.ow = (int32_t)ow; g.num = num; g.den = den;
  g.strip = (int32_t)(((int64_t)(kSrcPx - 2) * den) / num);     // ceil((x0 + strip) num / den) - floor(x0 num / den) <= kSrcPx
  g.strips = (int32_t)((ow + g.strip - 1) / g.strip);
  const uint64_t magic = UINT64_MAX / (2 * (uint64_t)num * (uint64_t)num) + 1;
  g.mlo = (uint32_t)magic;
  g.mhi = (uint32_t)(magic >> 32);
  const uint64_t dmagic = den == 1 ? 0 : UINT64_MAX / (uint64_t)den + 1;
  g.dlo = (uint32_t)dmagic;
  g.dhi = (uint32_t)(dmagic >> 32);
  const int64_t bands = (oh + kBandH - 1) / kBandH;
  DH_REQUIRE(bands <= 65535, "resample_area: %lld bands of output rows exceed the grid limit", (long long)bands);
  hipLaunchKernelGGL(resample_area_kernel, dim3((unsigned)g.strips, (unsigned)bands), dim3(kThreads), 0, dh::as_stream(stream), src_dev,
                     dst_dev, g);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
