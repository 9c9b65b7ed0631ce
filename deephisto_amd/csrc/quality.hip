// q1: tile quality for whole-slide prediction: out-of-focus and ink-marked tiles.
//
// Per pixel (quality_rule.h): luma Y, the tissue filter's chroma test, the ink test.  Per tile of side P at any origin: over its
// tissue pixels the count n_t and the sums S1, S2 of the 4-neighbour Laplacian L of Y and of L*L, and over all its pixels the
// ink count.  Neighbours outside the tile are the slide's pixels, neighbours outside the slide repeat the edge pixel (clamped
// coordinates).  Everything is integer work on the resident uint8 HWC slide, so the result is exact and the same on every rank.
//
//   quality_stats_kernel   one workgroup per tile, sweeping its window in bands of kBand rows.  A band's (rows + 2) x (P + 2)
//                          pixels are staged in LDS as 16-bit words (Y | tissue << 8 | ink << 9): four pixels per lane from one
//                          12-byte load (rows of a slide start at any byte, so this is an unaligned global_load_dwordx3) into
//                          one 8-byte LDS store; the two halo columns and the ragged last P % 4 pixels by byte loads.  Then four
//                          pixels per lane again: three 8-byte LDS reads (the rows above, at and below) and the two words left
//                          and right.  Every lane keeps n_t, S1, n_ink in 32 bits (a lane sees about P*P/256 <= 4 096 pixels,
//                          |S1| <= 4.2e6) and S2 in 64; the sums meet by wave shuffles, then through LDS, and lane 0 stores the
//                          four int64 values.  No atomics.
//   quality_flags_kernel   the reason mask and the keep flag of every tile from its four sums (qr::reason)
//
// All slide offsets are 64-bit (50 000^2 x 3 bytes > 2^32).  No float arithmetic anywhere.
#include "dh_common.h"
#include "quality_rule.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBand = 16;    // rows per band: the halo rows cost 2 / 16 more reads; 18 rows of 1 032 words are 37 152 bytes of LDS
constexpr int kLeft = 4;     // LDS column of the tile's first pixel: every four-pixel group starts on an 8-byte boundary

__host__ __device__ constexpr int row_pitch(int P) { return ((P + 3) & ~3) + 8; }   // words: 4 left (halo at 3), P, halo, padding

__device__ __forceinline__ uint32_t px_word(int r, int g, int b, int t, int ink_chroma, int ink_margin, int dark_max) {
  return (uint32_t)qr::luma(r, g, b) | (uint32_t)qr::tissue(r, g, b, t) << 8 |
         (uint32_t)qr::ink(r, g, b, ink_chroma, ink_margin, dark_max) << 9;
}

__global__ __launch_bounds__(kThreads) void quality_stats_kernel(const uint8_t* __restrict__ slide, int64_t h, int64_t w,
                                                                 const int32_t* __restrict__ yx, int P, int t, int ink_chroma,
                                                                 int ink_margin, int dark_max, int64_t* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) uint16_t s_px[];   // [kBand + 2][row_pitch(P)]
  __shared__ int64_t s_red[kWaves][4];
  const int64_t tile = blockIdx.x;
  const int64_t y0 = yx[2 * tile], x0 = yx[2 * tile + 1];
  if (y0 < 0 || x0 < 0 || y0 > h - P || x0 > w - P) {   // an origin nobody checked on the host: flagged, nothing is read
    if (threadIdx.x < 4) stats[4 * tile + threadIdx.x] = -1;
    return;
  }
  const int pitch = row_pitch(P);
  const int nchunks = (P + 3) >> 2;                      // four-pixel groups of a row; the last may be ragged
  const int per_row = nchunks + 1;                       // staging: plus one item for the two halo columns
  const int64_t xl = x0 > 0 ? x0 - 1 : 0, xr = x0 + P < w ? x0 + P : w - 1;   // clamped halo columns
  int n_t = 0, n_ink = 0, s1 = 0;
  uint64_t s2 = 0;

  for (int band0 = 0; band0 < P; band0 += kBand) {
    const int rows = min(kBand, P - band0);
    // ---- stage rows band0 - 1 .. band0 + rows of the window
    {
      int r = threadIdx.x / per_row, k = threadIdx.x - r * per_row;
      const int dr = kThreads / per_row, dk = kThreads - dr * per_row;
      while (r < rows + 2) {
        int64_t yy = y0 + band0 + r - 1;
        yy = yy < 0 ? 0 : yy > h - 1 ? h - 1 : yy;
        const uint8_t* row = slide + 3 * (yy * w);
        uint16_t* to = s_px + r * pitch;
        if (k == nchunks) {
          const uint8_t *a = row + 3 * xl, *b = row + 3 * xr;
          to[kLeft - 1] = (uint16_t)px_word(a[0], a[1], a[2], t, ink_chroma, ink_margin, dark_max);
          to[kLeft + P] = (uint16_t)px_word(b[0], b[1], b[2], t, ink_chroma, ink_margin, dark_max);
        } else if (4 * k + 4 <= P) {
          uint32_t v[3];
          __builtin_memcpy(v, row + 3 * (x0 + 4 * k), 12);   // pixels 4k .. 4k+3 of the window: inside the slide
          uint32_t o[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int b0 = 3 * j, b1 = 3 * j + 1, b2 = 3 * j + 2;
            o[j] = px_word((v[b0 >> 2] >> (8 * (b0 & 3))) & 0xFF, (v[b1 >> 2] >> (8 * (b1 & 3))) & 0xFF,
                           (v[b2 >> 2] >> (8 * (b2 & 3))) & 0xFF, t, ink_chroma, ink_margin, dark_max);
          }
          *reinterpret_cast<uint2*>(to + kLeft + 4 * k) = make_uint2(o[0] | o[1] << 16, o[2] | o[3] << 16);
        } else {
          for (int c = 4 * k; c < P; ++c) {
            const uint8_t* a = row + 3 * (x0 + c);
            to[kLeft + c] = (uint16_t)px_word(a[0], a[1], a[2], t, ink_chroma, ink_margin, dark_max);
          }
        }
        r += dr;
        k += dk;
        if (k >= per_row) { k -= per_row; ++r; }
      }
    }
    __syncthreads();
    // ---- Laplacian and sums of window rows band0 .. band0 + rows - 1 (LDS rows 1 .. rows)
    {
      int r = threadIdx.x / nchunks, k = threadIdx.x - r * nchunks;
      const int dr = kThreads / nchunks, dk = kThreads - dr * nchunks;
      while (r < rows) {
        const uint16_t* mid = s_px + (r + 1) * pitch + kLeft + 4 * k;
        const uint2 up = *reinterpret_cast<const uint2*>(mid - pitch);
        const uint2 cc = *reinterpret_cast<const uint2*>(mid);
        const uint2 dn = *reinterpret_cast<const uint2*>(mid + pitch);
        int c[6];
        c[0] = mid[-1];
        c[1] = cc.x & 0xFFFF; c[2] = cc.x >> 16; c[3] = cc.y & 0xFFFF; c[4] = cc.y >> 16;
        c[5] = mid[4];
        const int u[4] = {(int)(up.x & 0xFF), (int)((up.x >> 16) & 0xFF), (int)(up.y & 0xFF), (int)((up.y >> 16) & 0xFF)};
        const int d[4] = {(int)(dn.x & 0xFF), (int)((dn.x >> 16) & 0xFF), (int)(dn.y & 0xFF), (int)((dn.y >> 16) & 0xFF)};
        const int live = min(4, P - 4 * k);   // words past the window's last column (a ragged group) are not pixels
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j >= live) break;
          const int L = 4 * (c[j + 1] & 0xFF) - u[j] - d[j] - (c[j] & 0xFF) - (c[j + 2] & 0xFF);
          const int tis = (c[j + 1] >> 8) & 1;
          n_t += tis;
          n_ink += (c[j + 1] >> 9) & 1;
          s1 += tis ? L : 0;
          s2 += tis ? (uint32_t)(L * L) : 0u;
        }
        r += dr;
        k += dk;
        if (k >= nchunks) { k -= nchunks; ++r; }
      }
    }
    __syncthreads();   // the next band overwrites what was just read
  }

  int64_t v[4] = {n_t, s1, (int64_t)s2, n_ink};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[i] += __shfl_xor(v[i], o, 64);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0)
    for (int i = 0; i < 4; ++i) s_red[wid][i] = v[i];
  __syncthreads();
  if (threadIdx.x < 4) {
    int64_t s = 0;
    for (int k = 0; k < kWaves; ++k) s += s_red[k][threadIdx.x];
    stats[4 * tile + threadIdx.x] = s;
  }
}

// a tile whose sums are -1 (origin outside the slide) gets keep = -1, which dh_tissue_select counts and refuses
__global__ __launch_bounds__(kThreads) void quality_flags_kernel(const int64_t* __restrict__ stats, int64_t n, int64_t min_sharpness,
                                                                 int64_t max_ink_pixels, uint8_t* __restrict__ reason,
                                                                 int32_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t n_t = stats[4 * i], S1 = stats[4 * i + 1], S2 = stats[4 * i + 2], n_ink = stats[4 * i + 3];
  if (n_t < 0) {
    reason[i] = 0xFF;
    keep[i] = -1;
    return;
  }
  const uint8_t m = qr::reason(n_t, S1, S2, n_ink, min_sharpness, max_ink_pixels);
  reason[i] = m;
  keep[i] = m == 0;
}

}  // namespace

extern "C" int dh_quality_tile_stats(const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* yx_dev,
                                     const int32_t* yx_host_check, int64_t n, int32_t patch, int32_t threshold, int32_t ink_chroma,
                                     int32_t ink_margin, int32_t dark_max, int64_t* stats_dev, void* stream) {
  DH_REQUIRE(slide_dev && (n == 0 || (yx_dev && stats_dev)), "quality_tile_stats: null pointer");
  DH_REQUIRE(h > 0 && w > 0 && n >= 0, "quality_tile_stats: bad sizes");
  DH_REQUIRE(patch > 0 && patch <= h && patch <= w, "quality_tile_stats: patch %d larger than the %lld x %lld slide", patch,
             (long long)h, (long long)w);
  DH_REQUIRE(patch <= qr::kMaxPatch, "quality_tile_stats: patch %d above %d (the int64 bound of the sharpness test)", patch,
             qr::kMaxPatch);
  DH_REQUIRE(threshold >= -1 && threshold <= 255, "quality_tile_stats: threshold %d outside [-1, 255]", threshold);
  DH_REQUIRE(ink_chroma >= 0 && ink_chroma <= 255, "quality_tile_stats: ink_chroma %d outside [0, 255]", ink_chroma);
  DH_REQUIRE(ink_margin >= 0 && ink_margin <= 255, "quality_tile_stats: ink_margin %d outside [0, 255]", ink_margin);
  DH_REQUIRE(dark_max >= -1 && dark_max <= 255, "quality_tile_stats: dark_max %d outside [-1, 255]", dark_max);
  DH_REQUIRE(((uintptr_t)stats_dev & 7) == 0, "quality_tile_stats: stats must be 8-byte aligned");
  DH_REQUIRE(n <= (int64_t)INT32_MAX, "quality_tile_stats: too many tiles");
  if (yx_host_check)
    for (int64_t i = 0; i < n; ++i) {
      const int64_t y = yx_host_check[2 * i], x = yx_host_check[2 * i + 1];
      DH_REQUIRE(y >= 0 && x >= 0 && y <= h - patch && x <= w - patch,
                 "quality_tile_stats: origin %lld (%lld, %lld) outside the %lld x %lld slide at patch %d", (long long)i,
                 (long long)y, (long long)x, (long long)h, (long long)w, patch);
    }
  if (n == 0) return DH_OK;
  const size_t lds = (size_t)(kBand + 2) * row_pitch(patch) * sizeof(uint16_t);
  hipLaunchKernelGGL(quality_stats_kernel, dim3((unsigned)n), dim3(kThreads), lds, dh::as_stream(stream), slide_dev, h, w, yx_dev,
                     (int)patch, (int)threshold, (int)ink_chroma, (int)ink_margin, (int)dark_max, stats_dev);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_quality_flags(const int64_t* stats_dev, int64_t n, int64_t min_sharpness, int64_t max_ink_pixels,
                                uint8_t* reason_dev, int32_t* keep_dev, void* stream) {
  DH_REQUIRE(n == 0 || (stats_dev && reason_dev && keep_dev), "quality_flags: null pointer");
  DH_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX, "quality_flags: bad tile count %lld", (long long)n);
  DH_REQUIRE(min_sharpness >= 0 && min_sharpness <= qr::kMaxSharpness, "quality_flags: min_sharpness %lld outside [0, %lld]",
             (long long)min_sharpness, (long long)qr::kMaxSharpness);
  DH_REQUIRE(max_ink_pixels >= 0 && max_ink_pixels <= (int64_t)qr::kMaxPatch * qr::kMaxPatch,
             "quality_flags: max_ink_pixels %lld outside [0, %lld]", (long long)max_ink_pixels,
             (long long)qr::kMaxPatch * qr::kMaxPatch);
  if (n == 0) return DH_OK;
  hipLaunchKernelGGL(quality_flags_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, dh::as_stream(stream),
                     stats_dev, n, min_sharpness, max_ink_pixels, reason_dev, keep_dev);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
