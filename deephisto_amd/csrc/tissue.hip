// t1: tissue mask for whole-slide prediction.
//
// A pixel is tissue when its chroma c = max(R,G,B) - min(R,G,B) exceeds the threshold t; a tile is kept when its P x P window
// holds at least min_pixels tissue pixels.  Everything here is integer work on the resident uint8 HWC slide, so the result is
// exact and the same on every rank:
//
//   tissue_hist_kernel     256-bin chroma histogram (LDS bins per wave, run-length merged, flushed with 64-bit integer atomics)
//   tissue_bitmap_kernel   1 bit per pixel in FLAT pixel order (bit p of the bitmap = pixel p = y*w + x), 16 bits per lane
//   tissue_count_kernel    per tile, popcount of its P row segments of P bits (one wave per tile, one lane per row)
//   tissue_select_kernel   order-preserving compaction of the kept tiles (one workgroup, block scans; no atomic append)
//   cover_mark / cover_fill  class-map cells outside every kept tile's footprint get the fill class
//
// Both slide passes read the flat byte stream in 16-byte loads: 48 bytes = 16 whole pixels per lane and iteration, which needs
// a 16-byte aligned slide; the h*w % 16 trailing pixels are done by one wave with byte loads.  Flat offsets are 64-bit
// (50 000^2 x 3 bytes > 2^32).  No float arithmetic and no float atomics anywhere.
#include <algorithm>

#include "dh_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int64_t kMaxGrid = 256 * 8;   // 8 workgroups per CU on 256 CUs: enough loads in flight for a streaming pass

__device__ __forceinline__ int px_byte(const uint32_t (&v)[12], int k) { return (v[k >> 2] >> (8 * (k & 3))) & 0xFF; }

__device__ __forceinline__ int chroma3(int r, int g, int b) { return max(r, max(g, b)) - min(r, min(g, b)); }

// 16 chroma values of the 16-pixel group g (48 bytes at byte offset 48*g)
__device__ __forceinline__ void load_group(const uint4* __restrict__ src, int64_t g, int (&c)[16]) {
  uint32_t v[12];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const uint4 q = src[3 * g + j];
    v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) c[i] = chroma3(px_byte(v, 3 * i), px_byte(v, 3 * i + 1), px_byte(v, 3 * i + 2));
}

__global__ __launch_bounds__(kThreads) void tissue_hist_kernel(const uint8_t* __restrict__ slide, int64_t npix,
                                                               unsigned long long* __restrict__ hist) {
  __shared__ uint32_t s_bins[kWaves][256];   // one copy per wave: glass is one chroma value, so a shared copy would serialise
  const int wid = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < kWaves * 256; i += kThreads) (&s_bins[0][0])[i] = 0;
  __syncthreads();
  const uint4* src = reinterpret_cast<const uint4*>(slide);
  const int64_t groups = npix >> 4;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += stride) {
    int c[16];
    load_group(src, g, c);
    int prev = c[0], run = 1;   // runs of equal chroma (glass, flat stain) cost one LDS atomic
#pragma unroll
    for (int i = 1; i < 16; ++i) {
      if (c[i] == prev) {
        ++run;
      } else {
        atomicAdd(&s_bins[wid][prev], (uint32_t)run);
        prev = c[i];
        run = 1;
      }
    }
    atomicAdd(&s_bins[wid][prev], (uint32_t)run);
  }
  if (blockIdx.x == 0 && threadIdx.x < (npix & 15)) {   // the trailing h*w % 16 pixels
    const int64_t p = (groups << 4) + threadIdx.x;
    atomicAdd(&s_bins[wid][chroma3(slide[3 * p], slide[3 * p + 1], slide[3 * p + 2])], 1u);
  }
  __syncthreads();
  // per-wave counts stay below 2^32: a wave sees at most npix / (kMaxGrid * kWaves) + 16 pixels
  uint64_t s = 0;
#pragma unroll
  for (int k = 0; k < kWaves; ++k) s += s_bins[k][threadIdx.x];
  if (s) atomicAdd(&hist[threadIdx.x], (unsigned long long)s);
}

__global__ __launch_bounds__(kThreads) void tissue_bitmap_kernel(const uint8_t* __restrict__ slide, int64_t npix, int t,
                                                                 uint16_t* __restrict__ bits) {
  const uint4* src = reinterpret_cast<const uint4*>(slide);
  const int64_t groups = npix >> 4;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += stride) {
    int c[16];
    load_group(src, g, c);
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) m |= (uint32_t)(c[i] > t) << i;
    bits[g] = (uint16_t)m;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && (npix & 15)) {
    uint32_t m = 0;
    for (int i = 0; i < (int)(npix & 15); ++i) {
      const int64_t p = (groups << 4) + i;
      m |= (uint32_t)(chroma3(slide[3 * p], slide[3 * p + 1], slide[3 * p + 2]) > t) << i;
    }
    bits[groups] = (uint16_t)m;
  }
}

// one wave per tile: lane r sums rows r, r+64, ...; an out-of-slide origin gets count -1 and reads nothing
__global__ __launch_bounds__(kThreads) void tissue_count_kernel(const uint64_t* __restrict__ bm, int64_t h, int64_t w,
                                                                const int32_t* __restrict__ yx, int64_t n, int P,
                                                                int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t tile = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (tile >= n) return;
  const int64_t y = yx[2 * tile], x = yx[2 * tile + 1];
  if (y < 0 || x < 0 || y > h - P || x > w - P) {
    if (lane == 0) counts[tile] = -1;
    return;
  }
  int cnt = 0;
  for (int r = lane; r < P; r += 64) {
    const uint64_t b = (uint64_t)(y + r) * (uint64_t)w + (uint64_t)x;   // first bit of the row segment
    const uint64_t w0 = b >> 6, w1 = (b + P - 1) >> 6;
    const uint64_t lo_mask = ~0ull << (b & 63), hi_mask = ~0ull >> (63 - ((b + P - 1) & 63));
    for (uint64_t k = w0; k <= w1; ++k) {
      uint64_t v = bm[k];
      if (k == w0) v &= lo_mask;
      if (k == w1) v &= hi_mask;
      cnt += __popcll(v);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) counts[tile] = cnt;
}

constexpr int kSelThreads = 1024;
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kSelPer = 4;   // consecutive tiles per thread and round: a round covers 4 096 tiles

// status[0] = kept count, status[1] = number of tiles with a negative count (origin outside the slide)
__global__ __launch_bounds__(kSelThreads) void tissue_select_kernel(const int32_t* __restrict__ counts,
                                                                    const int32_t* __restrict__ yx, int64_t n, int min_pixels,
                                                                    int32_t* __restrict__ kept_idx, int32_t* __restrict__ kept_yx,
                                                                    int32_t* __restrict__ status) {
  __shared__ int s_w[kSelWaves];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int base_out = 0, bad = 0;
  for (int64_t r0 = 0; r0 < n; r0 += (int64_t)kSelThreads * kSelPer) {
    const int64_t i0 = r0 + (int64_t)threadIdx.x * kSelPer;
    bool keep[kSelPer];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < kSelPer; ++j) {
      const int c = i0 + j < n ? counts[i0 + j] : 0;
      bad += c < 0;
      keep[j] = i0 + j < n && c >= 0 && c >= min_pixels;
      mine += keep[j];
    }
    int v = mine;   // inclusive scan over the wave, then over the waves
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(v, o, 64);
      if (lane >= o) v += u;
    }
    if (lane == 63) s_w[wid] = v;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kSelWaves; ++k) {
      const int x = s_w[k];
      before += k < wid ? x : 0;
      total += x;
    }
    __syncthreads();
    int o = base_out + before + v - mine;
#pragma unroll
    for (int j = 0; j < kSelPer; ++j)
      if (keep[j]) {
        kept_idx[o] = (int32_t)(i0 + j);
        if (kept_yx) { kept_yx[2 * o] = yx[2 * (i0 + j)]; kept_yx[2 * o + 1] = yx[2 * (i0 + j) + 1]; }
        ++o;
      }
    base_out += total;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
  if (lane == 0) s_w[wid] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    int b = 0;
    for (int k = 0; k < kSelWaves; ++k) b += s_w[k];
    status[0] = base_out;
    status[1] = b;
  }
}

// one workgroup per kept tile: every cell of its footprint [y//d, (y+P)//d) x [x//d, (x+P)//d) (clipped) is marked covered
__global__ __launch_bounds__(kThreads) void cover_mark_kernel(const int32_t* __restrict__ yx, int P, int d, int64_t dh,
                                                              int64_t dw, uint8_t* __restrict__ cover) {
  const int64_t y = yx[2 * blockIdx.x], x = yx[2 * blockIdx.x + 1];
  if (y < 0 || x < 0) return;   // as dh_accumulate_logits, which refuses such origins
  const int64_t cy0 = y / d, cy1 = std::min<int64_t>((y + P) / d, dh);
  const int64_t cx0 = x / d, cx1 = std::min<int64_t>((x + P) / d, dw);
  if (cy1 <= cy0 || cx1 <= cx0) return;
  const int64_t fw = cx1 - cx0, cells = (cy1 - cy0) * fw;
  for (int64_t i = threadIdx.x; i < cells; i += kThreads) cover[(cy0 + i / fw) * dw + cx0 + i % fw] = 1;
}

__global__ __launch_bounds__(kThreads) void cover_fill_kernel(const uint8_t* __restrict__ cover, int64_t cells, int64_t fill,
                                                              int64_t* __restrict__ map) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < cells; i += (int64_t)gridDim.x * kThreads)
    if (!cover[i]) map[i] = fill;
}

int grid_for(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>((items + kThreads - 1) / kThreads, kMaxGrid)); }

}  // namespace

extern "C" int dh_tissue_histogram(const uint8_t* slide_dev, int64_t h, int64_t w, uint64_t* hist_dev, void* stream) {
  DH_REQUIRE(slide_dev && hist_dev, "tissue_histogram: null pointer");
  DH_REQUIRE(h > 0 && w > 0, "tissue_histogram: bad slide size %lld x %lld", (long long)h, (long long)w);
  DH_REQUIRE(((uintptr_t)slide_dev & 15) == 0, "tissue_histogram: slide must be 16-byte aligned");
  hipStream_t st = dh::as_stream(stream);
  const int64_t npix = h * w;
  DH_HIP(hipMemsetAsync(hist_dev, 0, 256 * sizeof(uint64_t), st));
  hipLaunchKernelGGL(tissue_hist_kernel, dim3(grid_for(npix >> 4)), dim3(kThreads), 0, st, slide_dev, npix,
                     reinterpret_cast<unsigned long long*>(hist_dev));
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_tissue_tile_counts(const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* yx_dev,
                                     const int32_t* yx_host_check, int64_t n, int32_t patch, int32_t threshold,
                                     uint64_t* bitmap_dev, int64_t bitmap_words, int32_t* counts_dev, void* stream) {
  DH_REQUIRE(slide_dev && bitmap_dev && (n == 0 || (yx_dev && counts_dev)), "tissue_tile_counts: null pointer");
  DH_REQUIRE(h > 0 && w > 0 && n >= 0, "tissue_tile_counts: bad sizes");
  DH_REQUIRE(patch > 0 && patch <= h && patch <= w, "tissue_tile_counts: patch %d larger than the %lld x %lld slide", patch,
             (long long)h, (long long)w);
  DH_REQUIRE(threshold >= 0 && threshold <= 255, "tissue_tile_counts: threshold %d outside [0, 255]", threshold);
  DH_REQUIRE(((uintptr_t)slide_dev & 15) == 0, "tissue_tile_counts: slide must be 16-byte aligned");
  DH_REQUIRE(((uintptr_t)bitmap_dev & 7) == 0, "tissue_tile_counts: bitmap must be 8-byte aligned");
  const int64_t npix = h * w;
  DH_REQUIRE(bitmap_words >= (npix + 63) / 64, "tissue_tile_counts: bitmap of %lld words, %lld needed", (long long)bitmap_words,
             (long long)((npix + 63) / 64));
  DH_REQUIRE(n <= (int64_t)INT32_MAX, "tissue_tile_counts: too many tiles");
  if (yx_host_check)
    for (int64_t i = 0; i < n; ++i) {
      const int64_t y = yx_host_check[2 * i], x = yx_host_check[2 * i + 1];
      DH_REQUIRE(y >= 0 && x >= 0 && y <= h - patch && x <= w - patch,
                 "tissue_tile_counts: origin %lld (%lld, %lld) outside the %lld x %lld slide at patch %d", (long long)i,
                 (long long)y, (long long)x, (long long)h, (long long)w, patch);
    }
  hipStream_t st = dh::as_stream(stream);
  hipLaunchKernelGGL(tissue_bitmap_kernel, dim3(grid_for(npix >> 4)), dim3(kThreads), 0, st, slide_dev, npix, (int)threshold,
                     reinterpret_cast<uint16_t*>(bitmap_dev));
  DH_LAUNCH_CHECK();
  if (n > 0) {
    hipLaunchKernelGGL(tissue_count_kernel, dim3((unsigned)((n + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, bitmap_dev, h, w,
                       yx_dev, n, (int)patch, counts_dev);
    DH_LAUNCH_CHECK();
  }
  return DH_OK;
}

extern "C" int dh_tissue_select(const int32_t* counts_dev, const int32_t* yx_dev, int64_t n, int32_t min_pixels,
                                int32_t* kept_idx_dev, int32_t* kept_yx_dev, int32_t* status_dev, int64_t* n_kept_host,
                                void* stream) {
  DH_REQUIRE(status_dev && (n == 0 || (counts_dev && kept_idx_dev)) && (!kept_yx_dev || yx_dev || n == 0),
             "tissue_select: null pointer");
  DH_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX, "tissue_select: bad tile count %lld", (long long)n);
  DH_REQUIRE(min_pixels >= 0, "tissue_select: negative min_pixels %d", min_pixels);
  hipStream_t st = dh::as_stream(stream);
  hipLaunchKernelGGL(tissue_select_kernel, dim3(1), dim3(kSelThreads), 0, st, counts_dev, yx_dev, n, (int)min_pixels,
                     kept_idx_dev, kept_yx_dev, status_dev);
  DH_LAUNCH_CHECK();
  if (n_kept_host) {
    int32_t s[2];
    DH_HIP(hipMemcpyAsync(s, status_dev, sizeof s, hipMemcpyDeviceToHost, st));
    DH_HIP(hipStreamSynchronize(st));
    DH_REQUIRE(s[1] == 0, "tissue_select: %d origins lie outside the slide", s[1]);
    *n_kept_host = s[0];
  }
  return DH_OK;
}

extern "C" int dh_fill_uncovered(const int32_t* yx_dev, int64_t n, int32_t patch, int32_t downscale, int64_t h, int64_t w,
                                 int64_t fill_class, uint8_t* cover_dev, int64_t* map_dev, void* stream) {
  DH_REQUIRE(cover_dev && map_dev && (n == 0 || yx_dev), "fill_uncovered: null pointer");
  DH_REQUIRE(patch > 0 && downscale > 0 && h > 0 && w > 0 && n >= 0 && n <= (int64_t)INT32_MAX, "fill_uncovered: bad sizes");
  const int64_t dh_ = h / downscale, dw_ = w / downscale, cells = dh_ * dw_;
  if (cells == 0) return DH_OK;
  hipStream_t st = dh::as_stream(stream);
  DH_HIP(hipMemsetAsync(cover_dev, 0, (size_t)cells, st));
  if (n > 0) {
    hipLaunchKernelGGL(cover_mark_kernel, dim3((unsigned)n), dim3(kThreads), 0, st, yx_dev, (int)patch, (int)downscale, dh_, dw_,
                       cover_dev);
    DH_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(cover_fill_kernel, dim3(grid_for(cells)), dim3(kThreads), 0, st, cover_dev, cells, fill_class, map_dev);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
