// Whole-slide probability maps for MI355X (gfx950, wave64):
//   dh_softmax_rows     per-tile softmax of the logits (expf, sums in class order)
//   dh_accumulate_mean  ordered per-cell sums of the tile probabilities + int32 hit counts, with the finish fused in on request
//   dh_accumulate_cam_mean  the same over S x S rows per tile, each on its own 32 x 32-pixel block
//   dh_finish_mean      proba = sum / count, first-maximum class, confidence; fill for cells nothing covers
//   dh_heatmap_blend    a scalar field times a colour blended over the slide in float64
// HBM-bound like the class-map kernels of tile_kernels.hip, whose bin plan (one workgroup per G x G bin, one writer per cell,
// tile lists staged through LDS) dh_accumulate_mean shares.  No atomics: every result is bit-identical to the NumPy loop.
#include <algorithm>

#include "dh_common.h"

namespace {
using dh::BinGeom;

constexpr int MAX_CLS = 64;

__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* x, int64_t n, int n_cls, float* p) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float* xi = x + i * n_cls;
    float* pi = p + i * n_cls;
    float m = xi[0];
    for (int c = 1; c < n_cls; ++c) { const float v = xi[c]; m = v > m ? v : m; }
    float s = 0.f;
    for (int c = 0; c < n_cls; ++c) {   // e_c is parked in the output row: the thread reads back its own stores
      const float e = expf(xi[c] - m);
      pi[c] = e;
      s = s + e;
    }
    for (int c = 0; c < n_cls; ++c) pi[c] = pi[c] / s;
  }
}

// NumPy argmax over one cell's classes: the first maximum; a NaN wins once (argmax_kernel's rule)
template <typename Ptr>
__device__ __forceinline__ int first_max(Ptr p, int n_cls, float* best_out) {
  float best = p[0];
  int bi = 0;
  for (int c = 1; c < n_cls; ++c) {
    const float v = p[c];
    if (v > best || (v != v && best == best)) { best = v; bi = c; }
  }
  *best_out = best;
  return bi;
}

// One workgroup per bin.  A pass handles cpp = 256 / n_cls whole cells, one thread per (cell, class): the thread carries the
// cell's running sum of its class and the cell's hit count through the bin's tile list (256 tiles per LDS stage), in list
// order.  FINISH: the pass ends with proba = sum / count through LDS and the class-0 thread of each cell takes the first
// maximum -- the sums never travel to HBM and back for the finish.  Bins without tiles still run then (their cells get the
// fill, or the finish of what the state held).
// CAM (dh_accumulate_cam_mean): `probs` holds S x S rows per tile and a covered cell takes the row dh::cam_row names, as in
// accumulate_bins_kernel<true>.
template <bool FINISH, bool CAM = false>
__global__ __launch_bounds__(256) void accumulate_mean_kernel(
    const float* __restrict__ probs, const int32_t* __restrict__ yx, const int32_t* __restrict__ bin_start,
    const int32_t* __restrict__ bin_tiles, BinGeom g, float* __restrict__ sum, int32_t* __restrict__ count,
    int64_t* __restrict__ map, float* __restrict__ conf, int fill_class) {
  __shared__ int32_t s_t[256], s_y0[256], s_y1[256], s_x0[256], s_x1[256];
  __shared__ float s_p[256];
  __shared__ int32_t s_y[CAM ? 256 : 1], s_x[CAM ? 256 : 1];
  const int S = g.P >> 5;
  const int bin = blockIdx.x;
  const int beg = bin_start[bin], end = bin_start[bin + 1];
  if (!FINISH && beg == end) return;  // uniform for the block
  const int by = bin / g.bins_x, bx = bin - by * g.bins_x;
  const int cells = g.G * g.G, cpp = 256 / g.n_cls;
  const int lc = threadIdx.x / g.n_cls, cls = threadIdx.x - lc * g.n_cls;
  for (int c0 = 0; c0 < cells; c0 += cpp) {
    const int cell = c0 + lc;
    const int cy = by * g.G + cell / g.G, cx = bx * g.G + cell % g.G;
    const bool live = lc < cpp && cell < cells && cy < g.dh && cx < g.dw;
    const int64_t cidx = (int64_t)cy * g.dw + cx, addr = cidx * g.n_cls + cls;
    float acc = live ? sum[addr] : 0.f;
    int32_t cnt = live ? count[cidx] : 0;
    for (int l0 = beg; l0 < end; l0 += 256) {
      __syncthreads();
      const int l = l0 + threadIdx.x;
      if (l < end) {
        const int t = bin_tiles[l];
        const int y = yx[2 * t], x = yx[2 * t + 1];
        s_t[threadIdx.x] = t;
        s_y0[threadIdx.x] = y / g.d; s_y1[threadIdx.x] = (y + g.P) / g.d;
        s_x0[threadIdx.x] = x / g.d; s_x1[threadIdx.x] = (x + g.P) / g.d;
        if constexpr (CAM) { s_y[threadIdx.x] = y; s_x[threadIdx.x] = x; }
      }
      __syncthreads();
      const int m = min(256, end - l0);
      if (live)
        for (int k = 0; k < m; ++k)
          if (cy >= s_y0[k] && cy < s_y1[k] && cx >= s_x0[k] && cx < s_x1[k]) {
            int64_t row = s_t[k];
            if constexpr (CAM) row = dh::cam_row(row, S, g.d, cy, cx, s_y[k], s_x[k]);
            acc = acc + probs[row * g.n_cls + cls];
            ++cnt;
          }
    }
    if constexpr (FINISH) {
      const float p = cnt > 0 ? acc / (float)cnt : 0.f;
      __syncthreads();   // the previous pass has read s_p
      s_p[threadIdx.x] = p;
      __syncthreads();
      if (live) {
        sum[addr] = p;
        if (cls == 0) {
          count[cidx] = cnt;
          float best = 0.f;
          const int bi = cnt > 0 ? first_max(s_p + threadIdx.x, g.n_cls, &best) : fill_class;
          map[cidx] = bi;
          conf[cidx] = cnt > 0 ? best : 0.f;
        }
      }
    } else if (live) {
      sum[addr] = acc;
      if (cls == 0) count[cidx] = cnt;
    }
  }
}

__global__ __launch_bounds__(256) void finish_mean_kernel(const float* sum, const int32_t* __restrict__ count, int64_t n_cells,
                                                          int n_cls, int fill_class, float* proba, int64_t* __restrict__ map,
                                                          float* __restrict__ conf) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t cnt = count[i];
    const float* s = sum + i * n_cls;   // may be the same memory as p: every element is read before it is written
    float* p = proba + i * n_cls;
    if (cnt > 0) {
      const float k = (float)cnt;
      for (int c = 0; c < n_cls; ++c) p[c] = s[c] / k;
      float best;
      map[i] = first_max(p, n_cls, &best);
      conf[i] = best;
    } else {
      for (int c = 0; c < n_cls; ++c) p[c] = 0.f;
      map[i] = fill_class;
      conf[i] = 0.f;
    }
  }
}

__global__ __launch_bounds__(256) void heatmap_kernel(const uint8_t* __restrict__ img, const float* __restrict__ field,
                                                      int64_t field_stride, int64_t n_cells, double r, double gr, double b,
                                                      double alpha, uint8_t* __restrict__ out) {
  const double beta = 1.0 - alpha;   // NumPy evaluates (1 - alpha) in float64 first
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += (int64_t)gridDim.x * blockDim.x) {
    const double f = (double)field[i * field_stride];
    out[3 * i] = (uint8_t)((double)img[3 * i] * alpha + (f * r) * beta);   // values are in [0, 255]: the cast truncates
    out[3 * i + 1] = (uint8_t)((double)img[3 * i + 1] * alpha + (f * gr) * beta);
    out[3 * i + 2] = (uint8_t)((double)img[3 * i + 2] * alpha + (f * b) * beta);
  }
}

inline unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 256 * 16); }
}  // namespace

extern "C" int dh_softmax_rows(const float* logits, int64_t n, int32_t n_cls, float* probs, void* stream) {
  DH_REQUIRE(n >= 0, "softmax rows: n=%lld is negative", (long long)n);
  DH_REQUIRE(n_cls > 0 && n_cls <= MAX_CLS, "softmax rows: n_cls=%d outside [1, %d]", n_cls, MAX_CLS);
  if (n == 0) return DH_OK;
  DH_REQUIRE(logits && probs, "softmax rows: null pointer (logits, probs)");
  hipLaunchKernelGGL(softmax_rows_kernel, dim3(grid_for(n)), dim3(256), 0, dh::as_stream(stream), logits, n, n_cls, probs);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_finish_mean(const float* sum, const int32_t* count, int64_t n_cells, int32_t n_cls, int32_t fill_class,
                              float* proba, int64_t* map, float* conf, void* stream) {
  DH_REQUIRE(n_cells >= 0, "finish mean: n_cells=%lld is negative", (long long)n_cells);
  DH_REQUIRE(n_cls > 0 && n_cls <= MAX_CLS, "finish mean: n_cls=%d outside [1, %d]", n_cls, MAX_CLS);
  if (n_cells == 0) return DH_OK;
  DH_REQUIRE(sum && count && proba && map && conf, "finish mean: null pointer (sum, count, proba, map, confidence)");
  hipLaunchKernelGGL(finish_mean_kernel, dim3(grid_for(n_cells)), dim3(256), 0, dh::as_stream(stream), sum, count, n_cells,
                     n_cls, fill_class, proba, map, conf);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

namespace {
// both ordered mean accumulations: one row per tile (dh_accumulate_mean), or S x S rows per tile (CAM: dh_accumulate_cam_mean)
template <bool CAM>
int accumulate_mean(const float* probs, const int32_t* yx_host, int64_t n, int32_t P, int32_t d, int32_t n_cls, int64_t h, int64_t w,
                    float* sum, int32_t* count, int64_t* map, float* conf, int32_t fill_class, void* stream) {
  DH_REQUIRE(n >= 0 && n <= INT32_MAX / 8, "accumulate mean: n=%lld outside [0, %d]", (long long)n, INT32_MAX / 8);
  DH_REQUIRE(n_cls > 0 && n_cls <= MAX_CLS, "accumulate mean: n_cls=%d outside [1, %d]", n_cls, MAX_CLS);
  DH_REQUIRE(P > 0 && d > 0, "accumulate mean: patch=%d and downscale=%d must be > 0", P, d);
  DH_REQUIRE(h > 0 && w > 0, "accumulate mean: h=%lld, w=%lld must be > 0", (long long)h, (long long)w);
  DH_REQUIRE(sum && count, "accumulate mean: null pointer (sum, count)");
  DH_REQUIRE((map == nullptr) == (conf == nullptr), "accumulate mean: map and confidence go together (both or neither)");
  DH_REQUIRE(n == 0 || (probs && yx_host), "accumulate mean: null pointer (probs, yx_host)");
  const int64_t dh_ = h / d, dw_ = w / d;
  if (dh_ == 0 || dw_ == 0) return DH_OK;
  DH_REQUIRE(dh_ * dw_ <= (int64_t)INT32_MAX, "accumulate mean: canvas of %lld x %lld cells is too large", (long long)dh_, (long long)dw_);
  hipStream_t st = dh::as_stream(stream);
  dh::BinPlan plan{};
  if (n > 0)
    if (const int rc = dh::bin_plan(yx_host, n, P, d, h, w, st, &plan)) return rc;
  if (plan.total == 0)   // no tile touches the canvas: the state stays as it is
    return map ? dh_finish_mean(sum, count, dh_ * dw_, n_cls, fill_class, sum, map, conf, stream) : DH_OK;
  const BinGeom g{plan.G, plan.bins_x, (int32_t)dh_, (int32_t)dw_, n_cls, P, d};
  if (map)
    hipLaunchKernelGGL((accumulate_mean_kernel<true, CAM>), dim3((unsigned)plan.nbins), dim3(256), 0, st, probs, plan.d_yx, plan.d_start,
                       plan.d_tiles, g, sum, count, map, conf, fill_class);
  else
    hipLaunchKernelGGL((accumulate_mean_kernel<false, CAM>), dim3((unsigned)plan.nbins), dim3(256), 0, st, probs, plan.d_yx, plan.d_start,
                       plan.d_tiles, g, sum, count, map, conf, fill_class);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
}  // namespace

extern "C" int dh_accumulate_mean(const float* probs, const int32_t* yx_host, int64_t n, int32_t P, int32_t d, int32_t n_cls,
                                  int64_t h, int64_t w, float* sum, int32_t* count, int64_t* map, float* conf,
                                  int32_t fill_class, void* stream) {
  return accumulate_mean<false>(probs, yx_host, n, P, d, n_cls, h, w, sum, count, map, conf, fill_class, stream);
}

extern "C" int dh_accumulate_cam_mean(const float* probs, const int32_t* yx_host, int64_t n, int32_t P, int32_t d, int32_t n_cls,
                                      int64_t h, int64_t w, float* sum, int32_t* count, int64_t* map, float* conf,
                                      int32_t fill_class, void* stream) {
  DH_REQUIRE(P > 0 && P % 32 == 0, "accumulate cam mean: patch %d is not a positive multiple of 32", P);
  DH_REQUIRE(h <= dh::CAM_MAX_SIDE && w <= dh::CAM_MAX_SIDE, "accumulate cam mean: h=%lld, w=%lld above %lld", (long long)h,
             (long long)w, (long long)dh::CAM_MAX_SIDE);
  return accumulate_mean<true>(probs, yx_host, n, P, d, n_cls, h, w, sum, count, map, conf, fill_class, stream);
}

extern "C" int dh_heatmap_blend(const uint8_t* img, const float* field, int64_t field_stride, int64_t n_cells,
                                const uint8_t* color, double alpha, uint8_t* out, void* stream) {
  DH_REQUIRE(n_cells >= 0, "heatmap blend: n_cells=%lld is negative", (long long)n_cells);
  DH_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "heatmap blend: alpha=%g outside [0, 1]", alpha);
  DH_REQUIRE(field_stride >= 1, "heatmap blend: field_stride=%lld must be >= 1", (long long)field_stride);
  DH_REQUIRE(color, "heatmap blend: null pointer (color)");
  if (n_cells == 0) return DH_OK;
  DH_REQUIRE(img && field && out, "heatmap blend: null pointer (img, field, out)");
  hipLaunchKernelGGL(heatmap_kernel, dim3(grid_for(n_cells)), dim3(256), 0, dh::as_stream(stream), img, field, field_stride,
                     n_cells, (double)color[0], (double)color[1], (double)color[2], alpha, out);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
