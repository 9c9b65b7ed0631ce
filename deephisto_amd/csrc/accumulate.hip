// Everything that writes the whole-slide canvas, for MI355X (gfx950, wave64):
//   a8  dh_accumulate_logits    ordered (bit-exact) canvas accumulation, dh_argmax_map; dh_accumulate_cam: S x S rows per tile
//   dh_softmax_rows     per-tile softmax of the logits (expf, sums in class order)                  
//   dh_accumulate_mean  ordered per-cell sums of the tile probabilities + int32 hit counts, with the finish fused in on request
//   dh_accumulate_cam_mean  the same over S x S rows per tile, each on its own 32 x 32-pixel block
//   dh_finish_mean      proba = sum / count, first-maximum class, confidence; fill for cells nothing covers
// HBM-bound.  The four accumulations share one bin plan (one workgroup per G x G bin, one writer per cell, tile lists staged
// through LDS).  No atomics: every result is bit-identical to the NumPy loop.
#include <string.h>

#include <algorithm>
#include <vector>

#include "dh_common.h"

// ---------------------------------------------------------------------------
// a8: ordered accumulation.  The canvas is cut into bins of G x G cells
// (G = max(1, P/d)); the host builds, per bin, the list of tiles that touch it,
// in tile order.  One workgroup owns one bin, so every canvas cell has exactly
// one writer that applies the covering tiles' logits sequentially in the
// reference's order: float32 results are bit-identical to the NumPy `+=` loop,
// with no atomics.  Traffic: canvas read+write once, logits/lists from L2.
// ---------------------------------------------------------------------------
namespace dh {
// Bin plan of the ordered canvas accumulations.  The canvas is cut into bins of G x G cells,
// G = max(1, min(P/d, 64)); bin b's covering tiles, in list order, are d_tiles[d_start[b] .. d_start[b+1]).  bin_plan builds the
// plan of (yx_host, P, d, h, w), or returns the cached one when the last call on this thread and device had the same arguments
// (no rebuild, no upload, no synchronisation).  The device arrays stay valid until the next call that misses the cache, which
// synchronises `st` before it frees them.
struct BinPlan { int32_t G, bins_x; int64_t nbins, total; const int32_t *d_start, *d_tiles, *d_yx; };
struct BinGeom { int32_t G, bins_x, dh, dw, n_cls, P, d; };

// Row of a class activation map (float32 [n][S * S][n_cls], S = P / 32) that tile t at origin (y, x) contributes to canvas cell
// (cy, cx), a cell the tile covers: position i = ceil(((cy + 1) d - y) / 32) - 1 along y and j likewise along x, the one position
// whose 32-pixel sub-tile owns the cell.  (cy + 1) d <= h, so 32-bit arithmetic holds up to CAM_MAX_SIDE.
constexpr int64_t CAM_MAX_SIDE = INT32_MAX - 64;
__host__ __device__ inline int64_t cam_row(int64_t t, int S, int d, int cy, int cx, int y, int x) {
  const int i = ((cy + 1) * d - y + 31) / 32 - 1, j = ((cx + 1) * d - x + 31) / 32 - 1;
  return (t * S + i) * S + j;
}

// The bin lists depend only on (origins, P, d, h, w): whole-slide prediction repeats the same
// grid slide after slide, so the last plan (host CSR + its device copies) is kept and reused
// when the origins compare equal -- no rebuild, no upload, no stream synchronisation.  Shared by
// every ordered accumulation (dh_accumulate_logits, dh_accumulate_mean): the class map and the
// probabilities of one slide are built from one plan.
int bin_plan(const int32_t* yx_host, int64_t n, int32_t P, int32_t d, int64_t h, int64_t w, hipStream_t st, BinPlan* out) {
  struct Plan {
    std::vector<int32_t> yx; int32_t P = 0, d = 0; int64_t h = 0, w = 0, nbins = 0, total = 0; int G = 0, bins_x = 0;
    int32_t *d_start = nullptr, *d_tiles = nullptr, *d_yx = nullptr; int device = -1;
  };
  static thread_local Plan plan;
  const int64_t dh_ = h / d, dw_ = w / d;
  int dev_id = 0;
  DH_HIP(hipGetDevice(&dev_id));
  const bool hit = plan.device == dev_id && plan.P == P && plan.d == d && plan.h == h && plan.w == w &&
                   (int64_t)plan.yx.size() == 2 * n && memcmp(plan.yx.data(), yx_host, (size_t)n * 8) == 0;
  if (!hit) {
    const int G = std::max(1, std::min(P / d, 64));
    const int64_t bins_y = (dh_ + G - 1) / G, bins_x = (dw_ + G - 1) / G;
    const int64_t nbins = bins_y * bins_x;
    DH_REQUIRE(nbins < INT32_MAX, "accumulate: too many bins");
    std::vector<int32_t> start(nbins + 1, 0);
    auto span = [&](int64_t i, int64_t& cy0, int64_t& cy1, int64_t& cx0, int64_t& cx1) {
      const int64_t y = yx_host[2 * i], x = yx_host[2 * i + 1];
      cy0 = std::max<int64_t>(y / d, 0); cy1 = std::min<int64_t>((y + P) / d, dh_);
      cx0 = std::max<int64_t>(x / d, 0); cx1 = std::min<int64_t>((x + P) / d, dw_);
      return y >= 0 && x >= 0 && cy1 > cy0 && cx1 > cx0;
    };
    int64_t total = 0;
    for (int64_t i = 0; i < n; ++i) {
      int64_t a, b, c, e;
      DH_REQUIRE(yx_host[2 * i] >= 0 && yx_host[2 * i + 1] >= 0, "accumulate: negative origin");
      if (!span(i, a, b, c, e)) continue;
      for (int64_t by = a / G; by <= (b - 1) / G; ++by)
        for (int64_t bx = c / G; bx <= (e - 1) / G; ++bx) { ++start[by * bins_x + bx + 1]; ++total; }
    }
    DH_REQUIRE(total < INT32_MAX, "accumulate: incidence list too long");
    for (int64_t b = 0; b < nbins; ++b) start[b + 1] += start[b];
    std::vector<int32_t> fill(start.begin(), start.end() - 1), tiles((size_t)std::max<int64_t>(total, 1));
    for (int64_t i = 0; i < n; ++i) {
      int64_t a, b, c, e;
      if (!span(i, a, b, c, e)) continue;
      for (int64_t by = a / G; by <= (b - 1) / G; ++by)
        for (int64_t bx = c / G; bx <= (e - 1) / G; ++bx) tiles[fill[by * bins_x + bx]++] = (int32_t)i;
    }
    DH_HIP(hipStreamSynchronize(st));  // the previous plan's buffers may still be in use on this stream
    if (plan.d_start) { (void)hipFree(plan.d_start); (void)hipFree(plan.d_tiles); (void)hipFree(plan.d_yx); }
    plan = Plan();
    const size_t sb = (size_t)(nbins + 1) * 4, tb = (size_t)std::max<int64_t>(total, 1) * 4, yb = (size_t)n * 8;
    DH_HIP(hipMalloc((void**)&plan.d_start, sb));
    DH_HIP(hipMalloc((void**)&plan.d_tiles, tb));
    DH_HIP(hipMalloc((void**)&plan.d_yx, yb));
    DH_HIP(hipMemcpy(plan.d_start, start.data(), sb, hipMemcpyHostToDevice));
    DH_HIP(hipMemcpy(plan.d_tiles, tiles.data(), tb, hipMemcpyHostToDevice));
    DH_HIP(hipMemcpy(plan.d_yx, yx_host, yb, hipMemcpyHostToDevice));
    plan.yx.assign(yx_host, yx_host + 2 * n);
    plan.P = P; plan.d = d; plan.h = h; plan.w = w; plan.nbins = nbins; plan.total = total; plan.G = G;
    plan.bins_x = (int)bins_x; plan.device = dev_id;
  }
  *out = BinPlan{plan.G, (int32_t)plan.bins_x, plan.nbins, plan.total, plan.d_start, plan.d_tiles, plan.d_yx};
  return DH_OK;
}
}  // namespace dh

using dh::BinGeom;

// CAM (dh_accumulate_cam): `logits` holds S x S rows per tile, S = P / 32, one per 32 x 32-pixel position,
// and a covered cell takes the row of the one position whose 32-pixel sub-tile owns it -- position i = ceil(((cy + 1) d - y) / 32) - 1
// along y, likewise along x: the sub-tiles' cell ranges partition the tile's.  Same plan, same bins, same order of additions.
// The walk over the bin's list (stage 256 tiles, barrier, add the covering ones in list order) is spelled out here and again in
// accumulate_mean_kernel: with both kernels over one shared walk, dh_accumulate_logits at 224 / 112 measured 1.8 % slower than the
// parent, past the same code's own spread (profiles/tile_split_ab.json), and argmax_kernel keeps its own loop for the same reason.
template <bool CAM>
__global__ __launch_bounds__(256) void accumulate_bins_kernel(
    const float* __restrict__ logits, const int32_t* __restrict__ yx,
    const int32_t* __restrict__ bin_start, const int32_t* __restrict__ bin_tiles, BinGeom g,
    float* __restrict__ canvas) {
  __shared__ int32_t s_t[256], s_y0[256], s_y1[256], s_x0[256], s_x1[256];
  __shared__ int32_t s_y[CAM ? 256 : 1], s_x[CAM ? 256 : 1];
  const int S = g.P >> 5;
  const int bin = blockIdx.x;
  const int beg = bin_start[bin], end = bin_start[bin + 1];
  if (beg == end) return;  // uniform for the block
  const int by = bin / g.bins_x, bx = bin - by * g.bins_x;
  const int cells = g.G * g.G, items = cells * g.n_cls;
  for (int it0 = 0; it0 < items; it0 += 256) {
    const int it = it0 + threadIdx.x;
    const int cell = it / g.n_cls, cls = it - cell * g.n_cls;
    const int cy = by * g.G + cell / g.G, cx = bx * g.G + cell % g.G;
    const bool live = it < items && cy < g.dh && cx < g.dw;
    const int64_t addr = ((int64_t)cy * g.dw + cx) * g.n_cls + cls;
    float acc = live ? canvas[addr] : 0.f;
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
            acc = acc + logits[row * g.n_cls + cls];
          }
    }
    if (live) canvas[addr] = acc;
  }
}

__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ canvas, int64_t n_cells,
                                                     int n_cls, int64_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_cells;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float* p = canvas + i * n_cls;
    float best = p[0];
    int bi = 0;
    for (int c = 1; c < n_cls; ++c) {  // NumPy argmax: first maximum; a NaN wins once
      const float v = p[c];
      if (v > best || (v != v && best == best)) { best = v; bi = c; }
    }
    out[i] = bi;
  }
}

namespace {
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

inline unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 256 * 16); }
}  // namespace

extern "C" int dh_argmax_map(const float* canvas, int64_t n_cells, int32_t n_cls, int64_t* map,
                             void* stream) {
  DH_REQUIRE(canvas && map && n_cells >= 0 && n_cls > 0, "argmax map: bad arguments");
  if (n_cells == 0) return DH_OK;
  hipLaunchKernelGGL(argmax_kernel, dim3(grid_for(n_cells)), dim3(256), 0, dh::as_stream(stream), canvas, n_cells,
                     n_cls, map);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

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
// both ordered sum accumulations: one row per tile (dh_accumulate_logits), or S x S rows per tile (CAM: dh_accumulate_cam)
template <bool CAM>
int accumulate_sum(const float* rows, const int32_t* yx_host, int64_t n, int32_t P, int32_t d, int32_t n_cls, int64_t h, int64_t w,
                   float* canvas, int64_t* map, void* stream) {
  constexpr const char* who = CAM ? "accumulate cam" : "accumulate";
  DH_REQUIRE(rows && yx_host && canvas, "%s: null pointer", who);
  DH_REQUIRE(P > 0 && d > 0 && n_cls > 0 && h > 0 && w > 0 && n >= 0, "%s: bad sizes", who);
  DH_REQUIRE(n <= INT32_MAX / 8, "%s: too many tiles", who);
  const int64_t dh_ = h / d, dw_ = w / d;
  hipStream_t st = dh::as_stream(stream);
  if (dh_ == 0 || dw_ == 0) return DH_OK;
  DH_REQUIRE(dh_ * dw_ <= (int64_t)INT32_MAX, "%s: canvas too large", who);
  if (n > 0) {
    dh::BinPlan plan;
    if (const int rc = dh::bin_plan(yx_host, n, P, d, h, w, st, &plan)) return rc;
    if (plan.total > 0) {
      const BinGeom g{plan.G, plan.bins_x, (int32_t)dh_, (int32_t)dw_, n_cls, P, d};
      hipLaunchKernelGGL(accumulate_bins_kernel<CAM>, dim3((unsigned)plan.nbins), dim3(256), 0, st, rows, plan.d_yx, plan.d_start,
                         plan.d_tiles, g, canvas);
      DH_LAUNCH_CHECK();
    }
  }
  if (map) return dh_argmax_map(canvas, dh_ * dw_, n_cls, map, stream);
  return DH_OK;
}

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

extern "C" int dh_accumulate_logits(const float* logits, const int32_t* yx_host, int64_t n,
                                    int32_t P, int32_t d, int32_t n_cls, int64_t h, int64_t w,
                                    float* canvas, int64_t* map, void* stream) {
  return accumulate_sum<false>(logits, yx_host, n, P, d, n_cls, h, w, canvas, map, stream);
}

extern "C" int dh_accumulate_cam(const float* cam, const int32_t* yx_host, int64_t n, int32_t P, int32_t d, int32_t n_cls, int64_t h,
                                 int64_t w, float* canvas, int64_t* map, void* stream) {
  DH_REQUIRE(P > 0 && P % 32 == 0, "accumulate cam: patch %d is not a positive multiple of 32", P);
  DH_REQUIRE(h > 0 && w > 0 && h <= dh::CAM_MAX_SIDE && w <= dh::CAM_MAX_SIDE, "accumulate cam: h=%lld, w=%lld outside [1, %lld]",
             (long long)h, (long long)w, (long long)dh::CAM_MAX_SIDE);
  return accumulate_sum<true>(cam, yx_host, n, P, d, n_cls, h, w, canvas, map, stream);
}

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
