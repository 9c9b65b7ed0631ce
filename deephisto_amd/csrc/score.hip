// Scoring a whole-slide class map against its polygon annotation for MI355X (gfx950, wave64):
//   dh_rasterize_regions  polygons -> int32 label map on the prediction's canvas (even-odd rule at the cell centres, float64)
//   dh_confusion_matrix   truth x prediction counts (+ the "no prediction" column) and the per-cell outcome map, one pass
// The rasteriser cuts the canvas into bins of 32 x 32 cells, one workgroup per bin (one writer per cell, no atomics on
// the result); the host lists, per bin, the rings whose bounding box reaches it, in the manner of dh::bin_plan.  A ring's edges
// pass through LDS once per bin; the x-intercept of an edge depends on the map ROW only, so it is computed once per
// (edge, row) that straddles and turned into "the first k cells of this row lie left of it" with exact comparisons.
// Every float64 operation is the one of the NumPy restatement, in its order (-ffp-contract=off): results are bit-identical.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dh_common.h"

namespace {
constexpr int MAX_CLS = 64;   // as accumulate.hip
constexpr int RG = 32;        // bin side in cells: one uint32 of inside bits per row
constexpr int CH = 512;       // edges of a ring per LDS stage
constexpr double MAX_COORD = 1e15;

// Thread t owns row t / 8 of the bin and its cells 4 * (t % 8) .. + 3; the 8 threads of a row share the ring's edges.
// state per cell: -1 no class yet, c >= 0 exactly class c so far, -2 two different classes (final: -1).
__global__ __launch_bounds__(256) void rasterize_kernel(const double2* __restrict__ xy, const int32_t* __restrict__ ring_start,
                                                        const int32_t* __restrict__ ring_class, const double2* __restrict__ ring_y,
                                                        const int32_t* __restrict__ bin_start, const int32_t* __restrict__ bin_rings,
                                                        int bins_x, int dh_, int dw_, double d, int32_t* __restrict__ labels) {
  __shared__ double s_x[CH + 1], s_y[CH + 1];
  __shared__ unsigned int s_mask[RG];
  const int tid = threadIdx.x, row = tid >> 3, sub = tid & 7;
  const int bin = blockIdx.x, by = bin / bins_x, bx = bin - by * bins_x;
  const int cy = by * RG + row, cx0 = bx * RG;
  const int ncol = min(RG, dw_ - cx0);
  const double py = ((double)cy + 0.5) * d;
  int state[4] = {-1, -1, -1, -1};
  const int beg = bin_start ? bin_start[bin] : 0, end = bin_start ? bin_start[bin + 1] : 0;   // uniform for the block
  if (tid < RG) s_mask[tid] = 0u;
  for (int l = beg; l < end; ++l) {
    const int r = bin_rings[l];
    const int v0 = ring_start[r], nv = ring_start[r + 1] - v0, cls = ring_class[r];
    const double2 yb = ring_y[r];   // (min y, max y): an edge can straddle py only if min y <= py < max y
    const bool row_live = cy < dh_ && yb.x <= py && py < yb.y;
    for (int e0 = 0; e0 < nv; e0 += CH) {
      const int m = min(CH, nv - e0);
      __syncthreads();   // the previous stage has been read; the cleared masks are visible
      for (int i = tid; i <= m; i += 256) {
        int j = e0 + i;
        if (j == nv) j = 0;   // the closing edge
        const double2 v = xy[v0 + j];
        s_x[i] = v.x;
        s_y[i] = v.y;
      }
      __syncthreads();
      if (row_live)
        for (int i = sub; i < m; i += 8) {
          const double ay = s_y[i], by_ = s_y[i + 1];
          if ((ay > py) != (by_ > py)) {
            const double ax = s_x[i], bx_ = s_x[i + 1];
            const double xi = ax + (py - ay) * (bx_ - ax) / (by_ - ay);
            int lo = 0, hi = ncol;   // k = number of cells of the row with p.x < xi (p.x grows with the column)
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (((double)(cx0 + mid) + 0.5) * d < xi) lo = mid + 1; else hi = mid;
            }
            if (lo > 0) atomicXor(&s_mask[row], lo >= 32 ? 0xffffffffu : ((1u << lo) - 1u));   // integer, order-free
          }
        }
    }
    __syncthreads();
    const unsigned int mk = s_mask[row] >> (4 * sub);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((mk >> j) & 1u) state[j] = (state[j] == -1 || state[j] == cls) ? cls : -2;
    __syncthreads();
    if (tid < RG) s_mask[tid] = 0u;
  }
  if (cy < dh_) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int cx = cx0 + 4 * sub + j;
      if (cx < dw_) labels[(int64_t)cy * dw_ + cx] = state[j] >= 0 ? state[j] : -1;
    }
  }
}

// counts: [n_cls][n_cls + 1] then one word that counts predictions outside [-1, n_cls).  A thread takes 8 consecutive cells and
// merges runs of one (truth, prediction) pair before it touches the workgroup's LDS histogram: class maps are made of patches.
constexpr int CELLS_PER_THREAD = 8;
__global__ __launch_bounds__(256) void confusion_kernel(const int64_t* __restrict__ pred, const int32_t* __restrict__ truth,
                                                        int64_t n_cells, int n_cls, unsigned long long* __restrict__ counts,
                                                        int64_t* __restrict__ outcome) {
  __shared__ unsigned int s_hist[MAX_CLS * (MAX_CLS + 1) + 1];
  const int n_hist = n_cls * (n_cls + 1) + 1;
  for (int i = threadIdx.x; i < n_hist; i += 256) s_hist[i] = 0u;
  __syncthreads();
  const int64_t chunk = (int64_t)256 * CELLS_PER_THREAD;
  for (int64_t c0 = (int64_t)blockIdx.x * chunk; c0 < n_cells; c0 += (int64_t)gridDim.x * chunk) {
    const int64_t i0 = c0 + (int64_t)threadIdx.x * CELLS_PER_THREAD;
    int key = -1;
    unsigned int run = 0u;
    for (int k = 0; k < CELLS_PER_THREAD; ++k) {
      const int64_t i = i0 + k;
      if (i >= n_cells) break;
      const int32_t t = truth[i];
      const int64_t p = pred[i];
      int kk = -1;
      int64_t oc = -1;
      if (p < -1 || p >= n_cls) { kk = n_hist - 1; oc = t >= 0 && t < n_cls ? 1 : -1; }   // refused by the entry
      else if (t >= 0 && t < n_cls) { kk = t * (n_cls + 1) + (p < 0 ? n_cls : (int)p); oc = p == t ? 0 : 1; }
      if (outcome) outcome[i] = oc;
      if (kk != key) {
        if (run) atomicAdd(&s_hist[key], run);
        key = kk;
        run = 0u;
      }
      if (kk >= 0) ++run;
    }
    if (run) atomicAdd(&s_hist[key], run);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_hist; i += 256)
    if (s_hist[i]) atomicAdd(&counts[i], (unsigned long long)s_hist[i]);
}

// The rasteriser's plan: ring data and per-bin ring lists on the device, kept for the next call with the same arguments
// (thread and device local, like dh::bin_plan).
struct RasterPlan {
  std::vector<double> xy; std::vector<int64_t> start; std::vector<int32_t> cls;
  int64_t dh = 0, dw = 0, total = 0; int32_t d = 0; int device = -1; int bins_x = 0; int64_t nbins = 0;
  double2 *d_xy = nullptr, *d_ring_y = nullptr; int32_t *d_ring_start = nullptr, *d_ring_class = nullptr, *d_bin_start = nullptr,
          *d_bin_rings = nullptr;
};

// [lo, hi) of the cells c in [0, n) whose centre (c + 0.5) * d satisfies a <= centre (lo) and centre < b resp. <= b (hi):
// an estimate from the division, then exact comparisons.
inline int64_t first_centre_at_least(double a, double d, int64_t n) {
  double e = floor(a / d - 0.5) - 2.0;
  int64_t c = e < 0.0 ? 0 : (e > (double)n ? n : (int64_t)e);
  while (c < n && ((double)c + 0.5) * d < a) ++c;
  return c;
}
inline int64_t first_centre_above(double b, double d, int64_t n) {
  double e = floor(b / d - 0.5) - 2.0;
  int64_t c = e < 0.0 ? 0 : (e > (double)n ? n : (int64_t)e);
  while (c < n && ((double)c + 0.5) * d <= b) ++c;
  return c;
}

int raster_plan(const double* xy, const int64_t* ring_start, const int32_t* ring_class, int64_t n_rings, int64_t dh_, int64_t dw_,
                int32_t d, hipStream_t st, RasterPlan** out) {
  static thread_local RasterPlan plan;
  int dev_id = 0;
  DH_HIP(hipGetDevice(&dev_id));
  const int64_t nv = ring_start[n_rings];
  const bool hit = plan.device == dev_id && plan.dh == dh_ && plan.dw == dw_ && plan.d == d &&
                   (int64_t)plan.cls.size() == n_rings && (int64_t)plan.xy.size() == 2 * nv &&
                   memcmp(plan.start.data(), ring_start, (size_t)(n_rings + 1) * 8) == 0 &&
                   memcmp(plan.cls.data(), ring_class, (size_t)n_rings * 4) == 0 &&
                   memcmp(plan.xy.data(), xy, (size_t)nv * 16) == 0;
  if (!hit) {
    const double dd = (double)d;
    const int64_t bins_y = (dh_ + RG - 1) / RG, bins_x = (dw_ + RG - 1) / RG, nbins = bins_y * bins_x;
    DH_REQUIRE(nbins < INT32_MAX, "rasterize regions: too many bins");
    std::vector<double> ring_y((size_t)n_rings * 2);
    std::vector<int32_t> start32((size_t)n_rings + 1), box((size_t)n_rings * 4), bstart((size_t)nbins + 1, 0);
    int64_t total = 0;
    for (int64_t r = 0; r < n_rings; ++r) {
      start32[r] = (int32_t)ring_start[r];
      double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
      for (int64_t v = ring_start[r]; v < ring_start[r + 1]; ++v) {
        x0 = std::min(x0, xy[2 * v]); x1 = std::max(x1, xy[2 * v]);
        y0 = std::min(y0, xy[2 * v + 1]); y1 = std::max(y1, xy[2 * v + 1]);
      }
      ring_y[2 * r] = y0; ring_y[2 * r + 1] = y1;
      // rows: min y <= p.y < max y, exact.  columns: a computed intercept lies within a few ulp of [min x, max x]; the margin
      // is far wider than that.  Left of all of them no edge counts, right of all of them an even number does: no change.
      const double mx = 1e-6 * (1.0 + std::max(fabs(x0), fabs(x1)));
      const int64_t cy0 = first_centre_at_least(y0, dd, dh_), cy1 = first_centre_at_least(y1, dd, dh_);
      const int64_t cx0 = first_centre_at_least(x0 - mx, dd, dw_), cx1 = first_centre_above(x1 + mx, dd, dw_);
      const bool any = cy1 > cy0 && cx1 > cx0;
      box[4 * r] = any ? (int32_t)(cy0 / RG) : 0; box[4 * r + 1] = any ? (int32_t)((cy1 - 1) / RG) : -1;
      box[4 * r + 2] = any ? (int32_t)(cx0 / RG) : 0; box[4 * r + 3] = any ? (int32_t)((cx1 - 1) / RG) : -1;
      for (int64_t b = box[4 * r]; b <= box[4 * r + 1]; ++b)
        for (int64_t c = box[4 * r + 2]; c <= box[4 * r + 3]; ++c) { ++bstart[b * bins_x + c + 1]; ++total; }
    }
    start32[n_rings] = (int32_t)nv;
    DH_REQUIRE(total < INT32_MAX, "rasterize regions: ring lists too long");
    for (int64_t b = 0; b < nbins; ++b) bstart[b + 1] += bstart[b];
    std::vector<int32_t> fill(bstart.begin(), bstart.end() - 1), rings((size_t)std::max<int64_t>(total, 1));
    for (int64_t r = 0; r < n_rings; ++r)
      for (int64_t b = box[4 * r]; b <= box[4 * r + 1]; ++b)
        for (int64_t c = box[4 * r + 2]; c <= box[4 * r + 3]; ++c) rings[fill[b * bins_x + c]++] = (int32_t)r;
    DH_HIP(hipStreamSynchronize(st));   // the previous plan's buffers may still be in use on this stream
    if (plan.d_xy) {
      (void)hipFree(plan.d_xy); (void)hipFree(plan.d_ring_y); (void)hipFree(plan.d_ring_start); (void)hipFree(plan.d_ring_class);
      (void)hipFree(plan.d_bin_start); (void)hipFree(plan.d_bin_rings);
    }
    plan = RasterPlan();
    const size_t xb = (size_t)nv * 16, yb = (size_t)n_rings * 16, sb = (size_t)(n_rings + 1) * 4, cb = (size_t)n_rings * 4,
                 bb = (size_t)(nbins + 1) * 4, rb = rings.size() * 4;
    DH_HIP(hipMalloc((void**)&plan.d_xy, xb));
    DH_HIP(hipMalloc((void**)&plan.d_ring_y, yb));
    DH_HIP(hipMalloc((void**)&plan.d_ring_start, sb));
    DH_HIP(hipMalloc((void**)&plan.d_ring_class, cb));
    DH_HIP(hipMalloc((void**)&plan.d_bin_start, bb));
    DH_HIP(hipMalloc((void**)&plan.d_bin_rings, rb));
    DH_HIP(hipMemcpy(plan.d_xy, xy, xb, hipMemcpyHostToDevice));
    DH_HIP(hipMemcpy(plan.d_ring_y, ring_y.data(), yb, hipMemcpyHostToDevice));
    DH_HIP(hipMemcpy(plan.d_ring_start, start32.data(), sb, hipMemcpyHostToDevice));
    DH_HIP(hipMemcpy(plan.d_ring_class, ring_class, cb, hipMemcpyHostToDevice));
    DH_HIP(hipMemcpy(plan.d_bin_start, bstart.data(), bb, hipMemcpyHostToDevice));
    DH_HIP(hipMemcpy(plan.d_bin_rings, rings.data(), rb, hipMemcpyHostToDevice));
    plan.xy.assign(xy, xy + 2 * nv);
    plan.start.assign(ring_start, ring_start + n_rings + 1);
    plan.cls.assign(ring_class, ring_class + n_rings);
    plan.dh = dh_; plan.dw = dw_; plan.d = d; plan.total = total; plan.bins_x = (int)bins_x; plan.nbins = nbins;
    plan.device = dev_id;
  }
  *out = &plan;
  return DH_OK;
}
}  // namespace

extern "C" int dh_rasterize_regions(const double* xy_host, const int64_t* ring_start_host, const int32_t* ring_class_host,
                                    int64_t n_rings, int32_t n_cls, int64_t dh_, int64_t dw_, int32_t d, int32_t* labels,
                                    void* stream) {
  DH_REQUIRE(n_rings >= 0 && n_rings <= INT32_MAX / 8, "rasterize regions: n_rings=%lld outside [0, %d]", (long long)n_rings,
             INT32_MAX / 8);
  DH_REQUIRE(n_cls > 0 && n_cls <= MAX_CLS, "rasterize regions: n_cls=%d outside [1, %d]", n_cls, MAX_CLS);
  DH_REQUIRE(dh_ > 0 && dw_ > 0, "rasterize regions: dh=%lld, dw=%lld must be > 0", (long long)dh_, (long long)dw_);
  DH_REQUIRE(d > 0, "rasterize regions: downscale=%d must be > 0", d);
  DH_REQUIRE(dh_ * dw_ <= (int64_t)INT32_MAX, "rasterize regions: canvas of %lld x %lld cells is too large", (long long)dh_,
             (long long)dw_);
  DH_REQUIRE(labels, "rasterize regions: null pointer (labels)");
  DH_REQUIRE(n_rings == 0 || (xy_host && ring_start_host && ring_class_host),
             "rasterize regions: null pointer (xy, ring_start, ring_class)");
  if (n_rings > 0) {
    DH_REQUIRE(ring_start_host[0] == 0, "rasterize regions: ring_start[0]=%lld must be 0", (long long)ring_start_host[0]);
    for (int64_t r = 0; r < n_rings; ++r) {
      const int64_t nv = ring_start_host[r + 1] - ring_start_host[r];
      DH_REQUIRE(nv >= 3, "rasterize regions: ring %lld has %lld vertices (a ring needs 3)", (long long)r, (long long)nv);
      DH_REQUIRE(ring_start_host[r + 1] <= INT32_MAX / 2, "rasterize regions: more than %d vertices", INT32_MAX / 2);
      DH_REQUIRE(ring_class_host[r] >= 0 && ring_class_host[r] < n_cls, "rasterize regions: ring %lld has class id %d outside [0, %d)",
                 (long long)r, ring_class_host[r], n_cls);
    }
    for (int64_t i = 0, n = 2 * ring_start_host[n_rings]; i < n; ++i)
      DH_REQUIRE(fabs(xy_host[i]) <= MAX_COORD, "rasterize regions: coordinate %lld (%g) is not finite or beyond 1e15", (long long)i,
                 xy_host[i]);   // NaN fails the comparison too
  }
  hipStream_t st = dh::as_stream(stream);
  const int64_t bins_x = (dw_ + RG - 1) / RG, nbins = ((dh_ + RG - 1) / RG) * bins_x;
  if (n_rings == 0) {   // every bin is empty: all -1
    hipLaunchKernelGGL(rasterize_kernel, dim3((unsigned)nbins), dim3(256), 0, st, nullptr, nullptr, nullptr, nullptr, nullptr,
                       nullptr, (int)bins_x, (int)dh_, (int)dw_, (double)d, labels);
    DH_LAUNCH_CHECK();
    return DH_OK;
  }
  RasterPlan* plan = nullptr;
  if (const int rc = raster_plan(xy_host, ring_start_host, ring_class_host, n_rings, dh_, dw_, d, st, &plan)) return rc;
  hipLaunchKernelGGL(rasterize_kernel, dim3((unsigned)plan->nbins), dim3(256), 0, st, plan->d_xy, plan->d_ring_start,
                     plan->d_ring_class, plan->d_ring_y, plan->d_bin_start, plan->d_bin_rings, plan->bins_x, (int)dh_, (int)dw_,
                     (double)d, labels);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_confusion_matrix(const int64_t* pred, const int32_t* truth, int64_t n_cells, int32_t n_cls, int64_t* counts_host,
                                   int64_t* outcome, void* stream) {
  DH_REQUIRE(n_cells >= 0 && n_cells <= ((int64_t)1 << 40), "confusion matrix: n_cells=%lld outside [0, 2^40]", (long long)n_cells);
  DH_REQUIRE(n_cls > 0 && n_cls <= MAX_CLS, "confusion matrix: n_cls=%d outside [1, %d]", n_cls, MAX_CLS);
  DH_REQUIRE(counts_host, "confusion matrix: null pointer (counts)");
  const int n_hist = n_cls * (n_cls + 1);
  memset(counts_host, 0, (size_t)n_hist * 8);
  if (n_cells == 0) return DH_OK;
  DH_REQUIRE(pred && truth, "confusion matrix: null pointer (pred, truth)");
  struct Scratch { unsigned long long* d = nullptr; int device = -1; };
  static thread_local Scratch sc;   // the device histogram + the refusal word
  int dev_id = 0;
  DH_HIP(hipGetDevice(&dev_id));
  if (sc.device != dev_id) {
    sc = Scratch();
    DH_HIP(hipMalloc((void**)&sc.d, (size_t)(MAX_CLS * (MAX_CLS + 1) + 1) * 8));
    sc.device = dev_id;
  }
  hipStream_t st = dh::as_stream(stream);
  DH_HIP(hipMemsetAsync(sc.d, 0, (size_t)(n_hist + 1) * 8, st));
  const int64_t chunk = 256 * CELLS_PER_THREAD;
  const unsigned grid = (unsigned)std::min<int64_t>((n_cells + chunk - 1) / chunk, 256 * 8);
  hipLaunchKernelGGL(confusion_kernel, dim3(grid), dim3(256), 0, st, pred, truth, n_cells, n_cls, sc.d, outcome);
  DH_LAUNCH_CHECK();
  std::vector<int64_t> host((size_t)n_hist + 1);
  DH_HIP(hipMemcpyAsync(host.data(), sc.d, host.size() * 8, hipMemcpyDeviceToHost, st));
  DH_HIP(hipStreamSynchronize(st));   // the status depends on the data
  DH_REQUIRE(host[n_hist] == 0, "confusion matrix: %lld predictions outside [-1, %d)", (long long)host[n_hist], n_cls);
  memcpy(counts_host, host.data(), (size_t)n_hist * 8);
  return DH_OK;
}
