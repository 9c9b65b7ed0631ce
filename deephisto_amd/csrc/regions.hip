// Regions of a whole-slide class map for MI355X (gfx950, wave64):
//   dh_label_components     4-connected components of equal class -> int32 label map, ids 1..K in order of first cell
//   dh_region_stats         per component: class, area, bounding box, coordinate sums, first cell, quantised confidence sum
//   dh_clean_small_regions  one cleanup round: components below min_cells take the class most of their large neighbours have
// Labelling is union-find whose parent links always point to a SMALLER linear cell index:
//   cc_local_kernel    one workgroup per tile of 64 x 64 cells: the tile's classes in LDS, every cell linked to its left
//                      neighbour of the same class (a row run), runs of adjacent rows united with LDS atomicMin, then every
//                      cell's root written out as a global linear index (the smallest of its set within the tile)
//   cc_border_kernel   one thread per cell on a tile's top row or left column: united with the cell across the border
//   cc_flatten_kernel  every cell's link replaced by its root
//   cc_count_kernel, cc_scan_kernel, cc_number_kernel, cc_relabel_kernel
//                      roots (link == own index) counted per chunk of 2 048 cells, the chunk counts scanned by one workgroup
//                      (the block scans of tissue_select_kernel), roots numbered 1..K in index order, every cell given its
//                      root's number
// All atomics are integer atomics.  atomicMin only ever lowers a link to another member of the same set, so whatever order
// the atomics land in, a set's root is its smallest cell index and the partition is the one of the rule: label map, K and the
// table do not depend on the schedule.  Sums, minima and maxima of the table are integers too.  Indices are 32-bit inside a
// canvas (fewer than 2^31 cells, the other kernels' limit) and 64-bit wherever they are scaled into a byte offset.
#include <algorithm>

#include "dh_common.h"

namespace {

constexpr int MAX_CLS = 64;      // as accumulate.hip, score.hip
constexpr int kThreads = 256;
constexpr int TS = 64;           // tile side in cells
constexpr int kTileCells = TS * TS;
constexpr int kPer = 8;          // consecutive cells per thread in the streaming kernels
constexpr int kChunk = kThreads * kPer;
constexpr int64_t kMaxGrid = 256 * 8;
constexpr int kCols = 10;        // columns of the region table, see deephisto_hip.h
enum { C_CLASS, C_AREA, C_Y0, C_X0, C_Y1, C_X1, C_SUMY, C_SUMX, C_FIRST, C_CONF };

// ---- union-find on a link array whose entries only decrease ---------------------------------------------------------------
// The loads are relaxed agent-scope atomics: served by L2, where the atomicMin of other workgroups land, never by a stale L1 line.
// A stale link would still be a member of the same set; the loop ends on what atomicMin returns.
__device__ __forceinline__ int32_t g_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int32_t g_find(const int32_t* link, int32_t i) {
  int32_t p = g_load(link + i);
  while (p != i) { i = p; p = g_load(link + i); }
  return i;
}

__device__ void g_unite(int32_t* link, int32_t a, int32_t b) {
  for (;;) {
    a = g_find(link, a);
    b = g_find(link, b);
    if (a == b) return;
    if (a < b) { const int32_t t = a; a = b; b = t; }   // a > b: hang a below b
    const int32_t old = atomicMin(link + a, b);
    if (old == a) return;    // a was a root: done
    a = old;                 // somebody hung a elsewhere meanwhile; min(old, b) is stored, unite the other one with b
  }
}

__device__ __forceinline__ int l_find(volatile int* link, int i) {
  int p = link[i];
  while (p != i) { i = p; p = link[i]; }
  return i;
}

__device__ void l_unite(int* link, int a, int b) {
  for (;;) {
    a = l_find(link, a);
    b = l_find(link, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(link + a, b);
    if (old == a) return;
    a = old;
  }
}

// status[0]: cells whose class lies outside [-1, n_cls); status[1]: K; status[2]: changed cells of a cleanup round
// (four words per thread and device, allocated once, like the histogram of dh_confusion_matrix)
__global__ __launch_bounds__(kThreads) void cc_local_kernel(const int64_t* __restrict__ map, int dh_, int dw_, int n_cls, int tiles_x,
                                                            int32_t* __restrict__ link, int32_t* __restrict__ status) {
  __shared__ int8_t s_cls[kTileCells];
  __shared__ int s_link[kTileCells];
  const int ty0 = (blockIdx.x / tiles_x) * TS, tx0 = (blockIdx.x % tiles_x) * TS;
  int bad = 0;
  for (int i = threadIdx.x; i < kTileCells; i += kThreads) {   // a row of the tile is 64 consecutive int64: coalesced
    const int y = ty0 + (i >> 6), x = tx0 + (i & 63);
    int c = -1;
    if (y < dh_ && x < dw_) {
      const int64_t v = map[(int64_t)y * dw_ + x];
      if (v < -1 || v >= n_cls) ++bad; else c = (int)v;
    }
    s_cls[i] = (int8_t)c;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTileCells; i += kThreads)
    s_link[i] = ((i & 63) && s_cls[i] >= 0 && s_cls[i - 1] == s_cls[i]) ? i - 1 : i;   // row runs: a chain to the run's first cell
  __syncthreads();
  // the cell above has the same class: unite, unless the pair to the left is joined the same way (then this one follows from
  // the two row links and that pair's union)
  for (int i = threadIdx.x + TS; i < kTileCells; i += kThreads) {
    const int c = s_cls[i];
    if (c < 0 || s_cls[i - TS] != c) continue;
    if ((i & 63) && s_cls[i - 1] == c && s_cls[i - TS - 1] == c) continue;
    l_unite(s_link, i, i - TS);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTileCells; i += kThreads) {
    const int y = ty0 + (i >> 6), x = tx0 + (i & 63);
    if (y >= dh_ || x >= dw_) continue;
    int32_t out = -1;
    if (s_cls[i] >= 0) {
      const int r = l_find(s_link, i);
      out = (int32_t)((int64_t)(ty0 + (r >> 6)) * dw_ + tx0 + (r & 63));
    }
    link[(int64_t)y * dw_ + x] = out;
  }
  if (bad) atomicAdd(status, bad);
}

// item < tiles_y1 * dw: cell (64 * (1 + item / dw), item % dw) and the cell above it; the rest: cell (y, 64 * (1 + k)) and the
// cell left of it.  A pair whose four cells (with the pair to the left) are of one class is skipped as in the tile, but only
// for the vertical pairs: every horizontal pair is united, so the argument does not run in a circle.
__global__ __launch_bounds__(kThreads) void cc_border_kernel(const int64_t* __restrict__ map, int dh_, int dw_, int64_t n_top,
                                                             int64_t n_items, int n_cls, int32_t* __restrict__ link) {
  for (int64_t it = (int64_t)blockIdx.x * kThreads + threadIdx.x; it < n_items; it += (int64_t)gridDim.x * kThreads) {
    if (it < n_top) {
      const int y = TS * (int)(1 + it / dw_), x = (int)(it % dw_);
      const int64_t i = (int64_t)y * dw_ + x;
      const int64_t c = map[i];
      if (c < 0 || c >= n_cls || map[i - dw_] != c) continue;   // a class out of range has no link (the entry refuses the map)
      if (x > 0 && map[i - 1] == c && map[i - dw_ - 1] == c) continue;
      g_unite(link, (int32_t)i, (int32_t)(i - dw_));
    } else {
      const int64_t k = it - n_top;
      const int y = (int)(k % dh_), x = TS * (int)(1 + k / dh_);
      const int64_t i = (int64_t)y * dw_ + x;
      const int64_t c = map[i];
      if (c < 0 || c >= n_cls || map[i - 1] != c) continue;
      g_unite(link, (int32_t)i, (int32_t)(i - 1));
    }
  }
}

__global__ __launch_bounds__(kThreads) void cc_flatten_kernel(int32_t* __restrict__ link, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int32_t p = g_load(link + i);
    if (p >= 0 && p != (int32_t)i) __hip_atomic_store(link + i, g_find(link, p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // others may read this entry meanwhile: old or new, both lead to the root
  }
}

// roots of chunk b (cells b * 2 048 ..): thread t owns the 8 cells from t * 8 on
__device__ __forceinline__ int chunk_roots(const int32_t* __restrict__ link, int64_t n, int64_t i0, bool (&root)[kPer]) {
  int mine = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    root[j] = i0 + j < n && link[i0 + j] == (int32_t)(i0 + j);
    mine += root[j];
  }
  return mine;
}

__global__ __launch_bounds__(kThreads) void cc_count_kernel(const int32_t* __restrict__ link, int64_t n, int32_t* __restrict__ counts) {
  __shared__ int s_w[kThreads / 64];
  bool root[kPer];
  int v = chunk_roots(link, n, (int64_t)blockIdx.x * kChunk + (int64_t)threadIdx.x * kPer, root);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

constexpr int kScanThreads = 1024;
constexpr int kScanWaves = kScanThreads / 64;

// counts -> exclusive prefix sums, in place; status[1] = the total.  One workgroup, 1 024 entries (2 M cells) per round.
__global__ __launch_bounds__(kScanThreads) void cc_scan_kernel(int32_t* __restrict__ counts, int64_t nb, int32_t* __restrict__ status) {
  __shared__ int s_w[kScanWaves];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int base = 0;
  for (int64_t r0 = 0; r0 < nb; r0 += kScanThreads) {
    const int64_t i = r0 + threadIdx.x;
    const int mine = i < nb ? counts[i] : 0;
    int v = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(v, o, 64);
      if (lane >= o) v += u;
    }
    if (lane == 63) s_w[wid] = v;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kScanWaves; ++k) {
      const int x = s_w[k];
      before += k < wid ? x : 0;
      total += x;
    }
    __syncthreads();
    if (i < nb) counts[i] = base + before + v - mine;
    base += total;
  }
  if (threadIdx.x == 0) status[1] = base;
}

// roots get their number 1..K (index order: chunk offset + position among the chunk's roots); background gets 0
__global__ __launch_bounds__(kThreads) void cc_number_kernel(const int32_t* __restrict__ link, int64_t n, const int32_t* __restrict__ offsets,
                                                             int32_t* __restrict__ labels) {
  __shared__ int s_w[kThreads / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * kChunk + (int64_t)threadIdx.x * kPer;
  bool root[kPer];
  const int mine = chunk_roots(link, n, i0, root);
  int v = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  if (lane == 63) s_w[wid] = v;
  __syncthreads();
  int before = 0;
  for (int k = 0; k < wid; ++k) before += s_w[k];
  int id = offsets[blockIdx.x] + before + v - mine;
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (i0 + j < n) {
      if (root[j]) labels[i0 + j] = ++id;
      else if (link[i0 + j] < 0) labels[i0 + j] = 0;
    }
}

__global__ __launch_bounds__(kThreads) void cc_relabel_kernel(const int32_t* __restrict__ link, int64_t n, int32_t* __restrict__ labels) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int32_t r = link[i];
    if (r >= 0 && r != (int32_t)i) labels[i] = labels[r];   // a root's entry was written by the kernel before and is not written here
  }
}

// ---- the region table ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void table_init_kernel(unsigned long long* __restrict__ table, int64_t k) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < k * kCols; i += (int64_t)gridDim.x * kThreads) {
    const int c = (int)(i % kCols);
    table[i] = (c == C_Y0 || c == C_X0 || c == C_FIRST) ? ~0ull : 0ull;
  }
}

struct Run { unsigned long long area, y0, x0, y1, x1, sum_y, sum_x, first, conf; };

__device__ __forceinline__ void add_run(unsigned long long* row, const Run& r, bool conf) {
  atomicAdd(row + C_AREA, r.area);
  atomicMin(row + C_Y0, r.y0);
  atomicMin(row + C_X0, r.x0);
  atomicMax(row + C_Y1, r.y1);
  atomicMax(row + C_X1, r.x1);
  atomicAdd(row + C_SUMY, r.sum_y);
  atomicAdd(row + C_SUMX, r.sum_x);
  atomicMin(row + C_FIRST, r.first);
  if (conf) atomicAdd(row + C_CONF, r.conf);
}

// A thread takes 8 consecutive cells and merges runs of one id within a map row (class maps are made of patches).  A run goes
// to one of 64 slots in LDS, slot id % 64, when that slot is free or already holds the id, else straight to the table; the
// slots are added to the table at the end.  That keeps a region that covers the whole chunk from sending 256 threads' atomics
// to one table row.
constexpr int kSlots = 64;
__global__ __launch_bounds__(kThreads) void region_stats_kernel(const int64_t* __restrict__ map, const int32_t* __restrict__ labels,
                                                                const float* __restrict__ conf, int64_t n, int dw_, int64_t k,
                                                                unsigned long long* __restrict__ table) {
  __shared__ int s_tag[kSlots];
  __shared__ unsigned long long s_row[kSlots][kCols];
  for (int i = threadIdx.x; i < kSlots * kCols; i += kThreads) {
    const int c = i % kCols;
    (&s_row[0][0])[i] = (c == C_Y0 || c == C_X0 || c == C_FIRST) ? ~0ull : 0ull;
  }
  if (threadIdx.x < kSlots) s_tag[threadIdx.x] = 0;
  __syncthreads();
  auto flush = [&](int id, const Run& r) {
    const int s = id & (kSlots - 1);
    const int seen = atomicCAS(&s_tag[s], 0, id);
    if (seen == 0 || seen == id) add_run(s_row[s], r, conf != nullptr);
    else add_run(table + (int64_t)(id - 1) * kCols, r, conf != nullptr);
  };
  const int64_t chunk = (int64_t)kChunk;
  for (int64_t c0 = (int64_t)blockIdx.x * chunk; c0 < n; c0 += (int64_t)gridDim.x * chunk) {
    const int64_t i0 = c0 + (int64_t)threadIdx.x * kPer;
    if (i0 >= n) continue;
    int y = (int)(i0 / dw_), x = (int)(i0 - (int64_t)y * dw_);
    int id = 0;
    Run r = {};
    for (int j = 0; j < kPer && i0 + j < n; ++j) {
      int cur = labels[i0 + j];
      if (cur > k) cur = 0;   // not a label of this table: never an address
      if (cur != id || x == 0) {   // a new id or a new map row ends the run
        if (id > 0) flush(id, r);
        id = cur;
        if (cur > 0) {
          r = Run{0ull, (unsigned long long)y, (unsigned long long)x, (unsigned long long)y + 1, 0ull, 0ull, 0ull,
                  (unsigned long long)(i0 + j), 0ull};
          table[(int64_t)(cur - 1) * kCols + C_CLASS] = (unsigned long long)map[i0 + j];   // every cell of the region writes the same value
        }
      }
      if (cur > 0) {
        r.area += 1ull;
        r.x1 = (unsigned long long)x + 1;
        r.sum_y += (unsigned long long)y;
        r.sum_x += (unsigned long long)x;
        if (conf) r.conf += (unsigned long long)(long long)rint((double)conf[i0 + j] * 4294967296.0);   // exact product; half to even
      }
      if (++x == dw_) { x = 0; ++y; }
    }
    if (id > 0) flush(id, r);
  }
  __syncthreads();
  if (threadIdx.x < kSlots && s_tag[threadIdx.x] > 0) {
    const unsigned long long* s = s_row[threadIdx.x];
    const Run r = {s[C_AREA], s[C_Y0], s[C_X0], s[C_Y1], s[C_X1], s[C_SUMY], s[C_SUMX], s[C_FIRST], s[C_CONF]};
    add_run(table + (int64_t)(s_tag[threadIdx.x] - 1) * kCols, r, conf != nullptr);
  }
}

// ---- cleanup ---------------------------------------------------------------------------------------------------------------
// one thread per cell of a small component: a vote per 4-neighbour that lies in a component that is not small
__global__ __launch_bounds__(kThreads) void region_vote_kernel(const int64_t* __restrict__ map, const int32_t* __restrict__ labels,
                                                               const unsigned long long* __restrict__ table, int64_t n, int dh_,
                                                               int dw_, int n_cls, int64_t k, unsigned long long min_cells,
                                                               int32_t* __restrict__ votes) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int s = labels[i];
    if (s <= 0 || s > k || table[(int64_t)(s - 1) * kCols + C_AREA] >= min_cells) continue;
    const int y = (int)(i / dw_), x = (int)(i - (int64_t)y * dw_);
    const int64_t nb[4] = {y > 0 ? i - dw_ : -1, x > 0 ? i - 1 : -1, x + 1 < dw_ ? i + 1 : -1, y + 1 < dh_ ? i + dw_ : -1};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (nb[j] < 0) continue;
      const int t = labels[nb[j]];
      if (t <= 0 || t > k || t == s || table[(int64_t)(t - 1) * kCols + C_AREA] < min_cells) continue;
      const int64_t c = map[nb[j]];
      if (c >= 0 && c < n_cls) atomicAdd(votes + (int64_t)(s - 1) * n_cls + (int)c, 1);
    }
  }
}

// one thread per component: votes[s][0] becomes the class the component takes, or -1 when it stays as it is
__global__ __launch_bounds__(kThreads) void region_decide_kernel(const unsigned long long* __restrict__ table, int64_t k, int n_cls,
                                                                 unsigned long long min_cells, int32_t* __restrict__ votes) {
  for (int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x; s < k; s += (int64_t)gridDim.x * kThreads) {
    int32_t* v = votes + s * n_cls;
    int best = -1, most = 0;
    if (table[s * kCols + C_AREA] < min_cells)
      for (int c = 0; c < n_cls; ++c)
        if (v[c] > most) { most = v[c]; best = c; }   // strictly more: the lowest class id wins a tie
    v[0] = best;
  }
}

__global__ __launch_bounds__(kThreads) void region_apply_kernel(const int64_t* __restrict__ map, const int32_t* __restrict__ labels,
                                                                const int32_t* __restrict__ votes, int64_t n, int n_cls, int64_t k,
                                                                int64_t* __restrict__ out, int32_t* __restrict__ status) {
  int changed = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int s = labels[i];
    const int to = s > 0 && s <= k ? votes[(int64_t)(s - 1) * n_cls] : -1;
    const int64_t c = map[i];
    out[i] = to >= 0 ? (int64_t)to : c;
    changed += to >= 0 && (int64_t)to != c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) changed += __shfl_xor(changed, o, 64);
  if ((threadIdx.x & 63) == 0 && changed) atomicAdd(status + 2, changed);
}

int grid_for(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>((items + kThreads - 1) / kThreads, kMaxGrid)); }

inline int64_t n_chunks(int64_t n) { return (n + kChunk - 1) / kChunk; }

}  // namespace

#define REGION_CANVAS(what)                                                                                                  \
  DH_REQUIRE(dh_ > 0 && dw_ > 0, what ": dh=%lld, dw=%lld must be > 0", (long long)dh_, (long long)dw_);                      \
  DH_REQUIRE(dh_ <= INT32_MAX && dw_ <= INT32_MAX && dh_ * dw_ < (int64_t)INT32_MAX - kChunk,                                 \
             what ": canvas of %lld x %lld cells is too large", (long long)dh_, (long long)dw_)
#define REGION_CLASSES(what) DH_REQUIRE(n_cls > 0 && n_cls <= MAX_CLS, what ": n_cls=%d outside [1, %d]", n_cls, MAX_CLS)

namespace {
int region_status(int32_t** out) {
  struct Scratch { int32_t* d = nullptr; int device = -1; };
  static thread_local Scratch sc;
  int dev_id = 0;
  DH_HIP(hipGetDevice(&dev_id));
  if (sc.device != dev_id) {
    sc = Scratch();
    DH_HIP(hipMalloc((void**)&sc.d, 4 * sizeof(int32_t)));
    sc.device = dev_id;
  }
  *out = sc.d;
  return DH_OK;
}
}  // namespace

extern "C" int64_t dh_label_work_size(int64_t n_cells) { return n_cells < 0 ? 0 : n_cells + n_chunks(n_cells); }

extern "C" int dh_label_components(const int64_t* map, int64_t dh_, int64_t dw_, int32_t n_cls, int32_t* labels, int32_t* work,
                                   int64_t* n_components_host, void* stream) {
  REGION_CANVAS("label components");
  REGION_CLASSES("label components");
  DH_REQUIRE(map && labels && work && n_components_host, "label components: null pointer (map, labels, work, n_components)");
  *n_components_host = 0;
  const int64_t n = dh_ * dw_, nb = n_chunks(n);
  int32_t *link = work, *counts = work + n, *status = nullptr;
  if (const int rc = region_status(&status)) return rc;
  hipStream_t st = dh::as_stream(stream);
  DH_HIP(hipMemsetAsync(status, 0, 4 * sizeof(int32_t), st));
  const int64_t tiles_y = (dh_ + TS - 1) / TS, tiles_x = (dw_ + TS - 1) / TS;
  hipLaunchKernelGGL(cc_local_kernel, dim3((unsigned)(tiles_y * tiles_x)), dim3(kThreads), 0, st, map, (int)dh_, (int)dw_, (int)n_cls,
                     (int)tiles_x, link, status);
  DH_LAUNCH_CHECK();
  const int64_t n_top = (tiles_y - 1) * dw_, n_items = n_top + (tiles_x - 1) * dh_;
  if (n_items > 0) {
    hipLaunchKernelGGL(cc_border_kernel, dim3(grid_for(n_items)), dim3(kThreads), 0, st, map, (int)dh_, (int)dw_, n_top, n_items, (int)n_cls, link);
    DH_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(grid_for(n)), dim3(kThreads), 0, st, link, n);
    DH_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(cc_count_kernel, dim3((unsigned)nb), dim3(kThreads), 0, st, link, n, counts);
  DH_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, counts, nb, status);
  DH_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_number_kernel, dim3((unsigned)nb), dim3(kThreads), 0, st, link, n, counts, labels);
  DH_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_relabel_kernel, dim3(grid_for(n)), dim3(kThreads), 0, st, link, n, labels);
  DH_LAUNCH_CHECK();
  int32_t s[2];
  DH_HIP(hipMemcpyAsync(s, status, sizeof s, hipMemcpyDeviceToHost, st));
  DH_HIP(hipStreamSynchronize(st));   // K, and the status, depend on the data
  DH_REQUIRE(s[0] == 0, "label components: %d cells hold a class outside [-1, %d)", s[0], n_cls);
  *n_components_host = s[1];
  return DH_OK;
}

extern "C" int dh_region_stats(const int64_t* map, const int32_t* labels, const float* confidence, int64_t dh_, int64_t dw_,
                               int64_t n_components, int64_t* table, void* stream) {
  REGION_CANVAS("region stats");
  DH_REQUIRE(n_components >= 0 && n_components <= dh_ * dw_, "region stats: n_components=%lld outside [0, %lld]",
             (long long)n_components, (long long)(dh_ * dw_));
  if (n_components == 0) return DH_OK;
  DH_REQUIRE(map && labels && table, "region stats: null pointer (map, labels, table)");
  hipStream_t st = dh::as_stream(stream);
  const int64_t n = dh_ * dw_;
  unsigned long long* t = reinterpret_cast<unsigned long long*>(table);
  hipLaunchKernelGGL(table_init_kernel, dim3(grid_for(n_components * kCols)), dim3(kThreads), 0, st, t, n_components);
  DH_LAUNCH_CHECK();
  hipLaunchKernelGGL(region_stats_kernel, dim3((unsigned)std::min<int64_t>(n_chunks(n), kMaxGrid)), dim3(kThreads), 0, st, map, labels,
                     confidence, n, (int)dw_, n_components, t);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_clean_small_regions(const int64_t* map, const int32_t* labels, const int64_t* table, int64_t n_components,
                                      int64_t dh_, int64_t dw_, int32_t n_cls, int64_t min_cells, int32_t* votes, int64_t* out_map, int64_t* n_changed_host, void* stream) {
  REGION_CANVAS("clean small regions");
  REGION_CLASSES("clean small regions");
  DH_REQUIRE(min_cells >= 1, "clean small regions: min_cells=%lld must be >= 1", (long long)min_cells);
  DH_REQUIRE(n_components >= 0 && n_components <= dh_ * dw_, "clean small regions: n_components=%lld outside [0, %lld]",
             (long long)n_components, (long long)(dh_ * dw_));
  DH_REQUIRE(map && labels && out_map && n_changed_host && (n_components == 0 || (table && votes)),
             "clean small regions: null pointer (map, labels, table, votes, out_map, n_changed)");
  DH_REQUIRE(out_map != map, "clean small regions: out_map must not be the input map");
  *n_changed_host = 0;
  const int64_t n = dh_ * dw_;
  hipStream_t st = dh::as_stream(stream);
  const unsigned long long* t = reinterpret_cast<const unsigned long long*>(table);
  if (n_components == 0) {   // all -1: the copy
    DH_HIP(hipMemcpyAsync(out_map, map, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    return DH_OK;
  }
  int32_t* status = nullptr;
  if (const int rc = region_status(&status)) return rc;
  DH_HIP(hipMemsetAsync(status + 2, 0, sizeof(int32_t), st));
  DH_HIP(hipMemsetAsync(votes, 0, (size_t)n_components * n_cls * sizeof(int32_t), st));
  hipLaunchKernelGGL(region_vote_kernel, dim3(grid_for(n)), dim3(kThreads), 0, st, map, labels, t, n, (int)dh_, (int)dw_, (int)n_cls,
                     n_components, (unsigned long long)min_cells, votes);
  DH_LAUNCH_CHECK();
  hipLaunchKernelGGL(region_decide_kernel, dim3(grid_for(n_components)), dim3(kThreads), 0, st, t, n_components, (int)n_cls,
                     (unsigned long long)min_cells, votes);
  DH_LAUNCH_CHECK();
  hipLaunchKernelGGL(region_apply_kernel, dim3(grid_for(n)), dim3(kThreads), 0, st, map, labels, votes, n, (int)n_cls, n_components, out_map, status);
  DH_LAUNCH_CHECK();
  int32_t changed = 0;
  DH_HIP(hipMemcpyAsync(&changed, status + 2, sizeof changed, hipMemcpyDeviceToHost, st));
  DH_HIP(hipStreamSynchronize(st));
  *n_changed_host = changed;
  return DH_OK;
}
