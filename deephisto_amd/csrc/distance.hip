// Distance maps of a whole-slide class map for MI355X (gfx950, wave64):
//   dh_class_mask          uint8 mask of a class set: its members, its boundary, or every label change
//   dh_distance_transform  exact squared Euclidean distance of every cell to the nearest mask cell, and that cell's index
// The transform is separable and all integer:
//   edt_col_down_kernel  one thread per (segment of 128 rows, column): the last mask row at or above every cell within the
//                        segment, and the segment's first and last mask row in two small tables
//   edt_col_up_kernel    the same threads: the carries from the segments above and below out of the two tables, then upwards
//                        through the segment: per cell the row of the nearest mask cell of its column, the upper of two equals
//   edt_row_kernel       one workgroup per map row: the signed row offsets dy(x') of that row in LDS as int16, the least
//                        dy^2 per block of 64 columns beside them; per cell the minimum over x' of (x - x')^2 + dy(x')^2 with the
//                        smaller linear index among equals: outwards from x while r^2 <= best for 32 steps, then block by block,
//                        a block being skipped when (distance to its near edge)^2 + its least dy^2 exceeds the best so far
// A candidate is only ever left out when it is strictly worse than one already seen, and candidates are compared by
// (d^2, index), so the result is the lexicographic minimum whatever the order they are met in: no atomics, no floats, and
// nothing depends on the launch geometry.  dh, dw <= 32 767, so 2 * 32 766^2 < 2^31 and dy fits an int16 with -32 768 to spare.
#include <algorithm>

#include "dh_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxGrid = 256 * 8;
constexpr int kMaxSide = 32767;
constexpr int kSeg = 128;        // rows per segment of the column pass
constexpr int kColThreads = 64;
constexpr int kBlk = 64;         // columns per block of the row pass
constexpr int kNear = 32;        // steps of the plain outward scan before the row pass goes block by block
constexpr int16_t kNone = INT16_MIN;

__device__ __forceinline__ bool is_member(int64_t v, unsigned long long bits, int incl) {
  return v < 0 ? (v == -1 && incl) : (v < 64 && ((bits >> v) & 1ull));
}

__global__ __launch_bounds__(kThreads) void class_mask_kernel(const int64_t* __restrict__ map, int dh_, int dw_, unsigned long long bits,
                                                              int incl, int mode, uint8_t* __restrict__ mask, int32_t* __restrict__ status) {
  const int64_t n = (int64_t)dh_ * dw_;
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int64_t v = map[i];
    bad += v < -1 || v > 63;
    const int y = (int)(i / dw_), x = (int)(i - (int64_t)y * dw_);
    const int64_t nb[4] = {y > 0 ? i - dw_ : -1, x > 0 ? i - 1 : -1, x + 1 < dw_ ? i + 1 : -1, y + 1 < dh_ ? i + dw_ : -1};
    bool out;
    if (mode == 2) {
      out = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) out = out || (nb[j] >= 0 && map[nb[j]] != v);
    } else {
      out = is_member(v, bits, incl);
      if (mode == 1 && out) {
        bool edge = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) edge = edge || (nb[j] >= 0 && !is_member(map[nb[j]], bits, incl));
        out = edge;
      }
    }
    mask[i] = out ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(status, bad);
}

// rows s * 128 .. of column x, downwards: near[y][x] = the last mask row <= y of the segment, or -1
__global__ __launch_bounds__(kColThreads) void edt_col_down_kernel(const uint8_t* __restrict__ mask, int dh_, int dw_, int32_t* __restrict__ near,
                                                                   int32_t* __restrict__ seg_first, int32_t* __restrict__ seg_last) {
  const int x = blockIdx.x * kColThreads + threadIdx.x, s = blockIdx.y;
  if (x >= dw_) return;
  const int y0 = s * kSeg, y1 = min(y0 + kSeg, dh_);
  int last = -1, first = -1;
#pragma unroll 8
  for (int y = y0; y < y1; ++y) {
    const int64_t i = (int64_t)y * dw_ + x;
    if (mask[i]) {
      last = y;
      if (first < 0) first = y;
    }
    near[i] = last;
  }
  seg_first[(int64_t)s * dw_ + x] = first;
  seg_last[(int64_t)s * dw_ + x] = last;
}

// the same segment upwards: `up` the nearest mask row above (from the segment, else from the segments before it), `next` the
// nearest below; the upper one on a tie
__global__ __launch_bounds__(kColThreads) void edt_col_up_kernel(const uint8_t* __restrict__ mask, int dh_, int dw_, int n_seg,
                                                                 int32_t* __restrict__ near, const int32_t* __restrict__ seg_first,
                                                                 const int32_t* __restrict__ seg_last) {
  const int x = blockIdx.x * kColThreads + threadIdx.x, s = blockIdx.y;
  if (x >= dw_) return;
  int above = -1, next = -1;
  for (int t = s - 1; t >= 0 && above < 0; --t) above = seg_last[(int64_t)t * dw_ + x];
  for (int t = s + 1; t < n_seg && next < 0; ++t) next = seg_first[(int64_t)t * dw_ + x];
  const int y0 = s * kSeg, y1 = min(y0 + kSeg, dh_);
#pragma unroll 8
  for (int y = y1 - 1; y >= y0; --y) {
    const int64_t i = (int64_t)y * dw_ + x;
    if (mask[i]) next = y;
    int up = near[i];
    if (up < 0) up = above;
    near[i] = up < 0 ? next : (next < 0 || y - up <= next - y) ? up : next;
  }
}

// s_dy[x'] = near[y][x'] - y as int16 (kNone: the column holds no mask cell); s_min[b] = the least dy^2 of block b
__global__ __launch_bounds__(kThreads) void edt_row_kernel(const int32_t* __restrict__ near, int dw_, int n_blk, int32_t* __restrict__ d2,
                                                           int32_t* __restrict__ nearest) {
  extern __shared__ __attribute__((aligned(16))) char edt_lds[];
  int32_t* s_min = reinterpret_cast<int32_t*>(edt_lds);                  // [n_blk]
  int16_t* s_dy = reinterpret_cast<int16_t*>(edt_lds + (size_t)n_blk * 4);   // [n_blk * 64]
  const int y = blockIdx.x;
  const int32_t* row = near + (int64_t)y * dw_;
  for (int x = threadIdx.x; x < n_blk * kBlk; x += kThreads) {
    const int r = x < dw_ ? row[x] : -1;
    s_dy[x] = r < 0 ? kNone : (int16_t)(r - y);
  }
  __syncthreads();
  for (int b = threadIdx.x >> 6; b < n_blk; b += kThreads / 64) {
    const int v = s_dy[b * kBlk + (threadIdx.x & 63)];
    int m = v == kNone ? INT32_MAX : v * v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) s_min[b] = m;
  }
  __syncthreads();
  for (int x = threadIdx.x; x < dw_; x += kThreads) {
    int best = INT32_MAX, bidx = -1;
    auto take = [&](int xc) {   // 0 <= xc < n_blk * 64; the padding holds kNone
      const int v = s_dy[xc];
      if (v == kNone) return;
      const int dx = xc - x, d = v * v + dx * dx;
      if (d > best) return;
      const int idx = (y + v) * dw_ + xc;
      if (d < best || idx < bidx) { best = d; bidx = idx; }
    };
    take(x);
    int r = 1;
    for (; r <= kNear && r * r <= best && (x - r >= 0 || x + r < dw_); ++r) {
      if (x - r >= 0) take(x - r);
      if (x + r < dw_) take(x + r);
    }
    if (r > kNear && r * r <= best) {   // columns x - 32 .. x + 32 are done: the blocks that reach beyond them
      const int bl = (x - kNear) >> 6, br = (x + kNear) >> 6;   // the blocks the plain scan ended in (arithmetic shift: -1 left of the row)
      for (int b = bl; b >= 0; --b) {
        const int e = max(x - (b * kBlk + kBlk - 1), 0);   // distance to the block's near edge
        if (e * e > best) break;
        const int m = s_min[b];
        if (m == INT32_MAX || e * e + m > best) continue;
        for (int xc = b * kBlk; xc < b * kBlk + kBlk; ++xc) take(xc);
      }
      for (int b = br; b < n_blk; ++b) {
        const int e = max(b * kBlk - x, 0);
        if (e * e > best) break;
        const int m = s_min[b];
        if (m == INT32_MAX || e * e + m > best) continue;
        for (int xc = b * kBlk; xc < b * kBlk + kBlk; ++xc) take(xc);
      }
    }
    const int64_t o = (int64_t)y * dw_ + x;
    d2[o] = best;
    if (nearest) nearest[o] = bidx;
  }
}

int grid_for(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>((items + kThreads - 1) / kThreads, kMaxGrid)); }

inline int64_t n_segments(int64_t dh_) { return (dh_ + kSeg - 1) / kSeg; }

int mask_status(int32_t** out) {
  struct Scratch { int32_t* d = nullptr; int device = -1; };
  static thread_local Scratch sc;
  int dev_id = 0;
  DH_HIP(hipGetDevice(&dev_id));
  if (sc.device != dev_id) {
    sc = Scratch();
    DH_HIP(hipMalloc((void**)&sc.d, sizeof(int32_t)));
    sc.device = dev_id;
  }
  *out = sc.d;
  return DH_OK;
}

}  // namespace

#define DISTANCE_CANVAS(what)                                                                                                    \
  DH_REQUIRE(dh_ >= 1 && dw_ >= 1 && dh_ <= kMaxSide && dw_ <= kMaxSide, what ": dh=%lld, dw=%lld must lie in [1, %d]", (long long)dh_, \
             (long long)dw_, kMaxSide)

extern "C" int dh_class_mask(const int64_t* map, int64_t dh_, int64_t dw_, uint64_t class_bits, int32_t include_unclassified, int32_t mode,
                             uint8_t* mask, void* stream) {
  DISTANCE_CANVAS("class mask");
  DH_REQUIRE(mode >= 0 && mode <= 2, "class mask: mode=%d is not 0 (members), 1 (boundary) or 2 (label changes)", mode);
  DH_REQUIRE(map && mask, "class mask: null pointer (map, mask)");
  int32_t* status = nullptr;
  if (const int rc = mask_status(&status)) return rc;
  hipStream_t st = dh::as_stream(stream);
  DH_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(class_mask_kernel, dim3(grid_for(dh_ * dw_)), dim3(kThreads), 0, st, map, (int)dh_, (int)dw_,
                     (unsigned long long)class_bits, include_unclassified ? 1 : 0, (int)mode, mask, status);
  DH_LAUNCH_CHECK();
  int32_t bad = 0;
  DH_HIP(hipMemcpyAsync(&bad, status, sizeof bad, hipMemcpyDeviceToHost, st));
  DH_HIP(hipStreamSynchronize(st));   // the status depends on the data
  DH_REQUIRE(bad == 0, "class mask: %d cells hold a class outside [-1, 63]", bad);
  return DH_OK;
}

extern "C" int64_t dh_distance_work_size(int64_t dh_, int64_t dw_) {
  if (dh_ < 1 || dw_ < 1 || dh_ > kMaxSide || dw_ > kMaxSide) return 0;
  return dh_ * dw_ + 2 * n_segments(dh_) * dw_;
}

extern "C" int dh_distance_transform(const uint8_t* mask, int64_t dh_, int64_t dw_, int32_t* d2, int32_t* nearest, int32_t* work,
                                     void* stream) {
  DISTANCE_CANVAS("distance transform");
  DH_REQUIRE(mask && d2 && work, "distance transform: null pointer (mask, d2, work)");
  hipStream_t st = dh::as_stream(stream);
  const int n_seg = (int)n_segments(dh_), n_blk = (int)((dw_ + kBlk - 1) / kBlk);
  int32_t *near = work, *seg_first = work + dh_ * dw_, *seg_last = seg_first + (int64_t)n_seg * dw_;
  const dim3 col_grid((unsigned)((dw_ + kColThreads - 1) / kColThreads), (unsigned)n_seg);
  hipLaunchKernelGGL(edt_col_down_kernel, col_grid, dim3(kColThreads), 0, st, mask, (int)dh_, (int)dw_, near, seg_first, seg_last);
  DH_LAUNCH_CHECK();
  hipLaunchKernelGGL(edt_col_up_kernel, col_grid, dim3(kColThreads), 0, st, mask, (int)dh_, (int)dw_, n_seg, near, seg_first, seg_last);
  DH_LAUNCH_CHECK();
  const size_t lds = (size_t)n_blk * (4 + kBlk * 2);   // at most 512 * 132 = 67 584 bytes
  if (lds > 64 * 1024)
    DH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(edt_row_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(edt_row_kernel, dim3((unsigned)dh_), dim3(kThreads), lds, st, near, (int)dw_, n_blk, d2, nearest);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
