// f1: coverage map of FullImageRndSampler on the device (patch_samplers/full_samplers.py:63-153).
//
// The host planner (deephisto_amd/coverage.py) draws every random number in the reference's order and reduces
// `np.random.choice(dh*dw, B, replace=False, p)` to RANKS among the eligible cells (count < dense_level) in row-major
// order.  This file owns the int32 hit-count map and turns a batch of ranks into cells, tile origins and hits:
//
//   cov_step_kernel (ONE workgroup of 1024 threads, one launch per batch):
//     1. rank -> 1024-cell chunk: block scan of the per-chunk eligible counts (never the map itself);
//     2. chunk -> cell: one wave per rank loads the chunk's 1024 counts (16 loads in flight per lane), ballots
//        `count < dense_level` and picks the rank's set bit;
//     3. origins: (cell // dw - P//d//2) * d + jitter, clamped to [0, h-P] x [0, w-P] (the reference's clamp);
//     4. hits: integer atomicAdd over [y//d, (y+P)//d) x [x//d, (x+P)//d) per origin, duplicates included; the returned
//        old values drive the counters exactly (0 -> 1: filled + 1; dense_level-1 -> dense_level: eligible - 1 and the
//        chunk's count - 1).  Integer atomics are exact and order-independent (no float atomics anywhere).
//   Counters (+ origins when asked) return in ONE device->pinned copy; ranks / explicit cells / jitter come up in ONE
//   pinned->device copy.  Eligible-cell compaction (the rare top-up path) and a float32 read-back of the map are
//   separate kernels.
#include <string.h>

#include <algorithm>
#include <vector>

#include "dh_common.h"

namespace {

constexpr int kChunk = 1024;      // cells per eligible-count chunk (flat row-major index)
constexpr int kThreads = 1024;    // the step kernel's single workgroup
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBatch = 4096;
constexpr int kHdr = 4;           // out[0] filled, out[1] eligible, out[2] status, out[3] unused; origins follow

__device__ __forceinline__ int block_inclusive_scan(int v, int* s_w, int* total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  if (lane == 63) s_w[wid] = v;
  __syncthreads();
  int add = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    const int x = s_w[i];
    add += i < wid ? x : 0;
    tot += x;
  }
  __syncthreads();
  *total = tot;
  return v + add;
}

// in: int32[3n] = idx[n] (ranks, or flat cells when explicit_cells) then jitter[n][2] (jy, jx)
__global__ __launch_bounds__(kThreads) void cov_step_kernel(int32_t* __restrict__ map, int32_t* __restrict__ chunk_cnt,
                                                            int32_t* __restrict__ state, int32_t nchunks, int32_t cells,
                                                            int32_t dh, int32_t dw, int32_t h, int32_t w, int32_t P, int32_t d,
                                                            int32_t dl, const int32_t* __restrict__ in, int32_t n,
                                                            int32_t explicit_cells, int32_t* __restrict__ origins_dev,
                                                            int32_t* __restrict__ out) {
  __shared__ int s_a[kMaxBatch];   // rank, then packed (chunk << 10 | rank in chunk), then y
  __shared__ int s_b[kMaxBatch];   // cell, then x
  __shared__ int s_w[kWaves];
  __shared__ int s_nf, s_ne, s_bad;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) { s_nf = 0; s_ne = 0; s_bad = 0; }
  for (int k = tid; k < n; k += kThreads) {
    s_a[k] = explicit_cells ? 0 : in[k];
    s_b[k] = explicit_cells ? in[k] : -1;
  }
  __syncthreads();

  if (!explicit_cells) {
    // 1. rank -> chunk
    int running = 0;
    for (int base = 0; base < nchunks; base += kThreads) {
      const int c = base + tid;
      const int cnt = c < nchunks ? chunk_cnt[c] : 0;
      int tot;
      const int excl = running + block_inclusive_scan(cnt, s_w, &tot) - cnt;
      if (cnt > 0)
        for (int k = 0; k < n; ++k) {
          const int r = s_a[k];
          if (r >= excl && r < excl + cnt) s_b[k] = (c << 10) | (r - excl);   // s_b: packed until step 2
        }
      running += tot;
    }
    __syncthreads();
    // 2. chunk -> cell, one wave per rank
    for (int k = wid; k < n; k += kWaves) {
      const int packed = s_b[k];
      if (packed < 0) {                       // rank beyond the eligible count: refused on the host, flagged here
        if (lane == 0) s_bad = 1;
        continue;
      }
      const int c0 = (packed >> 10) * kChunk;
      int b = packed & (kChunk - 1);
      int v[kChunk / 64];
#pragma unroll
      for (int j = 0; j < kChunk / 64; ++j) {
        const int cell = c0 + j * 64 + lane;
        v[j] = cell < cells ? map[cell] : dl;
      }
      int found = -1;
#pragma unroll
      for (int j = 0; j < kChunk / 64; ++j) {
        const unsigned long long m = __ballot(v[j] < dl);
        const int pc = __popcll(m);
        if (found < 0 && b < pc) {
          if (((m >> lane) & 1ull) && __popcll(m & ((1ull << lane) - 1ull)) == b) found = c0 + j * 64 + lane;
          found = __shfl(found, __ffsll((long long)__ballot(found >= 0)) - 1, 64);
        } else if (found < 0) {
          b -= pc;
        }
      }
      if (lane == 0) {
        if (found < 0) s_bad = 1;
        s_a[k] = found;
      }
    }
    __syncthreads();
    for (int k = tid; k < n; k += kThreads) s_b[k] = s_a[k];
    __syncthreads();
  }

  // 3. origins
  const int pd2 = P / d / 2;
  for (int k = tid; k < n; k += kThreads) {
    int cell = s_b[k];
    if (cell < 0 || cell >= cells) { s_bad = 1; cell = 0; }
    const int r = cell / dw, c = cell - r * dw;
    int y = (r - pd2) * d + in[n + 2 * k], x = (c - pd2) * d + in[n + 2 * k + 1];
    y = max(min(y, h - P), 0);
    x = max(min(x, w - P), 0);
    if (origins_dev) { origins_dev[2 * k] = y; origins_dev[2 * k + 1] = x; }
    out[kHdr + 2 * k] = y;
    out[kHdr + 2 * k + 1] = x;
    s_a[k] = y;
    s_b[k] = x;
  }
  __syncthreads();

  // 4. hits: one wave per origin, lanes over the rectangle's cells
  int nf = 0, ne = 0;
  for (int k = wid; k < n; k += kWaves) {
    const int y = s_a[k], x = s_b[k];
    const int r0 = y / d, r1 = min((y + P) / d, dh), c0 = x / d, c1 = min((x + P) / d, dw);
    const int nc = c1 - c0, tot = (r1 - r0) * nc;
    for (int i = lane; i < tot; i += 64) {
      const int q = i / nc;
      const int cell = (r0 + q) * dw + c0 + (i - q * nc);
      const int old = atomicAdd(&map[cell], 1);
      nf += old == 0;
      if (old == dl - 1) {
        ++ne;
        atomicSub(&chunk_cnt[cell / kChunk], 1);
      }
    }
  }
  // per-wave sums, then one LDS add per wave (Guideline 12)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nf += __shfl_xor(nf, o, 64);
    ne += __shfl_xor(ne, o, 64);
  }
  if (lane == 0 && (nf | ne)) {
    atomicAdd(&s_nf, nf);
    atomicAdd(&s_ne, ne);
  }
  __syncthreads();
  if (tid == 0) {   // the only workgroup of the step: the counters need no atomics
    const int f = state[0] + s_nf, e = state[1] - s_ne;
    state[0] = f;
    state[1] = e;
    out[0] = f;
    out[1] = e;
    out[2] = s_bad;
    out[3] = 0;
  }
}

__global__ __launch_bounds__(256) void cov_init_kernel(int32_t* __restrict__ chunk_cnt, int32_t* __restrict__ state,
                                                       int32_t nchunks, int32_t cells) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < nchunks) chunk_cnt[c] = min(kChunk, cells - c * kChunk);
  if (c == 0) { state[0] = 0; state[1] = cells; }
}

// one wave per chunk: chunk_cnt from the map, filled / eligible totals into state (zeroed by the caller)
__global__ __launch_bounds__(64) void cov_recount_kernel(const int32_t* __restrict__ map, int32_t* __restrict__ chunk_cnt,
                                                         int32_t* __restrict__ state, int32_t cells, int32_t dl) {
  const int c = blockIdx.x, lane = threadIdx.x;
  int e = 0, f = 0;
  for (int j = 0; j < kChunk / 64; ++j) {
    const int cell = c * kChunk + j * 64 + lane;
    if (cell < cells) {
      const int v = map[cell];
      e += v < dl;
      f += v != 0;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    e += __shfl_xor(e, o, 64);
    f += __shfl_xor(f, o, 64);
  }
  if (lane == 0) {
    chunk_cnt[c] = e;
    atomicAdd(&state[0], f);
    atomicAdd(&state[1], e);
  }
}

// the rare top-up path: flat indices of the eligible cells (unordered; count in *count, at most cap written)
__global__ __launch_bounds__(64) void cov_eligible_kernel(const int32_t* __restrict__ map, const int32_t* __restrict__ chunk_cnt,
                                                          int32_t cells, int32_t dl, int32_t* __restrict__ count,
                                                          int32_t* __restrict__ out, int32_t cap) {
  const int c = blockIdx.x, lane = threadIdx.x;
  if (chunk_cnt[c] == 0) return;
  for (int j = 0; j < kChunk / 64; ++j) {
    const int cell = c * kChunk + j * 64 + lane;
    const bool e = cell < cells && map[cell] < dl;
    const unsigned long long m = __ballot(e);
    if (!m) continue;
    int base = 0;
    if (lane == 0) base = atomicAdd(count, __popcll(m));
    base = __shfl(base, 0, 64);
    const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
    if (e && pos < cap) out[pos] = cell;
  }
}

__global__ __launch_bounds__(256) void cov_read_map_kernel(const int32_t* __restrict__ map, float* __restrict__ out, int64_t cells) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (float)map[i];
}

}  // namespace

struct dh_coverage {
  int32_t h, w, P, d, dl, dh, dw, cells, nchunks, max_batch;
  int32_t* map = nullptr;        // [cells]
  int32_t* chunk_cnt = nullptr;  // [nchunks]
  int32_t* state = nullptr;      // [2] filled, eligible
  int32_t* in_dev = nullptr;     // [3 * max_batch]
  int32_t* out_dev = nullptr;    // [kHdr + 2 * max_batch]
  int32_t* elig_dev = nullptr;   // [1 + max_batch]: count, cells
  int32_t* pin_in = nullptr;
  int32_t* pin_out = nullptr;
  int32_t* pin_elig = nullptr;
  hipEvent_t done = nullptr;
  bool pending = false;          // a step's read-back is in flight
  int32_t last_n = 0, last_host_origins = 0;
  int64_t filled = 0, eligible = 0;
  int32_t status = 0;
};

namespace {
void cov_free(dh_coverage* cv) {
  if (!cv) return;
  if (cv->done) (void)hipEventDestroy(cv->done);
  for (int32_t* p : {cv->map, cv->chunk_cnt, cv->state, cv->in_dev, cv->out_dev, cv->elig_dev})
    if (p) (void)hipFree(p);
  for (int32_t* p : {cv->pin_in, cv->pin_out, cv->pin_elig})
    if (p) (void)hipHostFree(p);
  delete cv;
}

// wait for the last step's read-back and take its counters
int cov_settle(dh_coverage* cv) {
  if (!cv->pending) return DH_OK;
  DH_HIP(hipEventSynchronize(cv->done));
  cv->pending = false;
  cv->filled = cv->pin_out[0];
  cv->eligible = cv->pin_out[1];
  cv->status = cv->pin_out[2];
  DH_REQUIRE(cv->status == 0, "dh_coverage: a rank or cell of the last step had no eligible cell (map and counts disagree)");
  return DH_OK;
}
}  // namespace

extern "C" int dh_coverage_create(dh_coverage** out, int64_t h, int64_t w, int32_t patch, int32_t speedup, int32_t dense_level,
                                  int32_t max_batch, void* stream) {
  DH_REQUIRE(out != nullptr, "dh_coverage_create: null handle pointer");
  *out = nullptr;
  DH_REQUIRE(patch > 0 && speedup > 0, "dh_coverage_create: patch (%d) and speedup (%d) must be > 0", patch, speedup);
  DH_REQUIRE(h >= patch && w >= patch, "dh_coverage_create: slide %lldx%lld smaller than patch %d", (long long)h, (long long)w, patch);
  DH_REQUIRE(h <= INT32_MAX / 2 && w <= INT32_MAX / 2, "dh_coverage_create: slide side exceeds int32");
  DH_REQUIRE(dense_level >= 1, "dh_coverage_create: dense_level must be an integer >= 1 (got %d)", dense_level);
  DH_REQUIRE(max_batch >= 1 && max_batch <= kMaxBatch, "dh_coverage_create: max_batch %d outside [1, %d]", max_batch, kMaxBatch);
  const int64_t dh = h / speedup, dw = w / speedup, cells = dh * dw;
  DH_REQUIRE(cells >= max_batch, "dh_coverage_create: map of %lldx%lld cells is smaller than the batch %d", (long long)dh, (long long)dw,
             max_batch);
  DH_REQUIRE(cells <= INT32_MAX - kChunk, "dh_coverage_create: map of %lld cells exceeds int32", (long long)cells);
  dh_coverage* cv = new dh_coverage();
  cv->h = (int32_t)h; cv->w = (int32_t)w; cv->P = patch; cv->d = speedup; cv->dl = dense_level;
  cv->dh = (int32_t)dh; cv->dw = (int32_t)dw; cv->cells = (int32_t)cells;
  cv->nchunks = (int32_t)((cells + kChunk - 1) / kChunk);
  cv->max_batch = max_batch;
  auto fail = [&](hipError_t e) {
    dh::set_error("dh_coverage_create: %s", hipGetErrorString(e));
    cov_free(cv);
    return e == hipErrorOutOfMemory ? DH_ENOMEM : DH_EHIP;
  };
  hipError_t e;
#define DH_COV_TRY(call) if ((e = (call)) != hipSuccess) return fail(e)
  DH_COV_TRY(hipMalloc(&cv->map, sizeof(int32_t) * cells));
  DH_COV_TRY(hipMalloc(&cv->chunk_cnt, sizeof(int32_t) * cv->nchunks));
  DH_COV_TRY(hipMalloc(&cv->state, sizeof(int32_t) * 2));
  DH_COV_TRY(hipMalloc(&cv->in_dev, sizeof(int32_t) * 3 * max_batch));
  DH_COV_TRY(hipMalloc(&cv->out_dev, sizeof(int32_t) * (kHdr + 2 * max_batch)));
  DH_COV_TRY(hipMalloc(&cv->elig_dev, sizeof(int32_t) * (1 + max_batch)));
  DH_COV_TRY(hipHostMalloc(&cv->pin_in, sizeof(int32_t) * 3 * max_batch, hipHostMallocDefault));
  DH_COV_TRY(hipHostMalloc(&cv->pin_out, sizeof(int32_t) * (kHdr + 2 * max_batch), hipHostMallocDefault));
  DH_COV_TRY(hipHostMalloc(&cv->pin_elig, sizeof(int32_t) * (1 + max_batch), hipHostMallocDefault));
  DH_COV_TRY(hipEventCreateWithFlags(&cv->done, hipEventDisableTiming));
  hipStream_t s = dh::as_stream(stream);
  DH_COV_TRY(hipMemsetAsync(cv->map, 0, sizeof(int32_t) * cells, s));
  hipLaunchKernelGGL(cov_init_kernel, dim3((cv->nchunks + 255) / 256), dim3(256), 0, s, cv->chunk_cnt, cv->state, cv->nchunks,
                     cv->cells);
  DH_COV_TRY(hipGetLastError());
#undef DH_COV_TRY
  cv->filled = 0;
  cv->eligible = cells;
  *out = cv;
  return DH_OK;
}

extern "C" void dh_coverage_destroy(dh_coverage* cv) {
  if (!cv) return;
  if (cv->pending) (void)hipEventSynchronize(cv->done);
  (void)hipDeviceSynchronize();   // nothing of this handle may still run when its buffers go
  cov_free(cv);
}

extern "C" int dh_coverage_step(dh_coverage* cv, const int32_t* idx_host, const int32_t* jitter_host, int32_t n,
                                int32_t explicit_cells, int32_t* origins_dev, int32_t host_origins, void* stream) {
  DH_REQUIRE(cv != nullptr, "dh_coverage_step: null handle");
  DH_REQUIRE(idx_host && jitter_host, "dh_coverage_step: null ranks / jitter");
  DH_REQUIRE(n >= 1 && n <= cv->max_batch, "dh_coverage_step: n = %d outside [1, %d]", n, cv->max_batch);
  int rc = cov_settle(cv);   // the previous read-back has landed: the staging buffers are free and the counts are current
  if (rc) return rc;
  if (explicit_cells) {
    for (int32_t k = 0; k < n; ++k)
      DH_REQUIRE(idx_host[k] >= 0 && idx_host[k] < cv->cells, "dh_coverage_step: cell %d of entry %d outside [0, %d)", idx_host[k], k,
                 cv->cells);
  } else {
    for (int32_t k = 0; k < n; ++k)
      DH_REQUIRE(idx_host[k] >= 0 && idx_host[k] < cv->eligible, "dh_coverage_step: rank %d of entry %d outside [0, %lld eligible)",
                 idx_host[k], k, (long long)cv->eligible);
  }
  for (int32_t k = 0; k < 2 * n; ++k)
    DH_REQUIRE(jitter_host[k] >= 0 && jitter_host[k] < cv->d, "dh_coverage_step: jitter %d outside [0, %d)", jitter_host[k], cv->d);
  memcpy(cv->pin_in, idx_host, sizeof(int32_t) * n);
  memcpy(cv->pin_in + n, jitter_host, sizeof(int32_t) * 2 * n);
  hipStream_t s = dh::as_stream(stream);
  DH_HIP(hipMemcpyAsync(cv->in_dev, cv->pin_in, sizeof(int32_t) * 3 * n, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(cov_step_kernel, dim3(1), dim3(kThreads), 0, s, cv->map, cv->chunk_cnt, cv->state, cv->nchunks, cv->cells, cv->dh,
                     cv->dw, cv->h, cv->w, cv->P, cv->d, cv->dl, cv->in_dev, n, explicit_cells ? 1 : 0, origins_dev, cv->out_dev);
  DH_LAUNCH_CHECK();
  DH_HIP(hipMemcpyAsync(cv->pin_out, cv->out_dev, sizeof(int32_t) * (kHdr + (host_origins ? 2 * n : 0)), hipMemcpyDeviceToHost, s));
  DH_HIP(hipEventRecord(cv->done, s));
  cv->pending = true;
  cv->last_n = n;
  cv->last_host_origins = host_origins ? 1 : 0;
  return DH_OK;
}

extern "C" int dh_coverage_counters(dh_coverage* cv, int64_t* filled, int64_t* eligible, int32_t* origins_host) {
  DH_REQUIRE(cv != nullptr, "dh_coverage_counters: null handle");
  DH_REQUIRE(!origins_host || (cv->last_n > 0 && cv->last_host_origins),
             "dh_coverage_counters: the last step did not ask for host origins");
  int rc = cov_settle(cv);
  if (rc) return rc;
  if (filled) *filled = cv->filled;
  if (eligible) *eligible = cv->eligible;
  if (origins_host) memcpy(origins_host, cv->pin_out + kHdr, sizeof(int32_t) * 2 * cv->last_n);
  return DH_OK;
}

extern "C" int dh_coverage_eligible_cells(dh_coverage* cv, int32_t* cells_host, int32_t cap, int32_t* n_out, void* stream) {
  DH_REQUIRE(cv != nullptr && cells_host && n_out, "dh_coverage_eligible_cells: null argument");
  int rc = cov_settle(cv);
  if (rc) return rc;
  DH_REQUIRE(cv->eligible <= cap && cv->eligible <= cv->max_batch,
             "dh_coverage_eligible_cells: %lld eligible cells exceed the capacity %d (or the handle's batch %d)", (long long)cv->eligible,
             cap, cv->max_batch);
  hipStream_t s = dh::as_stream(stream);
  DH_HIP(hipMemsetAsync(cv->elig_dev, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(cov_eligible_kernel, dim3(cv->nchunks), dim3(64), 0, s, cv->map, cv->chunk_cnt, cv->cells, cv->dl, cv->elig_dev,
                     cv->elig_dev + 1, cv->max_batch);
  DH_LAUNCH_CHECK();
  DH_HIP(hipMemcpyAsync(cv->pin_elig, cv->elig_dev, sizeof(int32_t) * (1 + cv->max_batch), hipMemcpyDeviceToHost, s));
  DH_HIP(hipStreamSynchronize(s));
  const int32_t cnt = cv->pin_elig[0];
  DH_REQUIRE(cnt == cv->eligible, "dh_coverage_eligible_cells: %d cells found, the counter says %lld", cnt, (long long)cv->eligible);
  std::vector<int32_t> v(cv->pin_elig + 1, cv->pin_elig + 1 + cnt);
  std::sort(v.begin(), v.end());
  memcpy(cells_host, v.data(), sizeof(int32_t) * cnt);
  *n_out = cnt;
  return DH_OK;
}

extern "C" int dh_coverage_read_map(dh_coverage* cv, float* map_dev, void* stream) {
  DH_REQUIRE(cv != nullptr && map_dev, "dh_coverage_read_map: null argument");
  const int grid = (int)std::min<int64_t>((cv->cells + 255) / 256, 4096);
  hipLaunchKernelGGL(cov_read_map_kernel, dim3(grid), dim3(256), 0, dh::as_stream(stream), cv->map, map_dev, (int64_t)cv->cells);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// test hook: replace the map by int32 host counts [dh][dw] (>= 0) and recount chunks, filled and eligible; synchronises
extern "C" int dh_debug_coverage_set_map(dh_coverage* cv, const int32_t* map_host, void* stream) {
  DH_REQUIRE(cv != nullptr && map_host, "dh_debug_coverage_set_map: null argument");
  for (int32_t i = 0; i < cv->cells; ++i) DH_REQUIRE(map_host[i] >= 0, "dh_debug_coverage_set_map: negative count at %d", i);
  int rc = cov_settle(cv);
  if (rc) return rc;
  hipStream_t s = dh::as_stream(stream);
  DH_HIP(hipMemcpyAsync(cv->map, map_host, sizeof(int32_t) * cv->cells, hipMemcpyHostToDevice, s));
  DH_HIP(hipMemsetAsync(cv->state, 0, sizeof(int32_t) * 2, s));
  hipLaunchKernelGGL(cov_recount_kernel, dim3(cv->nchunks), dim3(64), 0, s, cv->map, cv->chunk_cnt, cv->state, cv->cells, cv->dl);
  DH_LAUNCH_CHECK();
  DH_HIP(hipMemcpyAsync(cv->pin_out, cv->state, sizeof(int32_t) * 2, hipMemcpyDeviceToHost, s));
  DH_HIP(hipStreamSynchronize(s));
  cv->filled = cv->pin_out[0];
  cv->eligible = cv->pin_out[1];
  return DH_OK;
}
