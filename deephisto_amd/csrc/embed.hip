// Embedding rows for MI355X (gfx950, wave64): what a prototype (nearest-class-mean) scorer needs on top of
// the per-tile features of dh_resnet*_features_tiles.
//   dh_embed_normalize    row / sqrt(sum row^2): one wave per row, lane sums in column order, one butterfly over the wave
//   dh_embed_scores       scale * feat . proto^T: a skinny f32 GEMM, 32 rows x 64 prototypes per workgroup through LDS (sc_tile, the
//                         one tile under this, dh_embed_assign for K > 16 and dh_embed_project)
//   dh_embed_class_sums   per-class sums of labelled rows in a fixed chunked order + int64 counts
//   dh_embed_assign       per row, the nearest of K centres and its squared distance: sc_tile on a subtract-and-FMA step
//                         for K > 16, one row per lane against centres broadcast from LDS for K <= 16
//   dh_embed_scatter      the scatter matrix of the rows about a mean: one triangle of 64 x 64 tiles, chunk
//                         partials in a fixed order, the other triangle a mirrored store
//   dh_embed_project      scale * (feat - mean) . comp^T: sc_tile with the subtract at staging
//   dh_embed_knn          per query row, the k nearest rows of a bank: 64 query rows against the bank in panels
//                         of 64 rows on packed f32 subtracts and FMAs, a sorted list of k (distance, index) pairs per row in LDS
//   dh_embed_knn_votes    the neighbours' labels counted per class, the winner with the nearer neighbour ahead at equal counts
// No atomics, and every reduction has one fixed order that the launch geometry cannot change: a row's result is the same bits
// whatever n, the row's place and the grid are (the house rule of the canvas kernels).
//
// The arithmetic of dh_embed_scores at the slide's size (n = 198 916, D = 2048, K = 64): 26 G FMA against 1.6 GB of feature reads.
// The card's f32 vector peak (157.3 TFLOPS = 78.6 T FMA/s packed, half that with plain v_fma_f32) makes that 0.33-0.67 ms, its HBM
// ~0.33 ms: the two are of one size, so plain FMAs are enough (the f32 MFMA runs at the vector peak's rate, not above it).  What
// decides is the LDS: a thread owns 2 rows x 4 prototypes, so a float4 step along D costs 6 ds_read_b128 for 32 FMAs.  Measured:
// 1.06 ms, 24.6 T FMA/s.
#include <algorithm>

#include "dh_common.h"

namespace {

constexpr int SC_ROWS = 32;    // rows of a workgroup's tile
constexpr int SC_K = 64;       // prototypes of a workgroup's tile: all of them (K <= 64)
constexpr int SC_CK = 64;      // columns per LDS stage (D % 64 == 0)
constexpr int SC_LD = SC_CK + 4;   // padded row of the LDS tiles: prototype rows k, k + 1, ... start 4 banks apart
constexpr int CHUNK = DH_EMBED_CHUNK_ROWS;

// One wave per row.  Lane l adds the squares of columns l, l + 64, ... in that order; the butterfly leaves every lane with the same sum
// (a + b == b + a).  In place is safe: a lane writes only the elements it alone reads.
__global__ __launch_bounds__(256) void embed_normalize_kernel(const float* in, int64_t n, int D, float* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < n; row += (int64_t)gridDim.x * 4) {
    const float* src = in + row * D;
    float* dst = out + row * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) { const float v = src[c]; s = __builtin_fmaf(v, v, s); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float norm = sqrtf(s);
    for (int c = lane; c < D; c += 64) { const float v = src[c]; dst[c] = s > 0.f ? v / norm : 0.f; }
  }
}

// The global loads of one LDS stage (columns c0 .. c0 + 63): float4 number q of a tile is (row q / 16, columns 4 (q % 16) ..); a thread
// moves numbers tid and tid + 256 of the features and tid + 256 j, j < 4, of the prototypes.  Rows past n and prototypes past K are
// loaded from the last real one (in bounds) and zeroed.
struct ScStage { float4 f0, f1, p0, p1, p2, p3; };
__device__ __forceinline__ float4 sc_load(const float* __restrict__ base, int64_t row, int64_t last, int D, int col) {
  const float4 v = *reinterpret_cast<const float4*>(base + (row <= last ? row : last) * D + col);
  return row <= last ? v : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ ScStage sc_fetch(const float* __restrict__ feat, const float* __restrict__ proto, int64_t n, int D, int K,
                                            int64_t row0, int c0, int tid) {
  const int r = tid >> 4, col = c0 + (tid & 15) * 4;
  ScStage g;
  g.f0 = sc_load(feat, row0 + r, n - 1, D, col);
  g.f1 = sc_load(feat, row0 + r + 16, n - 1, D, col);
  g.p0 = sc_load(proto, r, K - 1, D, col);
  g.p1 = sc_load(proto, r + 16, K - 1, D, col);
  g.p2 = sc_load(proto, r + 32, K - 1, D, col);
  g.p3 = sc_load(proto, r + 48, K - 1, D, col);
  return g;
}

// The 32 x 64 tile under embed_scores_kernel, embed_assign_kernel and embed_project_kernel: one workgroup per 32 rows, 256 threads.
//   Ownership.  Thread (rt = tid / 16, kt = tid % 16) owns rows rt and rt + 16 of the tile and prototypes kt, kt + 16, kt + 32,
//               kt + 48: eight accumulators, returned as ScAcc.
//   One chain.  Every accumulator starts from 0 and is ONE chain of STEP over c = 0 .. D - 1 in ascending order, four columns
//               (a float4 of the row, a float4 of the prototype) per call: acc = STEP(f, p, acc).
//   Padding.    Rows past n and prototypes past K are loaded from the last real one (in bounds) and zeroed; the caller never stores
//               their accumulators.
//   Staging.    Feature and prototype columns go through LDS 64 at a time; the next stage's global loads are issued before the
//               current stage's arithmetic.  CENTRE: mean[c] is taken off a feature element as it is parked (one float32 subtract,
//               before any multiply), a zeroed padding row included.
//   LDS cost.   A float4 step along D is 6 ds_read_b128 (2 rows, 4 prototypes) for 32 element pairs.
//   SKIP_IDLE.  A thread none of whose prototypes exists (K <= 16 leaves kt >= K idle) skips the arithmetic, never a barrier.
__device__ __forceinline__ float sc_dot4(float4 f, float4 p, float acc) {   // the step of a dot product: four fused multiply-adds
  acc = __builtin_fmaf(f.x, p.x, acc);
  acc = __builtin_fmaf(f.y, p.y, acc);
  acc = __builtin_fmaf(f.z, p.z, acc);
  return __builtin_fmaf(f.w, p.w, acc);
}
__device__ __forceinline__ float4 sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

struct ScAcc { float v[2][4]; };   // v[i][j]: the accumulator of (row rt + 16 i, prototype kt + 16 j)
template <float (*STEP)(float4, float4, float), bool CENTRE, bool SKIP_IDLE>
__device__ __forceinline__ ScAcc sc_tile(const float* __restrict__ feat, int64_t n, int D, const float* __restrict__ proto, int K,
                                        const float* __restrict__ mean, int64_t row0) {
  __shared__ __attribute__((aligned(16))) float s_f[SC_ROWS * SC_LD];
  __shared__ __attribute__((aligned(16))) float s_p[SC_K * SC_LD];
  const int tid = threadIdx.x, rt = tid >> 4, kt = tid & 15;
  ScAcc acc;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc.v[i][j] = 0.f;
  ScStage g = sc_fetch(feat, proto, n, D, K, row0, 0, tid);
  float4 m = make_float4(0.f, 0.f, 0.f, 0.f);   // the mean of this thread's four columns of the stage
  if constexpr (CENTRE) m = *reinterpret_cast<const float4*>(mean + kt * 4);
  float* const st_f = &s_f[rt * SC_LD + kt * 4];   // where this thread parks its loads: (row tid / 16 [+ 16 j], columns 4 (tid % 16) ..)
  float* const st_p = &s_p[rt * SC_LD + kt * 4];
  for (int c0 = 0; c0 < D; c0 += SC_CK) {
    __syncthreads();   // the previous stage's readers are done
    *reinterpret_cast<float4*>(st_f) = CENTRE ? sub4(g.f0, m) : g.f0;
    *reinterpret_cast<float4*>(st_f + 16 * SC_LD) = CENTRE ? sub4(g.f1, m) : g.f1;
    *reinterpret_cast<float4*>(st_p) = g.p0;
    *reinterpret_cast<float4*>(st_p + 16 * SC_LD) = g.p1;
    *reinterpret_cast<float4*>(st_p + 32 * SC_LD) = g.p2;
    *reinterpret_cast<float4*>(st_p + 48 * SC_LD) = g.p3;
    __syncthreads();
    if (c0 + SC_CK < D) {
      g = sc_fetch(feat, proto, n, D, K, row0, c0 + SC_CK, tid);
      if constexpr (CENTRE) m = *reinterpret_cast<const float4*>(mean + c0 + SC_CK + kt * 4);
    }
    if (!SKIP_IDLE || kt < K) {
#pragma unroll 4
      for (int c = 0; c < SC_CK; c += 4) {
        float4 f[2], p[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) f[i] = *reinterpret_cast<const float4*>(&s_f[(rt + 16 * i) * SC_LD + c]);
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = *reinterpret_cast<const float4*>(&s_p[(kt + 16 * j) * SC_LD + c]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc.v[i][j] = STEP(f[i], p[j], acc.v[i][j]);
      }
    }
  }
  return acc;
}

// scores[row][k] = scale * (feat[row] . proto[k]): the tile on sc_dot4, idle threads skipped.
__global__ __launch_bounds__(256) void embed_scores_kernel(const float* __restrict__ feat, int64_t n, int D,
                                                           const float* __restrict__ proto, int K, float scale,
                                                           float* __restrict__ scores) {
  const int rt = threadIdx.x >> 4, kt = threadIdx.x & 15;
  const int64_t row0 = (int64_t)blockIdx.x * SC_ROWS;
  const ScAcc acc = sc_tile<sc_dot4, false, true>(feat, n, D, proto, K, nullptr, row0);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t row = row0 + rt + 16 * i;
    if (row >= n) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = kt + 16 * j;
      if (k < K) scores[row * K + k] = scale * acc.v[i][j];
    }
  }
}

// ---- dh_embed_assign -------------------------------------------------------------------------------------
// One squared distance: ONE accumulator from 0, for c ascending t = x[c] - m[c] (one subtract), acc = fma(t, t, acc).
__device__ __forceinline__ float as_dist4(float4 x, float4 m, float acc) {
  float t = x.x - m.x;
  acc = __builtin_fmaf(t, t, acc);
  t = x.y - m.y;
  acc = __builtin_fmaf(t, t, acc);
  t = x.z - m.z;
  acc = __builtin_fmaf(t, t, acc);
  t = x.w - m.w;
  return __builtin_fmaf(t, t, acc);
}

// The choice is the lexicographic minimum of (dist, index): commutative and associative, so any order of taking it gives the same
// pair.  A NaN distance compares false and never wins; neither does +inf against the start (+inf, -1).
__device__ __forceinline__ void as_take(float& bd, int& bk, float d, int k) {
  if (d < bd || (d == bd && k < bk)) { bd = d; bk = k; }
}

// K > 16: the tile on as_dist4 (32 rows x 64 centres), no thread idle.  Centres past K are never compared.  Epilogue: the thread's
// minimum over its (up to) four centres, a butterfly over the 16 lanes of one rt, lane kt == 0 stores.
__global__ __launch_bounds__(256) void embed_assign_kernel(const float* __restrict__ feat, int64_t n, int D,
                                                           const float* __restrict__ centre, int K, int k0, int merge,
                                                           int32_t* __restrict__ label, float* __restrict__ dist) {
  const int rt = threadIdx.x >> 4, kt = threadIdx.x & 15;
  const int64_t row0 = (int64_t)blockIdx.x * SC_ROWS;
  const ScAcc acc = sc_tile<as_dist4, false, false>(feat, n, D, centre, K, nullptr, row0);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t row = row0 + rt + 16 * i;
    const bool live = row < n;   // uniform over the 16 lanes of one rt
    float bd = __builtin_inff();
    int bk = -1;
    if (merge && live && kt == 0) { bd = dist[row]; bk = label[row]; }   // the held pair enters once; its index is the lower
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = kt + 16 * j;
      if (k < K) as_take(bd, bk, acc.v[i][j], k0 + k);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const float od = __shfl_xor(bd, o, 64);
      const int ok = __shfl_xor(bk, o, 64);
      as_take(bd, bk, od, ok);
    }
    if (live && kt == 0) { dist[row] = bd; label[row] = bk; }
  }
}

// K <= 16: one row per lane, so no lane waits on a centre that is not there.  A workgroup takes 256 rows; every wave stages its own
// 64 rows x 64 columns in LDS by row-contiguous float4 loads (16 per lane and stage, the next stage's issued before this stage's
// arithmetic) and reads its lane's row back into registers; the centres' 64 columns sit in LDS once per workgroup and every lane reads
// the same address (a broadcast).  KC accumulators per lane, each one chain over c ascending; centres j >= K are skipped by a
// branch the whole grid takes alike.
constexpr int AS_ROWS = 256;   // rows of a workgroup's tile: one per thread
constexpr int AS_KC = 16;      // centres of this instantiation

__global__ __launch_bounds__(256) void embed_assign_rows_kernel(const float* __restrict__ feat, int64_t n, int D,
                                                                const float* __restrict__ centre, int K, int k0, int merge,
                                                                int32_t* __restrict__ label, float* __restrict__ dist) {
  __shared__ __attribute__((aligned(16))) float s_f[AS_ROWS * SC_LD];
  __shared__ __attribute__((aligned(16))) float s_p[AS_KC * SC_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t wrow0 = (int64_t)blockIdx.x * AS_ROWS + wave * 64;   // the wave's first row
  float* const w_f = &s_f[wave * 64 * SC_LD];
  const int lr = lane >> 4, lc = (lane & 15) * 4;   // float4 number q = lane + 64 u of the wave's stage: row 4 u + lr, columns lc ..
  float acc[AS_KC];
#pragma unroll
  for (int j = 0; j < AS_KC; ++j) acc[j] = 0.f;
  float4 g[16], gp;
#pragma unroll
  for (int u = 0; u < 16; ++u) g[u] = sc_load(feat, wrow0 + 4 * u + lr, n - 1, D, lc);
  gp = sc_load(centre, tid >> 4, K - 1, D, (tid & 15) * 4);
  for (int c0 = 0; c0 < D; c0 += SC_CK) {
    __syncthreads();   // the previous stage's readers are done
#pragma unroll
    for (int u = 0; u < 16; ++u) *reinterpret_cast<float4*>(&w_f[(4 * u + lr) * SC_LD + lc]) = g[u];
    *reinterpret_cast<float4*>(&s_p[(tid >> 4) * SC_LD + (tid & 15) * 4]) = gp;
    __syncthreads();
    if (c0 + SC_CK < D) {
#pragma unroll
      for (int u = 0; u < 16; ++u) g[u] = sc_load(feat, wrow0 + 4 * u + lr, n - 1, D, c0 + SC_CK + lc);
      gp = sc_load(centre, tid >> 4, K - 1, D, c0 + SC_CK + (tid & 15) * 4);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {   // 32 columns of the lane's row in registers at a time
      float4 f[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) f[q] = *reinterpret_cast<const float4*>(&w_f[lane * SC_LD + 32 * h + 4 * q]);
#pragma unroll
      for (int j = 0; j < AS_KC; ++j) {
        if (j < K) {
          float a = acc[j];
#pragma unroll
          for (int q = 0; q < 8; ++q) a = as_dist4(f[q], *reinterpret_cast<const float4*>(&s_p[j * SC_LD + 32 * h + 4 * q]), a);
          acc[j] = a;
        }
      }
    }
  }
  const int64_t row = wrow0 + lane;
  if (row >= n) return;
  float bd = __builtin_inff();
  int bk = -1;
  if (merge) { bd = dist[row]; bk = label[row]; }
#pragma unroll
  for (int j = 0; j < AS_KC; ++j)
    if (j < K) as_take(bd, bk, acc[j], k0 + j);
  dist[row] = bd;
  label[row] = bk;
}

// Stage 1, one workgroup per (chunk of 1024 rows, slab of 256 columns).  The chunk's labels are sorted by class in LDS, stably (thread k
// scans them in row order), so class k's rows are idx[start[k] .. start[k + 1]) in ascending order; thread c then adds, class by class,
// those rows' column c into ONE accumulator from 0 and writes partial[chunk][k][c], zeros included.  The slab-0 workgroup also writes the
// chunk's per-class row counts (int32, behind the partials).
__global__ __launch_bounds__(256) void embed_class_partial_kernel(const float* __restrict__ feat, const int32_t* __restrict__ label,
                                                                  int64_t n, int D, int K, float* __restrict__ partial,
                                                                  int32_t* __restrict__ chunk_count) {
  __shared__ int32_t s_lab[CHUNK];
  __shared__ int32_t s_idx[CHUNK];
  __shared__ int32_t s_cnt[64], s_start[65];
  const int tid = threadIdx.x;
  const int64_t chunk = blockIdx.x, base = chunk * CHUNK;
  const int rows = (int)std::min<int64_t>(CHUNK, n - base);
  for (int r = tid; r < rows; r += 256) s_lab[r] = label[base + r];
  __syncthreads();
  if (tid < K) {
    int cnt = 0;
    for (int r = 0; r < rows; ++r) cnt += s_lab[r] == tid ? 1 : 0;
    s_cnt[tid] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    int p = 0;
    for (int k = 0; k < K; ++k) { s_start[k] = p; p += s_cnt[k]; }
    s_start[K] = p;   // <= rows
  }
  __syncthreads();
  if (tid < K) {
    int p = s_start[tid];
    for (int r = 0; r < rows; ++r)
      if (s_lab[r] == tid) s_idx[p++] = r;
    if (blockIdx.y == 0) chunk_count[chunk * K + tid] = s_cnt[tid];
  }
  __syncthreads();
  const int c = blockIdx.y * 256 + tid;
  if (c >= D) return;
  const float* col = feat + base * D + c;
  for (int k = 0; k < K; ++k) {
    const int beg = s_start[k], end = s_start[k + 1];
    float acc = 0.f;
    int j = beg;
    for (; j + 8 <= end; j += 8) {   // eight loads in flight, added in row order
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = col[(int64_t)s_idx[j + u] * D];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = acc + v[u];
    }
    for (; j < end; ++j) acc = acc + col[(int64_t)s_idx[j] * D];
    partial[(chunk * K + k) * D + c] = acc;
  }
}

// Stage 2, one thread per (class, column): the partials of all chunks, added in ascending chunk order from 0; the first K threads also
// add up the counts.
__global__ __launch_bounds__(256) void embed_class_final_kernel(const float* __restrict__ partial, const int32_t* __restrict__ chunk_count,
                                                                int64_t n_chunks, int D, int K, float* __restrict__ sums,
                                                                int64_t* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;   // K * D <= 64 * 4096
  if (i < K * D) {
    float acc = 0.f;
    for (int64_t ch = 0; ch < n_chunks; ++ch) acc = acc + partial[ch * K * D + i];
    sums[i] = acc;
  }
  if (i < K) {
    int64_t cnt = 0;
    for (int64_t ch = 0; ch < n_chunks; ++ch) cnt += chunk_count[ch * K + i];
    counts[i] = cnt;
  }
}

// ---- dh_embed_project ------------------------------------------------------------------------------------
// out[row][k] = scale[k] * ((feat[row] - mean) . comp[k]): the tile on sc_dot4 with the mean taken off at staging, idle threads
// skipped; an output row is ld floats of which only the first K are written.
__global__ __launch_bounds__(256) void embed_project_kernel(const float* __restrict__ feat, int64_t n, int D,
                                                            const float* __restrict__ mean, const float* __restrict__ comp, int K,
                                                            const float* __restrict__ scale, float* __restrict__ out, int ld) {
  const int rt = threadIdx.x >> 4, kt = threadIdx.x & 15;
  const int64_t row0 = (int64_t)blockIdx.x * SC_ROWS;
  const ScAcc acc = sc_tile<sc_dot4, true, true>(feat, n, D, comp, K, mean, row0);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = kt + 16 * j;
    if (k >= K) continue;
    const float s = scale ? scale[k] : 1.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t row = row0 + rt + 16 * i;
      if (row < n) out[row * ld + k] = s * acc.v[i][j];
    }
  }
}

// ---- dh_embed_scatter ------------------------------------------------------------------------------------
// S = T^T T of the centred rows, one triangle of 64 x 64 output tiles.  Workgroup (group of chunks, tile pair (ta, tb), ta <= tb);
// thread (ra = tid / 16, rb = tid % 16) owns S[a0 + 4 ra + i][b0 + 4 rb + j], i, j < 4: sixteen accumulators, each ONE chain of fused
// multiply-adds over the rows of a chunk in ascending order, added to the thread's running totals at the end of every chunk
// (tot = tot + acc, from 0, in ascending chunk order).  Rows go through LDS 32 at a time as two slabs [row][64 columns] (a diagonal
// tile parks one and reads it twice), the mean already taken off; a row step is 2 ds_read_b128 (16 lanes share the a-slab address,
// the 16 b-slab addresses fill one 256-byte bank row: no conflicts, no padding) for 16 FMAs.  The next stage's global loads are
// issued before the current stage's arithmetic.  Rows past the chunk's (or the matrix's) end are loaded from the last real row
// (in bounds) and parked as zeros, which leave a chain as it is.
//   direct != 0: the workgroup walks ALL chunks and stores its totals into S, the off-diagonal tile a second time transposed
//                (S[b][a] is S[a][b]'s bits: the product commutes); no scratch.
//   direct == 0: one chunk per workgroup (chunk ch0 + blockIdx.x), its partial goes to work[blockIdx.x][pair][64][64];
//                embed_scatter_fold_kernel adds the partials in ascending chunk order.  The host launches the pair once per batch
//                of chunks, batch after batch, so the scratch holds one batch (see sk_batch).
constexpr int SK_T = 64;       // the side of an output tile
constexpr int SK_ROWS = 32;    // rows per LDS stage (CHUNK % SK_ROWS == 0)

__device__ __forceinline__ void sk_pair(int pair, int T, int& ta, int& tb) {   // pairs in the order (0,0) (0,1) .. (0,T-1) (1,1) ..
  ta = 0;
  while (pair >= T - ta) { pair -= T - ta; ++ta; }
  tb = ta + pair;
}
__device__ __forceinline__ float4 sk_centre(float4 v, float4 m, bool live) {
  return live ? sub4(v, m) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(256) void embed_scatter_kernel(const float* __restrict__ feat, int64_t n, int D,
                                                            const float* __restrict__ mean, int64_t n_chunks, int64_t ch0,
                                                            int direct, float* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) float s_a[SK_ROWS * SK_T];
  __shared__ __attribute__((aligned(16))) float s_b[SK_ROWS * SK_T];
  const int tid = threadIdx.x, ra = tid >> 4, rb = tid & 15;
  const int T = D / SK_T;
  int ta, tb;
  sk_pair(blockIdx.y, T, ta, tb);
  const bool diag = ta == tb;
  const int a0 = ta * SK_T, b0 = tb * SK_T;
  const float* const rd_b = diag ? s_a : s_b;
  const int lr = tid >> 4, lc = (tid & 15) * 4;   // this thread parks rows lr and lr + 16, columns lc .. lc + 3 of each slab
  const float4 ma = *reinterpret_cast<const float4*>(mean + a0 + lc);
  const float4 mb = *reinterpret_cast<const float4*>(mean + b0 + lc);
  float tot[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) tot[i][j] = 0.f;
  const int64_t ch_lo = direct ? 0 : ch0 + blockIdx.x, ch_hi = direct ? n_chunks : ch_lo + 1;
  for (int64_t ch = ch_lo; ch < ch_hi; ++ch) {
    const int64_t base = ch * CHUNK;
    const int64_t last = std::min<int64_t>(base + CHUNK, n) - 1;   // the chunk's last row, >= base
    const int rows = (int)(last - base + 1);
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    float4 ga0 = sc_load(feat, base + lr, last, D, a0 + lc), ga1 = sc_load(feat, base + lr + 16, last, D, a0 + lc);
    float4 gb0 = ga0, gb1 = ga1;
    if (!diag) { gb0 = sc_load(feat, base + lr, last, D, b0 + lc); gb1 = sc_load(feat, base + lr + 16, last, D, b0 + lc); }
    for (int r0 = 0; r0 < rows; r0 += SK_ROWS) {
      __syncthreads();   // the previous stage's readers are done
      const bool live0 = base + r0 + lr <= last, live1 = base + r0 + lr + 16 <= last;
      *reinterpret_cast<float4*>(&s_a[lr * SK_T + lc]) = sk_centre(ga0, ma, live0);
      *reinterpret_cast<float4*>(&s_a[(lr + 16) * SK_T + lc]) = sk_centre(ga1, ma, live1);
      if (!diag) {
        *reinterpret_cast<float4*>(&s_b[lr * SK_T + lc]) = sk_centre(gb0, mb, live0);
        *reinterpret_cast<float4*>(&s_b[(lr + 16) * SK_T + lc]) = sk_centre(gb1, mb, live1);
      }
      __syncthreads();
      if (r0 + SK_ROWS < rows) {
        const int64_t nx = base + r0 + SK_ROWS + lr;
        ga0 = sc_load(feat, nx, last, D, a0 + lc);
        ga1 = sc_load(feat, nx + 16, last, D, a0 + lc);
        if (!diag) { gb0 = sc_load(feat, nx, last, D, b0 + lc); gb1 = sc_load(feat, nx + 16, last, D, b0 + lc); }
      }
#pragma unroll 8
      for (int r = 0; r < SK_ROWS; ++r) {
        const float4 va = *reinterpret_cast<const float4*>(&s_a[r * SK_T + 4 * ra]);
        const float4 vb = *reinterpret_cast<const float4*>(&rd_b[r * SK_T + 4 * rb]);
        const float a[4] = {va.x, va.y, va.z, va.w}, b[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(a[i], b[j], acc[i][j]);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) tot[i][j] = tot[i][j] + acc[i][j];
  }
  if (!direct) {   // work[chunk of the batch][pair][64][64]
    float* w = dst + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * (SK_T * SK_T) + (4 * ra) * SK_T + 4 * rb;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(w + i * SK_T) = make_float4(tot[i][0], tot[i][1], tot[i][2], tot[i][3]);
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    *reinterpret_cast<float4*>(dst + (int64_t)(a0 + 4 * ra + i) * D + b0 + 4 * rb) = make_float4(tot[i][0], tot[i][1], tot[i][2], tot[i][3]);
  if (!diag) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<float4*>(dst + (int64_t)(b0 + 4 * rb + j) * D + a0 + 4 * ra) = make_float4(tot[0][j], tot[1][j], tot[2][j], tot[3][j]);
  }
}

// The second pass of direct == 0: thread (pair, ra, rb) adds its 4 x 4 block of the partials of a batch's chunks in ascending chunk
// order (eight loads in flight, added in order) to what S holds from the batches before it (its own triangle's element; 0 for the
// first batch) and stores it into S as the kernel above does.
__global__ __launch_bounds__(256) void embed_scatter_fold_kernel(const float* __restrict__ work, int64_t n_chunks, int D, int first,
                                                                 float* __restrict__ S) {
  const int tid = threadIdx.x, ra = tid >> 4, rb = tid & 15;
  const int n_pairs = gridDim.x;
  int ta, tb;
  sk_pair(blockIdx.x, D / SK_T, ta, tb);
  const int a0 = ta * SK_T, b0 = tb * SK_T;
  const int64_t step = (int64_t)n_pairs * (SK_T * SK_T);
  float4 tot[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float* w = work + (int64_t)blockIdx.x * (SK_T * SK_T) + (4 * ra + i) * SK_T + 4 * rb;
    float* const s_row = S + (int64_t)(a0 + 4 * ra + i) * D + b0 + 4 * rb;
    float4 t = first ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(s_row);
    int64_t ch = 0;
    for (; ch + 8 <= n_chunks; ch += 8) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(w + (ch + u) * step);
#pragma unroll
      for (int u = 0; u < 8; ++u) { t.x = t.x + v[u].x; t.y = t.y + v[u].y; t.z = t.z + v[u].z; t.w = t.w + v[u].w; }
    }
    for (; ch < n_chunks; ++ch) {
      const float4 v = *reinterpret_cast<const float4*>(w + ch * step);
      t.x = t.x + v.x; t.y = t.y + v.y; t.z = t.z + v.z; t.w = t.w + v.w;
    }
    tot[i] = t;
    *reinterpret_cast<float4*>(s_row) = t;
  }
  if (ta != tb) {
    float* m = S + (int64_t)(b0 + 4 * rb) * D + a0 + 4 * ra;
    *reinterpret_cast<float4*>(m) = make_float4(tot[0].x, tot[1].x, tot[2].x, tot[3].x);
    *reinterpret_cast<float4*>(m + D) = make_float4(tot[0].y, tot[1].y, tot[2].y, tot[3].y);
    *reinterpret_cast<float4*>(m + 2 * (int64_t)D) = make_float4(tot[0].z, tot[1].z, tot[2].z, tot[3].z);
    *reinterpret_cast<float4*>(m + 3 * (int64_t)D) = make_float4(tot[0].w, tot[1].w, tot[2].w, tot[3].w);
  }
}

// Which decomposition dh_embed_scatter takes: the chunks of one batch are spread over the grid, their partials held in scratch of
// at most SK_WORK_FLOATS floats and at most half the feature matrix; a matrix too small for a batch of two chunks is walked by one
// workgroup per tile pair, without scratch (sk_batch == 0).
constexpr int64_t SK_WORK_FLOATS = (int64_t)1 << 26;
int64_t sk_pairs(int D) { return (int64_t)(D / SK_T) * (D / SK_T + 1) / 2; }
int64_t sk_batch(int64_t n, int D) {
  const int64_t n_chunks = (n + CHUNK - 1) / CHUNK;
  const int64_t b = std::min(n_chunks, std::min(SK_WORK_FLOATS, n * D / 2) / (sk_pairs(D) * SK_T * SK_T));
  return b < 2 ? 0 : b;
}

// ---- dh_embed_knn ----------------------------------------------------------------------------------------
// The order of the selection: lexicographic on (distance, index).  It is total on the pairs that may enter (finite distances,
// distinct indices), so the k smallest are one list however the bank is walked.  A NaN compares false and never precedes anything.
__device__ __forceinline__ bool kn_less(float d, int j, float od, int oj) { return d < od || (d == od && j < oj); }

// A workgroup owns 64 query rows and walks the bank in panels of 64 rows; thread (ra = tid / 16, rb = tid % 16) holds the 4 x 4
// distances of query rows ra + 16 i to bank rows pb + rb + 16 j of the panel, each the chain of as_dist4 over all D columns (the
// query rows go through LDS again for every panel; they come from L2).  The query stage sits in LDS as in the scores tile
// ([row][68]); the bank stage sits transposed, [rb][column][j] with the slabs of rb 4 banks apart, so that one ds_read_b128 hands a
// thread column c of its four bank rows: the pairs (j = 0, 1) and (j = 2, 3) are then adjacent registers and a column costs two
// packed subtracts and two packed fused multiply-adds per query row, the query element read from one half of its register pair.
// A float4 step along D is 8 ds_read_b128 for 64 element pairs (the 32 x 64 tile: 6 for 32).  The arithmetic per element pair
// is that of as_dist4, operation for operation.
// Per query row a list of k pairs, ascending, sits in LDS.  After a panel a thread compares each of its sixteen pairs with its
// row's k-th pair; the few that precede it are parked in s_p (free between panels) and the 16-lane group of ra learns which by a
// ballot.  Lane rb == i of the group then inserts them into row ra + 16 i's list, checking each against the k-th pair as it now
// stands.  The next panel's first loads are in flight during all this.  KMAX: the list's capacity (k <= KMAX), 16 or 64.
constexpr int KN_ROWS = 64;              // query rows of a workgroup's tile
constexpr int KN_PLD = 4 * SC_CK + 4;    // floats of one rb's slab of the transposed bank stage

typedef float kn_f2 __attribute__((ext_vector_type(2)));

struct KnStage { float4 f[4], p[4]; };
__device__ __forceinline__ KnStage kn_fetch(const float* __restrict__ query, const float* __restrict__ panel, int64_t n, int D, int rows,
                                            int64_t row0, int c0, int tid) {
  const int r = tid >> 4, col = c0 + (tid & 15) * 4;
  KnStage g;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    g.f[u] = sc_load(query, row0 + r + 16 * u, n - 1, D, col);
    g.p[u] = sc_load(panel, r + 16 * u, rows - 1, D, col);
  }
  return g;
}

template <int KMAX>
__global__ __launch_bounds__(256) void embed_knn_kernel(const float* __restrict__ query, int64_t n, int D,
                                                        const float* __restrict__ bank, int64_t m, int k, int m0, int merge,
                                                        int32_t* __restrict__ index, float* __restrict__ dist) {
  __shared__ __attribute__((aligned(16))) float s_f[KN_ROWS * SC_LD];
  __shared__ __attribute__((aligned(16))) float s_p[16 * KN_PLD];
  __shared__ float s_ld[KN_ROWS * KMAX];   // row r's k distances at k r
  __shared__ int s_li[KN_ROWS * KMAX];     // and their indices
  const int tid = threadIdx.x, ra = tid >> 4, rb = tid & 15;
  const int64_t row0 = (int64_t)blockIdx.x * KN_ROWS;
  float* const s_cand = s_p;   // [64][64] distances of a panel's survivors (16 * KN_PLD >= 64 * 64)
  for (int e = tid; e < KN_ROWS * k; e += 256) {
    const int r = e / k;
    float d = __builtin_inff();
    int j = -1;
    if (merge && row0 + r < n) {
      d = dist[row0 * k + e];
      j = index[row0 * k + e];
      if (!(d < __builtin_inff())) { d = __builtin_inff(); j = -1; }   // what could not have entered counts as padding
    }
    s_ld[e] = d;
    s_li[e] = j;
  }
  const int stages = D / SC_CK;
  KnStage g = {};
  if (m > 0) g = kn_fetch(query, bank, n, D, (int)std::min<int64_t>(SC_K, m), row0, 0, tid);
  float* const st_f = &s_f[ra * SC_LD + rb * 4];      // rows ra + 16 u, columns 4 rb ..
  float* const st_p = &s_p[ra * KN_PLD + rb * 16];    // slab of bank rows ra + 16 j, columns 4 rb ..
  for (int64_t pb = 0; pb < m; pb += SC_K) {
    const int rows = (int)std::min<int64_t>(SC_K, m - pb);   // bank rows of this panel
    kn_f2 acc[4][2];   // acc[i][h] = the distances of query row ra + 16 i to bank rows rb + 16 (2 h), rb + 16 (2 h + 1)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = kn_f2{0.f, 0.f};
    for (int s = 0; s < stages; ++s) {
      __syncthreads();   // the previous stage's readers, and the previous panel's inserters, are done
#pragma unroll
      for (int u = 0; u < 4; ++u) *reinterpret_cast<float4*>(st_f + 16 * u * SC_LD) = g.f[u];
      *reinterpret_cast<float4*>(st_p) = make_float4(g.p[0].x, g.p[1].x, g.p[2].x, g.p[3].x);
      *reinterpret_cast<float4*>(st_p + 4) = make_float4(g.p[0].y, g.p[1].y, g.p[2].y, g.p[3].y);
      *reinterpret_cast<float4*>(st_p + 8) = make_float4(g.p[0].z, g.p[1].z, g.p[2].z, g.p[3].z);
      *reinterpret_cast<float4*>(st_p + 12) = make_float4(g.p[0].w, g.p[1].w, g.p[2].w, g.p[3].w);
      __syncthreads();
      if (s + 1 < stages) g = kn_fetch(query, bank + pb * D, n, D, rows, row0, (s + 1) * SC_CK, tid);
      else if (pb + SC_K < m)
        g = kn_fetch(query, bank + (pb + SC_K) * D, n, D, (int)std::min<int64_t>(SC_K, m - pb - SC_K), row0, 0, tid);
#pragma unroll 2
      for (int c = 0; c < SC_CK; c += 4) {
        float4 f[4], p[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = *reinterpret_cast<const float4*>(&s_f[(ra + 16 * i) * SC_LD + c]);
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = *reinterpret_cast<const float4*>(&s_p[rb * KN_PLD + (c + u) * 4]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float x[4] = {f[i].x, f[i].y, f[i].z, f[i].w};
#pragma unroll
          for (int u = 0; u < 4; ++u) {   // column c + u: t = q - b (one subtract), acc = fma(t, t, acc)
            kn_f2 t = kn_f2{x[u], x[u]} - kn_f2{p[u].x, p[u].y};
            acc[i][0] = __builtin_elementwise_fma(t, t, acc[i][0]);
            t = kn_f2{x[u], x[u]} - kn_f2{p[u].z, p[u].w};
            acc[i][1] = __builtin_elementwise_fma(t, t, acc[i][1]);
          }
        }
      }
    }
    __syncthreads();   // s_p is read out: it takes the survivors
    const int base = m0 + (int)pb;   // m0 + m <= 2^31 - 1
    unsigned mine[4] = {0u, 0u, 0u, 0u};   // lane rb == i keeps row ra + 16 i's masks: bit b of mine[j] = bank row pb + b + 16 j was parked
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = ra + 16 * i;
      const float kd = s_ld[r * k + k - 1];
      const int kj = s_li[r * k + k - 1];
      const float dd[4] = {acc[i][0].x, acc[i][0].y, acc[i][1].x, acc[i][1].y};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int b = rb + 16 * j;
        const float d = dd[j];
        const bool in = b < rows && d < __builtin_inff() && kn_less(d, base + b, kd, kj);
        if (in) s_cand[r * SC_K + b] = d;
        const unsigned seg = (unsigned)(__ballot(in) >> (16 * (ra & 3))) & 0xffffu;
        if (rb == i) mine[j] = seg;
      }
    }
    __syncthreads();
    if (rb < 4) {
      const int r = ra + 16 * rb;
      float* const ld = &s_ld[r * k];
      int* const li = &s_li[r * k];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned bits = mine[j];
        while (bits) {
          const int b = __builtin_ctz(bits) + 16 * j;
          bits &= bits - 1;
          const float d = s_cand[r * SC_K + b];
          const int idx = base + b;
          if (!kn_less(d, idx, ld[k - 1], li[k - 1])) continue;
          int p = k - 1;
          for (; p > 0 && kn_less(d, idx, ld[p - 1], li[p - 1]); --p) { ld[p] = ld[p - 1]; li[p] = li[p - 1]; }
          ld[p] = d;
          li[p] = idx;
        }
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < KN_ROWS * k; e += 256) {
    if (row0 + e / k >= n) continue;
    dist[row0 * k + e] = s_ld[e];
    index[row0 * k + e] = s_li[e];
  }
}

// One thread per row.  The row's counts live in its own votes row (nobody else touches it): cleared, then one increment per
// neighbour in stored order; the label is found by a second walk in stored order that takes a class only when it has strictly
// more votes than the best so far, so at equal votes the class met first (the nearer neighbour's) stays.
__global__ __launch_bounds__(256) void embed_knn_votes_kernel(const int32_t* __restrict__ index, int64_t n, int k,
                                                              const int32_t* __restrict__ bank_label, int64_t m, int C,
                                                              int32_t* votes, int32_t* __restrict__ label) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  int32_t* const v = votes + row * C;
  for (int c = 0; c < C; ++c) v[c] = 0;
  for (int p = 0; p < k; ++p) {
    const int j = index[row * k + p];
    if (j < 0 || j >= m) continue;
    const int c = bank_label[j];
    if (c >= 0 && c < C) v[c] = v[c] + 1;
  }
  int best = 0, lab = -1;
  for (int p = 0; p < k; ++p) {
    const int j = index[row * k + p];
    if (j < 0 || j >= m) continue;
    const int c = bank_label[j];
    if (c >= 0 && c < C && v[c] > best) { best = v[c]; lab = c; }
  }
  label[row] = lab;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int check_dims(const char* what, int64_t n, int32_t D, int32_t K) {
  DH_REQUIRE(n >= 0 && n <= ((int64_t)1 << 40), "%s: n = %lld out of range [0, 2^40]", what, (long long)n);
  DH_REQUIRE(D >= 64 && D <= 4096 && D % 64 == 0, "%s: D = %d unsupported (64 <= D <= 4096, D %% 64 == 0)", what, D);
  DH_REQUIRE(K >= 1 && K <= 64, "%s: K = %d out of range [1, 64]", what, K);
  return DH_OK;
}

// The launch of a 32 x 64 tile kernel: one workgroup per SC_ROWS rows, as many as one grid dimension holds.
int sc_grid(const char* what, int64_t n, unsigned* grid) {
  DH_REQUIRE(n <= (int64_t)SC_ROWS * 0x7fffffff, "%s: n = %lld exceeds one launch", what, (long long)n);
  *grid = (unsigned)((n + SC_ROWS - 1) / SC_ROWS);
  return DH_OK;
}

}  // namespace

extern "C" int dh_embed_normalize(const float* in, int64_t n, int32_t D, float* out, void* stream) {
  if (int rc = check_dims("dh_embed_normalize", n, D, 1)) return rc;
  if (n == 0) return DH_OK;
  DH_REQUIRE(in && out, "dh_embed_normalize: null in_dev or out_dev");
  DH_REQUIRE(aligned16(in) && aligned16(out), "dh_embed_normalize: in_dev / out_dev not 16-byte aligned");
  const int grid = (int)std::min<int64_t>((n + 3) / 4, 1 << 20);
  hipLaunchKernelGGL(embed_normalize_kernel, dim3(grid), dim3(256), 0, dh::as_stream(stream), in, n, D, out);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_embed_scores(const float* feat, int64_t n, int32_t D, const float* proto, int32_t K, float scale, float* scores,
                               void* stream) {
  if (int rc = check_dims("dh_embed_scores", n, D, K)) return rc;
  unsigned grid;
  if (int rc = sc_grid("dh_embed_scores", n, &grid)) return rc;
  if (n == 0) return DH_OK;
  DH_REQUIRE(feat && proto && scores, "dh_embed_scores: null feat_dev, proto_dev or scores_dev");
  DH_REQUIRE(aligned16(feat) && aligned16(proto), "dh_embed_scores: feat_dev / proto_dev not 16-byte aligned");
  hipLaunchKernelGGL(embed_scores_kernel, dim3(grid), dim3(256), 0, dh::as_stream(stream), feat, n, D, proto, K, scale, scores);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_embed_assign(const float* feat, int64_t n, int32_t D, const float* centres, int32_t K, int32_t k0, int32_t merge,
                               int32_t* label, float* dist, void* stream) {
  if (int rc = check_dims("dh_embed_assign", n, D, K)) return rc;
  DH_REQUIRE(k0 >= 0 && k0 <= 0x7fffffff - 64, "dh_embed_assign: k0 = %d out of range [0, 2^31 - 65]", k0);
  unsigned grid;
  if (int rc = sc_grid("dh_embed_assign", n, &grid)) return rc;
  if (n == 0) return DH_OK;
  DH_REQUIRE(feat && centres && label && dist, "dh_embed_assign: null feat_dev, centres_dev, label_dev or dist_dev");
  DH_REQUIRE(aligned16(feat) && aligned16(centres), "dh_embed_assign: feat_dev / centres_dev not 16-byte aligned");
  DH_REQUIRE((reinterpret_cast<uintptr_t>(label) & 3) == 0 && (reinterpret_cast<uintptr_t>(dist) & 3) == 0,
             "dh_embed_assign: label_dev / dist_dev not 4-byte aligned");
  hipStream_t st = dh::as_stream(stream);
  if (K <= AS_KC) {
    grid = (unsigned)((n + AS_ROWS - 1) / AS_ROWS);
    hipLaunchKernelGGL(embed_assign_rows_kernel, dim3(grid), dim3(256), 0, st, feat, n, D, centres, K, k0, merge, label, dist);
  } else {
    hipLaunchKernelGGL(embed_assign_kernel, dim3(grid), dim3(256), 0, st, feat, n, D, centres, K, k0, merge, label, dist);
  }
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int64_t dh_embed_class_work_size(int64_t n, int32_t D, int32_t K) {
  if (check_dims("dh_embed_class_work_size", n, D, K)) return -1;
  const int64_t n_chunks = (n + CHUNK - 1) / CHUNK;
  return std::max<int64_t>(4, n_chunks * K * ((int64_t)D + 1));   // partials float32[n_chunks][K][D], then counts int32[n_chunks][K]
}

extern "C" int dh_embed_class_sums(const float* feat, const int32_t* label, int64_t n, int32_t D, int32_t K, float* sums,
                                   int64_t* counts, float* work, void* stream) {
  if (int rc = check_dims("dh_embed_class_sums", n, D, K)) return rc;
  const int64_t n_chunks = (n + CHUNK - 1) / CHUNK;
  DH_REQUIRE(n_chunks <= 0x7fffffff, "dh_embed_class_sums: n = %lld exceeds one launch", (long long)n);
  DH_REQUIRE(sums && counts && work, "dh_embed_class_sums: null sums_dev, counts_dev or work_dev");
  DH_REQUIRE(n == 0 || (feat && label), "dh_embed_class_sums: null feat_dev or label_dev");
  hipStream_t st = dh::as_stream(stream);
  int32_t* chunk_count = reinterpret_cast<int32_t*>(work + n_chunks * K * D);
  if (n_chunks) {
    hipLaunchKernelGGL(embed_class_partial_kernel, dim3((unsigned)n_chunks, (D + 255) / 256), dim3(256), 0, st, feat, label, n, D, K,
                       work, chunk_count);
    DH_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(embed_class_final_kernel, dim3((K * D + 255) / 256), dim3(256), 0, st, work, chunk_count, n_chunks, D, K, sums,
                     counts);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int64_t dh_embed_scatter_work_size(int64_t n, int32_t D) {
  if (check_dims("dh_embed_scatter_work_size", n, D, 1)) return -1;
  return sk_batch(n, D) * sk_pairs(D) * (SK_T * SK_T);   // partials float32[chunks of a batch][pairs][64][64]
}

extern "C" int dh_embed_scatter(const float* feat, int64_t n, int32_t D, const float* mean, float* scatter, float* work,
                                void* stream) {
  if (int rc = check_dims("dh_embed_scatter", n, D, 1)) return rc;
  const int64_t n_chunks = (n + CHUNK - 1) / CHUNK;
  DH_REQUIRE(n_chunks <= 0x7fffffff, "dh_embed_scatter: n = %lld exceeds one launch", (long long)n);
  hipStream_t st = dh::as_stream(stream);
  if (n == 0) {   // needs no pointer; a matrix that is given becomes all zero
    if (!scatter) return DH_OK;
    DH_REQUIRE(aligned16(scatter), "dh_embed_scatter: scatter_dev not 16-byte aligned");
    DH_HIP(hipMemsetAsync(scatter, 0, sizeof(float) * (size_t)D * D, st));
    return DH_OK;
  }
  const int64_t batch = sk_batch(n, D);
  const bool direct = batch == 0;
  DH_REQUIRE(feat && mean && scatter, "dh_embed_scatter: null feat_dev, mean_dev or scatter_dev");
  DH_REQUIRE(direct || work, "dh_embed_scatter: null work_dev (dh_embed_scatter_work_size(n, D) floats)");
  DH_REQUIRE(aligned16(feat) && aligned16(mean) && aligned16(scatter) && (direct || aligned16(work)),
             "dh_embed_scatter: feat_dev / mean_dev / scatter_dev / work_dev not 16-byte aligned");
  const int n_pairs = (int)sk_pairs(D);   // <= 2080
  if (direct) {
    hipLaunchKernelGGL(embed_scatter_kernel, dim3(1, n_pairs), dim3(256), 0, st, feat, n, D, mean, n_chunks, (int64_t)0, 1, scatter);
    DH_LAUNCH_CHECK();
    return DH_OK;
  }
  for (int64_t ch0 = 0; ch0 < n_chunks; ch0 += batch) {
    const int64_t count = std::min(batch, n_chunks - ch0);
    hipLaunchKernelGGL(embed_scatter_kernel, dim3((unsigned)count, n_pairs), dim3(256), 0, st, feat, n, D, mean, n_chunks, ch0, 0, work);
    DH_LAUNCH_CHECK();
    hipLaunchKernelGGL(embed_scatter_fold_kernel, dim3(n_pairs), dim3(256), 0, st, work, count, D, ch0 == 0 ? 1 : 0, scatter);
    DH_LAUNCH_CHECK();
  }
  return DH_OK;
}

extern "C" int dh_embed_project(const float* feat, int64_t n, int32_t D, const float* mean, const float* comp, int32_t K,
                                const float* scale, float* out, int32_t ld, void* stream) {
  if (int rc = check_dims("dh_embed_project", n, D, K)) return rc;
  DH_REQUIRE(ld >= K && ld <= 4096 && ld % 4 == 0, "dh_embed_project: ld = %d unsupported (K = %d <= ld <= 4096, ld %% 4 == 0)", ld, K);
  unsigned grid;
  if (int rc = sc_grid("dh_embed_project", n, &grid)) return rc;
  if (n == 0) return DH_OK;
  DH_REQUIRE(feat && mean && comp && out, "dh_embed_project: null feat_dev, mean_dev, comp_dev or out_dev");
  DH_REQUIRE(aligned16(feat) && aligned16(mean) && aligned16(comp) && aligned16(out),
             "dh_embed_project: feat_dev / mean_dev / comp_dev / out_dev not 16-byte aligned");
  DH_REQUIRE((reinterpret_cast<uintptr_t>(scale) & 3) == 0, "dh_embed_project: scale_dev not 4-byte aligned");
  hipLaunchKernelGGL(embed_project_kernel, dim3(grid), dim3(256), 0, dh::as_stream(stream), feat, n, D, mean, comp, K, scale, out,
                     ld);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_embed_knn(const float* query, int64_t n, const float* bank, int64_t m, int32_t D, int32_t k, int64_t m0,
                            int32_t merge, int32_t* index, float* dist, void* stream) {
  if (int rc = check_dims("dh_embed_knn", n, D, 1)) return rc;
  DH_REQUIRE(k >= 1 && k <= 64, "dh_embed_knn: k = %d out of range [1, 64]", k);
  DH_REQUIRE(m >= 0, "dh_embed_knn: m = %lld is negative", (long long)m);
  DH_REQUIRE(m0 >= 0 && m <= 0x7fffffff && m0 <= 0x7fffffff - m, "dh_embed_knn: m0 + m = %lld + %lld exceeds 2^31 - 1 (m0 >= 0)",
             (long long)m0, (long long)m);
  DH_REQUIRE(n <= (int64_t)SC_ROWS * 0x7fffffff, "dh_embed_knn: n = %lld exceeds one launch", (long long)n);
  if (n == 0 || (m == 0 && merge)) return DH_OK;
  DH_REQUIRE(query && index && dist && (m == 0 || bank), "dh_embed_knn: null query_dev, bank_dev, index_dev or dist_dev");
  DH_REQUIRE(aligned16(query) && aligned16(bank), "dh_embed_knn: query_dev / bank_dev not 16-byte aligned");
  DH_REQUIRE((reinterpret_cast<uintptr_t>(index) & 3) == 0 && (reinterpret_cast<uintptr_t>(dist) & 3) == 0,
             "dh_embed_knn: index_dev / dist_dev not 4-byte aligned");
  const int64_t grid = (n + KN_ROWS - 1) / KN_ROWS;
  hipStream_t st = dh::as_stream(stream);
  if (k <= 16) {   // the short list leaves LDS for a third workgroup per CU
    hipLaunchKernelGGL(embed_knn_kernel<16>, dim3((unsigned)grid), dim3(256), 0, st, query, n, D, bank, m, k, (int)m0, merge, index, dist);
  } else {
    hipLaunchKernelGGL(embed_knn_kernel<64>, dim3((unsigned)grid), dim3(256), 0, st, query, n, D, bank, m, k, (int)m0, merge, index, dist);
  }
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_embed_knn_votes(const int32_t* index, int64_t n, int32_t k, const int32_t* bank_label, int64_t m, int32_t n_classes,
                                  int32_t* votes, int32_t* label, void* stream) {
  DH_REQUIRE(n >= 0 && n <= (int64_t)256 * 0x7fffffff, "dh_embed_knn_votes: n = %lld out of range", (long long)n);
  DH_REQUIRE(k >= 1 && k <= 64, "dh_embed_knn_votes: k = %d out of range [1, 64]", k);
  DH_REQUIRE(m >= 0 && m <= 0x7fffffff, "dh_embed_knn_votes: m = %lld out of range [0, 2^31 - 1]", (long long)m);
  DH_REQUIRE(n_classes >= 1 && n_classes <= 64, "dh_embed_knn_votes: n_classes = %d out of range [1, 64]", n_classes);
  if (n == 0) return DH_OK;
  DH_REQUIRE(index && votes && label && (m == 0 || bank_label),
             "dh_embed_knn_votes: null index_dev, bank_label_dev, votes_dev or label_dev");
  DH_REQUIRE(((reinterpret_cast<uintptr_t>(index) | reinterpret_cast<uintptr_t>(bank_label) | reinterpret_cast<uintptr_t>(votes) |
               reinterpret_cast<uintptr_t>(label)) & 3) == 0,
             "dh_embed_knn_votes: index_dev / bank_label_dev / votes_dev / label_dev not 4-byte aligned");
  hipLaunchKernelGGL(embed_knn_votes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, dh::as_stream(stream), index, n, k,
                     bank_label, m, n_classes, votes, label);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
