// n3: the eight dihedral views of the resident slide, for test-time augmentation.
//
// Semantics (the header states the same): view = k + 4 f, k in 0..3, f in 0..1,
//   dst = np.rot90(np.fliplr(src) if f else src, k)          over axes (0, 1); the channel triple is never reordered
// dst is [h][w][3] for even k and [w][h][3] for odd k.  Every destination byte is a source byte: no arithmetic, no float, no
// atomics; all byte offsets are 64-bit.
//
// Every element of D4 is an optional transpose followed by an optional reversal of the rows and an optional reversal of the
// columns (kOps below), so there is one kernel with the transpose as a template parameter; the two reversals enter only the
// position of the destination tile and the order of the pixels inside it.  A workgroup moves one tile of kTile x kTile source
// pixels through LDS.  Load, as resample.hip: one 16-byte load per lane by memcpy, neighbouring lanes on neighbouring chunks of
// a tile row (rows of a slide start at any byte, so this is an unaligned global_load_dwordx4); a chunk that would reach past
// the end of the source is read by bytes.  The tile's row pitch in LDS is kPitch = 196 bytes = 49 dwords: in the transposing
// instantiation the lanes of a wave walk a column of the tile, and an odd number of dwords puts consecutive rows on different
// banks (192 = 48 dwords would repeat the bank every fourth row: a 16-way conflict).  Store, as resample.hip: every
// destination row segment is built in an LDS image at the phase of its destination address and leaves with aligned 16-byte
// stores, byte stores at the two ragged ends.
#include "dh_common.h"

namespace {

// the tiling constants; deephisto_amd/tta.py repeats them (TILE, THREADS, STORE_GROUP, LDS_PITCH) for the tests
constexpr int kThreads = 256;
constexpr int kTile = 64;                                 // pixels a side
constexpr int kChunk = 16;                                // bytes per load and per aligned store
constexpr int kRowBytes = 3 * kTile;                      // 192
constexpr int kRowChunks = kRowBytes / kChunk;            // 12 loads per tile row
constexpr int kPitch = kRowBytes + 4;                     // 196: an odd number of dwords
constexpr int kImgChunks = kRowChunks + 1;                // a row segment at phase 0..15 spans at most 13 aligned groups
constexpr int kImgPitch = kImgChunks * kChunk;            // 208
constexpr int64_t kMaxSide = 1 << 20;                     // resample.MAX_SIDE
static_assert(kRowBytes % kChunk == 0 && (kPitch / 4) % 2 == 1 && kPitch % 4 == 0, "tile row: whole chunks, odd dword pitch");
static_assert((kTile * kTile) % kThreads == 0 && kThreads % kTile == 0, "a wave fills one destination row of the tile");

// view -> transpose, reverse rows, reverse columns (applied in that order)
constexpr int kOps[8][3] = {{0, 0, 0}, {1, 1, 0}, {0, 1, 1}, {1, 0, 1}, {0, 0, 1}, {1, 0, 0}, {0, 1, 0}, {1, 1, 1}};

template <bool kTranspose>
__global__ __launch_bounds__(kThreads) void dihedral_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int32_t h,
                                                            int32_t w, int32_t rev_rows, int32_t rev_cols) {
  __shared__ __attribute__((aligned(16))) uint8_t s_tile[kTile * kPitch];
  __shared__ __attribute__((aligned(16))) uint8_t s_img[kTile * kImgPitch];
  __shared__ int32_t s_phase[kTile];
  const int t = threadIdx.x;
  const int tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;
  const int tw = min(kTile, w - tx0), th = min(kTile, h - ty0);          // the source tile: th rows of tw pixels
  const int64_t pitch = 3 * (int64_t)w, total = pitch * h;
  const int nb = 3 * tw;                                                 // bytes of a source tile row

  // ---- source tile -> s_tile
  for (int q = t; q < kTile * kRowChunks; q += kThreads) {
    const int r = q / kRowChunks, cb = kChunk * (q - r * kRowChunks);
    if (r >= th || cb >= nb) continue;
    const int64_t off = (int64_t)(ty0 + r) * pitch + 3 * (int64_t)tx0 + cb;
    uint8_t* to = &s_tile[r * kPitch + cb];
    if (off + kChunk <= total) {                                         // whole chunk inside the source (it may run past the tile)
      uint32_t v[4];
      __builtin_memcpy(v, src + off, kChunk);
#pragma unroll
      for (int m = 0; m < 4; ++m) reinterpret_cast<uint32_t*>(to)[m] = v[m];
    } else {                                                             // cut by the end of the last source row
      const int n = min(kChunk, nb - cb);
      for (int b = 0; b < n; ++b) to[b] = src[off + b];
    }
  }

  // ---- the destination tile: nr rows of nc pixels at (drow0, dcol0) of the [dh][dw][3] destination
  const int nr = kTranspose ? tw : th, nc = kTranspose ? th : tw;
  const int dh = kTranspose ? w : h, dw = kTranspose ? h : w;
  const int r0 = kTranspose ? tx0 : ty0, c0 = kTranspose ? ty0 : tx0;
  const int drow0 = rev_rows ? dh - (r0 + nr) : r0, dcol0 = rev_cols ? dw - (c0 + nc) : c0;
  const int64_t opitch = 3 * (int64_t)dw;
  uint8_t* const tile_out = dst + (int64_t)drow0 * opitch + 3 * (int64_t)dcol0;
  if (t < nr) s_phase[t] = (int)((uintptr_t)(tile_out + (int64_t)t * opitch) & (kChunk - 1));
  __syncthreads();

  // ---- pixels into the row images: a wave fills one destination row, lane = destination column
  const int dc = t & (kTile - 1);
  for (int dr = t / kTile; dr < nr; dr += kThreads / kTile) {
    if (dc >= nc) continue;
    const int a = rev_rows ? nr - 1 - dr : dr, b = rev_cols ? nc - 1 - dc : dc;     // the pixel of the (transposed) source tile
    const uint8_t* px = &s_tile[kTranspose ? b * kPitch + 3 * a : a * kPitch + 3 * b];
    uint8_t* o = &s_img[dr * kImgPitch + s_phase[dr] + 3 * dc];
    const uint8_t p0 = px[0], p1 = px[1], p2 = px[2];
    o[0] = p0; o[1] = p1; o[2] = p2;
  }
  __syncthreads();

  // ---- images -> destination: byte k of row dr's image goes to its row start - phase + k; groups of 16 are aligned at both ends
  for (int q = t; q < nr * kImgChunks; q += kThreads) {
    const int dr = q / kImgChunks, k = kChunk * (q - dr * kImgChunks);
    const int phase = s_phase[dr], end = phase + 3 * nc;
    if (k >= end) continue;
    uint8_t* out = tile_out + (int64_t)dr * opitch - phase + k;
    const uint8_t* img = &s_img[dr * kImgPitch + k];
    if (k >= phase && k + kChunk <= end) {
      *reinterpret_cast<uint4*>(out) = *reinterpret_cast<const uint4*>(img);
    } else {
      for (int b = max(k, phase); b < min(k + kChunk, end); ++b) out[b - k] = img[b - k];
    }
  }
}

}  // namespace

extern "C" int dh_slide_dihedral(const uint8_t* src_dev, int64_t h, int64_t w, int32_t view, uint8_t* dst_dev, void* stream) {
  DH_REQUIRE(src_dev && dst_dev, "slide_dihedral: null pointer");
  DH_REQUIRE(view >= 0 && view < 8, "slide_dihedral: view %d outside 0..7", view);
  DH_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "slide_dihedral: bad slide size %lld x %lld (sides in [1, %lld])",
             (long long)h, (long long)w, (long long)kMaxSide);
  const uintptr_t a = (uintptr_t)src_dev, b = (uintptr_t)dst_dev, n = (uintptr_t)(3 * h * w);
  DH_REQUIRE(a + n <= b || b + n <= a, "slide_dihedral: dst must not overlap src");
  const dim3 grid((unsigned)((w + kTile - 1) / kTile), (unsigned)((h + kTile - 1) / kTile));   // at most 16 384 a side
  const int* op = kOps[view];
  if (op[0])
    hipLaunchKernelGGL(dihedral_kernel<true>, grid, dim3(kThreads), 0, dh::as_stream(stream), src_dev, dst_dev, (int32_t)h, (int32_t)w,
                       op[1], op[2]);
  else
    hipLaunchKernelGGL(dihedral_kernel<false>, grid, dim3(kThreads), 0, dh::as_stream(stream), src_dev, dst_dev, (int32_t)h, (int32_t)w,
                       op[1], op[2]);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
