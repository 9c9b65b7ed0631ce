// Shared host-side helpers for libdeephisto_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

#include "../../include/deephisto_hip.h"
#include "../../include/deephisto_hip_debug.h"   // test hooks: exported, unversioned

namespace dh {

void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Run-time switches: the table of env_knobs.h is the only way the library reads the environment (besides DH_RCCL_LIB, a path).
// env_int: the variable's value, or the knob's default when unset or unparsable (then recorded: env_check fails from then on).
// env_check: validates EVERY knob of the table now; DH_EINVAL + dh_last_error() naming the first bad variable.  Called by the
// create entry points, so a mistyped value stops a run before its first kernel instead of being atoi'd into something else.
int env_int(const char* name);
int env_check();

// Bin plan of the ordered canvas accumulations (tile_kernels.hip, proba.hip).  The canvas is cut into bins of G x G cells,
// G = max(1, min(P/d, 64)); bin b's covering tiles, in list order, are d_tiles[d_start[b] .. d_start[b+1]).  bin_plan builds the
// plan of (yx_host, P, d, h, w), or returns the cached one when the last call on this thread and device had the same arguments
// (no rebuild, no upload, no synchronisation).  The device arrays stay valid until the next call that misses the cache, which
// synchronises `st` before it frees them.
struct BinPlan { int32_t G, bins_x; int64_t nbins, total; const int32_t *d_start, *d_tiles, *d_yx; };
struct BinGeom { int32_t G, bins_x, dh, dw, n_cls, P, d; };
int bin_plan(const int32_t* yx_host, int64_t n, int32_t P, int32_t d, int64_t h, int64_t w, hipStream_t st, BinPlan* out);

// Row of a class activation map (float32 [n][S * S][n_cls], S = P / 32) that tile t at origin (y, x) contributes to canvas cell
// (cy, cx), a cell the tile covers: position i = ceil(((cy + 1) d - y) / 32) - 1 along y and j likewise along x, the one position
// whose 32-pixel sub-tile owns the cell.  (cy + 1) d <= h, so 32-bit arithmetic holds up to CAM_MAX_SIDE.
constexpr int64_t CAM_MAX_SIDE = INT32_MAX - 64;
__host__ __device__ inline int64_t cam_row(int64_t t, int S, int d, int cy, int cx, int y, int x) {
  const int i = ((cy + 1) * d - y + 31) / 32 - 1, j = ((cx + 1) * d - x + 31) / 32 - 1;
  return (t * S + i) * S + j;
}

}  // namespace dh

#define DH_REQUIRE(cond, ...)            \
  do {                                   \
    if (!(cond)) {                       \
      dh::set_error(__VA_ARGS__);        \
      return DH_EINVAL;                  \
    }                                    \
  } while (0)

#define DH_HIP(call)                                                              \
  do {                                                                            \
    hipError_t e_ = (call);                                                       \
    if (e_ != hipSuccess) {                                                       \
      dh::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      return e_ == hipErrorOutOfMemory ? DH_ENOMEM : DH_EHIP;                     \
    }                                                                             \
  } while (0)

#define DH_LAUNCH_CHECK()                                                         \
  do {                                                                            \
    hipError_t e_ = hipGetLastError();                                            \
    if (e_ != hipSuccess) {                                                       \
      dh::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
      return DH_EHIP;                                                             \
    }                                                                             \
  } while (0)
