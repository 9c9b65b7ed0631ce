// Pictures of the whole-slide maps for MI355X (gfx950, wave64): HBM-bound byte work, float64 where NumPy computes in float64.
//   dh_colorize_map   class map -> RGB through a colour table
//   dh_overlay_blend  a coloured map blended over the slide
//   dh_heatmap_blend  a scalar field times a colour blended over the slide
#include <algorithm>

#include "dh_common.h"

// Visualisation of the class map (examples/predict_full_patched.py:81-113).
namespace {
__global__ __launch_bounds__(256) void colorize_kernel(const int64_t* __restrict__ map, int64_t n, const uint8_t* __restrict__ lut,
                                                       int n_cls, uint8_t* __restrict__ rgb) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = map[i];
    uint8_t r = 0, g = 0, b = 0;
    if (c >= 0 && c < n_cls) { r = lut[3 * c]; g = lut[3 * c + 1]; b = lut[3 * c + 2]; }
    rgb[3 * i] = r; rgb[3 * i + 1] = g; rgb[3 * i + 2] = b;
  }
}
__global__ __launch_bounds__(256) void overlay_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ col, int64_t n,
                                                      double alpha, uint8_t* __restrict__ out) {
  const double beta = 1.0 - alpha;   // NumPy evaluates (1 - alpha) in float64 first
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (uint8_t)((double)img[i] * alpha + (double)col[i] * beta);   // values are in [0, 255]: the cast truncates
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
}  // namespace

extern "C" int dh_colorize_map(const int64_t* map, int64_t n, const uint8_t* lut, int32_t n_cls, uint8_t* rgb, void* stream) {
  DH_REQUIRE(n >= 0 && n_cls >= 0, "colorize: bad sizes");
  if (n == 0) return DH_OK;
  DH_REQUIRE(map && rgb && (lut || n_cls == 0), "colorize: null pointer");
  hipLaunchKernelGGL(colorize_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 65535)), dim3(256), 0, dh::as_stream(stream),
                     map, n, lut, n_cls, rgb);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_overlay_blend(const uint8_t* img, const uint8_t* col, int64_t n, double alpha, uint8_t* out, void* stream) {
  DH_REQUIRE(n >= 0 && alpha >= 0.0 && alpha <= 1.0, "overlay: bad arguments");
  if (n == 0) return DH_OK;
  DH_REQUIRE(img && col && out, "overlay: null pointer");
  hipLaunchKernelGGL(overlay_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 65535)), dim3(256), 0, dh::as_stream(stream),
                     img, col, n, alpha, out);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

extern "C" int dh_heatmap_blend(const uint8_t* img, const float* field, int64_t field_stride, int64_t n_cells,
                                const uint8_t* color, double alpha, uint8_t* out, void* stream) {
  DH_REQUIRE(n_cells >= 0, "heatmap blend: n_cells=%lld is negative", (long long)n_cells);
  DH_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "heatmap blend: alpha=%g outside [0, 1]", alpha);
  DH_REQUIRE(field_stride >= 1, "heatmap blend: field_stride=%lld must be >= 1", (long long)field_stride);
  DH_REQUIRE(color, "heatmap blend: null pointer (color)");
  if (n_cells == 0) return DH_OK;
  DH_REQUIRE(img && field && out, "heatmap blend: null pointer (img, field, out)");
  hipLaunchKernelGGL(heatmap_kernel, dim3((unsigned)std::min<int64_t>((n_cells + 255) / 256, 256 * 16)), dim3(256), 0,
                     dh::as_stream(stream), img, field, field_stride, n_cells, (double)color[0], (double)color[1], (double)color[2],
                     alpha, out);
  DH_LAUNCH_CHECK();
  return DH_OK;
}
