// q1: the tile quality rule, in plain C++ that compiles for the host and for the device: the kernels of
// quality.hip and the stand-alone program tests/helpers/quality_rule_check.cc evaluate this text.  Integers only.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define QR_HD __host__ __device__ inline
#else
#define QR_HD inline
#endif

namespace qr {

constexpr int kMaxPatch = 1024;                  // tile side the int64 decision below is proven for
constexpr int64_t kMaxSharpness = 1020 * 1020;   // |L| <= 4 * 255: the variance of L is at most 1 040 400
constexpr uint8_t kBlur = 2, kInk = 4;           // bits of the reason mask

QR_HD int imax(int a, int b) { return a > b ? a : b; }
QR_HD int imin(int a, int b) { return a < b ? a : b; }

// BT.601 luma in 8 fractional bits, rounded: (77 + 150 + 29) * 255 + 128 = 65 408, so Y lies in 0..255
QR_HD int luma(int r, int g, int b) { return (77 * r + 150 * g + 29 * b + 128) >> 8; }

QR_HD int chroma(int r, int g, int b) { return imax(r, imax(g, b)) - imin(r, imin(g, b)); }

// the tissue filter's own rule; t = -1 makes every pixel tissue
QR_HD bool tissue(int r, int g, int b, int t) { return chroma(r, g, b) > t; }

// saturated with green not the smallest channel (blue or green marker; H&E pink and purple both have green smallest), or very
// dark (black marker, a fold); dark_max = -1 switches the dark clause off
QR_HD bool ink(int r, int g, int b, int ink_chroma, int ink_margin, int dark_max) {
  return (chroma(r, g, b) > ink_chroma && g - imin(r, b) >= ink_margin) || imax(r, imax(g, b)) <= dark_max;
}

// Reason mask of a tile from its four sums: n_t tissue pixels, S1 = sum of L and S2 = sum of L*L over them, n_ink ink pixels.
// Blur is "variance of L over the tissue pixels < min_sharpness", cross-multiplied by n_t^2 so that nothing is divided.
// With P <= 1024: n_t <= 2^20, |S1| <= 1020 * 2^20, S2 <= 1020^2 * 2^20 and min_sharpness <= 1020^2, so each of n_t*S2, S1*S1 and
// min_sharpness*n_t*n_t is at most 2^20 * 1020^2 * 2^20 ~ 1.14e18 < 2^63 ~ 9.22e18, and n_t*S2 - S1*S1 >= 0 (Cauchy-Schwarz):
// the comparison is plain int64.  A tile without a tissue pixel has no variance: it counts as blurred iff min_sharpness > 0.
QR_HD uint8_t reason(int64_t n_t, int64_t S1, int64_t S2, int64_t n_ink, int64_t min_sharpness, int64_t max_ink_pixels) {
  const bool blur = n_t == 0 ? min_sharpness > 0 : n_t * S2 - S1 * S1 < min_sharpness * n_t * n_t;
  return (uint8_t)((blur ? kBlur : 0) | (n_ink > max_ink_pixels ? kInk : 0));
}

}  // namespace qr
