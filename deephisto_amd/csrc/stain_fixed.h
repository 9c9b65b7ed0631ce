// Fixed-point limits shared by the stain kernels (stain.hip) and the stain-jitter gather (gather.hip); the host's copies
// are in deephisto_amd/stain.py (OD_MAX, LUT_SIZE, COEF_MAX).
#pragma once
#include <stdint.h>

namespace dh_stain {
constexpr int kOdMax = 22713;              // round(ln(256) * 2^12): the largest table value the entries accept
constexpr int kLutMax = 24576;
constexpr int kCoefMax = 1 << 19;          // |fixed-point matrix entry|: 3 * 2^19 * kOdMax < 2^36
constexpr int kBiasMax = 1 << 30;          // |fixed-point bias| of the jitter: 3 * 2^19 * kOdMax + 2^30 < 2^37
}  // namespace dh_stain
