// pick_stride1_probe B Ho Wo cout min_tiles -> "th tw imgs variant tiles": the tile shape the stride-1 3x3 kernel's host code
// (deephisto_amd/csrc/conv3_tables_host.h) picks for a launch, so that a test can check that its shapes reach the variant it means
// (tests/test_layer_reference_host.py).
#include <cstdio>
#include <cstdlib>

#include "../../deephisto_amd/csrc/conv3_tables_host.h"

int main(int argc, char** argv) {
  if (argc != 6) { std::fprintf(stderr, "usage: %s B Ho Wo cout min_tiles\n", argv[0]); return 2; }
  const int B = std::atoi(argv[1]), Ho = std::atoi(argv[2]), Wo = std::atoi(argv[3]), cout = std::atoi(argv[4]), min_tiles = std::atoi(argv[5]);
  const dh_conv3::Cand c = dh_conv3::pick_stride1(B, Ho, Wo, cout, min_tiles);
  std::printf("%d %d %d %d %d\n", c.th, c.tw, c.imgs, c.variant, dh_conv3::tiles_of(c, B, Ho, Wo, cout));
  return 0;
}
