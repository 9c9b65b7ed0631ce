// Stand-alone host program over deephisto_amd/csrc/quality_rule.h (the text the kernels of quality.hip evaluate), built by
// tests/test_quality_host.py with -fsanitize=address,undefined.  It prints
//   "P r g b luma chroma tissue ink" per pixel of the lattice (tissue and ink under the parameters of the command line), then
//   "T n_t S1 S2 n_ink min_sharpness max_ink reason" per tile case read from stdin (six integers a line),
// which the test compares with the NumPy restatement.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../deephisto_amd/csrc/quality_rule.h"

int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: %s step threshold ink_chroma ink_margin dark_max < tile cases\n", argv[0]);
    return 2;
  }
  const int step = atoi(argv[1]), t = atoi(argv[2]), ink_chroma = atoi(argv[3]), ink_margin = atoi(argv[4]), dark_max = atoi(argv[5]);
  if (step < 1) return 2;
  // the coarse lattice 0, step, 2 step, ... plus 255 on every axis: the corners of the cube are in it
  int axis[258], n = 0;
  for (int v = 0; v < 255; v += step) axis[n++] = v;
  axis[n++] = 255;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      for (int k = 0; k < n; ++k) {
        const int r = axis[i], g = axis[j], b = axis[k];
        printf("P %d %d %d %d %d %d %d\n", r, g, b, qr::luma(r, g, b), qr::chroma(r, g, b), (int)qr::tissue(r, g, b, t),
               (int)qr::ink(r, g, b, ink_chroma, ink_margin, dark_max));
      }
  long long v[6];
  while (scanf("%lld %lld %lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) == 6)
    printf("T %lld %lld %lld %lld %lld %lld %d\n", v[0], v[1], v[2], v[3], v[4], v[5],
           (int)qr::reason(v[0], v[1], v[2], v[3], v[4], v[5]));
  return 0;
}
