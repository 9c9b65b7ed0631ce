// conv3_plan_probe esz B Hi cin cout stride blocked out16 wide ds -> one line in the format of conv3_plan_dump.cpp's print_launch: the launch the
// library plans (deephisto_amd/csrc/conv3_plan_host.h, plan_forward) for ONE forward 3x3 convolution, so that a test can check that its
// launch sizes reach the kernel variant and tile shape it means (tests/test_layer_reference_host.py).
#include "conv3_geom.h"

using namespace dh_conv3;

int main(int argc, char** argv) {
  if (argc != 11) { std::fprintf(stderr, "usage: %s esz B Hi cin cout stride blocked out16 wide ds\n", argv[0]); return 2; }
  int a[10];
  for (int i = 0; i < 10; ++i) a[i] = std::atoi(argv[i + 1]);
  ConvShape s;
  s.esz = a[0]; s.B = a[1]; s.Hi = s.Wi = a[2]; s.cin = a[3]; s.cout = a[4]; s.stride = a[5]; s.Ho = s.Wo = (s.Hi + 2 - 3) / s.stride + 1;
  s.blocked = a[6] != 0; s.out16 = a[7] != 0; s.in16 = a[8] != 0; s.wide_packed = a[8] != 0; s.ds = s.stride == 2 && a[9] != 0;
  Geom p{};
  Variant v;
  Launch ln;
  if (const char* why = plan_forward(s, Knobs{}, p, &v, &ln)) { std::printf("| refused: %s\n", why); return 0; }
  std::printf("| v %d %d %d %d %d %d %d %d | tile %d %d %d %d %d %d %d %d %d %d %d | nwin %d ntiles %d grid %d iters %d lds %zu\n", v.stride, v.nt, v.mt, v.ds, v.wres,
              v.cls, v.half, v.m16, p.TH, p.TW, p.IMGS, p.tiles_y, p.tiles_x, p.HR, p.HC, p.HP, p.HPH, p.WTAIL, p.FIT, p.n_win_instr, p.ntiles, ln.grid, p.iters, ln.lds);
  return 0;
}
