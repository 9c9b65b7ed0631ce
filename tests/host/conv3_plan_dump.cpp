// conv3_plan_dump: prints the launch plan the library chooses (deephisto_amd/csrc/conv3_plan_host.h) for every shape of the sweep's list
// (conv3_tables_sweep.cpp): one line per launch with the kernel variant, the tile geometry, n_win_instr, ntiles, grid, iters and the LDS bytes;
// for a merged stride-2 data gradient the class shares (first workgroup of each class set, its iterations).  A change to the host side of
// the 3x3 convolutions that means to leave every launch as it is shows that by an unchanged dump.
#include <string>

#include "conv3_geom.h"

using namespace dh_conv3;

static void print_launch(const Variant& v, const Geom& p, const Launch& ln) {
  printf("| v %d %d %d %d %d %d %d %d | tile %d %d %d %d %d %d %d %d %d %d %d | nwin %d ntiles %d grid %d iters %d lds %zu\n", v.stride, v.nt, v.mt, v.ds, v.wres, v.cls,
         v.half, v.m16, p.TH, p.TW, p.IMGS, p.tiles_y, p.tiles_x, p.HR, p.HC, p.HP, p.HPH, p.WTAIL, p.FIT, p.n_win_instr, p.ntiles, ln.grid, p.iters, ln.lds);
}

static void forward(int esz, int B, int Hi, int cin, int cout, int stride, bool blocked, bool out16 = false, bool wide = false, bool ds = true) {
  ConvShape s;
  s.esz = esz; s.B = B; s.Hi = s.Wi = Hi; s.cin = cin; s.cout = cout; s.stride = stride; s.Ho = s.Wo = (Hi + 2 - 3) / stride + 1;
  s.ds = stride == 2 && ds; s.blocked = blocked; s.in16 = wide; s.out16 = out16; s.wide_packed = wide;
  Geom p{};
  Variant v;
  Launch ln;
  printf("fwd esz %d B %d Hi %d %d->%d s%d blocked %d out16 %d wide %d ds %d ", esz, B, Hi, cin, cout, stride, blocked, out16, wide, s.ds);
  if (const char* why = plan_forward(s, Knobs{}, p, &v, &ln)) { printf("| refused: %s\n", why); return; }
  print_launch(v, p, ln);
}

static void dgrad(int esz, int B, int side, int cin, int cout) {
  const int Ho = (side + 2 - 3) / 2 + 1;
  DgradPlan<Geom> dp{};
  printf("dgrad esz %d B %d side %d %d->%d ", esz, B, side, cin, cout);
  if (const char* why = plan_dgrad_s2(esz, B, Ho, Ho, side, side, cout, cin, &dp)) { printf("| refused: %s\n", why); return; }
  if (dp.v.cls == 4) { print_launch(dp.v, dp.p[0], dp.ln[0]); return; }
  int first[5] = {0, 0, 0, 0, 0}, k0 = 0;
  for (int k = 0; k < 4; ++k) { first[k + 1] = first[k] + dp.wg[k]; if (dp.wg[k] > 0 && dp.wg[k0] == 0) k0 = k; }
  const Geom& p = dp.p[k0];
  printf("| merged nt %d mt %d | tile %d %d %d %d %d %d | nwin %d grid %d lds %zu | first %d %d %d %d iters %d %d %d %d\n", dp.v.nt, dp.v.mt, p.TH, p.TW, p.IMGS, p.HR, p.HC, p.HP,
         p.n_win_instr, first[4], dp.ln[k0].lds, first[0], first[1], first[2], first[3], dp.p[0].iters, dp.p[1].iters, dp.p[2].iters, dp.p[3].iters);
}

int main() {
  struct L { int cin, cout, stride, shift; };
  const L layers[] = {{64, 64, 1, 0}, {64, 128, 2, 0}, {128, 128, 1, 1}, {128, 256, 2, 1}, {256, 256, 1, 2}, {256, 512, 2, 2}, {512, 512, 1, 3}};
  for (int P : {32, 64, 96, 100, 200, 224, 256, 330, 512, 1024}) {
    const int H1 = (P + 6 - 7) / 2 + 1, H2 = (H1 + 2 - 3) / 2 + 1;
    for (const L& ly : layers) {
      int Hi = H2;
      for (int s = 0; s < ly.shift; ++s) Hi = (Hi + 2 - 3) / 2 + 1;
      for (int n : {1, 3, 64, 1024, 3842, 4096}) {
        forward(2, n, Hi, ly.cin, ly.cout, ly.stride, true);
        if (ly.stride == 1) forward(2, n, Hi, ly.cin, ly.cout, 1, true, true);
        if (ly.stride == 2 && ly.cout % 128 == 0 && (Hi + 2 - 3) / 2 + 1 > 4) forward(2, n, Hi, ly.cin, ly.cout, 2, true, false, true);
        forward(2, n, Hi, ly.cin, ly.cout, ly.stride, false);
        if (n <= 1024) forward(4, n, Hi, ly.cin, ly.cout, ly.stride, false);
      }
    }
  }
  forward(4, 2600, 64, 64, 64, 1, false);   // the float32 launch whose layer-1 map lies between 2^31 and 2^32 bytes
  for (int Hi : {56, 28, 14, 7})
    for (int c : {64, 128, 256, 512}) {
      forward(2, 64, Hi, c, c, 1, false);
      if (Hi > 7) forward(2, 64, Hi, c, c, 2, false, false, false, false);
    }
  for (int side : {7, 8, 9, 14, 15, 28, 56})
    for (int B : {1, 3, 40, 64})
      for (int cin : {64, 128, 256})
        for (int esz : {2, 4}) dgrad(esz, B, side, cin, 2 * cin);
  return 0;
}
