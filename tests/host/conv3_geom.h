// The geometry fields of Conv3Params, for the host programs that call the library's plan (deephisto_amd/csrc/conv3_plan_host.h) without HIP.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../deephisto_amd/csrc/conv3_plan_host.h"

struct Geom {
  int B, Hi, Wi, Cin, Ho, Wo, Cout;
  int in_px_bytes, in_chunk_bytes, out_px, out_cb, out_mt;
  int64_t o_img; int o_row, o_px, o_base;
  int cls_base[4];
  int out_pr, res_mt, res_pr, r_row, r_px, r_cb, r_base;   // output half-tile stride; the residual's own layout
  int TH, TW, IMGS, tiles_y, tiles_x, HR, HC, HP, HPH, WTAIL, FIT, IP, n_win_instr, ntiles, iters;
};

#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "VIOLATION %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); abort(); } } while (0)
