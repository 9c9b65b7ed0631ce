// conv3_plan_host.h -- HOST-ONLY launch plan of the 3x3 convolution kernels (conv3x3.inc): from a layer shape to the kernel variant, the
// geometry block of Conv3Params, the launch numbers and the key of the table cache.  No HIP, no environment (knobs are arguments):
// conv3x3_launch.inc calls it for the product, tests/host/ calls the same functions under sanitizers and prints the plans.
// `P`: any struct with the geometry fields of Conv3Params (tests/host/conv3_geom.h).  A plan function fills them and returns nullptr, or
// the reason the shape is refused; pointers, relu, stamps and the tables are the caller's.
#pragma once
#include <cstddef>

#include "conv3_tables_host.h"

namespace dh_conv3 {

constexpr int kSlabTapBytes = 4096;     // weights of one tap of one channel stage (SLAB_TAP)
constexpr int kLdsBytes = 160 * 1024;
constexpr int kGridMax = 256;           // one persistent workgroup per CU; also the tile count a tile shape must reach to be picked

inline bool operator==(const Variant& a, const Variant& b) {
  return a.stride == b.stride && a.nt == b.nt && a.mt == b.mt && a.ds == b.ds && a.wres == b.wres && a.cls == b.cls && a.half == b.half && a.m16 == b.m16;
}
inline Variant stride1_variant(const Cand& c) { Variant v; v.nt = c.variant == 0 ? 2 : 1; v.mt = c.variant == 2 ? 1 : 2; return v; }
inline int tile_variant(const Variant& v) { return v.nt == 2 ? 0 : v.mt == 2 ? 1 : 2; }   // Cand::variant of a stride-1 launch

struct Launch { int ncb = 0, grid = 0; size_t lds = 0; };   // cout blocks, workgroups, dynamic LDS bytes (n_win_instr, ntiles and iters live in P)

// 2-deep ring of [weight slab | window] (wres: all weight slabs once + ring of windows) + [2][scale | shift (| ds scale | ds shift)]
template <class P> inline size_t lds_bytes(const Variant& v, int esz, const P& p) {
  const int stage_px_bytes = v.half ? kChunkBytes / 2 : kChunkBytes;
  const size_t win_alloc = ((size_t)(p.IMGS * p.HR * p.HP + p.WTAIL) * stage_px_bytes + 1023) & ~(size_t)1023;
  const size_t wslab = (size_t)(9 + v.ds) * kSlabTapBytes, nchunks = (size_t)p.Cin * esz / stage_px_bytes;
  return (v.wres ? nchunks * wslab + 2 * win_alloc : 2 * (wslab + win_alloc)) + (v.half ? 4096 : v.ds ? 2048 : 1024);
}
template <class P> inline bool resident_weights_fit(Variant v, int esz, const P& p) { v.wres = 1; return lds_bytes(v, esz, p) <= (size_t)kLdsBytes; }

// The launch numbers of a geometry: n_win_instr, ntiles, iters into `p`, the rest into `ln`.  `grid_override` > 0: its share of a merged launch.
template <class P> const char* launch_numbers(const Variant& v, int esz, P& p, int grid_override, Launch* ln) {
  const int win_px = p.IMGS * p.HR * p.HP + p.WTAIL, slots = (v.half ? kWaves / 2 : kWaves * v.mt / 2) * v.nt * 32;
  ln->lds = lds_bytes(v, esz, p);
  p.n_win_instr = v.half ? (win_px + 31) / 32 : (win_px + 15) / 16;
  if (p.n_win_instr > max_window_pieces(v.stride, v.nt) * kWaves) return "conv3x3: staging window too large for the DMA plan";
  if (ln->lds > (size_t)kLdsBytes) return "conv3x3: LDS budget exceeded";
  if (p.FIT ? p.IMGS * p.TH * p.TW > slots || v.stride != 1 || v.half : p.IMGS * p.TH * p.TW != slots) return "conv3x3: tile/pixel mismatch";
  if (p.Cin * esz < 2 * kChunkBytes) return "conv3x3: needs at least two channel chunks";
  ln->ncb = p.Cout / (v.half ? 128 : 64);
  p.ntiles = ((p.B + p.IMGS - 1) / p.IMGS) * p.tiles_y * p.tiles_x * ln->ncb;
  if (p.ntiles < 1) return "conv3x3: empty launch";
  ln->grid = grid_override > 0 ? grid_override : std::min(kGridMax, p.ntiles);
  if (v.wres && ln->grid % (p.Cout / 64) != 0) return "conv3x3: resident weights need a fixed cout block per workgroup";
  p.iters = (p.ntiles + ln->grid - 1) / ln->grid;
  return nullptr;
}

// The key of the table cache: everything build_tables reads (conv3_tables_host.h lists the fields of `P`; out_px rides along), fixed size.
using TableKey = std::array<int, 42>;
template <class P> inline TableKey table_key(const Variant& v, int esz, const P& p, int ncb, int grid_override) {
  return {v.stride, v.nt, v.mt, v.half, v.m16, esz, ncb, grid_override,
          p.TH, p.TW, p.IMGS, p.HR, p.HC, p.HP, p.HPH, p.WTAIL, p.FIT, p.IP, p.Hi, p.Wi, p.Cin, p.B, p.tiles_y, p.tiles_x, p.n_win_instr, p.in_px_bytes,
          p.Ho, p.Wo, p.Cout, p.out_px, p.out_cb, (int)(p.o_img & 0x7FFFFFFF), (int)(p.o_img >> 31), p.o_row, p.o_px, p.o_base,
          p.r_row, p.r_px, p.r_cb, p.r_base, p.ntiles, p.iters};
}

template <class P> inline void residual_like_output(P& p) {
  p.out_pr = 16; p.res_mt = p.out_mt; p.res_pr = 16; p.r_row = p.o_row; p.r_px = p.o_px; p.r_cb = p.out_cb; p.r_base = p.o_base;
}
template <class P> inline void set_nhwc(P& p, int esz) {
  p.in_px_bytes = p.Cin * esz; p.in_chunk_bytes = kChunkBytes;
  p.out_px = p.Cout; p.out_mt = 32; p.out_cb = 64;
}

struct ConvShape {
  int esz, B, Hi, Wi, cin, cout, stride, Ho, Wo;
  bool ds = false, blocked = false;   // the block's 1x1 / stride-2 downsample rides along; [image][C/32][H][W][32] (bf16 inference), not NHWC
  bool in16 = false, out16 = false;   // ... with the input / the output in 16-channel planes [image][C/16][H][W][16]
  bool wide_packed = false;           // the weights of the conv and of its downsample exist in the wide stride-2 kernel's packing
};
struct Knobs { bool fit = true, s2_wide = true, mfma16 = true; };   // DH_CONV_FIT, DH_CONV_S2_WIDE, DH_CONV_MFMA16

// MFMA shape of a stride-1 bf16 layer (conv3x3.inc, M16): 16x16x32 where the per-layer A/B wins (profiles/conv_mfma16.txt): 64 -> 64, 256 -> 256 and
// 512 -> 512.  A function of the channel counts ONLY -- never of B, H, W or the tile variant: one layer gives the same bits at every launch size.
inline bool conv3_mfma16_layer(int cin, int cout, bool knob) { return knob && cin == cout && (cin == 64 || cin == 256 || cin == 512); }

// Will a 3x3 / stride-2 conv + fused downsample (output width Wo) run on the wide kernel (conv3x3.inc, HALF)?  Then the conv before it must
// write its INPUT in 16-channel planes.
inline bool s2_wide_eligible(bool knob, int esz, int cout, int Wo, bool wide_packed) { return knob && esz == 2 && wide_packed && cout % 128 == 0 && Wo > 4; }

// A forward convolution (a stride-1 data gradient is one): layouts, tile geometry, variant, launch numbers.  `force`: this stride-1 tile
// candidate instead of the picked one (the sweep runs them all).
template <class P> const char* plan_forward(const ConvShape& s, const Knobs& k, P& p, Variant* v, Launch* ln, const Cand* force = nullptr) {
  if (!s.blocked && (s.in16 || s.out16)) return "conv3x3: 16-channel planes are a variant of the channel-blocked layout";
  if (s.blocked && s.esz != 2) return "conv3x3: the channel-blocked layout is the bf16 inference layout";
  const int Ho = s.Ho, Wo = s.Wo;
  p.B = s.B; p.Hi = s.Hi; p.Wi = s.Wi; p.Cin = s.cin; p.Cout = s.cout; p.Ho = Ho; p.Wo = Wo;
  if (s.blocked) {
    p.in_px_bytes = kChunkBytes; p.in_chunk_bytes = s.Hi * s.Wi * kChunkBytes;
    p.out_px = 32; p.out_mt = Ho * Wo * 32; p.out_cb = 2 * p.out_mt;
  } else {
    set_nhwc(p, s.esz);
  }
  p.o_img = (int64_t)Ho * Wo * s.cout; p.o_row = Wo * p.out_px; p.o_px = p.out_px; p.o_base = 0;
  residual_like_output(p);
  // ... unless this conv writes 16-channel planes for the wide stride-2 kernel that follows; the residual stays in 32-channel planes
  if (s.out16) {
    p.out_px = 16; p.out_pr = Ho * Wo * 16; p.out_mt = 2 * p.out_pr; p.out_cb = 2 * p.out_mt;
    p.o_row = Wo * 16; p.o_px = 16;
  }
  if (s.in16) { p.in_px_bytes = 32; p.in_chunk_bytes = s.Hi * s.Wi * 32; }
  *v = Variant{};
  if (s.stride == 1) {
    // the largest tile that still gives every CU one (small batches of small maps drop to 256- and 128-pixel tiles)
    const Cand cd = force ? *force : pick_stride1(s.B, Ho, Wo, s.cout, kGridMax, k.fit);
    set_stride1_geometry(p, cd, Ho, Wo);
    *v = stride1_variant(cd);
    if (s.esz == 2) {
      v->m16 = conv3_mfma16_layer(s.cin, s.cout, k.mfma16);
      // weights resident in LDS when the layer's slabs fit beside the window ring (bf16 64 -> 64)
      v->wres = cd.variant == 0 && resident_weights_fit(*v, s.esz, p);
    }
  } else if (s.in16) {
    // the wide variant: 128 couts x 256 pixels per workgroup on half-chunk stages
    if (!(s.ds && s.blocked && s2_wide_eligible(k.s2_wide, s.esz, s.cout, Wo, s.wide_packed) && set_stride2_wide_geometry(p, Ho, Wo)))
      return "conv3x3: an input in 16-channel planes needs the wide stride-2 kernel";
    p.out_cb = 4 * p.out_mt; p.r_cb = p.out_cb;   // a workgroup's cout block = four 32-cout planes
    v->stride = 2; v->nt = 2; v->mt = 2; v->ds = 1; v->half = 1;
  } else {
    // 128-pixel tiles: wave pairs share pixels and split the 64 couts
    set_stride2_geometry(p, Ho, Wo);
    v->stride = 2; v->nt = 1; v->mt = 1; v->ds = s.ds;
    v->wres = s.ds && s.esz == 2 && resident_weights_fit(*v, s.esz, p);
  }
  return launch_numbers(*v, s.esz, p, 0, ln);
}

// Data gradient of a 3x3 / stride-2 / pad-1 convolution: four stride-1 convolutions over dZ [B][Ho][Wo][cin], one per parity class (py, px) =
// (id >> 1, id & 1) of the dX pixel (1, 2, 2 and 4 taps), written into dX [B][Hi][Wi][cout] at pixels (2 i + py, 2 j + px).  NHWC.
constexpr int kClassOrder[4] = {3, 1, 2, 0}, kClassTaps[4] = {4, 2, 2, 1};   // parameter set k is class kClassOrder[k]: most taps first

// workgroups per class: one at a time to the class whose (tiles per workgroup) x (taps) is largest
inline void split_workgroups(const int (&tiles)[4], const int (&taps)[4], int total_wg, int (&wg)[4]) {
  int total = 0;
  for (int k = 0; k < 4; ++k) { wg[k] = tiles[k] > 0 ? 1 : 0; total += wg[k]; }
  auto cost = [&](int k) { return wg[k] > 0 ? ((tiles[k] + wg[k] - 1) / wg[k]) * taps[k] : 0; };
  while (total < total_wg) {
    int best = -1;
    for (int k = 0; k < 4; ++k)
      if (wg[k] > 0 && wg[k] < tiles[k] && (best < 0 || cost(k) > cost(best))) best = k;
    if (best < 0) break;
    ++wg[best]; ++total;
  }
}

template <class P> struct DgradPlan {
  Variant v;       // cls == 4: ONE parameter set, all classes from one staged dZ window (even maps); cls == -1: four sets in one merged
  int nsets = 0;   // launch (conv3x3_s2dgrad_kernel<T, nt, kWaves, mt>), set k on wg[k] workgroups
  P p[4];
  Launch ln[4];
  int wg[4] = {0, 0, 0, 0};
};

template <class P> const char* plan_dgrad_s2(int esz, int B, int Ho, int Wo, int Hi, int Wi, int cin, int cout, DgradPlan<P>* dp) {
  if (Ho != (Hi + 2 - 3) / 2 + 1 || Wo != (Wi + 2 - 3) / 2 + 1) return "dgrad s2: dZ is not the stride-2 output of dX";
  const int re = (Hi + 1) / 2, ro = Hi / 2, ce = (Wi + 1) / 2, co = Wi / 2;   // rows / columns of dX with even / odd index
  const bool even = Hi % 2 == 0 && Wi % 2 == 0;
  const int rows_of[4] = {re, re, ro, ro}, cols_of[4] = {ce, co, ce, co};   // by class id
  auto class_set = [&](P& p, int id, int rows, int cols, const Cand& cd) {
    p.B = B; p.Hi = Ho; p.Wi = Wo; p.Cin = cin; p.Cout = cout; p.Ho = rows; p.Wo = cols;
    set_nhwc(p, esz);
    p.o_img = (int64_t)Hi * Wi * cout; p.o_row = 2 * Wi * cout; p.o_px = 2 * cout; p.o_base = ((id >> 1) * Wi + (id & 1)) * cout;
    residual_like_output(p);
    set_stride1_geometry(p, cd, rows, cols);
  };
  Cand c[kMaxCands];
  int nc = 0, pick;
  if (even) {
    // four accumulator sets: 256- or 128-pixel tiles only (NT = 1), so NOT stride1_candidates: no 512-pixel candidate, and the 128-pixel
    // tile is the fallback of wide maps too
    if (ce > 8) c[nc++] = {16, 16, 1, 18, 1};
    else c[nc++] = {8, 8, 4, 12, 1};
    c[nc++] = {8, 8, 2, 12, 2};
    pick = tiles_of(c[0], B, re, ce, cout) >= kGridMax ? 0 : 1;
    dp->nsets = 1;
    class_set(dp->p[0], 0, re, ce, c[pick]);
    for (int id = 0; id < 4; ++id) dp->p[0].cls_base[id] = ((id >> 1) * Wi + (id & 1)) * cout;
    dp->v = stride1_variant(c[pick]); dp->v.cls = 4;
    return launch_numbers(dp->v, esz, dp->p[0], 0, &dp->ln[0]);
  }
  // one tile shape for all classes, from the power-of-two list of the largest (even, even) class: the largest that gives the launch 256 tiles
  nc = stride1_candidates(re, ce, c, false);
  pick = nc - 1;
  for (int i = 0; i < nc; ++i) {
    int tot = 0;
    for (int id = 0; id < 4; ++id) tot += tiles_of(c[i], B, rows_of[id], cols_of[id], cout);
    if (tot >= kGridMax) { pick = i; break; }
  }
  dp->nsets = 4;
  dp->v = stride1_variant(c[pick]);
  int tiles[4];
  for (int k = 0; k < 4; ++k) {
    const int id = kClassOrder[k];
    class_set(dp->p[k], id, rows_of[id], cols_of[id], c[pick]);
    tiles[k] = tiles_of(c[pick], B, rows_of[id], cols_of[id], cout);
    dp->p[k].n_win_instr = 0; dp->p[k].ntiles = 0; dp->p[k].iters = 0;
  }
  split_workgroups(tiles, kClassTaps, kGridMax, dp->wg);
  for (int k = 0; k < 4; ++k) {
    if (dp->wg[k] == 0) continue;
    if (const char* why = launch_numbers(dp->v, esz, dp->p[k], dp->wg[k], &dp->ln[k])) return why;
  }
  return nullptr;
}

}  // namespace dh_conv3
