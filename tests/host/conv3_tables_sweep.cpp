// Sanitizer sweep of the HOST tables behind conv3x3_kernel (deephisto_amd/csrc/conv3_tables_host.h) -- VERDICT r3 item 6.
// Built by tests/test_conv_tables_host.py with `g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all`.
//
// For every (dtype, layout, patch P, tiles per launch n, layer of ResNet-18 / the 3x3 layers of ResNet-50, stride, tile
// candidate) it asks the library's own launch plan (deephisto_amd/csrc/conv3_plan_host.h: plan_forward, plan_dgrad_s2 -- the functions
// conv3x3_launch.inc calls) for the parameters, builds the lane / tile / mask tables from them and replays the kernel's address arithmetic
// on the host (conv3x3.inc: enter_tile, dma_piece, epilogue_of):
//   * every window piece whose mask bit is set reads 16 bytes INSIDE the input tensor, at the pixel / channel slot the LDS image
//     expects, and every in-image pixel of the staged window IS covered by a set bit (no padding where data should be);
//   * every output pixel x cout block is written exactly once, inside the output tensor;
//   * window byte offsets and output element offsets fit the 32-bit unsigned words of the schedule, per-lane offsets fit int32 (one float32 case,
//     n = 2 600 at P = 256, is REQUIRED to carry byte offsets past 2^31: the band between the signed and the unsigned limit);
//   * a workgroup keeps one cout block over all iterations (resident weights), mask rows < 4096;
//   * the stride-2 data gradients (sweep_dgrad): the same per launch, and across the four parity classes together -- through cls_base of the
//     one-window launch, or through the class sets' own tables on their shares of the merged launch -- every dX pixel x cout block is written
//     exactly once; the shares are >= 1 and <= the tiles of a class that has tiles and sum to 256 whenever there are that many tiles.
// Prints one line per case class and "OK <cases>"; any violation aborts with a message (non-zero exit).
#include <cinttypes>
#include <set>
#include <string>

#include "conv3_geom.h"

using namespace dh_conv3;

static long g_cases = 0;
static uint64_t g_max_win_byte = 0, g_max_out_byte = 0;   // the largest window / output BYTE offset of a valid tile descriptor since last reset

// Replays the launch `plan` (the kernel variant `v`, the parameters `p` and the launch numbers `ln`, as the library's plan functions made them;
// `plan_why`: their refusal) on the tables the library builds for it.
// layout of the output / input: 0 NHWC, 1 channel-blocked in 32-channel planes, 2 in 16-channel planes (out16 / in16).
// `dx_written`: the launch is (a share of) a stride-2 data gradient: [dX pixel][cout block] of the whole dX, marked here and checked by the caller
static void check_case(const Variant& v, int ESZ, const Geom& p, const Launch& ln, const char* plan_why, int in_layout, int out_layout, int grid_override,
                       const char* what, std::vector<uint8_t>* dx_written = nullptr) {
  REQUIRE(!plan_why, "%s: the plan refuses: %s", what, plan_why);
  const int STRIDE = v.stride, NT = v.nt, MT = v.mt, WAVES = kWaves, NB = v.m16 ? 2 * NT : NT;
  const bool HALF = v.half != 0;
  const int MAXJ = max_window_pieces(STRIDE, NT);
  const int CO_BLK = HALF ? 128 : 64, PXB = HALF ? 32 : 64;   // couts per workgroup; bytes of a pixel per stage
  const bool blocked = in_layout != 0;
  const int ncb = ln.ncb, grid = ln.grid;
  const int win_px = p.IMGS * p.HR * p.HP + p.WTAIL;
  REQUIRE(ncb == p.Cout / CO_BLK && ln.lds <= (size_t)kLdsBytes && p.IP >= p.HR * p.HP, "%s: launch numbers", what);
  HostTables ht;
  const char* why = build_tables(v, ESZ, p, ncb, grid_override, &ht);
  const int64_t in_bytes = (int64_t)p.B * p.Hi * p.Wi * p.Cin * ESZ;
  const int64_t out_elems = (int64_t)p.B * p.o_img;
  if (why) {   // the only legitimate refusal: a tensor past 4 Gi bytes / elements
    REQUIRE(in_bytes >= ((int64_t)1 << 32) || out_elems >= ((int64_t)1 << 32), "%s: refused (%s) although the tensors fit", what, why);
    ++g_cases;
    return;
  }
  REQUIRE(ht.grid == grid && ht.mask_rows < 4096 && (int)ht.tile.size() == p.iters * grid, "%s: table sizes", what);
  REQUIRE(ht.lane_stride == 2 * NT + NB + MAXJ, "%s: lane stride", what);
  const int threads = WAVES * 64;
  const int nchunks = p.Cin * ESZ / PXB;
  // the classes a lane's accumulators go to: one, or (CLS == 4) the four parity classes of dX through cls_base
  const int ncls = v.cls == 4 ? 4 : 1;
  // written[(pixel, cout block)] exactly once
  std::vector<uint8_t> written((size_t)p.B * p.Ho * p.Wo * ncb, 0);
  std::vector<int> wg_cb(grid, -1);
  std::vector<uint8_t> staged;
  for (int it = 0; it < p.iters; ++it)
    for (int w = 0; w < grid; ++w) {
      const TileDesc td = ht.tile[(size_t)it * grid + w];
      const int cb = td.x & 0xFFFF, valid = (td.x >> 16) & 1, mrow = (unsigned)td.x >> 20;
      REQUIRE(cb < ncb && mrow < ht.mask_rows, "%s: descriptor fields", what);
      if (wg_cb[w] < 0) wg_cb[w] = cb;
      REQUIRE(wg_cb[w] == cb, "%s: workgroup %d changes its cout block (%d -> %d)", what, w, wg_cb[w], cb);
      if (!valid) continue;
      const uint32_t win_off = (uint32_t)td.y, out_off = (uint32_t)td.z;
      g_max_win_byte = std::max<uint64_t>(g_max_win_byte, win_off); g_max_out_byte = std::max<uint64_t>(g_max_out_byte, (uint64_t)out_off * ESZ);
      // recover the tile position from the window offset (NHWC and blocked alike: img * img_bytes + (y * Wi + x) * px_bytes)
      const int64_t img_bytes = (int64_t)p.Hi * p.Wi * p.Cin * ESZ;
      const int img0 = (int)(win_off / img_bytes);
      const int64_t rpx = (win_off % img_bytes) / p.in_px_bytes;
      REQUIRE((win_off % img_bytes) % p.in_px_bytes == 0, "%s: window offset not on a pixel", what);
      const int iy0 = (int)(rpx / p.Wi), ix0 = (int)(rpx % p.Wi);
      REQUIRE(iy0 % STRIDE == 0 && ix0 % STRIDE == 0, "%s: window origin off the stride grid", what);
      const int oy0 = iy0 / STRIDE, ox0 = ix0 / STRIDE;
      const int imgs_here = std::min(p.IMGS, p.B - img0);
      REQUIRE(imgs_here > 0, "%s: tile beyond the batch", what);
      staged.assign((size_t)win_px * 4, 0);   // [LDS pixel][16-byte slot]: filled from the tensor?
      for (int tid = 0; tid < threads; ++tid) {
        const int* row = &ht.lane[(size_t)tid * ht.lane_stride];
        const unsigned mk = ht.mask[(size_t)mrow * threads + tid];
        const int l = tid & 63, wave = tid >> 6;
        // ---- window pieces (dma_piece): src = in + win_off + chunk * in_chunk_bytes + rel_off[j], 16 bytes
        for (int j = 0; j < MAXJ; ++j) {
          const int i = wave + WAVES * j;
          if (i >= p.n_win_instr) { REQUIRE(!((mk >> j) & 1u), "%s: mask bit on an unissued piece", what); continue; }
          const int px = HALF ? i * 32 + (l >> 1) : i * 16 + (l >> 2);
          if (!((mk >> j) & 1u)) continue;
          for (int ch = 0; ch < nchunks; ch += std::max(1, nchunks - 1)) {   // first and last chunk
            const int64_t src = (int64_t)win_off + (int64_t)ch * p.in_chunk_bytes + row[2 * NT + NB + j];
            REQUIRE(src >= 0 && src + 16 <= in_bytes, "%s: window piece reads [%" PRId64 ", +16) outside the %" PRId64 "-byte input (tile it %d wg %d tid %d j %d)",
                    what, src, in_bytes, it, w, tid, j);
            // which pixel / slot is it?  NHWC: byte = ((img * Hi + y) * Wi + x) * Cin * ESZ + chunk * 64 + slot * 16
            //                            blocked: byte = (img * nchunks + chunk) * Hi * Wi * 64 + (y * Wi + x) * 64 + slot * 16
            int64_t simg, sy, sx, sch, sslot;
            if (in_layout == 2) {          // 16-channel planes: [image][C/16][H][W][16] -- a plane IS a half-chunk
              simg = src / img_bytes; const int64_t r = src % img_bytes;
              sch = r / ((int64_t)p.Hi * p.Wi * 32); const int64_t r2 = r % ((int64_t)p.Hi * p.Wi * 32);
              sy = r2 / (p.Wi * 32); sx = (r2 % (p.Wi * 32)) / 32; sslot = (r2 % 32) / 16;
            } else if (blocked) {
              simg = src / img_bytes; const int64_t r = src % img_bytes;
              sch = r / ((int64_t)p.Hi * p.Wi * 64); const int64_t r2 = r % ((int64_t)p.Hi * p.Wi * 64);
              sy = r2 / (p.Wi * 64); sx = (r2 % (p.Wi * 64)) / 64; sslot = (r2 % 64) / 16;
            } else {
              simg = src / img_bytes; const int64_t r = src % img_bytes;
              const int64_t pxb = (int64_t)p.Cin * ESZ;
              sy = r / (p.Wi * pxb); sx = (r % (p.Wi * pxb)) / pxb; sch = ((r % pxb) / 64); sslot = (r % 64) / 16;
            }
            const int limg = px / p.IP, lr = px % p.IP;
            REQUIRE(lr < p.HR * p.HP, "%s: a gap pixel of the window is staged", what);
            const int hy = lr / p.HP, c = lr % p.HP;
            const int hx = STRIDE == 2 ? 2 * (c % p.HPH) + c / p.HPH : c;
            REQUIRE(simg == img0 + limg && sy == iy0 + hy - 1 && sx == ix0 + hx - 1 && sch == ch, "%s: window piece lands on the wrong pixel", what);
            if (HALF) { REQUIRE(sslot == ((l & 1) ^ ((px >> 3) & 1)), "%s: swizzle slot (half)", what); if (ch == 0) { staged[(size_t)px * 4 + (l & 1)] = 1; staged[(size_t)px * 4 + 2 + (l & 1)] = 1; } }
            else { REQUIRE(sslot == ((l & 3) ^ ((px >> 2) & 3)), "%s: swizzle slot", what); if (ch == 0) staged[(size_t)px * 4 + (l & 3)] = 1; }
          }
        }
        // ---- output pixels (epilogue_of): out + out_off + out_rel[nt] + mt * out_mt + 32 couts
        for (int nt = 0; nt < NT; ++nt) {
          if (!((mk >> (16 + nt)) & 1u)) continue;
          const int64_t base = (int64_t)out_off + row[nt];
          REQUIRE(base <= UINT32_MAX, "%s: output offset past 32 bits", what);
          for (int c = 0; c < ncls; ++c)   // (CLS == 4: class c's accumulators go to out + cls_base[c], its residual comes from res + cls_base[c])
            for (int ml = 0; ml < MT; ++ml) {
              const int mt = HALF ? 2 * (wave & 1) + ml : MT == 2 ? ml : (wave & 1);
              for (int pr = 0; pr < 2; ++pr) {   // the two 16-cout halves of a 32-cout tile (epilogue_of: + pr * out_pr + h * 8)
                const int64_t e0 = base + (ncls == 4 ? p.cls_base[c] : 0) + (int64_t)mt * p.out_mt + (int64_t)pr * p.out_pr;
                REQUIRE(e0 >= 0 && e0 + 16 <= out_elems, "%s: output [%" PRId64 ", +16) outside %" PRId64 " elements", what, e0, out_elems);
              }
            }
          {   // the residual tile (prefetch_residual: res + td.w + res_rel + mt * res_mt + pr * res_pr + h * 8), always in its own layout
            const int64_t rbase = (int64_t)(uint32_t)td.w + row[NT + NB + nt];
            for (int c = 0; c < ncls; ++c)
              for (int ml = 0; ml < MT; ++ml) {
                const int mt = HALF ? 2 * (wave & 1) + ml : MT == 2 ? ml : (wave & 1);
                const int64_t e0 = rbase + (ncls == 4 ? p.cls_base[c] : 0) + (int64_t)mt * p.res_mt + p.res_pr;
                REQUIRE(e0 >= 0 && e0 + 16 <= out_elems, "%s: residual [%" PRId64 ", +16) outside %" PRId64 " elements", what, e0, out_elems);
              }
            // ... and it is the SAME pixel / cout block as the output (NHWC / 32-channel planes)
            int64_t rpix;
            if (blocked) { const int64_t r = rbase % p.o_img; rpix = (rbase / p.o_img) * p.Ho * p.Wo + (r % ((int64_t)p.Ho * p.Wo * 32)) / 32; REQUIRE(r / ((int64_t)p.Ho * p.Wo * 32) == (CO_BLK / 32) * cb, "%s: residual cout block", what); }
            else { rpix = rbase / p.Cout; REQUIRE(rbase % p.Cout == cb * CO_BLK, "%s: residual cout block (NHWC)", what); }
            int64_t opix;
            if (out_layout == 2) { const int64_t r = base % p.o_img; opix = (base / p.o_img) * p.Ho * p.Wo + (r % ((int64_t)p.Ho * p.Wo * 16)) / 16; }
            else if (out_layout == 1) { const int64_t r = base % p.o_img; opix = (base / p.o_img) * p.Ho * p.Wo + (r % ((int64_t)p.Ho * p.Wo * 32)) / 32; }
            else opix = base / p.Cout;
            REQUIRE(rpix == opix, "%s: residual pixel %" PRId64 " != output pixel %" PRId64, what, rpix, opix);
          }
          if ((l >> 5) == 0 && ((MT == 2 && !HALF) || (wave & 1) == 0)) {   // one owner per pixel: half-wave 0 (the other half holds the other couts)
            // pixel index from the element offset (dense maps only: o_px == out_px)
            if (p.o_px == p.out_px && p.o_base == 0) {
              int64_t pix;
              if (out_layout == 2) { const int64_t r = base % p.o_img; pix = (base / p.o_img) * p.Ho * p.Wo + (r % ((int64_t)p.Ho * p.Wo * 16)) / 16; REQUIRE(r / ((int64_t)p.Ho * p.Wo * 16) == (CO_BLK / 16) * cb, "%s: 16-plane cout block", what); }
              else if (out_layout == 1) { const int64_t r = base % p.o_img; pix = (base / p.o_img) * p.Ho * p.Wo + (r % ((int64_t)p.Ho * p.Wo * 32)) / 32; REQUIRE(r / ((int64_t)p.Ho * p.Wo * 32) == (CO_BLK / 32) * cb, "%s: blocked cout block", what); }
              else { pix = base / p.Cout; REQUIRE(base % p.Cout == cb * CO_BLK, "%s: NHWC cout block", what); }
              REQUIRE(pix >= 0 && pix < (int64_t)p.B * p.Ho * p.Wo, "%s: pixel index", what);
              uint8_t& f = written[(size_t)pix * ncb + cb];
              REQUIRE(f == 0, "%s: output pixel %" PRId64 " cout block %d written twice", what, pix, cb);
              f = 1;
            }
            // a data gradient: the pixel of the FULL-SIZE dX (NHWC) each class's store lands on
            if (dx_written)
              for (int c = 0; c < ncls; ++c) {
                const int64_t e = base + (ncls == 4 ? p.cls_base[c] : 0);
                REQUIRE(e % p.Cout == cb * CO_BLK && e / p.Cout < (int64_t)dx_written->size() / ncb, "%s: dX element %" PRId64, what, e);
                uint8_t& f = (*dx_written)[(size_t)(e / p.Cout) * ncb + cb];
                REQUIRE(f == 0, "%s: dX pixel %" PRId64 " cout block %d written twice", what, e / p.Cout, cb);
                f = 1;
              }
          }
        }
      }
      // every tap of every existing output pixel reads INSIDE the window, on a pixel staged from the tensor exactly when the tap is inside
      // the image and on a zero (unstaged) pixel otherwise -- this is what makes shared halo rows / columns of fit tiles legal
      if (STRIDE == 1 && !HALF)
        for (int tid = 0; tid < threads; tid += 1) {
          if ((tid & 63) >= 32) continue;   // lanes l and l + 32 own the same pixel
          const int* row = &ht.lane[(size_t)tid * ht.lane_stride];
          const unsigned mk = ht.mask[(size_t)mrow * threads + tid];
          for (int nt = 0; nt < NT; ++nt) {
            if (!((mk >> (16 + nt)) & 1u)) continue;
            const int base_lin = row[NT + (v.m16 ? 2 * nt + ((tid >> 4) & 1) : nt)];   // M16: of the 16-pixel tile the lane stores in
            // recover (img, ty, tx) of the pixel from its output offset (dense NHWC / blocked maps only)
            if (!(p.o_px == p.out_px && p.o_base == 0)) continue;
            const int64_t e = (int64_t)out_off + row[nt];
            int64_t pix;
            if (out_layout == 2) pix = (e / p.o_img) * p.Ho * p.Wo + ((e % p.o_img) % ((int64_t)p.Ho * p.Wo * 16)) / 16;
            else if (out_layout == 1) pix = (e / p.o_img) * p.Ho * p.Wo + ((e % p.o_img) % ((int64_t)p.Ho * p.Wo * 32)) / 32;
            else pix = e / p.Cout;
            const int oy = (int)((pix % ((int64_t)p.Ho * p.Wo)) / p.Wo), ox = (int)(pix % p.Wo);
            for (int kh = 0; kh < 3; ++kh)
              for (int kw = 0; kw < 3; ++kw) {
                const int lin = base_lin + kh * p.HP + kw;
                REQUIRE(lin >= 0 && lin < win_px, "%s: tap (%d, %d) of pixel (%d, %d) reads window index %d of %d", what, kh, kw, oy, ox, lin, win_px);
                const int iy = oy + kh - 1, ix = ox + kw - 1;
                const bool inside = iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
                REQUIRE((staged[(size_t)lin * 4] != 0) == inside, "%s: tap (%d, %d) of pixel (%d, %d): window index %d is %s but the tap is %s the image",
                        what, kh, kw, oy, ox, lin, staged[(size_t)lin * 4] ? "data" : "zero", inside ? "inside" : "outside");
              }
          }
        }
      // every in-image pixel of the window must have all four slots staged from the tensor
      for (int limg = 0; limg < imgs_here; ++limg)
        for (int hy = 0; hy < p.HR; ++hy)
          for (int hx = 0; hx < p.HC; ++hx) {
            const int iy = iy0 + hy - 1, ix = ix0 + hx - 1;
            if (iy < 0 || iy >= p.Hi || ix < 0 || ix >= p.Wi) continue;
            const int c = STRIDE == 2 ? (hx & 1) * p.HPH + (hx >> 1) : hx;
            const size_t px = (size_t)limg * p.IP + (size_t)hy * p.HP + c;
            for (int sl = 0; sl < 4; ++sl)
              REQUIRE(staged[px * 4 + sl], "%s: in-image window pixel (%d, %d, %d) slot %d is padded", what, limg, hy, hx, sl);
          }
    }
  if (p.o_px == p.out_px && p.o_base == 0)
    for (size_t i = 0; i < written.size(); ++i) REQUIRE(written[i], "%s: output pixel %zu / cout block %zu never written", what, i / ncb, i % ncb);
  ++g_cases;
}

// One forward layer through the library's plan (plan_forward), on ALL its stride-1 tile candidates, not only the picked one.
// out16: the output in 16-channel planes (the conv before a wide stride-2 conv); wide: the wide stride-2 variant itself (input in 16-channel planes);
// ds: with the block's fused downsample (the LDS budget and the resident-weight choice depend on it, the tables do not)
template <int ESZ>
static void sweep_layer(int B, int Hi, int cin, int cout, int stride, bool blocked, const std::string& tag, bool out16 = false, bool wide = false, bool ds = true) {
  ConvShape s;
  s.esz = ESZ; s.B = B; s.Hi = s.Wi = Hi; s.cin = cin; s.cout = cout; s.stride = stride; s.Ho = s.Wo = (Hi + 2 - 3) / stride + 1;
  s.ds = stride == 2 && ds; s.blocked = blocked; s.in16 = wide; s.out16 = out16; s.wide_packed = wide;
  const std::string what = tag + " B=" + std::to_string(B) + " Hi=" + std::to_string(Hi) + " " + std::to_string(cin) + "->" + std::to_string(cout) +
                           " s" + std::to_string(stride) + (blocked ? " blocked" : " nhwc") + (out16 ? " out16" : "") + (wide ? " wide" : "") + " esz" + std::to_string(ESZ);
  const int in_l = wide ? 2 : blocked ? 1 : 0, out_l = out16 ? 2 : blocked ? 1 : 0;
  Geom p{};
  Variant v;
  Launch ln;
  if (stride == 2) {
    const char* why = plan_forward(s, Knobs{}, p, &v, &ln);
    REQUIRE(v.half == (wide ? 1 : 0), "%s: %s stride-2 kernel planned", what.c_str(), v.half ? "the wide" : "the 128-pixel");
    check_case(v, ESZ, p, ln, why, in_l, out_l, 0, what.c_str());
    return;
  }
  Cand c[kMaxCands];
  const int nc = stride1_candidates(s.Ho, s.Wo, c);
  const Cand picked = pick_stride1(B, s.Ho, s.Wo, cout, kGridMax);
  // a layer that ships on 16x16x32 MFMAs: its tables as shipped, and those of DH_CONV_MFMA16=0
  for (int m16 = ESZ == 2 && conv3_mfma16_layer(cin, cout, true) ? 1 : 0; m16 >= 0; --m16)
    for (int i = 0; i < nc; ++i) {
      Knobs k;
      k.mfma16 = m16 != 0;
      const char* why = plan_forward(s, k, p, &v, &ln, &c[i]);
      const std::string w2 = what + " cand" + std::to_string(i) + (c[i].fit ? "fit" : "") + (m16 ? " m16" : "") + (c[i].th == picked.th && c[i].tw == picked.tw && c[i].imgs == picked.imgs ? "*" : "");
      REQUIRE(tile_variant(v) == c[i].variant && v.m16 == m16, "%s: planned variant", w2.c_str());
      check_case(v, ESZ, p, ln, why, in_l, out_l, 0, w2.c_str());
    }
}

// The data gradient of the stride-2 3x3 conv cin -> cout of a `side` x `side` map through the library's plan (plan_dgrad_s2): dZ [B][Ho][Ho][cout]
// -> dX [B][side][side][cin], NHWC.  Even maps: ONE launch writes the four parity classes through cls_base; other maps: four parameter sets share
// the workgroups of one merged launch, each on its own tables built with grid_override = its share.
template <int ESZ>
static void sweep_dgrad(int B, int side, int cin, int cout) {
  const int Ho = (side + 2 - 3) / 2 + 1, ncb = cin / 64;
  const std::string what = "dgrad-s2 B=" + std::to_string(B) + " side=" + std::to_string(side) + " " + std::to_string(cin) + "->" + std::to_string(cout) + " esz" + std::to_string(ESZ);
  DgradPlan<Geom> dp{};
  const char* why = plan_dgrad_s2(ESZ, B, Ho, Ho, side, side, cout, cin, &dp);
  REQUIRE(!why, "%s: the plan refuses: %s", what.c_str(), why);
  std::vector<uint8_t> dx_written((size_t)B * side * side * ncb, 0);
  if (side % 2 == 0) {
    REQUIRE(dp.nsets == 1 && dp.v.cls == 4 && dp.v.nt == 1, "%s: an even map runs the one-window kernel", what.c_str());
    check_case(dp.v, ESZ, dp.p[0], dp.ln[0], nullptr, 0, 0, 0, what.c_str(), &dx_written);
  } else {
    REQUIRE(dp.nsets == 4 && dp.v.cls == -1, "%s: an odd map runs the merged launch", what.c_str());
    long sum = 0, tiles = 0;
    for (int k = 0; k < 4; ++k) {
      const Geom& p = dp.p[k];
      const bool has_tiles = p.Ho > 0 && p.Wo > 0;
      REQUIRE(has_tiles ? dp.wg[k] >= 1 && dp.wg[k] <= p.ntiles : dp.wg[k] == 0, "%s: class set %d has %d workgroups for %d tiles", what.c_str(), k, dp.wg[k], has_tiles ? p.ntiles : 0);
      sum += dp.wg[k]; tiles += has_tiles ? p.ntiles : 0;
    }
    REQUIRE(sum <= kGridMax && (tiles < kGridMax || sum == kGridMax), "%s: %ld workgroups for %ld tiles", what.c_str(), sum, tiles);
    for (int k = 0; k < 4; ++k)
      if (dp.wg[k] > 0) {
        REQUIRE(dp.ln[k].grid == dp.wg[k], "%s: class set %d launches %d workgroups, its share is %d", what.c_str(), k, dp.ln[k].grid, dp.wg[k]);
        check_case(dp.v, ESZ, dp.p[k], dp.ln[k], nullptr, 0, 0, dp.wg[k], (what + " class set " + std::to_string(k)).c_str(), &dx_written);
      }
  }
  for (size_t i = 0; i < dx_written.size(); ++i) REQUIRE(dx_written[i], "%s: dX pixel %zu / cout block %zu never written", what.c_str(), i / ncb, i % ncb);
}

int main(int argc, char** argv) {
  const bool full = argc > 1 && std::string(argv[1]) == "full";
  const int Ps[] = {32, 64, 96, 100, 200, 224, 256, 330, 512, 1024};
  const int ns_small[] = {1, 3, 64};
  const int ns_big[] = {1024, 3842, 4096};
  // ResNet-18 body: (cin, cout, stride, input map = pooled size / 2^stage)
  struct L { int cin, cout, stride, shift; };
  const L layers[] = {{64, 64, 1, 0}, {64, 128, 2, 0}, {128, 128, 1, 1}, {128, 256, 2, 1}, {256, 256, 1, 2}, {256, 512, 2, 2}, {512, 512, 1, 3}};
  for (int P : Ps) {
    const int H1 = (P + 6 - 7) / 2 + 1, H2 = (H1 + 2 - 3) / 2 + 1;
    for (const L& ly : layers) {
      int Hi = H2;
      for (int s = 0; s < ly.shift; ++s) Hi = (Hi + 2 - 3) / 2 + 1;
      for (int n : ns_small) {
        if (P >= 512 && n > 3) continue;   // 128- and 256-wide maps: the tile positions are the subject, not the batch
        sweep_layer<2>(n, Hi, ly.cin, ly.cout, ly.stride, true, "inf-bf16");    // bf16 inference: channel-blocked
        if (ly.stride == 1 && ly.cin == ly.cout) sweep_layer<2>(n, Hi, ly.cin, ly.cout, 1, true, "inf-bf16", true);   // ... writing 16-channel planes
        if (ly.stride == 2 && ly.cout % 128 == 0 && (Hi + 2 - 3) / 2 + 1 > 4) sweep_layer<2>(n, Hi, ly.cin, ly.cout, 2, true, "inf-bf16", false, true);   // the wide stride-2 variant
        sweep_layer<2>(n, Hi, ly.cin, ly.cout, ly.stride, false, "train-bf16"); // bf16 training: NHWC
        sweep_layer<4>(n, Hi, ly.cin, ly.cout, ly.stride, false, "f32");
      }
      // the launch sizes the headline number is timed at: only where the coverage bitmap stays small enough for a unit test,
      // i.e. the large n on the layers of P in {64, 256} (P = 256, n = 4096, layer 1 is THE 2^31-byte map of VERDICT r3 missing #1)
      if (P == 256 || P == 64 || (full && P <= 330))
        for (int n : ns_big) {
          if (!full && P == 256 && ly.shift > 1 && n != 4096) continue;
          sweep_layer<2>(n, Hi, ly.cin, ly.cout, ly.stride, true, "inf-bf16");
          if (ly.stride == 1 && ly.cin == ly.cout && ly.shift < 3) sweep_layer<2>(n, Hi, ly.cin, ly.cout, 1, true, "inf-bf16", true);
          if (ly.stride == 2 && ly.cout % 128 == 0 && (Hi + 2 - 3) / 2 + 1 > 4) sweep_layer<2>(n, Hi, ly.cin, ly.cout, 2, true, "inf-bf16", false, true);
          if (n <= 1024) sweep_layer<4>(n, Hi, ly.cin, ly.cout, ly.stride, false, "f32");
        }
    }
    printf("P=%d done (%ld cases)\n", P, g_cases);
    fflush(stdout);
  }
  // float32 at 4 096 tiles of 256^2: the layer-1 map is 2^32 bytes -- must be REFUSED, not wrapped
  sweep_layer<4>(4096, 64, 64, 64, 1, false, "f32-oversize");
  // float32 at 2 600 tiles of 256^2: a layer-1 map of 2.73e9 bytes, inside the band (2^31, 2^32) the launch check admits -- the replay must
  // pass with window and output byte offsets past 2^31 (the kernel reads the 32-bit words as unsigned)
  g_max_win_byte = g_max_out_byte = 0;
  sweep_layer<4>(2600, 64, 64, 64, 1, false, "f32-band");
  REQUIRE(g_max_win_byte > ((uint64_t)1 << 31) && g_max_out_byte > ((uint64_t)1 << 31), "f32-band: largest window / output byte offset %" PRIu64 " / %" PRIu64 " does not exceed 2^31",
          g_max_win_byte, g_max_out_byte);
  printf("f32-band: largest window / output byte offset %" PRIu64 " / %" PRIu64 "\n", g_max_win_byte, g_max_out_byte);
  // odd maps of training shapes (224 -> 56 / 28 / 14 / 7) at batch 64 with the 3x3 layers of ResNet-50
  for (int Hi : {56, 28, 14, 7})
    for (int c : {64, 128, 256, 512}) {
      sweep_layer<2>(64, Hi, c, c, 1, false, "r50-3x3");
      if (Hi > 7) sweep_layer<2>(64, Hi, c, c, 2, false, "r50-3x3", false, false, false);   // (no downsample rides on ResNet-50's 3x3 convs)
    }
  // ---- refusal paths: the invariants the kernel relies on are refused by build_tables, not assumed by its callers
  {
    // the library's plan of a bf16 NHWC layer on a forced tile shape (its own verdict is not the subject here), then build_tables on it
    auto tables = [](int B, int Hi, int Wi, int cin, int cout, const Cand& c, HostTables* ht) {
      ConvShape s;
      s.esz = 2; s.B = B; s.Hi = s.Ho = Hi; s.Wi = s.Wo = Wi; s.cin = cin; s.cout = cout; s.stride = 1;
      Geom p{};
      Variant v;
      Launch ln;
      Knobs k;
      k.mfma16 = false;
      (void)plan_forward(s, k, p, &v, &ln, &c);
      ++g_cases;
      return build_tables(v, 2, p, std::max(1, cout / 64), 0, ht);
    };
    auto refused = [&](int B, int Hi, int Wi, int cin, int cout, const Cand& c, const char* expect) {
      HostTables ht;
      const char* why = tables(B, Hi, Wi, cin, cout, c, &ht);
      REQUIRE(why && std::string(why).find(expect) != std::string::npos, "expected a refusal containing '%s', got '%s'", expect, why ? why : "(accepted)");
    };
    const Cand c512 = {16, 32, 1, 34, 0};
    refused(4, 64, 64, 32, 64, c512, "two whole channel stages");          // bf16, 32 channels: ONE 64-byte stage per tile
    refused(4, 64, 64, 80, 64, c512, "two whole channel stages");          // 160 bytes per pixel: not whole stages
    refused(1, 1040, 2048, 64, 64, c512, "too many distinct tile positions");   // 65 x 64 = 4 160 tile positions > 4 096 mask rows
    {   // exactly 4 096 positions (mask rows 0 .. 4095: the descriptor word's bit 31 is used) is accepted and decodes
      HostTables ht;
      const char* why = tables(1, 1024, 2048, 64, 64, c512, &ht);
      REQUIRE(!why && ht.mask_rows == 4096, "4 096 tile positions: %s, %d rows", why ? why : "accepted", ht.mask_rows);
      unsigned top = 0;
      for (const TileDesc& td : ht.tile) top = std::max(top, (unsigned)td.x >> 20);
      REQUIRE(top == 4095, "highest mask row decodes as %u", top);
    }
    // a window past 64 KiB: 24 x 44 pixels x 64 bytes = 66 KiB (the 16-bit hoisted offsets would wrap)
    refused(4, 64, 64, 64, 64, Cand{22, 32, 1, 44, 0}, "64 KiB");
  }
  // ---- the stride-2 data gradients of the three stride-2 layers, in both element types: even maps (one window, four classes) and odd maps
  // (four class sets sharing one launch); B = 40 at side 56 reaches the 512-pixel tile of the merged launch's list ... on an even map it is
  // the 256-pixel tile of the one-window kernel at more than 256 tiles
  for (int side : {7, 8, 9, 14, 15, 28, 56})
    for (int B : {1, 3, 64, 40}) {
      if (B == 40 && side != 56) continue;
      for (int cin : {64, 128, 256}) {
        sweep_dgrad<2>(B, side, cin, 2 * cin);
        sweep_dgrad<4>(B, side, cin, 2 * cin);
      }
    }
  printf("dgrad done (%ld cases)\n", g_cases);
  // ---- fit tiles: bank-conflict census of the dealt lane order (a 16-lane service group reads conflict-free when its pixels have 16
  // different window indices mod 16)
  {
    struct F { int imgs, th, tw, ip, hp, ntile32, max_conflict_groups; const char* name; };
    for (const F& f : {F{10, 7, 7, 67, 8, 16, 0, "7x7 x10"}, F{5, 7, 7, 67, 8, 8, 8, "7x7 x5"}, F{5, 7, 14, 135, 15, 16, 0, "7x14 x5"}, F{8, 8, 8, 82, 9, 16, 0, "8x8 x8"}}) {
      const std::vector<int> slot = deal_fit_pixels(f.imgs, f.th, f.tw, f.ip, f.hp, f.ntile32);
      std::set<int> seen;
      int conflict_groups = 0;
      static const int ga[16] = {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27};
      for (int t = 0; t < f.ntile32; ++t)
        for (int half = 0; half < 2; ++half) {
          int cnt[16] = {0};
          bool in_a[32] = {false};
          for (int k = 0; k < 16; ++k) in_a[ga[k]] = true;
          for (int ll = 0; ll < 32; ++ll) {
            if (in_a[ll] != (half == 0)) continue;
            const int q = slot[(size_t)t * 32 + ll];
            if (q < 0) continue;
            REQUIRE(seen.insert(q).second, "%s: pixel %d dealt twice", f.name, q);
            const int img = q / (f.th * f.tw), ty = (q % (f.th * f.tw)) / f.tw, tx = q % f.tw;
            ++cnt[(img * f.ip + ty * f.hp + tx) & 15];
          }
          bool c2 = false;
          for (int r = 0; r < 16; ++r) { REQUIRE(cnt[r] <= 2, "%s: %d-way conflict", f.name, cnt[r]); c2 |= cnt[r] > 1; }
          conflict_groups += c2;
        }
      REQUIRE((int)seen.size() == f.imgs * f.th * f.tw, "%s: %zu of %d pixels dealt", f.name, seen.size(), f.imgs * f.th * f.tw);
      REQUIRE(conflict_groups <= f.max_conflict_groups, "%s: %d service groups with a 2-way conflict (bound %d)", f.name, conflict_groups, f.max_conflict_groups);
      printf("fit %s: %d of %d service groups with a 2-way bank conflict\n", f.name, conflict_groups, 2 * f.ntile32);
      ++g_cases;
    }
  }
  printf("OK %ld\n", g_cases);
  return 0;
}
