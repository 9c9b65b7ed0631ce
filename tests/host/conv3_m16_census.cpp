// Host check of the 16x16x32 lane tables of the stride-1 bf16 3x3 convolution (deephisto_amd/csrc/conv3_tables_host.h, M16), CPU only.
// Built and run by tests/test_conv_mfma16_host.py.
//
// For every stride-1 tile candidate of every map size the engines produce (patches of 32 ... 330 pixels, all four layers), on all three
// tile variants, it builds the M16 tables as the library does and
//   * replays the window reads of conv3x3.inc's M16 stage -- per wave, 16-pixel tile and tap, lane l = (column l & 15, group G = l >> 4)
//     reads chunk slot (0, 2, 1, 3)[G] of window pixel base_lin + kh * HP + kw -- and counts the bank conflicts of each ds_read_b128 over
//     its four 16-lane service groups (m16_read_conflicts): the census;
//   * checks the tables' own consistency: the four lanes of a column agree on the pixel they read, the pixel a lane STORES (out_rel) is the one
//     in its column of tile 2 nt + (G & 1), every tile pixel is stored by exactly one lane pair (l, l ^ 32 hold its two 8-cout halves), and every
//     tap of every column stays inside the staged window.
// Prints per shape "census <name> <conflicts>" and "census32 <name> <conflicts>" (the same count for the 32x32x16 lanes of the shape, over the same
// number of service-group passes per stage), and "OK <cases>".
#include <set>
#include <string>

#include "conv3_geom.h"

using namespace dh_conv3;

static long g_cases = 0;

// `v`, `p`, `ncb`: the library's plan of the layer on one tile candidate (main), here on 16x16x32 MFMAs whatever the layer ships on
static int census(Variant v, const Geom& p, int ncb, const char* what) {
  v.m16 = 1;
  const int WAVES = kWaves, NT = v.nt, MT = v.mt, NB = 2 * NT, MAXJ = max_window_pieces(1, NT);
  const int win_px = p.IMGS * p.HR * p.HP + p.WTAIL;
  HostTables ht;
  const char* why = build_tables(v, 2, p, ncb, 0, &ht);
  REQUIRE(!why, "%s: %s", what, why);
  REQUIRE(ht.lane_stride == 2 * NT + NB + MAXJ, "%s: lane stride", what);
  const int IP = p.IP ? p.IP : p.HR * p.HP;
  std::set<int> stored[2];   // window index of the pixels stored, per 8-cout half (l >> 5)
  int conflicts = 0;
  for (int wave = 0; wave < WAVES; ++wave) {
    if (MT == 1 && (wave & 1)) continue;   // wave pairs share pixels
    for (int nb = 0; nb < NB; ++nb) {
      int base[64];
      for (int l = 0; l < 64; ++l) base[l] = ht.lane[(size_t)(wave * 64 + l) * ht.lane_stride + NT + nb];
      for (int l = 0; l < 64; ++l) REQUIRE(base[l] == base[l & 15], "%s: the lanes of column %d disagree", what, l & 15);
      for (int kh = 0; kh < 3; ++kh)
        for (int kw = 0; kw < 3; ++kw) {
          int bl[64];
          for (int l = 0; l < 64; ++l) {
            bl[l] = base[l] + kh * p.HP + kw;
            REQUIRE(bl[l] >= 0 && bl[l] < win_px, "%s: tap reads window index %d of %d", what, bl[l], win_px);
          }
          conflicts += m16_read_conflicts(bl);
        }
    }
    // the pixel a lane stores: mask row 0 is a full tile (first tile of the launch, B >= IMGS)
    for (int l = 0; l < 64; ++l) {
      const int tid = wave * 64 + l;
      const int* row = &ht.lane[(size_t)tid * ht.lane_stride];
      const unsigned mk = ht.mask[tid];
      for (int nt = 0; nt < NT; ++nt) {
        if (!((mk >> (16 + nt)) & 1u)) continue;
        const int w = row[NT + 2 * nt + ((l >> 4) & 1)];   // what it reads in ITS tile
        // ... is the pixel of out_rel: img * o_img + ty * o_row + tx * o_px
        const int orel = row[nt];
        const int img = (int)(orel / p.o_img), ty = (int)((orel % p.o_img) / p.o_row), tx = (int)((orel % p.o_img) % p.o_row) / p.o_px;
        REQUIRE(w == img * IP + ty * p.HP + tx, "%s: lane %d stores pixel (%d, %d, %d) but reads window index %d", what, tid, img, ty, tx, w);
        REQUIRE(row[NT + NB + nt] == orel, "%s: residual offset", what);
        REQUIRE(stored[l >> 5].insert(w).second, "%s: pixel at window index %d stored twice", what, w);
      }
    }
  }
  const int npx = std::min(p.B, p.IMGS) * std::min(p.TH, p.Ho) * std::min(p.TW, p.Wo);
  REQUIRE((int)stored[0].size() == npx && (int)stored[1].size() == npx, "%s: %zu / %zu of %d tile pixels stored", what, stored[0].size(), stored[1].size(), npx);
  printf("census %s %d\n", what, conflicts);
  ++g_cases;
  return conflicts;
}

// the same count for the 32x32x16 lanes of the shape (conv3x3.inc: lane l reads slot 2 ks + (l >> 5) of the pixel of slot l & 31, two k-steps per
// tap; service groups A / B of each half-wave): what the M16 tables replace
static int census32(Variant v, const Geom& p, int ncb, const char* what) {
  v.m16 = 0;
  const int WAVES = kWaves, NT = v.nt, MT = v.mt;
  HostTables ht;
  const char* why = build_tables(v, 2, p, ncb, 0, &ht);
  REQUIRE(!why, "%s: %s", what, why);
  int conflicts = 0;
  for (int wave = 0; wave < WAVES; ++wave) {
    if (MT == 1 && (wave & 1)) continue;
    for (int nt = 0; nt < NT; ++nt)
      for (int tap = 0; tap < 9; ++tap)
        for (int ks = 0; ks < 2; ++ks)
          for (int sg = 0; sg < 4; ++sg) {
            int cnt[16] = {0};
            for (int ll = 0; ll < 32; ++ll) {
              const bool in_a = ll < 4 || (ll >= 12 && ll < 16) || (ll >= 20 && ll < 28);
              if (in_a != ((sg & 1) == 0)) continue;
              const int l = (sg >> 1) * 32 + ll, w = ht.lane[(size_t)(wave * 64 + l) * ht.lane_stride + NT + nt] + (tap / 3) * p.HP + tap % 3;
              ++cnt[((w & 3) << 2) | ((2 * ks + (l >> 5)) ^ ((w >> 2) & 3))];
            }
            for (int b = 0; b < 16; ++b) conflicts += cnt[b] > 1 ? cnt[b] - 1 : 0;
          }
  }
  printf("census32 %s %d\n", what, conflicts);
  return conflicts;
}

int main() {
  std::set<std::string> seen;
  for (int P : {32, 64, 96, 100, 224, 256, 330}) {
    int H = ((P + 6 - 7) / 2 + 1 + 2 - 3) / 2 + 1;
    for (int layer = 0; layer < 4; ++layer, H = (H + 2 - 3) / 2 + 1) {
      const int C = 64 << layer;
      Cand c[kMaxCands];
      const int nc = stride1_candidates(H, H, c);
      for (int i = 0; i < nc; ++i) {
        ConvShape s;   // bf16 inference: channel-blocked, batch 64
        s.esz = 2; s.B = 64; s.Hi = s.Wi = s.Ho = s.Wo = H; s.cin = s.cout = C; s.stride = 1; s.blocked = true;
        Geom p{};
        Variant v;
        Launch ln;
        const char* why = plan_forward(s, Knobs{}, p, &v, &ln, &c[i]);
        const std::string name = std::to_string(c[i].imgs) + "x" + std::to_string(c[i].th) + "x" + std::to_string(c[i].tw) + "/pitch" + std::to_string(c[i].hp) +
                                 (c[i].fit ? "/fit" : "") + "/v" + std::to_string(c[i].variant) + "/map" + std::to_string(H);
        if (!seen.insert(name).second) continue;
        REQUIRE(!why && tile_variant(v) == c[i].variant, "%s: %s", name.c_str(), why ? why : "planned on another tile variant");
        census(v, p, ln.ncb, name.c_str());
        census32(v, p, ln.ncb, name.c_str());
      }
    }
  }
  printf("OK %ld\n", g_cases);
  return 0;
}
