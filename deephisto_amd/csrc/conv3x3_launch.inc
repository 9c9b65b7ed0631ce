// conv3x3_launch.inc -- host side of the 3x3 convolution kernels (conv3x3.inc), inside the anonymous namespace of resnet_kernels.hip.
// Every integer a launch hands its kernel comes from the HIP-free plan (conv3_plan_host.h), every address from the tables
// (conv3_tables_host.h), both replayed on the CPU (tests/test_conv_tables_host.py); here: the table cache, the list of kernels, the launch.

// Host-built tables of the conv3x3 kernel, cached per (device, table_key), a few KiB each; past CONV3_TABLE_CAP entries (a caller that sweeps
// batch sizes) the cache is emptied (hipFree waits for kernels that still read a table).
struct Conv3Tables { int* lane = nullptr; int4* tile = nullptr; unsigned* mask = nullptr; };
std::map<std::pair<int, dh_conv3::TableKey>, Conv3Tables> g_conv3_tables;
constexpr size_t CONV3_TABLE_CAP = 256;

// fills p.lane_tab / tile_tab / mask_tab
int conv3_tables(const dh_conv3::Variant& v, int esz, Conv3Params& p, int ncb, int grid_override = 0) {
  const std::pair<int, dh_conv3::TableKey> key(current_device(), dh_conv3::table_key(v, esz, p, ncb, grid_override));
  std::lock_guard<std::mutex> lk(g_host_mu);
  auto it = g_conv3_tables.find(key);
  if (it == g_conv3_tables.end()) {
    if (g_conv3_tables.size() >= CONV3_TABLE_CAP) {
      for (auto& kv : g_conv3_tables) { (void)hipFree(kv.second.lane); (void)hipFree(kv.second.tile); (void)hipFree(kv.second.mask); }
      g_conv3_tables.clear();
    }
    dh_conv3::HostTables ht;
    if (const char* why = dh_conv3::build_tables(v, esz, p, ncb, grid_override, &ht)) { dh::set_error("%s", why); return DH_EINVAL; }
    static_assert(sizeof(dh_conv3::TileDesc) == sizeof(int4), "tile descriptor = int4");
    Conv3Tables tb;
    DH_HIP(hipMalloc((void**)&tb.lane, ht.lane.size() * sizeof(int)));
    DH_HIP(hipMalloc((void**)&tb.tile, ht.tile.size() * sizeof(int4)));
    DH_HIP(hipMalloc((void**)&tb.mask, ht.mask.size() * sizeof(unsigned)));
    DH_HIP(hipMemcpy(tb.lane, ht.lane.data(), ht.lane.size() * sizeof(int), hipMemcpyHostToDevice));
    DH_HIP(hipMemcpy(tb.tile, ht.tile.data(), ht.tile.size() * sizeof(int4), hipMemcpyHostToDevice));
    DH_HIP(hipMemcpy(tb.mask, ht.mask.data(), ht.mask.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    it = g_conv3_tables.emplace(key, tb).first;
  }
  p.lane_tab = it->second.lane; p.tile_tab = it->second.tile; p.mask_tab = it->second.mask;
  return DH_OK;
}

template <typename T, int STRIDE, int NT, int MT, bool DS, bool WRES, int CLS, bool HALF, bool M16>
int launch_conv3_kernel(const Conv3Params& p, const dh_conv3::Launch& ln, hipStream_t st) {
  constexpr int W = dh_conv3::kWaves;
  if (int rc = ensure_dyn_lds(reinterpret_cast<const void*>(&conv3x3_kernel<T, STRIDE, NT, W, false, DS, MT, WRES, CLS, HALF, M16>), dh_conv3::kLdsBytes)) return rc;
  if constexpr (CLS < 0) {   // every kernel but the data gradient's has a cycle-stamped twin
    if (int rc = ensure_dyn_lds(reinterpret_cast<const void*>(&conv3x3_kernel<T, STRIDE, NT, W, true, DS, MT, WRES, CLS, HALF, M16>), dh_conv3::kLdsBytes)) return rc;
    if (p.stamps) {
      hipLaunchKernelGGL((conv3x3_kernel<T, STRIDE, NT, W, true, DS, MT, WRES, CLS, HALF, M16>), dim3(ln.grid), dim3(W * 64), ln.lds, st, p);
      DH_LAUNCH_CHECK();
      return DH_OK;
    }
  }
  hipLaunchKernelGGL((conv3x3_kernel<T, STRIDE, NT, W, false, DS, MT, WRES, CLS, HALF, M16>), dim3(ln.grid), dim3(W * 64), ln.lds, st, p);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// THE list of conv3x3_kernel instantiations, one row per kernel (and its stamped twin), by the fields of dh_conv3::Variant:
//  types  stride nt mt ds wres cls half m16     (ANY: float32 and bf16)
#define DH_CONV3_KERNELS(K) \
  K(ANY,  1, 2, 2, 0, 0, -1, 0, 0)  /* stride 1: 512-pixel tiles */ \
  K(ANY,  1, 1, 2, 0, 0, -1, 0, 0)  /*           256 */ \
  K(ANY,  1, 1, 1, 0, 0, -1, 0, 0)  /*           128: wave pairs share pixels */ \
  K(BF16, 1, 2, 2, 0, 1, -1, 0, 0)  /*           512, weights resident in LDS */ \
  K(BF16, 1, 2, 2, 0, 0, -1, 0, 1)  /* ... and the same four on 16x16x32 MFMAs */ \
  K(BF16, 1, 1, 2, 0, 0, -1, 0, 1) \
  K(BF16, 1, 1, 1, 0, 0, -1, 0, 1) \
  K(BF16, 1, 2, 2, 0, 1, -1, 0, 1) \
  K(ANY,  2, 1, 1, 0, 0, -1, 0, 0)  /* stride 2: 128-pixel tiles */ \
  K(ANY,  2, 1, 1, 1, 0, -1, 0, 0)  /*           + the block's fused 1x1 downsample */ \
  K(ANY,  2, 1, 1, 1, 1, -1, 0, 0)  /*           + resident weights (planned for bf16 only) */ \
  K(BF16, 2, 2, 2, 1, 0, -1, 1, 0)  /*           wide: 128 couts x 256 pixels on half-chunk stages */ \
  K(ANY,  1, 1, 2, 0, 0,  4, 0, 0)  /* stride-2 data gradient of an even map: four classes from one dZ window, 256 pixels */ \
  K(ANY,  1, 1, 1, 0, 0,  4, 0, 0)  /*           128; neither has a stamped twin */

template <typename T>
int launch_conv3_variant(const dh_conv3::Variant& v, const Conv3Params& p, const dh_conv3::Launch& ln, hipStream_t st) {
  constexpr bool ANY = true, BF16 = sizeof(T) == 2;
#define DH_K(TYPES, S, NT, MT, DS, WRES, CLS, HALF, M16)   \
  if constexpr (TYPES && (DH_CONV_HOIST || !M16))          \
    if (v == dh_conv3::Variant{S, NT, MT, DS, WRES, CLS, HALF, M16}) return launch_conv3_kernel<T, S, NT, MT, DS, WRES, CLS, HALF, M16>(p, ln, st);
  DH_CONV3_KERNELS(DH_K)
#undef DH_K
  (void)ANY; (void)BF16;
  dh::set_error("conv3x3: no kernel for variant %d %d %d %d %d %d %d %d", v.stride, v.nt, v.mt, v.ds, v.wres, v.cls, v.half, v.m16);
  return DH_EINVAL;
}

// the knobs of the plan, read once
const dh_conv3::Knobs& conv3_knobs() {
  static const dh_conv3::Knobs k = {dh::env_int("DH_CONV_FIT") != 0, dh::env_int("DH_CONV_S2_WIDE") != 0, DH_CONV_HOIST && dh::env_int("DH_CONV_MFMA16") != 0};
  return k;
}
inline bool s2_wide_packed(const ConvLayer& c1, const ConvLayer* ds) { return ds && c1.w2_dev && ds->w2_dev; }
// forward_impl decides with this before launching the conv that writes the stride-2 conv's input
inline bool s2_wide_eligible(const ConvLayer& c1, const ConvLayer& ds, int esz, int Wo) {
  return dh_conv3::s2_wide_eligible(conv3_knobs().s2_wide, esz, c1.cout, Wo, s2_wide_packed(c1, &ds));
}

// row `row` of the cycle-stamp buffer (8 counters per row), allocated at first use
int stamp_row(int row, unsigned long long** out) {
  if (!g_stamps_dev) {
    DH_HIP(hipMalloc((void**)&g_stamps_dev, 64 * sizeof(unsigned long long)));
    DH_HIP(hipMemset(g_stamps_dev, 0, 64 * sizeof(unsigned long long)));
  }
  *out = g_stamps_dev + 8 * row;
  return DH_OK;
}

std::atomic<int> g_last_conv3_variant{-1}, g_last_conv3_mfma{0};   // dh_debug_last_conv3: of the last forward 3x3 launch

// what is not geometry
int conv3_operands(Conv3Params& p, const ConvLayer& L, const void* in, const void* res, void* out, bool relu) {
  p.in = in; p.w = L.w_dev; p.scale = L.scale_dev; p.shift = L.shift_dev; p.res = res; p.out = out;
  p.ds_w = nullptr; p.ds_scale = nullptr; p.ds_shift = nullptr; p.ds_out = nullptr;
  p.relu = relu ? 1 : 0; p.stamps = nullptr;
  p.lane_tab = nullptr; p.tile_tab = nullptr; p.mask_tab = nullptr;
  return zero_page(&p.zero_page);
}

template <typename T>
int launch_conv3x3(int stride, const ConvLayer& L, const void* in, const void* res, void* out, int B, int Hi, int Wi,
                   bool relu, hipStream_t st, int Ho, int Wo, const ConvLayer* ds = nullptr, void* ds_out = nullptr,
                   bool blocked = false, bool in16 = false, bool out16 = false) {
  dh_conv3::ConvShape s;
  s.esz = (int)sizeof(T); s.B = B; s.Hi = Hi; s.Wi = Wi; s.cin = L.cin; s.cout = L.cout; s.stride = stride; s.Ho = Ho; s.Wo = Wo;
  s.ds = ds != nullptr; s.blocked = blocked; s.in16 = in16; s.out16 = out16; s.wide_packed = s2_wide_packed(L, ds);
  Conv3Params p;
  dh_conv3::Variant v;
  dh_conv3::Launch ln;
  if (const char* why = dh_conv3::plan_forward(s, conv3_knobs(), p, &v, &ln)) { dh::set_error("%s", why); return DH_EINVAL; }
  int rc;
  if ((rc = conv3_operands(p, L, in, res, out, relu))) return rc;
  if (ds) { p.ds_w = ds->w_dev; p.ds_scale = ds->scale_dev; p.ds_shift = ds->shift_dev; p.ds_out = ds_out; }
  if (v.half) { p.w = L.w2_dev; p.ds_w = ds->w2_dev; }
  // one row of 8 counters per layer class: rows 0..3 stride 1 by cin 64..512, 4..6 stride 2
  if (g_stamps_on && (rc = stamp_row(stride == 1 ? (L.cin == 64 ? 0 : L.cin == 128 ? 1 : L.cin == 256 ? 2 : 3) : (L.cin == 64 ? 4 : L.cin == 128 ? 5 : 6), &p.stamps))) return rc;
  if ((rc = conv3_tables(v, s.esz, p, ln.ncb))) return rc;
  g_last_conv3_variant = stride == 1 ? dh_conv3::tile_variant(v) : -1;
  g_last_conv3_mfma = v.m16 ? 16 : 32;
  // the profiler samples the dominant variant only (stride 1, 512-slot tiles)
  const bool sample = stride == 1 && v.nt == 2 && g_prof.on && g_prof.used + 2 <= g_prof.ev.size() && (g_prof.counter++ % g_prof.every) == 0;
  if (sample) DH_HIP(hipEventRecord(g_prof.ev[g_prof.used], st));
  if ((rc = launch_conv3_variant<T>(v, p, ln, st))) return rc;
  if (sample) {
    DH_HIP(hipEventRecord(g_prof.ev[g_prof.used + 1], st));
    g_prof.used += 2;
    g_prof.flops += 2.0 * B * Ho * Wo * (double)L.cout * 9 * L.cin;
  }
  return DH_OK;
}

template <typename T, int NT, int MT>
int launch_s2dgrad_kernel(const Conv3Params& pl, const S2ClassSched& sch, const dh_conv3::Launch& ln, hipStream_t st) {
  if (int rc = ensure_dyn_lds(reinterpret_cast<const void*>(&conv3x3_s2dgrad_kernel<T, NT, dh_conv3::kWaves, MT>), dh_conv3::kLdsBytes)) return rc;
  hipLaunchKernelGGL((conv3x3_s2dgrad_kernel<T, NT, dh_conv3::kWaves, MT>), dim3(ln.grid), dim3(dh_conv3::kWaves * 64), ln.lds, st, pl, sch);
  DH_LAUNCH_CHECK();
  return DH_OK;
}

// Data gradient of a 3x3 / stride-2 / pad-1 convolution WITHOUT the zero-upsampled copy of dZ: the four parity classes of the dX pixel
// (plan_dgrad_s2; `L.w_dev` is the flipped + transposed operator) in ONE launch: even maps from one staged dZ window (CLS == 4), other maps
// side by side (conv3x3_s2dgrad_kernel).  dz [B][Ho][Wo][L.cin], dx (and res, a joining gradient, may be null) [B][Hi][Wi][L.cout], NHWC.
// (History: four launches on one stream; four streams joined by events -- slower still, 9.64 -> 10.63 ms per float32 step.)
template <typename T>
int launch_dgrad_s2(const ConvLayer& L, const void* dz, const void* res, void* dx, int B, int Ho, int Wo, int Hi, int Wi, hipStream_t st) {
  constexpr int ESZ = (int)sizeof(T);
  dh_conv3::DgradPlan<Conv3Params> dp;
  if (const char* why = dh_conv3::plan_dgrad_s2(ESZ, B, Ho, Wo, Hi, Wi, L.cin, L.cout, &dp)) { dh::set_error("%s", why); return DH_EINVAL; }
  int rc;
  for (int k = 0; k < dp.nsets; ++k)
    if ((rc = conv3_operands(dp.p[k], L, dz, res, dx, false))) return rc;
  if (dp.v.cls == 4) {
    if ((rc = conv3_tables(dp.v, ESZ, dp.p[0], dp.ln[0].ncb))) return rc;
    return launch_conv3_variant<T>(dp.v, dp.p[0], dp.ln[0], st);
  }
  S2ClassSched sch;
  Conv3Params pl = dp.p[0];   // the kernel's common parameters; the classes' own geometry is in their tables
  dh_conv3::Launch ln;
  sch.first[0] = 0;
  for (int k = 0; k < 4; ++k) {
    Conv3Params& p = dp.p[k];
    sch.first[k + 1] = sch.first[k] + dp.wg[k];
    if (dp.wg[k] > 0) {
      if ((rc = conv3_tables(dp.v, ESZ, p, dp.ln[k].ncb, dp.wg[k]))) return rc;
      ln = dp.ln[k]; pl.n_win_instr = p.n_win_instr;   // one tile shape: the same for every class
    }
    sch.iters[k] = p.iters; sch.lane[k] = p.lane_tab; sch.tile[k] = p.tile_tab; sch.mask[k] = p.mask_tab;
  }
  ln.grid = sch.first[4];
  pl.lane_tab = nullptr; pl.tile_tab = nullptr; pl.mask_tab = nullptr;
  // THE list of conv3x3_s2dgrad_kernel instantiations: 512-, 256- and 128-pixel tiles
  return dp.v.nt == 2 ? launch_s2dgrad_kernel<T, 2, 2>(pl, sch, ln, st) : dp.v.mt == 2 ? launch_s2dgrad_kernel<T, 1, 2>(pl, sch, ln, st) : launch_s2dgrad_kernel<T, 1, 1>(pl, sch, ln, st);
}
