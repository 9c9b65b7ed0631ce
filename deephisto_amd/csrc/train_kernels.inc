// train_kernels.inc -- the float32 training engine's OWN kernels (host side: train.inc; test hooks: train_hooks.inc).  Included in
// resnet_kernels.hip behind train_core_kernels.inc, whose kernels (BN finalize, slab reduces, head, loss, Adam) both engines launch; nothing here
// is used by the bf16 engine.  Weight packing, per-channel reductions, BN apply / backward, the pooled stem tail, the weight gradients, the
// downsample branch's upsample-add, the average pool -- and the two stand-alone maxpool kernels that only dh_debug_maxpool launches (the step
// uses the pooled stem tail; the pair is its reference).
namespace {

// ---------------- weight packing ----------------
// pack [cout][cin][ks][ks] f32 master weights into MFMA fragment order (see pack_conv_weights);
// FLIPT: pack the dgrad operator instead: Wd[co'=ci][ci'=co][kh][kw] = W[co][ci][ks-1-kh][ks-1-kw].
template <typename T, bool FLIPT>
__device__ __forceinline__ float pack_conv_elem(const float* __restrict__ w, int cout, int cin, int ks, int64_t o) {   // value of packed element o
  constexpr int ESZ = (int)sizeof(T);
  const int cpc = CHUNK_BYTES / ESZ, epl = 16 / ESZ, taps = ks * ks;
  const int pc_in = FLIPT ? cout : cin;  // packed operator's cin
  const int nch = pc_in / cpc;
  int64_t r = o;
  const int e = (int)(r % epl); r /= epl;
  const int l = (int)(r % 64); r /= 64;
  const int mt = (int)(r % 2); r /= 2;
  const int k2 = (int)(r % 2); r /= 2;
  const int tap = (int)(r % taps); r /= taps;
  const int ch = (int)(r % nch); r /= nch;
  const int cb = (int)r;
  const int co = cb * 64 + mt * 32 + (l & 31);
  const int ci = ch * cpc + k2 * (cpc / 2) + (l >> 5) * epl + e;
  if (FLIPT) return w[((int64_t)ci * cin + co) * taps + (taps - 1 - tap)];   // W[co_src=ci][ci_src=co][flipped]
  return w[((int64_t)co * cin + ci) * taps + tap];
}
template <typename T, bool FLIPT>
__global__ void pack_conv_dev_kernel(const float* __restrict__ w, int cout, int cin, int ks, T* __restrict__ out) {
  const int64_t total = (int64_t)cout * cin * ks * ks;
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
    const float v = pack_conv_elem<T, FLIPT>(w, cout, cin, ks, o);
    if constexpr (sizeof(T) == 4) out[o] = v;
    else reinterpret_cast<uint16_t*>(out)[o] = (uint16_t)f32_to_bf16(v);
  }
}

// Every convolution of the network in ONE launch (after every optimiser step; round 2 launched two kernels per conv: 44 launches
// of ~5.5 us for ResNet-18): a descriptor per conv names the master weights, both packed operators and its first workgroup.
struct PackDescF { const float* w; float* wf; float* wd; int cout, cin, ks, blk0; };
constexpr int PACKF_PER_BLOCK = 256 * 16;   // packed elements per workgroup (1x1 transposes)
// 3x3: one workgroup per SUB-TILE of 16 couts x 64 cins x 9 taps (round 5).  The element-wise form computed eight 64-bit divisions per packed
// element and read the master tensor in 4-byte pieces 36 bytes apart, twice (61 us per launch, 486 us per ResNet-18 step on the side stream).
// Here the sub-tile's 16 rows of 576 contiguous floats are read once as float4 and scattered into LDS as T[tap][co][ci] (pitch 68 floats:
// 16-byte aligned rows, conflict-free columns); both operators are then written as whole 16-byte pieces in runs of 16 / 32 consecutive lanes:
//   forward  piece (co, tap, 4 consecutive ci)            = T[tap][co][ci .. ci+3]
//   dgrad    piece (co' = ci, tap', 4 consecutive ci' = co) = T[8 - tap'][co .. co+3][ci]      (Wd[ci][co][tap'] = W[co][ci][8 - tap'])
// at the addresses of pack_conv_elem<float, false / true> (tests/test_gpu_train_kernels.py::test_pack_f32_tiles_match_the_elementwise_form).
constexpr int PACKF_T_PITCH = 68, PACKF_SUB_CO = 16;
constexpr int PACKF_LDS = 9 * PACKF_SUB_CO * PACKF_T_PITCH * 4;
inline int packf_blocks(int cout, int cin, int ks) {
  return ks == 3 ? (cout / PACKF_SUB_CO) * (cin / 64) : (int)(((int64_t)cout * cin * ks * ks + PACKF_PER_BLOCK - 1) / PACKF_PER_BLOCK);
}
__device__ __forceinline__ void pack3_f32_subtile(const PackDescF& d, int sub, float* T) {
  const int tid = threadIdx.x;
  const int cit = d.cin >> 6;
  const int cs = sub / cit, cik = sub % cit;          // 16-cout strip, 64-cin block
  const int co0 = cs * PACKF_SUB_CO, ci0 = cik * 64;
  for (int i = tid; i < PACKF_SUB_CO * 144; i += 256) {   // float4 pieces: row i / 144, floats (i % 144) * 4 .. of its 576
    const int r = i / 144, j0 = (i % 144) * 4;
    const float4 v = *reinterpret_cast<const float4*>(d.w + ((int64_t)(co0 + r) * d.cin + ci0) * 9 + j0);
    const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = j0 + k, ci_l = j / 9, tap = j - ci_l * 9;
      T[(tap * PACKF_SUB_CO + r) * PACKF_T_PITCH + ci_l] = f[k];
    }
  }
  __syncthreads();
  // packed element index: (((((cb * nch + ch) * 9 + tap) * 2 + k2) * 2 + mt) * 64 + l) * 4 + e, co = cb*64 + mt*32 + (l & 31), ci = ch*16 + k2*8 + (l >> 5)*4 + e
  const int nch_f = d.cin >> 4, nch_d = d.cout >> 4;
  for (int pc = tid; pc < 2 * 2304; pc += 256) {
    if (pc < 2304) {   // forward operator: 16 rows x 16 four-channel groups x 9 taps
      int q = pc;
      const int r = q & 15; q >>= 4;
      const int half = q & 1; q >>= 1;
      const int k2 = q & 1; q >>= 1;
      const int tap = q % 9, chl = q / 9;               // chl: which 16-channel chunk of the block's 64
      const int ci_l = chl * 16 + k2 * 8 + half * 4;
      const float4 v = *reinterpret_cast<const float4*>(T + (tap * PACKF_SUB_CO + r) * PACKF_T_PITCH + ci_l);
      const int co = co0 + r, cb = co >> 6, mt = (co >> 5) & 1, l = (half << 5) | (co & 31), ch = cik * 4 + chl;
      *reinterpret_cast<float4*>(d.wf + ((((((int64_t)cb * nch_f + ch) * 9 + tap) * 2 + k2) * 2 + mt) * 64 + l) * 4) = v;
    } else {           // dgrad operator: 64 rows (= source cins) x 4 four-cout groups x 9 taps
      int q = pc - 2304;
      const int ci_l = q & 63; q >>= 6;
      const int half = q & 1; q >>= 1;
      const int k2 = q & 1; q >>= 1;
      const int tap = q;                                 // 0..8, the packed operator's tap
      const int g = (k2 * 2 + half) * 4;                 // first of the 4 source couts of this piece inside the strip
      const float* src = T + ((8 - tap) * PACKF_SUB_CO + g) * PACKF_T_PITCH + ci_l;
      const float4 v = make_float4(src[0], src[PACKF_T_PITCH], src[2 * PACKF_T_PITCH], src[3 * PACKF_T_PITCH]);
      const int cop = ci0 + ci_l, cb = cop >> 6, mt = (cop >> 5) & 1, l = (half << 5) | (cop & 31), ch = cs;   // ch: the strip IS one 16-channel chunk
      *reinterpret_cast<float4*>(d.wd + ((((((int64_t)cb * nch_d + ch) * 9 + tap) * 2 + k2) * 2 + mt) * 64 + l) * 4) = v;
    }
  }
}
// `desc` .. `desc + nd`: the convolutions this launch packs, `blk_base` = blk0 of the first (a launch over a sub-range of the table)
__global__ __launch_bounds__(256) void pack_all_f32_kernel(const PackDescF* __restrict__ desc, int nd, int blk_base) {
  extern __shared__ __attribute__((aligned(16))) float packf_lds[];
  const int bid = (int)blockIdx.x + blk_base;
  int i = 0;
  while (i + 1 < nd && bid >= desc[i + 1].blk0) ++i;   // workgroup-uniform scan of ~20 descriptors
  const PackDescF d = desc[i];
  if (d.ks == 3) { pack3_f32_subtile(d, bid - d.blk0, packf_lds); return; }
  const int64_t total = (int64_t)d.cout * d.cin * d.ks * d.ks;
  const int64_t o0 = (int64_t)(bid - d.blk0) * PACKF_PER_BLOCK;
  if (d.ks == 1) {   // 1x1 (downsample branches): the GEMM (gemm1x1_f32.inc) reads the master tensor itself forward; its data gradient the transpose
    for (int64_t o = o0 + threadIdx.x; o < o0 + PACKF_PER_BLOCK && o < total; o += 256) {
      const int ci = (int)(o / d.cout), co = (int)(o % d.cout);
      d.wd[o] = d.w[(int64_t)co * d.cin + ci];   // Wt[cin][cout]
    }
    return;
  }
  for (int64_t o = o0 + threadIdx.x; o < o0 + PACKF_PER_BLOCK && o < total; o += 256) {   // any other kernel size: element by element
    d.wf[o] = pack_conv_elem<float, false>(d.w, d.cout, d.cin, d.ks, o);
    d.wd[o] = pack_conv_elem<float, true>(d.w, d.cout, d.cin, d.ks, o);
  }
}

// stem weights [64][3][7][7] -> f32 stem layout [kh][s][mt][lane] (see pack_stem_weights)
__global__ void pack_stem_dev_kernel(const float* __restrict__ w, float* __restrict__ out) {
  const int total = 7 * 11 * 2 * 64;
  for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < total; o += gridDim.x * blockDim.x) {
    int r = o;
    const int l = r % 64; r /= 64;
    const int mt = r % 2; r /= 2;
    const int s = r % 11; r /= 11;
    const int kh = r;
    const int i = 2 * s + (l >> 5), co = mt * 32 + (l & 31);
    float v = 0.f;
    if (i >= 1 && i <= 21) { const int kw = (i - 1) / 3, c = (i - 1) % 3; v = w[((co * 3 + c) * 7 + kh) * 7 + kw]; }
    out[o] = v;
  }
}

// ---------------- per-channel reductions over NHWC rows ----------------
// MODE 2: {sum g, sum g*xhat}, g = dy*(y>0 if relu)      MODE 3: {sum z, sum z^2}   (the numbers are those of the kernel's first form)
// relu (MODE 2): 0 none, 1 pattern from y, 2 pattern recomputed from z -- y = relu(fma(z, scale, shift)) without an identity term, so
// y > 0 <=> the same fma > 0 (bit-identical to what bn_apply_kernel stored) and y need not be read (a third of the kernel's traffic)
template <int MODE>
__global__ __launch_bounds__(256) void col_reduce_kernel(const float* __restrict__ z, const float* __restrict__ dy,
                                                         const float* __restrict__ y, const float* __restrict__ mean,
                                                         const float* __restrict__ invstd, int64_t rows, int C,
                                                         int relu, float* __restrict__ partial,
                                                         const float* __restrict__ scale = nullptr, const float* __restrict__ shift = nullptr) {
  __shared__ float4 red[2][256];
  const int c4n = C >> 2;                 // float4 lanes per row (16..128)
  const int rpi = 256 / c4n;              // rows per iteration of this workgroup
  const int cl = threadIdx.x % c4n, rl = threadIdx.x / c4n;
  float4 a = make_float4(0, 0, 0, 0), b = make_float4(0, 0, 0, 0);
  float4 mu = make_float4(0, 0, 0, 0), is = make_float4(0, 0, 0, 0);
  if (MODE == 2) { mu = reinterpret_cast<const float4*>(mean)[cl]; is = reinterpret_cast<const float4*>(invstd)[cl]; }
  float4 sc = make_float4(0, 0, 0, 0), sh = make_float4(0, 0, 0, 0);
  if (MODE == 2 && relu == 2) { sc = reinterpret_cast<const float4*>(scale)[cl]; sh = reinterpret_cast<const float4*>(shift)[cl]; }
  for (int64_t r = (int64_t)blockIdx.x * rpi + rl; r < rows; r += (int64_t)gridDim.x * rpi) {
    const float4 v = reinterpret_cast<const float4*>(z + r * C)[cl];
    if (MODE == 3) {
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
      b.x = __builtin_fmaf(v.x, v.x, b.x); b.y = __builtin_fmaf(v.y, v.y, b.y);
      b.z = __builtin_fmaf(v.z, v.z, b.z); b.w = __builtin_fmaf(v.w, v.w, b.w);
    }
    if (MODE == 2) {
      float4 g = reinterpret_cast<const float4*>(dy + r * C)[cl];
      if (relu == 1) {
        const float4 yy = reinterpret_cast<const float4*>(y + r * C)[cl];
        g.x = yy.x > 0.f ? g.x : 0.f; g.y = yy.y > 0.f ? g.y : 0.f;
        g.z = yy.z > 0.f ? g.z : 0.f; g.w = yy.w > 0.f ? g.w : 0.f;
      } else if (relu == 2) {
        g.x = __builtin_fmaf(v.x, sc.x, sh.x) > 0.f ? g.x : 0.f; g.y = __builtin_fmaf(v.y, sc.y, sh.y) > 0.f ? g.y : 0.f;
        g.z = __builtin_fmaf(v.z, sc.z, sh.z) > 0.f ? g.z : 0.f; g.w = __builtin_fmaf(v.w, sc.w, sh.w) > 0.f ? g.w : 0.f;
      }
      a.x += g.x; a.y += g.y; a.z += g.z; a.w += g.w;
      b.x += g.x * ((v.x - mu.x) * is.x); b.y += g.y * ((v.y - mu.y) * is.y);
      b.z += g.z * ((v.z - mu.z) * is.z); b.w += g.w * ((v.w - mu.w) * is.w);
    }
  }
  red[0][threadIdx.x] = a; red[1][threadIdx.x] = b;
  __syncthreads();
  if (rl == 0) {
    for (int k = 1; k < rpi; ++k) {
      const float4 t = red[0][k * c4n + cl], u = red[1][k * c4n + cl];
      a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
      b.x += u.x; b.y += u.y; b.z += u.z; b.w += u.w;
    }
    reinterpret_cast<float4*>(partial + (int64_t)blockIdx.x * 2 * C)[cl] = a;
    reinterpret_cast<float4*>(partial + (int64_t)blockIdx.x * 2 * C + C)[cl] = b;
  }
}

// y = [relu]( z*scale + shift [+ res] )
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ z, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, const float* __restrict__ res,
                                                       float* __restrict__ y, int64_t n4, int C, int relu) {
  // C/4 divides 256 (C = 64 ... 512): a thread meets the same 4 channels in every grid-stride iteration -> coefficients loaded once
  const int c4n = C >> 2;
  const int cl = (int)(threadIdx.x % c4n);
  const float4 sc = reinterpret_cast<const float4*>(scale)[cl], sh = reinterpret_cast<const float4*>(shift)[cl];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(z)[i];
    float4 o = make_float4(__builtin_fmaf(v.x, sc.x, sh.x), __builtin_fmaf(v.y, sc.y, sh.y),
                           __builtin_fmaf(v.z, sc.z, sh.z), __builtin_fmaf(v.w, sc.w, sh.w));
    if (res) { const float4 r = reinterpret_cast<const float4*>(res)[i]; o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w; }
    if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
    reinterpret_cast<float4*>(y)[i] = o;
  }
}

// g = dy*(y>0 if relu);  dz = k0*g + k1*z + k2;  optionally g_out = g (the residual branch's gradient)
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                           const float* __restrict__ z, const float* __restrict__ k0,
                                                           const float* __restrict__ k1, const float* __restrict__ k2,
                                                           float* __restrict__ dz, float* __restrict__ g_out,
                                                           int64_t n4, int C, int relu,
                                                           const float* __restrict__ scale = nullptr, const float* __restrict__ shift = nullptr) {
  const int c4n = C >> 2;
  const int cl = (int)(threadIdx.x % c4n);   // constant over the grid-stride loop (see bn_apply_kernel)
  const float4 a = reinterpret_cast<const float4*>(k0)[cl], b = reinterpret_cast<const float4*>(k1)[cl],
               c = reinterpret_cast<const float4*>(k2)[cl];
  float4 sc = make_float4(0, 0, 0, 0), sh = make_float4(0, 0, 0, 0);
  if (relu == 2) { sc = reinterpret_cast<const float4*>(scale)[cl]; sh = reinterpret_cast<const float4*>(shift)[cl]; }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 g = reinterpret_cast<const float4*>(dy)[i];
    const float4 v = reinterpret_cast<const float4*>(z)[i];
    if (relu == 1) {
      const float4 yy = reinterpret_cast<const float4*>(y)[i];
      g.x = yy.x > 0.f ? g.x : 0.f; g.y = yy.y > 0.f ? g.y : 0.f; g.z = yy.z > 0.f ? g.z : 0.f; g.w = yy.w > 0.f ? g.w : 0.f;
    } else if (relu == 2) {   // pattern from z (col_reduce_kernel)
      g.x = __builtin_fmaf(v.x, sc.x, sh.x) > 0.f ? g.x : 0.f; g.y = __builtin_fmaf(v.y, sc.y, sh.y) > 0.f ? g.y : 0.f;
      g.z = __builtin_fmaf(v.z, sc.z, sh.z) > 0.f ? g.z : 0.f; g.w = __builtin_fmaf(v.w, sc.w, sh.w) > 0.f ? g.w : 0.f;
    }
    float4 o;
    o.x = __builtin_fmaf(a.x, g.x, __builtin_fmaf(b.x, v.x, c.x)); o.y = __builtin_fmaf(a.y, g.y, __builtin_fmaf(b.y, v.y, c.y));
    o.z = __builtin_fmaf(a.z, g.z, __builtin_fmaf(b.z, v.z, c.z)); o.w = __builtin_fmaf(a.w, g.w, __builtin_fmaf(b.w, v.w, c.w));
    reinterpret_cast<float4*>(dz)[i] = o;
    if (g_out) reinterpret_cast<float4*>(g_out)[i] = g;
  }
}

// dx[b][2i][2j][:] += t[b][i][j][:]   (dgrad of the 1x1 stride-2 downsample, step 2)
__global__ __launch_bounds__(256) void upsample2_add_kernel(const float* __restrict__ t, float* __restrict__ dx,
                                                            int B, int Ho, int Wo, int C) {
  const int c4n = C >> 2;
  const int64_t n4 = (int64_t)B * Ho * Wo * c4n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int cl = (int)(i % c4n);
    int64_t r = i / c4n;
    const int x = (int)(r % Wo); r /= Wo;
    const int y = (int)(r % Ho);
    const int b = (int)(r / Ho);
    float4* d = reinterpret_cast<float4*>(dx + (((int64_t)b * 2 * Ho + 2 * y) * 2 * Wo + 2 * x) * C) + cl;
    const float4 v = reinterpret_cast<const float4*>(t)[i];
    float4 o = *d;
    o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
    *d = o;
  }
}

// ---------------- wgrad: dW[co][ci][tap] = sum_px dZ[px][co] * X[px @ tap][ci] ----------------
// One workgroup = one tap x 64 couts x 64 cins x one slab of output pixels; each wave walks
// pixel PAIRS (the K=2 of v_mfma_f32_32x32x2_f32: lane>>5 picks the pixel, lane&31 the channel,
// so both operands are plain coalesced rows of 32 channels); tiles are combined without atomics (below).
struct WgradParams {
  const float* dz; const float* x; float* slabs;   // [n_slabs][Cout][Cin][taps] partial gradients
  int B, Hi, Wi, Cin, Ho, Wo, Cout, KS, STRIDE, PAD;
  int64_t npx; int pairs_per_slab, n_slabs;
};

// One workgroup = one tap x 64 couts x 64 cins x one slab of output pixels.  Per chunk of 32
// pixels the dZ rows and the tap-shifted X rows (256 B each, zero outside the image) are staged
// in LDS with 16-byte loads; wave w then feeds pixel pairs 8w..8w+7 to the MFMA from LDS
// (lanes 0-31 / 32-63 read two rows of 32 consecutive floats: conflict-free).
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradParams p) {
  __shared__ __attribute__((aligned(16))) float lds[2 * 32 * 64];   // [dZ 32x64 | X 32x64]; reused as the 64x64 tile
  float* dzs = lds;
  float* xs = lds + 32 * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int taps = p.KS * p.KS, cot = p.Cout >> 6, cit = p.Cin >> 6;
  int r = blockIdx.x;
  const int ct = r % cit; r /= cit;
  const int ot = r % cot; r /= cot;
  const int tap = r % taps; r /= taps;
  const int slab = r;
  const int kh = tap / p.KS, kw = tap % p.KS;
  const int k = lane >> 5, cl = lane & 31;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
  const int64_t px0 = (int64_t)slab * p.pairs_per_slab * 2;
  const int64_t px1 = min(px0 + (int64_t)p.pairs_per_slab * 2, p.npx);
  const int srow = tid >> 4, scol = (tid & 15) * 4;  // staging: rows srow and srow+16, 4 floats at scol
  for (int64_t base = px0; base < px1; base += 32) {
    float4 dv[2], xv[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t px = base + srow + 16 * u;
      dv[u] = make_float4(0, 0, 0, 0); xv[u] = make_float4(0, 0, 0, 0);
      if (px < px1) {
        dv[u] = *reinterpret_cast<const float4*>(p.dz + px * p.Cout + ot * 64 + scol);
        const int ox = (int)(px % p.Wo);
        const int64_t t = px / p.Wo;
        const int oy = (int)(t % p.Ho), b = (int)(t / p.Ho);
        const int iy = oy * p.STRIDE + kh - p.PAD, ix = ox * p.STRIDE + kw - p.PAD;
        if (iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi)
          xv[u] = *reinterpret_cast<const float4*>(p.x + (((int64_t)b * p.Hi + iy) * p.Wi + ix) * p.Cin + ct * 64 + scol);
      }
    }
    __syncthreads();  // previous chunk consumed
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      *reinterpret_cast<float4*>(dzs + (srow + 16 * u) * 64 + scol) = dv[u];
      *reinterpret_cast<float4*>(xs + (srow + 16 * u) * 64 + scol) = xv[u];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = wave * 8 + 2 * j + k;
      const float a0 = dzs[row * 64 + cl], a1 = dzs[row * 64 + 32 + cl];
      const float b0 = xs[row * 64 + cl], b1 = xs[row * 64 + 32 + cl];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  // The four waves' 64x64 tiles are summed in LDS in a FIXED order (wave 0 stores, waves 1..3 add in turn: every
  // lane owns its own elements, no atomics) and the sum goes to this slab's buffer with plain stores;
  // wgrad_reduce_kernel adds the slabs in a fixed order -> bit-reproducible gradients.
  // D[co][ci]: lane col = ci (lane&31), rows co = (q&3) + 8*(q>>2) + 4*(lane>>5)
  for (int w = 0; w < 4; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            float* e = &lds[(mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * k) * 64 + nt * 32 + cl];
            *e = w == 0 ? acc[mt][nt][q] : *e + acc[mt][nt][q];
          }
    }
  }
  __syncthreads();
  float* out = p.slabs + (int64_t)slab * p.Cout * p.Cin * taps;
  for (int i = tid; i < 64 * 64; i += 256) {
    const int co = ot * 64 + (i >> 6), ci = ct * 64 + (i & 63);
    out[((int64_t)co * p.Cin + ci) * taps + tap] = lds[i];
  }
}

// ---------------- wgrad of the 3x3 convs: all 9 taps from ONE staging of dZ and X ----------------
// One workgroup = 64 couts x 64 cins x a slab of "steps"; a step = R output rows of one image
// (R*Wo <= 64 pixels).  Per step the dZ rows and the X window with halo (((R-1)*s+3) x ((Wo-1)*s+3) pixels,
// zero outside the image) are staged ONCE in LDS (double-buffered; the next step's global loads fly
// under this step's MFMAs) and feed all 9 taps -- the per-tap kernel above re-read both tensors nine times.
// 8 waves: wave = (pair parity g, cout half mt, cin half nt); it owns the nine 32x32 tap tiles of its
// (mt, nt) quadrant (144 accumulator VGPRs) and walks the pixel PAIRS j = g, g+2, ... of the step
// (K = 2 of v_mfma_f32_32x32x2_f32: lane>>5 picks the pixel, lane&31 the channel -> both operands are
// rows of 32 consecutive floats in LDS, conflict-free).  At the end the two parities are summed through
// LDS and the 64x64x9 tile goes to slabs[slab] with plain stores; wgrad_reduce_kernel adds the slabs in
// a fixed order: no atomics, bit-reproducible gradients.
struct Wgrad3Params {
  const float* dz; const float* x; float* slabs;
  int B, Hi, Wi, Cin, Ho, Wo, Cout, STRIDE;
  int R, XR, XC;            // output rows per step; staged window rows / cols (pixels)
  int rb_per_img;           // row blocks per image = ceil(Ho / R)
  int total_steps, steps_per_slab;
  int buf_floats;           // floats per LDS stage buffer (window + dz rows)
  int dzpix;                // dz rows staged per step (R*Wo rounded up to even)
};
constexpr int WG3_MAXX = 7;  // float4 window items per thread (512 threads): 198 px x 16 / 512
constexpr int WG3_MAXD = 2;  // float4 dz items per thread: 64 px x 16 / 512

__global__ __launch_bounds__(512, 2) void wgrad3_kernel(const Wgrad3Params p) {
  extern __shared__ __attribute__((aligned(16))) float wl[];
  int* pixoff = reinterpret_cast<int*>(wl);          // [64] float offset of pixel p inside the window
  float* bufs = wl + 64;                              // 2 stage buffers: [window XR*XC*64 | dz dzpix*64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = wave >> 2, mt = (wave >> 1) & 1, nt = wave & 1;
  const int k = lane >> 5, cl = lane & 31;
  const int cit = p.Cin >> 6, cot = p.Cout >> 6;
  int r = blockIdx.x;
  const int ct = r % cit; r /= cit;
  const int ot = r % cot; r /= cot;
  const int slab = r;
  const int step0 = slab * p.steps_per_slab, step1 = min(step0 + p.steps_per_slab, p.total_steps);
  const int win_floats = p.XR * p.XC * 64;
  if (tid < 64) {
    const int pp = min(tid, p.R * p.Wo - 1);
    pixoff[tid] = ((pp / p.Wo) * p.STRIDE * p.XC + (pp % p.Wo) * p.STRIDE) * 64;
  }
  // staging descriptors (the window geometry is the same for every step)
  const int nx_items = p.XR * p.XC * 16, nd_items = p.dzpix * 16;
  int x_wr[WG3_MAXX], x_ix[WG3_MAXX], x_c4[WG3_MAXX];
#pragma unroll
  for (int u = 0; u < WG3_MAXX; ++u) {
    const int i = tid + 512 * u;
    const int wr = i / (p.XC * 16), rem = i % (p.XC * 16);
    x_wr[u] = i < nx_items ? wr : -4096; x_ix[u] = rem / 16 - 1; x_c4[u] = rem % 16;
  }
  float4 xv[WG3_MAXX], dv[WG3_MAXD];
  auto load_step = [&](int step) __attribute__((always_inline)) {
    const int b = step / p.rb_per_img, oy0 = (step % p.rb_per_img) * p.R;
    const int npix = min(p.R, p.Ho - oy0) * p.Wo;
#pragma unroll
    for (int u = 0; u < WG3_MAXX; ++u) {
      const int iy = oy0 * p.STRIDE - 1 + x_wr[u], ix = x_ix[u];
      xv[u] = make_float4(0, 0, 0, 0);
      if (iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi)
        xv[u] = *reinterpret_cast<const float4*>(p.x + (((int64_t)b * p.Hi + iy) * p.Wi + ix) * p.Cin + ct * 64 + x_c4[u] * 4);
    }
#pragma unroll
    for (int u = 0; u < WG3_MAXD; ++u) {
      const int i = tid + 512 * u, px = i >> 4;
      dv[u] = make_float4(0, 0, 0, 0);
      if (i < nd_items && px < npix)
        dv[u] = *reinterpret_cast<const float4*>(p.dz + (((int64_t)b * p.Ho + oy0) * p.Wo + px) * p.Cout + ot * 64 + (i & 15) * 4);
    }
  };
  auto store_step = [&](int buf) __attribute__((always_inline)) {
    float* xs = bufs + buf * p.buf_floats;
    float* dzs = xs + win_floats;
#pragma unroll
    for (int u = 0; u < WG3_MAXX; ++u)
      if (tid + 512 * u < nx_items) *reinterpret_cast<float4*>(xs + (tid + 512 * u) * 4) = xv[u];
#pragma unroll
    for (int u = 0; u < WG3_MAXD; ++u)
      if (tid + 512 * u < nd_items) *reinterpret_cast<float4*>(dzs + (tid + 512 * u) * 4) = dv[u];
  };
  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
  int tapoff[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) tapoff[t] = ((t / 3) * p.XC + (t % 3)) * 64;

  if (step0 < step1) { load_step(step0); store_step(0); }
  __syncthreads();
  for (int step = step0; step < step1; ++step) {
    const int buf = (step - step0) & 1;
    const bool more = step + 1 < step1;
    if (more) load_step(step + 1);                       // global loads in flight under the MFMAs below
    const float* xs = bufs + buf * p.buf_floats;
    const float* dzs = xs + win_floats;
    const int oy0 = (step % p.rb_per_img) * p.R;
    const int npairs = (min(p.R, p.Ho - oy0) * p.Wo + 1) >> 1;
    for (int j = g; j < npairs; j += 2) {
      const int px = 2 * j + k;                          // this half-wave's pixel (a phantom odd tail has dz = 0)
      const float a = dzs[px * 64 + mt * 32 + cl];
      const float* xb = xs + pixoff[px] + nt * 32 + cl;
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xb[tapoff[t]], acc[t], 0, 0, 0);
    }
    if (more) store_step(buf ^ 1);                       // the other buffer was released by the last barrier
    __syncthreads();
  }
  // parity 1 hands its tiles over through LDS; parity 0 adds them and stores the slab
  float* xch = wl + (wave & 3) * (9 * 16 * 64);
  if (g == 1) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) xch[(t * 16 + q) * 64 + lane] = acc[t][q];
  }
  __syncthreads();
  if (g == 0) {
    float* out = p.slabs + (int64_t)slab * p.Cout * p.Cin * 9;
    const int ci = ct * 64 + nt * 32 + cl;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int co = ot * 64 + mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * k;   // D row of accumulator register q
      // tap-major slab [tap][co][ci]: a half-wave's 32 cins are one 128-byte store (wgrad_reduce_taps_kernel restores [co][ci][tap])
#pragma unroll
      for (int t = 0; t < 9; ++t) out[((int64_t)t * p.Cout + co) * p.Cin + ci] = acc[t][q] + xch[(t * 16 + q) * 64 + lane];
    }
  }
}

// stem wgrad: dW[co][e] = sum_px dZ[px][co] * x[b, c, 2oy+kh-3, 2ox+kw-3], e = (c*7+kh)*7+kw (147, padded
// to 160 = 5 MFMA column tiles).  A workgroup takes a range of output rows (b, oy).  Per row the 7 x 3 input row
// segments it touches (with the 3-pixel halo, zeros outside the image) are staged in LDS with coalesced loads; each
// wave then walks the row's pixel pairs: A = dZ rows (staged too), B = per-lane gather of the 32 e-values of a column
// tile FROM LDS (the first version gathered them from global memory: 21 short segments per pixel, 408 us).  Per-workgroup
// 64x160 tiles go to a slab buffer (plain stores) and a second kernel sums the slabs (no atomics on the 37 KB gradient).
// 8 waves = 4 pixel-pair groups x 2 cout halves: a wave holds 5 accumulator tiles (80 registers).  With all ten tiles in one
// wave (4 waves per workgroup) the kernel needed 336 registers -- one wave per SIMD, the row staging and the MFMAs strictly one
// after the other: 305 us per step against 125 us of f32 MFMA time.
__global__ __launch_bounds__(SWG_T, 2) void stem_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ x, float* __restrict__ slabs,
                                                              int B, int P, int Ho, int Wo, int rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) float swl[];
  const int Wx = P + 6;                       // staged row: columns -3 .. P+2
  float* xs = swl;                            // [21 = (c, kh)][Wx]
  float* dzs = swl + 21 * Wx;                 // [Wo][64]: the row's dZ (per-pair global loads were a latency chain)
  float* tile = swl;                          // reused at the end: [64][160]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pg = wave & 3, mt = wave >> 2;    // pixel-pair group, cout half
  const int k = lane >> 5, cl = lane & 31;
  int eoff[5];
  bool elive[5];
#pragma unroll
  for (int nt = 0; nt < 5; ++nt) {
    const int e = nt * 32 + cl;
    const int kw = e % 7, kh = (e / 7) % 7, c = e / 49;
    elive[nt] = e < 147;
    eoff[nt] = elive[nt] ? (c * 7 + kh) * Wx + kw : 0;
  }
  f32x16 acc[5];
#pragma unroll
  for (int j = 0; j < 5; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
  const int total_rows = B * Ho;
  const int row0 = blockIdx.x * rows_per_block, row1 = min(row0 + rows_per_block, total_rows);
  // Software pipeline over the output rows: the global loads of row r + 1 (21 input-row values of this thread's column, its pieces of the
  // dZ row) are issued BEFORE the MFMAs of row r and land in registers while they run; they are written to LDS after the barrier that
  // ends row r.  (Round 2 staged a row, waited, computed, staged the next: load latency and matrix work strictly alternated, and with
  // 135 registers only one workgroup fits a CU, so nothing else filled the gaps: 262 us against 105 us of f32 MFMA time.)
  float xv[21];
  uint4 dv0 = make_uint4(0, 0, 0, 0), dv1 = dv0, dv2 = dv0, dv3 = dv0;   // named: as an array hipcc parks them in scratch, and the scratch store waits for the loads
  const int xcol = tid;                        // this thread's column of the staged rows (Wx <= SWG_T: checked on the host)
  const int ndz = Wo * 16;   // 16-byte pieces of a dZ row
  // the global loads of row `nr` into xv / dv0..3
#define SWG_LOAD(nr)                                                                                                                   \
  {                                                                                                                                    \
    const int b_ = (nr) / Ho, oy_ = (nr) % Ho;                                                                                         \
    _Pragma("unroll") for (int r = 0; r < 21; ++r) { /* r = c*7 + kh */                                                                \
      const int c = r / 7, kh = r % 7;                                                                                                 \
      const int iy = 2 * oy_ + kh - 3;                                                                                                 \
      xv[r] = 0.f;                                                                                                                     \
      if (xcol < Wx && iy >= 0 && iy < P && xcol >= 3 && xcol < P + 3) xv[r] = x[(((int64_t)b_ * 3 + c) * P + iy) * P + xcol - 3];    \
    }                                                                                                                                  \
    /* the row's dZ: unconditional loads (an index past the row re-reads its last piece, which is then not stored) */                  \
    const uint4* dzr = reinterpret_cast<const uint4*>(dz + (int64_t)(nr) * Wo * 64);                                                   \
    dv0 = dzr[min(tid, ndz - 1)]; dv1 = dzr[min(tid + SWG_T, ndz - 1)];                                                                \
    dv2 = dzr[min(tid + 2 * SWG_T, ndz - 1)]; dv3 = dzr[min(tid + 3 * SWG_T, ndz - 1)];                                                \
  }
  // 152 registers, one workgroup per CU.  (The bf16 engine's stem_wgrad_bf16_kernel is NOT pipelined: two workgroups per CU cover each other's
  // staging there, profiles/r03_exp_stem.txt.)
  for (int row = row0 - 1; row < row1; ++row) {        // iteration row0 - 1 only loads
    if (row >= row0) {
      __syncthreads();                          // previous row consumed
      if (xcol < Wx) {
#pragma unroll
        for (int r = 0; r < 21; ++r) xs[r * Wx + xcol] = xv[r];
      }
      auto put = [&](const uint4& d, int u) __attribute__((always_inline)) {
        const int i = tid + SWG_T * u;
        if (i < ndz) reinterpret_cast<uint4*>(dzs)[i] = d;
      };
      put(dv0, 0); put(dv1, 1); put(dv2, 2); put(dv3, 3);
      __syncthreads();
    }
    if (row + 1 < row1) SWG_LOAD(row + 1)   // in flight during the MFMAs below
    if (row >= row0) {
      for (int pp = pg; 2 * pp < Wo; pp += 4) {
        const int ox = 2 * pp + k;
        float a0 = 0.f, bv[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (ox < Wo) {
          a0 = dzs[ox * 64 + mt * 32 + cl];
#pragma unroll
          for (int nt = 0; nt < 5; ++nt) bv[nt] = elive[nt] ? xs[eoff[nt] + 2 * ox] : 0.f;
        }
#pragma unroll
        for (int nt = 0; nt < 5; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv[nt], acc[nt], 0, 0, 0);
      }
    }
  }
#undef SWG_LOAD
  for (int w = 0; w < 4; ++w) {   // fixed-order combine of the four pixel-pair groups (no float atomics: reproducible)
    __syncthreads();
    if (pg == w) {
#pragma unroll
      for (int nt = 0; nt < 5; ++nt)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          float* e = &tile[(mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * k) * 160 + nt * 32 + cl];
          *e = w == 0 ? acc[nt][q] : *e + acc[nt][q];
        }
    }
  }
  __syncthreads();
  for (int i = tid; i < 64 * 160; i += SWG_T) slabs[(int64_t)blockIdx.x * (64 * 160) + i] = tile[i];
}

// maxpool 3x3/2 pad 1 for training: the forward also records, per output element, WHICH window element
// was the first maximum (row-major scan, torch's tie rule) as a byte 0..8; the backward then lets every
// input pixel ask its (at most 4) windows "was it me?" -- 4 byte + 4 float loads instead of re-scanning
// 4 x 8 neighbours.
__global__ __launch_bounds__(256) void maxpool_fwd_idx_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                              uint8_t* __restrict__ idx, int B, int Hi, int Wi, int C,
                                                              int Ho, int Wo) {
  const int c4n = C >> 2;
  const int64_t n4 = (int64_t)B * Ho * Wo * c4n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int cl = (int)(i % c4n);
    int64_t r = i / c4n;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int dyy = 0; dyy < 3; ++dyy) {
      const int yy = 2 * oy + dyy - 1;
      if (yy < 0 || yy >= Hi) continue;
#pragma unroll
      for (int dxx = 0; dxx < 3; ++dxx) {
        const int xx = 2 * ox + dxx - 1;
        if (xx < 0 || xx >= Wi) continue;
        const float4 v = reinterpret_cast<const float4*>(x + (((int64_t)b * Hi + yy) * Wi + xx) * C)[cl];
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (vv[q] > m[q]) { m[q] = vv[q]; w[q] = dyy * 3 + dxx; }   // strict: the earlier element keeps a tie
      }
    }
    reinterpret_cast<float4*>(y)[i] = make_float4(m[0], m[1], m[2], m[3]);
    reinterpret_cast<uchar4*>(idx)[i] = make_uchar4((uint8_t)w[0], (uint8_t)w[1], (uint8_t)w[2], (uint8_t)w[3]);
  }
}

__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const uint8_t* __restrict__ idx, const float* __restrict__ dy,
                                                          float* __restrict__ dx, int B, int Hi, int Wi, int C,
                                                          int Ho, int Wo) {
  const int c4n = C >> 2;
  const int64_t n4 = (int64_t)B * Hi * Wi * c4n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int cl = (int)(i % c4n);
    int64_t r = i / c4n;
    const int ix = (int)(r % Wi); r /= Wi;
    const int iy = (int)(r % Hi);
    const int b = (int)(r / Hi);
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    for (int oy = iy / 2; oy <= (iy + 1) / 2; ++oy) {
      if (oy >= Ho) continue;
      for (int ox = ix / 2; ox <= (ix + 1) / 2; ++ox) {
        if (ox >= Wo) continue;
        const int me = (iy - (2 * oy - 1)) * 3 + (ix - (2 * ox - 1));   // my position in that window
        const int64_t e = (((int64_t)b * Ho + oy) * Wo + ox) * c4n + cl;
        const uchar4 w = reinterpret_cast<const uchar4*>(idx)[e];
        const float4 g = reinterpret_cast<const float4*>(dy)[e];
        if (w.x == me) o[0] += g.x;
        if (w.y == me) o[1] += g.y;
        if (w.z == me) o[2] += g.z;
        if (w.w == me) o[3] += g.w;
      }
    }
    reinterpret_cast<float4*>(dx)[i] = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// ---- the stem's tail in one pass each way (round 3; see bn2_apply_pool_kernel / bn2_pool_bwd_* of the bf16 engine) ----
// forward: pooled = maxpool3x3/2(relu(fma(z, scale, shift))) + first-maximum positions straight from Z: the same float32 values the pair
// bn_apply_kernel + maxpool_fwd_idx_kernel compares, so maxima and positions are identical; the normalised 112 x 112 map is never stored.
__global__ __launch_bounds__(256) void bn_apply_pool_kernel(const float* __restrict__ z, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, float* __restrict__ y, uint8_t* __restrict__ idx,
                                                            int B, int Hi, int Wi, int C, int Ho, int Wo) {
  const int c4n = C >> 2;
  const int cf = (int)(threadIdx.x % c4n);   // 256 % c4n == 0: the same 4 channels in every grid-stride iteration
  const float4 sc = reinterpret_cast<const float4*>(scale)[cf], sh = reinterpret_cast<const float4*>(shift)[cf];
  const int64_t n4 = (int64_t)B * Ho * Wo * c4n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int cl = (int)(i % c4n);
    int64_t r = i / c4n;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int dyy = 0; dyy < 3; ++dyy) {
      const int yy = 2 * oy + dyy - 1;
      if (yy < 0 || yy >= Hi) continue;
#pragma unroll
      for (int dxx = 0; dxx < 3; ++dxx) {
        const int xx = 2 * ox + dxx - 1;
        if (xx < 0 || xx >= Wi) continue;
        const float4 v = reinterpret_cast<const float4*>(z + (((int64_t)b * Hi + yy) * Wi + xx) * C)[cl];
        const float vv[4] = {fmaxf(__builtin_fmaf(v.x, sc.x, sh.x), 0.f), fmaxf(__builtin_fmaf(v.y, sc.y, sh.y), 0.f),
                             fmaxf(__builtin_fmaf(v.z, sc.z, sh.z), 0.f), fmaxf(__builtin_fmaf(v.w, sc.w, sh.w), 0.f)};
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (vv[q] > m[q]) { m[q] = vv[q]; w[q] = dyy * 3 + dxx; }   // strict: the earlier element keeps a tie
      }
    }
    reinterpret_cast<float4*>(y)[i] = make_float4(m[0], m[1], m[2], m[3]);
    reinterpret_cast<uchar4*>(idx)[i] = make_uchar4((uint8_t)w[0], (uint8_t)w[1], (uint8_t)w[2], (uint8_t)w[3]);
  }
}

// maxpool gradient of the 2 x 2 block of input pixels (2a + py, 2q + px), 4 channels each: its four windows (a + wy, q + wx) are loaded once;
// window (wy, wx) reaches pixel (py, px) at its position (py + 1 - 2 wy, px + 1 - 2 wx) when both are >= 0.  g[2 py + px]; the same sums of
// at most four terms, in the same order, as maxpool_bwd_kernel.
struct PoolGrad4F { float g[4][4]; };
__device__ __forceinline__ PoolGrad4F pool_grad_2x2_f32(const uint8_t* __restrict__ idx, const float* __restrict__ dpool, int b, int a, int q,
                                                        int cl, int c4n, int Ho, int Wo) {
  PoolGrad4F o;
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) o.g[k][e] = 0.f;
#pragma unroll
  for (int wy = 0; wy < 2; ++wy)
#pragma unroll
    for (int wx = 0; wx < 2; ++wx) {
      const int oy = a + wy, ox = q + wx;
      if (oy >= Ho || ox >= Wo) continue;
      const int64_t e4 = (((int64_t)b * Ho + oy) * Wo + ox) * c4n + cl;
      const uchar4 w = reinterpret_cast<const uchar4*>(idx)[e4];
      const float4 g = reinterpret_cast<const float4*>(dpool)[e4];
#pragma unroll
      for (int py = wy; py < 2; ++py)
#pragma unroll
        for (int px = wx; px < 2; ++px) {
          const int me = (py + 1 - 2 * wy) * 3 + (px + 1 - 2 * wx);
          if (w.x == me) o.g[2 * py + px][0] += g.x;
          if (w.y == me) o.g[2 * py + px][1] += g.y;
          if (w.z == me) o.g[2 * py + px][2] += g.z;
          if (w.w == me) o.g[2 * py + px][3] += g.w;
        }
    }
  return o;
}

// col_reduce_kernel<2> (relu == 2) with dy = the maxpool's gradient gathered on the fly; a "row" is a 2 x 2 pixel block of Z
__global__ __launch_bounds__(256) void bn_pool_bwd_reduce_kernel(const float* __restrict__ z, const float* __restrict__ dpool,
                                                                 const uint8_t* __restrict__ idx, const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, int B, int Hi, int Wi, int C, int Ho, int Wo,
                                                                 float* __restrict__ partial) {
  __shared__ float4 red[2][256];
  const int c4n = C >> 2;
  const int rpi = 256 / c4n;
  const int cl = threadIdx.x % c4n, rl = threadIdx.x / c4n;
  const int Hb = (Hi + 1) >> 1, Wb = (Wi + 1) >> 1;
  const int64_t rows = (int64_t)B * Hb * Wb;
  const float4 mu4 = reinterpret_cast<const float4*>(mean)[cl], is4 = reinterpret_cast<const float4*>(invstd)[cl];
  const float4 sc4 = reinterpret_cast<const float4*>(scale)[cl], sh4 = reinterpret_cast<const float4*>(shift)[cl];
  const float mu[4] = {mu4.x, mu4.y, mu4.z, mu4.w}, is[4] = {is4.x, is4.y, is4.z, is4.w};
  const float sc[4] = {sc4.x, sc4.y, sc4.z, sc4.w}, sh[4] = {sh4.x, sh4.y, sh4.z, sh4.w};
  float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t r = (int64_t)blockIdx.x * rpi + rl; r < rows; r += (int64_t)gridDim.x * rpi) {
    const int qx = (int)(r % Wb);
    const int64_t t = r / Wb;
    const int ay = (int)(t % Hb), bb = (int)(t / Hb);
    float4 v4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // pixels past an odd map's edge re-read the block's first pixel with weight 0
      const int iy = 2 * ay + (k >> 1), ix = 2 * qx + (k & 1);
      const bool ok = iy < Hi && ix < Wi;
      v4[k] = reinterpret_cast<const float4*>(z + (((int64_t)bb * Hi + (ok ? iy : 2 * ay)) * Wi + (ok ? ix : 2 * qx)) * C)[cl];
    }
    const PoolGrad4F pg = pool_grad_2x2_f32(idx, dpool, bb, ay, qx, cl, c4n, Ho, Wo);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = 2 * ay + (k >> 1) < Hi && 2 * qx + (k & 1) < Wi;
      const float v[4] = {v4[k].x, v4[k].y, v4[k].z, v4[k].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gg = (ok && __builtin_fmaf(v[e], sc[e], sh[e]) > 0.f) ? pg.g[k][e] : 0.f;
        a[e] += gg;
        b[e] += gg * ((v[e] - mu[e]) * is[e]);
      }
    }
  }
  red[0][threadIdx.x] = make_float4(a[0], a[1], a[2], a[3]); red[1][threadIdx.x] = make_float4(b[0], b[1], b[2], b[3]);
  __syncthreads();
  if (rl == 0) {
    float4 sa = red[0][cl], sb = red[1][cl];
    for (int k = 1; k < rpi; ++k) {
      const float4 t = red[0][k * c4n + cl], u = red[1][k * c4n + cl];
      sa.x += t.x; sa.y += t.y; sa.z += t.z; sa.w += t.w;
      sb.x += u.x; sb.y += u.y; sb.z += u.z; sb.w += u.w;
    }
    reinterpret_cast<float4*>(partial + (int64_t)blockIdx.x * 2 * C)[cl] = sa;
    reinterpret_cast<float4*>(partial + (int64_t)blockIdx.x * 2 * C + C)[cl] = sb;
  }
}

// bn_bwd_apply_kernel (relu == 2) with dy gathered as above: dz = k0*g + k1*z + k2, one 2 x 2 pixel block per thread and iteration
__global__ __launch_bounds__(256) void bn_pool_bwd_apply_kernel(const float* __restrict__ z, const float* __restrict__ dpool,
                                                                const uint8_t* __restrict__ idx, const float* __restrict__ k0,
                                                                const float* __restrict__ k1, const float* __restrict__ k2,
                                                                const float* __restrict__ scale, const float* __restrict__ shift,
                                                                float* __restrict__ dz, int B, int Hi, int Wi, int C, int Ho, int Wo) {
  const int c4n = C >> 2;
  const int cf = (int)(threadIdx.x % c4n);
  const float4 a4 = reinterpret_cast<const float4*>(k0)[cf], b4 = reinterpret_cast<const float4*>(k1)[cf], c4 = reinterpret_cast<const float4*>(k2)[cf];
  const float4 sc4 = reinterpret_cast<const float4*>(scale)[cf], sh4 = reinterpret_cast<const float4*>(shift)[cf];
  const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w}, c[4] = {c4.x, c4.y, c4.z, c4.w};
  const float sc[4] = {sc4.x, sc4.y, sc4.z, sc4.w}, sh[4] = {sh4.x, sh4.y, sh4.z, sh4.w};
  const int Hb = (Hi + 1) >> 1, Wb = (Wi + 1) >> 1;
  const int64_t n4 = (int64_t)B * Hb * Wb * c4n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int cl = (int)(i % c4n);
    int64_t r = i / c4n;
    const int qx = (int)(r % Wb); r /= Wb;
    const int ay = (int)(r % Hb);
    const int bb = (int)(r / Hb);
    float4 v4[4];
    int64_t at[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int iy = 2 * ay + (k >> 1), ix = 2 * qx + (k & 1);
      ok[k] = iy < Hi && ix < Wi;
      at[k] = (((int64_t)bb * Hi + (ok[k] ? iy : 2 * ay)) * Wi + (ok[k] ? ix : 2 * qx)) * C;
      v4[k] = reinterpret_cast<const float4*>(z + at[k])[cl];
    }
    const PoolGrad4F pg = pool_grad_2x2_f32(idx, dpool, bb, ay, qx, cl, c4n, Ho, Wo);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float v[4] = {v4[k].x, v4[k].y, v4[k].z, v4[k].w};
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gg = __builtin_fmaf(v[e], sc[e], sh[e]) > 0.f ? pg.g[k][e] : 0.f;
        o[e] = __builtin_fmaf(a[e], gg, __builtin_fmaf(b[e], v[e], c[e]));
      }
      if (ok[k]) reinterpret_cast<float4*>(dz + at[k])[cl] = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

// global average pool (training forward keeps `pooled`), fc forward
__global__ __launch_bounds__(256) void avgpool_kernel(const float* __restrict__ x, int HW, int C, float* __restrict__ pooled) {
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += 256) {
    float s = 0.f;
    for (int q = 0; q < HW; ++q) s += x[((int64_t)b * HW + q) * C + c];
    pooled[(int64_t)b * C + c] = s / (float)HW;
  }
}
// dX[b][q][c] = (sum_k dl[b][k]*w[k][c]) / HW
__global__ __launch_bounds__(256) void avgpool_fc_dgrad_kernel(const float* __restrict__ dl, const float* __restrict__ w,
                                                               int HW, int C, int n_cls, float* __restrict__ dx) {
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += 256) {
    float s = 0.f;
    for (int k = 0; k < n_cls; ++k) s = __builtin_fmaf(dl[b * n_cls + k], w[k * C + c], s);
    s /= (float)HW;
    for (int q = 0; q < HW; ++q) dx[((int64_t)b * HW + q) * C + c] = s;
  }
}

}  // namespace
