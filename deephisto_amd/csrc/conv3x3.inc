// conv3x3.inc -- 3x3 convolution (stride 1 or 2, pad 1) as an LDS-staged implicit GEMM.
// Included inside the anonymous namespace of resnet_kernels.hip.
//
// Tile = 64 couts x (WAVES*NT*32) output pixels (IMGS images x TH x TW).  Per 64-byte
// channel chunk ("stage"):
//   * the input window of the output patch (patch + halo; for stride 2 the columns are
//     split by parity into two planes so that a wave's 32 pixels stay contiguous) sits in
//     LDS once and all 9 taps read shifted views of it (LDS-staged im2col);
//   * the chunk's weight slab (9 taps, pre-packed in MFMA fragment order) sits next to it.
// LDS pixel pitch is 64 B; the four 16-byte slots of a pixel are XOR-swizzled with bits
// 2..3 of the pixel index, so a ds_read_b128 of 32 consecutive pixels is conflict-free
// for every tap shift.
//
// Data movement is LDS-DMA (`global_load_lds_dwordx4`, 1 KiB per wave-instruction): weights
// are a linear copy; window pixels are gathered through the per-lane SOURCE address (the
// swizzle and the zero padding -- a lane outside the image reads a zero page -- live there,
// the LDS image stays lane-linear).  No staging registers, no VGPR->LDS write pass.
//
// Schedule: PERSISTENT workgroups, one per CU, walking a flat stream of (tile, chunk)
// stages over a 2-deep LDS ring: the DMA of stage s+1 is issued before the MFMAs of stage
// s and retired by the vmcnt(0)+barrier that ends stage s.  A finished tile's epilogue (BN
// scale/shift from LDS, residual prefetched at the tile's first stage, ReLU, stores) runs
// after the next stage's DMA has been issued, so its stores drain under the next MFMAs.
// MFMA operand fragments are double-buffered in registers.  (History: a one-tile-per-
// workgroup version ran its load / MFMA / store phases each near their roofline but
// serialised chip-wide; register-staged persistent versions lost the gain to per-stage
// address arithmetic and exposed latencies -- see DESIGN.md.)
struct Conv3Params {
  const void* in; const void* w; const float* scale; const float* shift; const void* res; void* out;
  const void* zero_page;  // >= 64 B of zeros in HBM (source of padding pixels)
  // optional fused 1x1 / stride-2 downsample branch of the same ResNet block (DS variants): its only tap is the
  // centre tap of this 3x3 / stride-2 window, so it rides on the staged pixels; own weights, BN, output
  const void* ds_w; const float* ds_scale; const float* ds_shift; void* ds_out;
  int B, Hi, Wi, Cin, Ho, Wo, Cout;
  // Activation layout.  NHWC: a pixel's channels are contiguous (pixel stride C elements, chunk stride one chunk).
  // Channel-blocked (bf16 inference): [image][C/32][H][W][32] -- the 64-byte chunk of consecutive pixels of a row is
  // contiguous, so the staged window rows are read as whole cache lines (-4...-14 % per layer).
  int in_px_bytes, in_chunk_bytes;     // byte stride between horizontally adjacent pixels / between channel chunks
  int out_px, out_cb, out_mt;          // element strides of the output: pixel, 64-cout block, 32-cout half
  int out_pr;                          // ... and between the two 16-cout halves of a 32-cout tile (16, or a plane of the 16-channel-blocked layout)
  // the residual has its OWN layout (round 4: the last conv of a stage may write 16-channel planes for the wide stride-2 kernel that
  // follows while its residual, the block input, is in 32-channel planes): strides as above; r_row / r_px / r_cb feed the host tables
  int res_mt, res_pr, r_row, r_px, r_cb, r_base;
  // output placement used by the host tables only: elements per image, per tile row, per tile pixel, and of the first pixel.
  // A plain convolution writes a dense [Ho][Wo] map (o_img = Ho Wo C, o_row = Wo out_px, o_px = out_px, o_base = 0); a parity
  // class of a stride-2 data gradient (CLS >= 0) writes every second pixel of every second row of the full-size dX.
  int64_t o_img; int o_row, o_px, o_base;
  int cls_base[4];       // CLS == 4: element offset of class c's first pixel in dX ((py * W + px) * Cout)
  int TH, TW, IMGS;      // output patch: IMGS x TH x TW = WAVES*NT*32 pixels
  int tiles_y, tiles_x;
  int HR, HC, HP, HPH;   // staged window: rows, real cols, row pitch (px), parity-plane pitch (stride 2)
  int WTAIL = 0;         // window pixels behind the last image segment (fit tiles with shared halos: conv3_tables_host.h; 0 otherwise)
  int FIT = 0;           // fit tile: IMGS * TH * TW <= the workgroup's slots, lanes dealt to pixels by the host (conv3_tables_host.h)
  int IP = 0;            // host tables only: pixels between the image segments of the window (HR * HP, or more in a fit window)
  int n_win_instr;       // DMA wave-instructions per window = ceil((IMGS*HR*HP + WTAIL) / 16)
  int relu;
  int ntiles, iters;     // tiles in the launch; tile iterations per workgroup
  unsigned long long* stamps;  // optional phase-cycle accumulators (diagnostic variant only)
  const int* lane_tab;         // host-built per-thread geometry: [threads][3*NT + MAXJ] = {out_rel[NT], base_lin[NT], res_rel[NT], rel_off[MAXJ]}
  const int4* tile_tab;        // host-built schedule: [iters][grid] x {cout block | valid << 16 | mask row << 20, window byte offset,
                               //                                        output element offset (incl. cout block), residual element offset}
  const unsigned* mask_tab;    // host-built [mask rows][threads]: bits 0..MAXJ-1 window piece j inside the image, bits 16.. pixel nt exists
};

#ifndef DH_CONV_HOIST
#define DH_CONV_HOIST 1   /* per-lane tap offsets of the window fragments computed once per kernel (0: per k-step, the round-3 form) */
#endif
#ifndef DH_ABL
#define DH_ABL 0   /* timing-only ablations (tools/build_variant.sh): 1 no MFMA, 2 no operand DMA, 4 no output stores, 8 no LDS fragment reads, 16 output stores to coalesced (wrong) addresses, 32 residual loads likewise, 64 no residual loads */
#endif
typedef __attribute__((address_space(1))) const void* dh_gptr_t;
typedef __attribute__((address_space(3))) void* dh_lptr_t;

// LDS-DMA as inline asm.  With the builtin, hipcc (ROCm 7.2) cannot prove that the ds_reads of
// ring slot s do not alias the DMA writes into slot s+1 and drains `vmcnt(0)` before every LDS
// read that follows a DMA -- the prefetch then runs serially with the MFMAs it was meant to
// hide under.  The asm form is invisible to that bookkeeping: completion is awaited by the
// explicit `s_waitcnt vmcnt(0)` in stage_barrier().  M0 (LDS destination base) is saved and
// restored inside the statement; the s_nop covers the M0 write -> LDS-DMA hazard.
// The compiler's own counted vmcnt waits stay safe: vmcnt retires in issue order, so untracked
// younger DMAs can only make such a wait longer, never shorter.
template <int BYTES>
__device__ __forceinline__ void lds_dma(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  if constexpr (BYTES == 16)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
  else
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ unsigned lds_addr_of(const void* p) {  // 32-bit LDS byte address of a __shared__ pointer
  return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}
__device__ __forceinline__ void stage_barrier() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // my DMAs landed; my LDS reads retired
  __builtin_amdgcn_s_barrier();                                  // ... and everyone else's
  asm volatile("" ::: "memory");
}

// base + one 16-bit half of `packed`, in ONE instruction (SDWA operand select), as opaque asm: written in C++ the compiler hoists the unpacking of
// the nine packed tap offsets out of the stage loop and is back at eighteen registers (conv3x3_body, HOIST).  Not volatile: a volatile asm fences the
// LDS reads around it and the fragment prefetch collapses into read - wait - MFMA.
template <int HI>
__device__ __forceinline__ unsigned add_half16(unsigned base, unsigned packed) {
  unsigned r;
  if constexpr (HI) asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(r) : "v"(base), "v"(packed));
  else asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(r) : "v"(base), "v"(packed));
  return r;
}
__device__ __forceinline__ unsigned xor_opaque(unsigned a, unsigned b) {
  unsigned r;
  asm("v_xor_b32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ const uint4* lds_ptr128(unsigned addr) {   // 32-bit LDS byte address -> pointer
  return (const uint4*)(__attribute__((address_space(3))) const uint4*)(uintptr_t)addr;
}

__device__ __forceinline__ int lds_slot_addr(int px_lin, int slot) {
  return px_lin * CHUNK_BYTES + ((slot ^ ((px_lin >> 2) & 3)) << 4);
}
// HALF stages (32 bytes = 16 channels per pixel): two 16-byte slots per pixel, swapped on pixels with bit 3 set -- a ds_read_b128 of
// 32 consecutive pixels (or of two 16-pixel rows in conv3_tables_host.h's lane order) then touches 16 different 16-byte bank groups
// per 16-lane service group
__device__ __forceinline__ int lds_slot_addr_half(int px_lin, int slot) {
  return px_lin * 32 + ((slot ^ ((px_lin >> 3) & 1)) << 4);
}

// CLS >= 0: one PARITY CLASS of the data gradient of a stride-2 convolution (round 3).  dX = conv_stride1(zero-upsampled dZ, Wd)
// spends three quarters of its MFMAs on the inserted zeros; split by the parity (py, px) = (CLS >> 1, CLS & 1) of the dX pixel,
//   dX[2i + py][2j + px] = sum over the taps (kh', kw') of Wd with kh' = 1 (py = 0) or kh' in {0, 2} (py = 1), kw' likewise,
//                          of dZ[i + (kh' == 2)][j + (kw' == 2)] . Wd[kh'][kw'],
// i.e. four stride-1 convolutions over dZ itself with 1, 2, 2 and 4 taps (9 in all instead of 36 tap-pixels per 2 x 2 block),
// reading the SAME packed operator Wd (only the used taps' slabs are DMA'd) and the same 3 x 3 window geometry (window position
// (1 + (kh' == 2), 1 + (kw' == 2)) of the (TH + 2) x (TW + 2) window), writing every second pixel of every second row of dX
// (the host tables carry the output pitches).
// CLS == 4 (round 3, late): ALL four classes from ONE staged dZ window -- the nine taps of Wd each feed the accumulator set of the class
// they belong to ((kh' != 1) << 1 | (kw' != 1)), read at window position (1 + (kh' == 2), 1 + (kw' == 2)).  Same window staging and the
// same MFMA count as a stride-1 convolution over the dZ grid, four output pixels per window pixel (a class launch re-stages the
// window for a quarter of the arithmetic: the merged class launches ran 3-4x longer than a convolution of their FLOPs).
template <int CLS> struct TapSet {
  static constexpr int NY = (CLS < 0 || CLS == 4) ? 3 : ((CLS >> 1) ? 2 : 1), NX = (CLS < 0 || CLS == 4) ? 3 : ((CLS & 1) ? 2 : 1), N = NY * NX;
  static constexpr int wrow(int a) { return (CLS < 0 || CLS == 4) ? a : ((CLS >> 1) ? 2 * a : 1); }   // tap row of the packed operator
  static constexpr int wcol(int b) { return (CLS < 0 || CLS == 4) ? b : ((CLS & 1) ? 2 * b : 1); }
  static constexpr int srow(int a) { return CLS < 0 ? a : CLS == 4 ? (a == 2 ? 2 : 1) : 1 + a; }       // row of the staged window
  static constexpr int scol(int b) { return CLS < 0 ? b : CLS == 4 ? (b == 2 ? 2 : 1) : 1 + b; }
  static constexpr int cls_of(int a, int b) { return CLS == 4 ? (((a != 1) ? 2 : 0) | ((b != 1) ? 1 : 0)) : 0; }   // accumulator set of tap (a, b)
  static constexpr unsigned wmask() {   // bit t: tap slab t of the packed operator is read
    unsigned m = 0;
    for (int a = 0; a < NY; ++a) for (int b = 0; b < NX; ++b) m |= 1u << (wrow(a) * 3 + wcol(b));
    return m;
  }
};

// MT = cout tiles (of 32) per wave: 2 -> a wave covers all 64 couts of its pixels; 1 -> waves come in pairs
// that share pixels and split the couts (stride-2 variant: twice the waves on the same 128-pixel tile, so two
// waves per SIMD hide each other's LDS latency).
//
// WRES ("weights resident"): when all weight slabs of ONE cout block fit beside the window ring (cin = 64 in bf16:
// 2 x 36 KiB, + 2 x 4 KiB with the fused downsample), they are DMA'd once per workgroup and every stage moves only
// its window -- half the operand ingest of the layers that are most ingest-bound (layer 1, the 64->128 stride-2 conv).
// The kernel body as a device function of (workgroup index, workgroup count, schedule): conv3x3_kernel runs it over the whole launch;
// conv3x3_s2dgrad_kernel gives each of the four parity classes of a stride-2 data gradient its own range of workgroups in ONE launch.
// HALF (round 4; stride 2 + fused downsample, bf16, channel-blocked input): the stride-2 kernel stages 77 KB per 20 MFMAs per wave -- 120 GB/s
// per CU at 1.9 GHz, 2-4x what a CU ingests, and its waves wait for their OWN DMA (profiles/r04_conv_phase_stamps.txt).  HALF doubles the
// FLOPs per staged byte twice over: a stage is HALF a channel chunk (16 channels = one k-step per tap: window 36 KB for 256 pixels
// instead of 37 KB for 128) and a workgroup owns 128 couts (the four 32-cout MFMA row tiles of a tap are one 4 KiB slab, so the
// weight image per stage stays 36 + 4 KiB).  Wave = (pixel group of 64 = wave >> 1, cout half = wave & 1): MT = 2 row tiles x NT = 2
// pixel tiles, four LDS fragment reads per four MFMAs as in the stride-1 kernel.
//
// M16 (bf16, stride 1, CLS < 0): the stage's MFMAs are v_mfma_f32_16x16x32_bf16 -- one 64-byte channel chunk of a tap is ONE k-step of 32 channels
// instead of two of 16 on 32x32x16.  Same wave tile (MT x NT blocks of 32 couts x 32 pixels = 2 x 2 tiles of 16 x 16 each), same LDS images, same
// MFMA cycles; the smaller shape costs less energy per FLOP and the chip holds a higher clock under it (DESIGN.md 4.2).  Lane l = (column c = l & 15,
// group G = l >> 4): operands are the 8 channels of chunk slot sigma(G) = (0, 2, 1, 3)[G] of cout 16 m + c (A) / of the pixel in column c (B);
// D holds couts 16 m + 4 G + {0..3} of that pixel.  Which pixel a column of a 16-pixel tile stands for is dealt by the host so that the window
// reads stay conflict-free (conv3_tables_host.h, M16).
template <typename T, int STRIDE, int NT, int WAVES, bool STAMP, bool DS, int MT, bool WRES = false, int CLS = -1, bool HALF = false, bool M16 = false>
__device__ __forceinline__ void conv3x3_body(const Conv3Params& p, const int wg, const int nwg, const int n_iters, const int* __restrict__ lane_tab,
                                             const int4* __restrict__ tile_tab, const unsigned* __restrict__ mask_tab) {
  static_assert(!DS || STRIDE == 2, "the fused downsample rides on the stride-2 kernel");
  static_assert(CLS < 0 || (STRIDE == 1 && !DS && !WRES && CLS <= 4), "parity classes: stride-1 kernel, streamed weights");
  static_assert(CLS != 4 || NT == 1, "all four classes at once: four accumulator sets, 256-pixel tiles at most");
  static_assert(!HALF || (STRIDE == 2 && DS && MT == 2 && NT == 2 && WAVES == 8 && !WRES && CLS < 0 && sizeof(T) == 2), "HALF: the wide stride-2 variant");
  static_assert(!M16 || (sizeof(T) == 2 && STRIDE == 1 && CLS < 0 && !DS && !HALF), "M16: the stride-1 bf16 kernels on whole-chunk stages");
  typedef TapSet<CLS> TS;
  constexpr int KSTEPS = (HALF || M16 ? 1 : 2) * TS::N;   // k-steps per stage: two per tap (HALF stages, M16: one)
  constexpr int NB = M16 ? 2 * NT : NT;                  // window fragments (pixel tiles) per k-step

  static_assert(MT == 1 || MT == 2, "MT");
  constexpr int ESZ = ElemTraits<T>::ESZ;
  constexpr int STAGE_PX_BYTES = HALF ? CHUNK_BYTES / 2 : CHUNK_BYTES;   // bytes of a pixel staged per stage
  constexpr int CPC = STAGE_PX_BYTES / ESZ;
  constexpr int WSLAB = 9 * SLAB_TAP;                       // 36 KiB of weights per stage
  constexpr int WTOT = WSLAB + (DS ? SLAB_TAP : 0);         // + 4 KiB: the 1x1 downsample's slab
  constexpr int WJ = (WTOT / 1024 + WAVES - 1) / WAVES;     // weight DMA instructions per wave
  constexpr int MAXJ = (STRIDE == 2) ? (WAVES == 8 ? 5 : 10) : (NT == 2 ? 6 : 4);  // window DMA instructions per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const unsigned long long t_entry = STAMP ? __builtin_readcyclecounter() : 0ull;
  const unsigned long long rt_entry = STAMP ? __builtin_amdgcn_s_memrealtime() : 0ull;  // 100 MHz
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
  const int G = lane >> 4;   // M16: the lane's k group (operands) / group of four couts (accumulators)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mt0 = HALF ? 2 * (wave & 1) : MT == 2 ? 0 : (wave & 1);   // first cout tile of this wave
  const int win_bytes = (p.IMGS * p.HR * p.HP + p.WTAIL) * STAGE_PX_BYTES;
  const int nchunks = p.Cin / CPC;
  // ring slot = [weight slab | window]; WRES: [all weight slabs][window | window]
  const int buf_bytes = (WRES ? 0 : WTOT) + ((win_bytes + 1023) & ~1023);
  const int ring_off = WRES ? nchunks * WTOT : 0;
  constexpr int SSN = HALF ? 512 : DS ? 256 : 128;     // floats per tile parity: [scale | shift (| ds scale | ds shift)], 64 (HALF: 128) each
  constexpr int SSH = HALF ? 128 : 64;                 // couts per workgroup = offset of the shift array
  float* ss_lds = reinterpret_cast<float*>(smem + ring_off + 2 * buf_bytes);  // [2 tile parities][scale 64 | shift 64 (| ds scale | ds shift)]
  const char* in = static_cast<const char*>(p.in);
  const char* zero_page = static_cast<const char*>(p.zero_page);

  // ---- tile-independent per-lane geometry: built once per layer shape on the HOST (integer
  // divisions by run-time tile dimensions cost ~40 VALU each; ~30 of them used to sit in this prologue)
  int out_rel[NT], base_lin[NB], res_rel[NT], rel_off[MAXJ];
  {
    const int* row = lane_tab + tid * (2 * NT + NB + MAXJ);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { out_rel[nt] = row[nt]; res_rel[nt] = row[NT + NB + nt]; }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) base_lin[nb] = row[NT + nb];
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) rel_off[j] = row[2 * NT + NB + j];
  }

  // ---- cursors --------------------------------------------------------------------------------
  // The LOAD cursor (L_*) runs one stage ahead of the COMPUTE cursor (C_*).  Everything a tile needs beyond two adds --
  // which window pieces of this lane lie inside the image, which of its output pixels exist, where the window and
  // the output tile start -- was worked out on the HOST per (tile position, images left) and sits in tile_tab /
  // mask_tab (round 1 did ~150 VALU operations of bounds tests and index arithmetic here, per tile and per wave,
  // with the matrix pipe idle: 7-20 % of the kernel's cycles).
  const int tile0 = wg, tile_step = nwg;
  const int nthreads = WAVES * 64;
  int L_it = 0, L_ch = 0;
  bool L_valid = false;
  const char* L_wsrc = nullptr;    // this lane's source of weight piece 0 of the load stage
  const char* L_winbase = nullptr; // window origin pixel of the load stage's tile, + chunk offset
  const float* L_ss = nullptr;     // scale (wave 0) / shift (wave 1) [/ ds scale (2) / ds shift (3)] source of the load tile
  const char* L_dsw = nullptr;     // this lane's source of the downsample slab of the load stage (DS)
  unsigned L_okmask = 0;           // bit j: window piece j of this lane lies inside the image
  unsigned N_off[NT], C_off[NT], D_off[NT];  // output element offsets (incl. cout block) per n-tile
  unsigned N_roff[NT], C_roff[NT];           // residual element offsets (its own layout) of the next / the compute tile
  unsigned N_ok = 0, C_ok = 0, D_ok = 0;     // bit nt: that pixel exists
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) { N_off[nt] = 0; C_off[nt] = 0; D_off[nt] = 0; N_roff[nt] = 0; C_roff[nt] = 0; }

  // The next tile's descriptor (scalar) is requested right before the MFMAs of the iteration that entered a tile (fetch_desc: the current one has been
  // consumed and its registers are free), and the lane's mask word of the next tile (its row index comes out of that descriptor) by the next iteration's
  // cursor step (fetch_mask): both land under a whole stage and are first read behind a stage barrier.  (Until round 4 both were requested inside enter_tile and rotated
  // through variables there; the rotation's register copies made the compiler wait for the load it had just issued -- a memory round trip per tile
  // with the matrix pipe idle, most of the "cursor" slot of the phase stamps.)
  auto tile_index = [&](int it) __attribute__((always_inline)) { return it < n_iters ? it * tile_step + tile0 : tile0; };
  int4 td_next = tile_tab[tile0];
  unsigned mk_next = mask_tab[((unsigned)td_next.x >> 20) * nthreads + tid];
  auto fetch_desc = [&](int it) __attribute__((always_inline)) { td_next = tile_tab[tile_index(it + 1)]; };
  auto fetch_mask = [&]() __attribute__((always_inline)) { mk_next = mask_tab[((unsigned)td_next.x >> 20) * nthreads + tid]; };
  auto enter_tile = [&](int it) __attribute__((always_inline)) {
    const int4 td = td_next;
    const unsigned mk = mk_next;
    L_valid = it < n_iters && ((td.x >> 16) & 1) != 0;
    const int cb = td.x & 0xFFFF;
    L_wsrc = static_cast<const char*>(p.w) + (int64_t)cb * nchunks * WSLAB + wave * 1024 + lane * 16;
    L_winbase = in + (unsigned)td.y;
    if constexpr (HALF) L_ss = ((wave >> 1) == 0 ? p.scale : (wave >> 1) == 1 ? p.shift : (wave >> 1) == 2 ? p.ds_scale : p.ds_shift) + cb * 128 + (wave & 1) * 64 + lane;
    else L_ss = (wave == 0 ? p.scale : wave == 1 ? p.shift : wave == 2 ? p.ds_scale : p.ds_shift) + cb * 64 + lane;
    if constexpr (DS) L_dsw = static_cast<const char*>(p.ds_w) + (int64_t)cb * nchunks * SLAB_TAP + lane * 16;
    L_okmask = mk & 0xFFFFu;
    N_ok = L_valid ? (mk >> 16) : 0u;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { N_off[nt] = (unsigned)td.z + (unsigned)out_rel[nt]; N_roff[nt] = (unsigned)td.w + (unsigned)res_rel[nt]; }
  };

  // ---- DMA of the load stage into ring slot `buf`, as NP independent pieces ----------------------
  // (pieces are issued one at a time between the k-steps of the compute stage's MFMAs, so the
  //  vector-memory issue cost hides under the matrix pipe)
  constexpr int NP = WJ + MAXJ + 1;
  constexpr int DMA_SPREAD = M16 ? 5 : 10;   // (an M16 k-step is a whole tap)
  auto dma_piece = [&](bool on, int buf, int tile_parity, int q) __attribute__((always_inline)) {
    if (!on) return;
    if ((DH_ABL & 2) && q < WJ + MAXJ) return;
    const unsigned wdst = lds_addr_of(smem) + ring_off + buf * buf_bytes + wave * 1024;
    if (q < WJ) {
      if constexpr (WRES) return;   // resident: loaded once, before the stage loop
      const int i = wave + WAVES * q;
      if (i < WSLAB / 1024) {
        if (CLS < 0 || ((TS::wmask() >> (i >> 2)) & 1u))   // 4 pieces per tap slab; unused taps of a parity class stay out
          lds_dma<16>(L_wsrc + q * WAVES * 1024, __builtin_amdgcn_readfirstlane(wdst + q * WAVES * 1024));
      }
      else if (DS && i < WTOT / 1024)
        lds_dma<16>(L_dsw + (i - WSLAB / 1024) * 1024, __builtin_amdgcn_readfirstlane(lds_addr_of(smem) + ring_off + buf * buf_bytes + i * 1024));
    } else if (q < WJ + MAXJ) {
      const int j = q - WJ;
      if (wave + WAVES * j < p.n_win_instr) {  // wave-uniform
        const char* src = ((L_okmask >> j) & 1u) ? L_winbase + rel_off[j] : zero_page + (lane & 3) * 16;
        lds_dma<16>(src, __builtin_amdgcn_readfirstlane(wdst + (WRES ? 0 : WTOT) + j * WAVES * 1024));
      }
    } else if (L_ch == 0 && wave < (HALF ? 8 : DS ? 4 : 2)) {  // BN scale (wave 0) / shift (wave 1) of the tile's cout block [+ ds: waves 2, 3]; HALF: 64 floats per wave, 8 waves
      lds_dma<4>(L_ss, __builtin_amdgcn_readfirstlane(lds_addr_of(ss_lds + tile_parity * SSN + wave * 64)));
    }
  };

  f32x16 acc[MT][NT];
  f32x16 acc_ds[MT][NT];  // fused 1x1 downsample (DS variants; dead otherwise)
  f32x16 acc_c[3][MT][NT];  // classes 1..3 of the all-classes stride-2 data gradient (CLS == 4; dead otherwise)
  f32x4 acc4[MT][NT][4];    // M16: block (ml, nt) as 2 x 2 tiles of 16 couts x 16 pixels, [2 * cout half + pixel half] (acc is dead then)
  // value 4 g + i of block (ml, nt): 32x32x16 -- cout 8 g + 4 h + i of pixel slot (nt, lane & 31); M16 -- cout 16 (g >> 1) + 4 G + i of column lane & 15
  // of pixel tile 2 nt + (g & 1)
  auto acc_at = [&](auto& A, int ml, int nt, int idx) __attribute__((always_inline)) -> float {
    if constexpr (M16) return A[ml][nt][idx >> 2][idx & 3];
    else return A[ml][nt][idx];
  };
  auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if constexpr (M16) { acc4[i][j][r >> 2][r & 3] = 0.f; continue; }
          acc[i][j][r] = 0.f;
          if constexpr (DS) acc_ds[i][j][r] = 0.f;
          if constexpr (CLS == 4) { acc_c[0][i][j][r] = 0.f; acc_c[1][i][j][r] = 0.f; acc_c[2][i][j][r] = 0.f; }
        }
  };
  zero_acc();

  const T* res = HALF ? nullptr : static_cast<const T*>(p.res);   // (the wide stride-2 variant never has a residual: the prefetch registers fold away)
  T* out = static_cast<T*>(p.out);
  // prefetched residual: 4 couts per (nt, mt, g) group = 8 B (bf16) / 16 B (f32)
  constexpr int RW = (ESZ == 2) ? 2 : 4;
  uint32_t rreg[NT][MT][4][RW];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < MT; ++b)
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int d = 0; d < RW; ++d) rreg[a][b][c][d] = 0u;

  // Output / residual addressing.  f32: a lane owns 4 consecutive couts (16 B) per (mt, g).  bf16: that
  // would be 8-byte accesses, so the two half-waves trade halves (v_permlane32_swap): for a pair of groups
  // (2p, 2p+1) lane h=0 ends up with all 8 couts of group 2p and lane h=1 with all 8 of group 2p+1 ->
  // one 16-byte store (and one 16-byte residual load) per pair.  The swap is its own inverse.
  // M16: the two values of a pair belong to the pixel tiles 2 nt and 2 nt + 1 and lanes G, G ^ 1 trade (v_permlane16_swap): lane G ends up with
  // all 8 couts 16 m + 8 (G >> 1) ... of ITS pixel, the one in column lane & 15 of tile 2 nt + (G & 1) -- the same 16-byte accesses at the same
  // "+ h * 8" (G >> 1 == h), one pixel per lane and n-tile as before.
  auto swap_pair = [&](uint32_t& a, uint32_t& b) __attribute__((always_inline)) {
    if constexpr (M16) { const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false); a = r[0]; b = r[1]; }
    else { const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false); a = r[0]; b = r[1]; }
  };
  auto prefetch_residual = [&]() __attribute__((always_inline)) {  // residual tile of the COMPUTE tile
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const bool ok = (C_ok >> nt) & 1u;
#pragma unroll
      for (int ml = 0; ml < MT; ++ml) {
        const int mt = mt0 + ml;
        if constexpr (ESZ == 2) {
#pragma unroll
          for (int pr = 0; pr < 2; ++pr) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (ok) v = *reinterpret_cast<const uint4*>((DH_ABL & 32) ? res + (C_off[0] - out_rel[0]) + wave * 4096 + (((nt * MT + ml) * 2 + pr) * 64 + lane) * 8
                                                                       : res + C_roff[nt] + mt * p.res_mt + pr * p.res_pr + h * 8);
            rreg[nt][ml][2 * pr][0] = v.x; rreg[nt][ml][2 * pr][1] = v.y;
            rreg[nt][ml][2 * pr + 1][0] = v.z; rreg[nt][ml][2 * pr + 1][1] = v.w;
          }
        } else {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (ok) v = *reinterpret_cast<const uint4*>(res + C_roff[nt] + mt * 32 + g * 8 + 4 * h);
            rreg[nt][ml][g][0] = v.x; rreg[nt][ml][g][1] = v.y; rreg[nt][ml][g][2] = v.z; rreg[nt][ml][g][3] = v.w;
          }
        }
      }
    }
  };
  // direct: the residual is loaded here (no prefetch registers; the all-classes variant has four output tiles per window tile)
  // HR (std::true_type / false_type): with / without a residual, as two instantiations -- the choice is uniform for the launch, and as a run-time
  // test inside the element loops the compiler turned it into per-element selects (66 v_cndmask + 79 v_mov per tile on top of ~250 useful VALU)
  auto epilogue_of = [&](auto HR, auto& A, const float* ss, const T* res, bool relu, T* out, bool direct = false)
      __attribute__((always_inline)) {  // of the DONE tile
    // (std::integral_constant<int, 2>: decided at run time, as before -- the float32 and all-classes variants, whose register budget is full: the two
    // instantiations cost them 4-46 spilled registers)
    constexpr int HRM = (int)decltype(HR)::value;
    const bool has_res = HRM == 2 ? res != nullptr : HRM == 1;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const bool ok = (D_ok >> nt) & 1u;
#pragma unroll
      for (int ml = 0; ml < MT; ++ml) {
        const int mt = mt0 + ml;
        if constexpr (ESZ == 2) {
#pragma unroll
          for (int pr = 0; pr < 2; ++pr) {
            uint32_t pk[2][2];  // [group 2pr / 2pr+1][dword]
            uint32_t ra[2] = {rreg[nt][ml][2 * pr][0], rreg[nt][ml][2 * pr][1]};
            uint32_t rb[2] = {rreg[nt][ml][2 * pr + 1][0], rreg[nt][ml][2 * pr + 1][1]};
            if (has_res && direct) {
              uint4 v = make_uint4(0, 0, 0, 0);
              if (ok) v = *reinterpret_cast<const uint4*>(res + D_off[nt] + mt * p.out_mt + pr * p.out_pr + h * 8);   // (direct: the residual shares the output's layout)
              ra[0] = v.x; ra[1] = v.y; rb[0] = v.z; rb[1] = v.w;
            }
            if (has_res) { swap_pair(ra[0], rb[0]); swap_pair(ra[1], rb[1]); }  // back to per-lane ownership
#pragma unroll
            for (int gg = 0; gg < 2; ++gg) {
              const int g = 2 * pr + gg, col = M16 ? mt * 32 + pr * 16 + 4 * G : mt * 32 + g * 8 + 4 * h;
              const float4 sc = *reinterpret_cast<const float4*>(ss + col);       // LDS: not on the vmcnt
              const float4 sh = *reinterpret_cast<const float4*>(ss + SSH + col);  // queue of the stores
              // pairs throughout: v_pk_fma_f32, v_pk_add_f32, v_cvt_pk_bf16_f32 (RNE), v_pk_max_i16
              typedef float f32x2_t __attribute__((ext_vector_type(2)));
              typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
              typedef short i16x2_t __attribute__((ext_vector_type(2)));
              f32x2_t v01 = __builtin_elementwise_fma(f32x2_t{acc_at(A, ml, nt, 4 * g + 0), acc_at(A, ml, nt, 4 * g + 1)}, f32x2_t{sc.x, sc.y}, f32x2_t{sh.x, sh.y});
              f32x2_t v23 = __builtin_elementwise_fma(f32x2_t{acc_at(A, ml, nt, 4 * g + 2), acc_at(A, ml, nt, 4 * g + 3)}, f32x2_t{sc.z, sc.w}, f32x2_t{sh.z, sh.w});
              if (has_res) {
                const uint32_t rx = gg ? rb[0] : ra[0], ry = gg ? rb[1] : ra[1];
                v01 += f32x2_t{bf16_bits_to_f32(rx & 0xFFFFu), bf16_bits_to_f32(rx >> 16)};
                v23 += f32x2_t{bf16_bits_to_f32(ry & 0xFFFFu), bf16_bits_to_f32(ry >> 16)};
              }
              // ReLU AFTER the conversion, on the packed pair as signed 16-bit integers: every negative bf16 has its sign bit set, so max(x, 0)
              // sends exactly those to +0 and relu(round(x)) == round(relu(x)) bit for bit; without ReLU the floor is INT16_MIN.  (fmaxf on the
              // four floats was 8 VALU per group -- a canonicalising max each -- and a branch: a third of this epilogue's VALU work, and VALU
              // work is what the epilogue slot of the phase stamps is made of.)
              const i16x2_t floor2 = __builtin_bit_cast(i16x2_t, relu ? 0u : 0x80008000u);
              pk[gg][0] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(i16x2_t, __builtin_convertvector(v01, bf16x2_t)), floor2));
              pk[gg][1] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(i16x2_t, __builtin_convertvector(v23, bf16x2_t)), floor2));
            }
            swap_pair(pk[0][0], pk[1][0]);
            swap_pair(pk[0][1], pk[1][1]);
            if constexpr (DH_ABL & 4) asm volatile("" :: "v"(pk[0][0]), "v"(pk[0][1]), "v"(pk[1][0]), "v"(pk[1][1]));
            else if (ok)
              *reinterpret_cast<uint4*>((DH_ABL & 16) ? out + (D_off[0] - out_rel[0]) + wave * 4096 + (((nt * MT + ml) * 2 + pr) * 64 + lane) * 8
                                                      : out + D_off[nt] + mt * p.out_mt + pr * p.out_pr + h * 8) = make_uint4(pk[0][0], pk[0][1], pk[1][0], pk[1][1]);
          }
        } else {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int col = mt * 32 + g * 8 + 4 * h;
            const float4 sc = *reinterpret_cast<const float4*>(ss + col);
            const float4 sh = *reinterpret_cast<const float4*>(ss + SSH + col);
            float v[4] = {__builtin_fmaf(acc_at(A, ml, nt, 4 * g + 0), sc.x, sh.x), __builtin_fmaf(acc_at(A, ml, nt, 4 * g + 1), sc.y, sh.y),
                          __builtin_fmaf(acc_at(A, ml, nt, 4 * g + 2), sc.z, sh.z), __builtin_fmaf(acc_at(A, ml, nt, 4 * g + 3), sc.w, sh.w)};
            if (has_res) {
              if (direct) {
                float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok) rv = *reinterpret_cast<const float4*>(res + D_off[nt] + col);
                v[0] += rv.x; v[1] += rv.y; v[2] += rv.z; v[3] += rv.w;
              } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] += __uint_as_float(rreg[nt][ml][g][i]);
              }
            }
            if (relu) {
#pragma unroll
              for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.f);
            }
            if (ok) *reinterpret_cast<float4*>(out + D_off[nt] + col) = make_float4(v[0], v[1], v[2], v[3]);
          }
        }
      }
    }
  };
  T* ds_out = static_cast<T*>(p.ds_out);
  auto epilogue = [&](int tile_parity) __attribute__((always_inline)) {
    const float* ss = ss_lds + tile_parity * SSN;
    if constexpr (CLS == 4) {   // four output tiles: class c = (py, px) owns the pixels (2 i + py, 2 j + px) of dX
      typedef std::integral_constant<int, 2> at_run_time;
      epilogue_of(at_run_time{}, acc, ss, res, p.relu != 0, out, true);
#pragma unroll
      for (int c = 1; c < 4; ++c) epilogue_of(at_run_time{}, acc_c[c - 1], ss, res ? res + p.cls_base[c] : res, p.relu != 0, out + p.cls_base[c], true);
    } else if constexpr (ESZ != 2) epilogue_of(std::integral_constant<int, 2>{}, acc, ss, res, p.relu != 0, out);
    else if constexpr (M16) {
      if (res) epilogue_of(std::true_type{}, acc4, ss, res, p.relu != 0, out);
      else epilogue_of(std::false_type{}, acc4, ss, res, p.relu != 0, out);
    }
    else if (res) epilogue_of(std::true_type{}, acc, ss, res, p.relu != 0, out);
    else epilogue_of(std::false_type{}, acc, ss, res, p.relu != 0, out);
    if constexpr (DS) epilogue_of(std::false_type{}, acc_ds, ss + 2 * SSH, (const T*)nullptr, false, ds_out);  // BN only: no ReLU, no residual
  };

  // KSTEPS = 18 k-steps (9 taps x 2) per stage (2 / 4 / 8 for a parity class); the operand fragments of k-step i+1 are read from LDS
  // before the MFMAs of k-step i are issued (register double buffer).
  struct Frags { uint4 a[MT], b[NT]; };
  // HOIST (round 4, bf16 kernels): the LDS byte offset of this lane's window fragment of tap (kh, kw), k-step parity 0, from the window's origin is
  // the same in every stage of the kernel.  Computed once and kept as 16-bit halves (a window is < 64 KB), two per register: NT = 2 packs the two
  // pixel tiles of a tap (9 registers), NT = 1 two taps (5).  A fragment address is then two VALU instructions (pick the half; + ring slot base, or
  // (offset ^ 32) + base as v_xad_u32) instead of six (add the tap, two shifts, the XOR swizzle, shift, add): 8 -> 4 VALU per k-step at NT = 2.
  // The chip holds these kernels at 1.6-1.9 GHz under load, and VALU instructions in the MFMA loop are energy the clock pays for
  // (cdna_hip_programming.md rule 28).  Unpacked (18 registers) the NT = 2 kernels spill; the float32 and parity-class variants have no
  // registers to spare at all and keep the per-k-step form.
  constexpr bool HOIST = DH_CONV_HOIST && sizeof(T) == 2 && CLS < 0;
  static_assert(!HOIST || MAXJ * WAVES * 1024 <= 65536, "HOIST: a staged window (<= MAXJ * WAVES DMA pieces of 1 KiB) must fit 16-bit offsets");
  // M16: the lane reads chunk slot sigma(G) of NB pixels per tap, all 32 channels in one k-step (no parity flip): NB halves per tap, 9 NB / 2 registers
  constexpr int NTOFF = M16 ? 9 * NB / 2 : NT == 2 ? 9 : 5;
  uint32_t toffp[NTOFF];
  {
    auto tap_off = [&](int nt, int t9) __attribute__((always_inline)) {
      const int kh = t9 / 3, kw = t9 % 3;
      const int tap_lin = STRIDE == 1 ? kh * p.HP + kw : kh * p.HP + (kw & 1) * p.HPH + (kw >> 1);
      if constexpr (M16) return (uint32_t)lds_slot_addr(base_lin[nt] + tap_lin, ((G & 1) << 1) | (G >> 1));
      return (uint32_t)(HALF ? lds_slot_addr_half(base_lin[nt] + tap_lin, h) : lds_slot_addr(base_lin[nt] + tap_lin, h));
    };
#pragma unroll
    for (int i = 0; i < NTOFF; ++i) {
      if constexpr (!HOIST) toffp[i] = 0u;
      else if constexpr (M16 && NB == 4) toffp[i] = tap_off(2 * (i & 1), i >> 1) | (tap_off(2 * (i & 1) + 1, i >> 1) << 16);
      else if constexpr (M16) toffp[i] = tap_off(0, i) | (tap_off(1, i) << 16);
      else if constexpr (NT == 2) toffp[i] = tap_off(0, i) | (tap_off(1, i) << 16);
      else toffp[i] = tap_off(0, 2 * i) | ((2 * i + 1 < 9 ? tap_off(0, 2 * i + 1) : 0u) << 16);
    }
  }
  unsigned ksflip = 0x00200020u;   // k-step parity 1: byte bit 5 of both halves
  auto read_frags = [&](int kstep, const int* bl, const char* w_lds, const char* a_lds)
      __attribute__((always_inline)) {
    const int t = HALF ? kstep : kstep >> 1, ks = HALF ? 0 : kstep & 1;
    const int tap = TS::wrow(t / TS::NX) * 3 + TS::wcol(t % TS::NX);   // slab of the packed operator
    const int kh = TS::srow(t / TS::NX), kw = TS::scol(t % TS::NX);   // position in the staged window
    const int tap_lin = STRIDE == 1 ? kh * p.HP + kw : kh * p.HP + (kw & 1) * p.HPH + (kw >> 1);
    const char* wt = w_lds + tap * SLAB_TAP + lane * 16 + ks * 2 * FRAG_BYTES;
    Frags f;
#pragma unroll
    for (int ml = 0; ml < MT; ++ml) f.a[ml] = *reinterpret_cast<const uint4*>(wt + (mt0 + ml) * FRAG_BYTES);
    if constexpr (HOIST) {
      const int t9 = kh * 3 + kw;
      const unsigned base = lds_addr_of(a_lds);
      unsigned pk = toffp[NT == 2 ? t9 : t9 >> 1];
      if (ks) pk = xor_opaque(pk, ksflip);
      if constexpr (NT == 2) { f.b[0] = *lds_ptr128(add_half16<0>(base, pk)); f.b[1] = *lds_ptr128(add_half16<1>(base, pk)); }
      else f.b[0] = (t9 & 1) ? *lds_ptr128(add_half16<1>(base, pk)) : *lds_ptr128(add_half16<0>(base, pk));
    } else {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)  // slot 2*ks + h: the k-step parity flips byte bit 5 of the slot address
        f.b[nt] = *reinterpret_cast<const uint4*>(a_lds + (HALF ? lds_slot_addr_half(bl[nt] + tap_lin, h) : (lds_slot_addr(bl[nt] + tap_lin, h) ^ (ks << 5))));
    }
    return f;
  };
  auto compute_stage = [&](int buf, int chunk, bool dma_on, int dma_buf, int dma_parity) __attribute__((always_inline)) {
    const char* w_lds = WRES ? smem + chunk * WTOT : smem + buf * buf_bytes;
    const char* a_lds = WRES ? smem + ring_off + buf * buf_bytes : w_lds + WTOT;
    (void)chunk;
    if constexpr (M16) {
      // A-major: the NB window fragments of a tap stay live while the 2 MT weight fragments (16 couts x 32 channels each) pass one at a time,
      // each read one ahead of the NB MFMAs -- on NB independent accumulators -- that it feeds.
      static_assert(HOIST, "M16 reads the window through the hoisted offsets");
      const unsigned wbase = lds_addr_of(a_lds);
      auto read_b = [&](int t, uint4 (&b)[NB]) __attribute__((always_inline)) {
        if constexpr (NB == 4) {
          const unsigned pk0 = toffp[2 * t], pk1 = toffp[2 * t + 1];
          b[0] = *lds_ptr128(add_half16<0>(wbase, pk0)); b[1] = *lds_ptr128(add_half16<1>(wbase, pk0));
          b[2] = *lds_ptr128(add_half16<0>(wbase, pk1)); b[3] = *lds_ptr128(add_half16<1>(wbase, pk1));
        } else {
          const unsigned pk = toffp[t];
          b[0] = *lds_ptr128(add_half16<0>(wbase, pk)); b[1] = *lds_ptr128(add_half16<1>(wbase, pk));
        }
      };
      // slab image [k-step][mt][lane][16 B] of the 32x32x16 lanes: (cout c, chunk slot s) sits at k-step s >> 1, lane (s & 1) * 32 + (c & 31)
      const char* wl = w_lds + (G & 1) * 2 * FRAG_BYTES + ((G >> 1) * 32 + (lane & 15)) * 16 + mt0 * FRAG_BYTES;
      auto read_a = [&](int t, int m) __attribute__((always_inline)) {
        return *reinterpret_cast<const uint4*>(wl + t * SLAB_TAP + (m >> 1) * FRAG_BYTES + (m & 1) * 256);
      };
      uint4 bc[NB];
      read_b(0, bc);
      uint4 an = read_a(0, 0);
      __builtin_amdgcn_s_setprio(3);
#pragma unroll
      for (int k = 0; k < KSTEPS; ++k) {
        if (k == (3 * KSTEPS + 4) / 8) __builtin_amdgcn_s_setprio(2);
        if (k == (5 * KSTEPS + 4) / 8) __builtin_amdgcn_s_setprio(1);
        if (k == (7 * KSTEPS + 4) / 8) __builtin_amdgcn_s_setprio(0);
        uint4 bn[NB];
#pragma unroll
        for (int n = 0; n < NB; ++n) bn[n] = bc[n];
        if (k + 1 < KSTEPS) read_b(k + 1, bn);
#pragma unroll
        for (int m = 0; m < 2 * MT; ++m) {
          const uint4 ac = an;
          if (m + 1 < 2 * MT) an = read_a(k, m + 1);
          else if (k + 1 < KSTEPS) an = read_a(k + 1, 0);
#pragma unroll
          for (int n = 0; n < NB; ++n)
            acc4[m >> 1][n >> 1][(m & 1) * 2 + (n & 1)] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                __builtin_bit_cast(bf16x8, ac), __builtin_bit_cast(bf16x8, bc[n]), acc4[m >> 1][n >> 1][(m & 1) * 2 + (n & 1)], 0, 0, 0);
        }
        constexpr int SPREAD = KSTEPS < DMA_SPREAD ? KSTEPS : DMA_SPREAD;
        if (k < SPREAD)
#pragma unroll
          for (int q = (k * NP) / SPREAD; q < ((k + 1) * NP) / SPREAD; ++q) dma_piece(dma_on, dma_buf, dma_parity, q);
#pragma unroll
        for (int n = 0; n < NB; ++n) bc[n] = bn[n];
      }
      __builtin_amdgcn_s_setprio(0);
      return;
    }
    int bl[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      bl[nt] = base_lin[nt];
      asm volatile("" : "+v"(bl[nt]));  // opaque per stage: keeps 18 tap addresses from being hoisted into VGPRs
    }
    if constexpr (HOIST) asm volatile("" : "+v"(ksflip));   // opaque per stage: the nine flipped copies are not worth nine registers either
    Frags cur = read_frags(0, bl, w_lds, a_lds);
    // Falling wave priority (round 4).  The two waves of a SIMD share its matrix pipe, arbitrated by priority, then AGE: at equal priority the
    // older wave runs ahead, finishes its MFMAs at ~2/3 of the stage and waits at the barrier while its partner works on alone with nobody
    // to fill its LDS bubbles (profiles/r04_conv_phase_stamps.txt: 18-19 % of wave 0's cycles).  Here a wave's priority falls as it
    // advances -- 3 for the first 3/8 of a stage's k-steps, 2 to 5/8, 1 to 7/8, then 0 (and 0 through barrier, cursor and epilogue) -- so
    // whichever wave is BEHIND wins the pipe and the pair finishes together: dominant kernel -2.0 %, whole slide +1.0 % on three boxes
    // (profiles/r04_exp_wave_priority.txt; a fixed s_setprio 1 for waves 4-7 had measured -0.6 %).
    __builtin_amdgcn_s_setprio(3);
#pragma unroll
    for (int k = 0; k < KSTEPS; ++k) {
      if (k == (3 * KSTEPS + 4) / 8) __builtin_amdgcn_s_setprio(2);
      if (k == (5 * KSTEPS + 4) / 8) __builtin_amdgcn_s_setprio(1);
      if (k == (7 * KSTEPS + 4) / 8) __builtin_amdgcn_s_setprio(0);
      Frags nxt = cur;
      if (k + 1 < KSTEPS && !(DH_ABL & 8)) nxt = read_frags(k + 1, bl, w_lds, a_lds);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int ml = 0; ml < MT; ++ml) {
          if constexpr (DH_ABL & 1) asm volatile("" :: "v"(cur.a[ml].x), "v"(cur.a[ml].y), "v"(cur.a[ml].z), "v"(cur.a[ml].w), "v"(cur.b[nt].x), "v"(cur.b[nt].y), "v"(cur.b[nt].z), "v"(cur.b[nt].w));
          else if constexpr (CLS == 4) {
            const int tcls = TS::cls_of((k >> 1) / TS::NX, (k >> 1) % TS::NX);   // compile-time after unrolling
            if (tcls == 0) mma_frag<T>(acc[ml][nt], cur.a[ml], cur.b[nt]);
            else mma_frag<T>(acc_c[tcls - 1][ml][nt], cur.a[ml], cur.b[nt]);
          }
          else mma_frag<T>(acc[ml][nt], cur.a[ml], cur.b[nt]);
        }
      }
      if constexpr (DS) {
        if (HALF ? k == 4 : (k == 8 || k == 9)) {  // centre tap (kh = kw = 1): the 1x1 stride-2 conv sees exactly these pixels
          const char* wd = w_lds + WSLAB + lane * 16 + (HALF ? 0 : (k & 1) * 2 * FRAG_BYTES);
#pragma unroll
          for (int ml = 0; ml < MT; ++ml) {
            const uint4 dw = *reinterpret_cast<const uint4*>(wd + (mt0 + ml) * FRAG_BYTES);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) mma_frag<T>(acc_ds[ml][nt], dw, cur.b[nt]);
          }
        }
      }
      // all pieces go out during the first DMA_SPREAD k-steps: the rest of the stage covers their latency
      constexpr int SPREAD = KSTEPS < DMA_SPREAD ? KSTEPS : DMA_SPREAD;   // (the wide stride-2 variant: 11 pieces over its 9 k-steps; over 3 / 5 / 7: +0.2 ... 0.4 %, noise)
      if (k < SPREAD)
#pragma unroll
        for (int q = (k * NP) / SPREAD; q < ((k + 1) * NP) / SPREAD; ++q) dma_piece(dma_on, dma_buf, dma_parity, q);
      cur = nxt;
    }
    __builtin_amdgcn_s_setprio(0);   // (short stages -- the parity classes' 2-8 k-steps -- may not have reached it inside the loop)
  };

  // ---- flat stage stream -------------------------------------------------------------------
  // STAMP builds (diagnostics only, never timed for results) accumulate per-phase cycles.
  unsigned long long tacc[6] = {0, 0, 0, 0, 0, 0};
  unsigned long long tprev = t_entry;
  auto stamp = [&](int slot) __attribute__((always_inline)) {
    if constexpr (STAMP) {
      __builtin_amdgcn_sched_barrier(0);
      const unsigned long long now = __builtin_readcyclecounter();
      __builtin_amdgcn_sched_barrier(0);
      if (slot >= 0) tacc[slot] += now - tprev;
      tprev = now;
    }
  };
  const int S = n_iters * nchunks;
  enter_tile(0);
  fetch_desc(0);
  if constexpr (WRES) {
    // all weight slabs of THIS workgroup's cout block, once: the host schedule gives a workgroup the same cout
    // block in every iteration
    const int cb = tile_tab[wg].x & 0xFFFF;
    const char* wsrc = static_cast<const char*>(p.w) + (int64_t)cb * nchunks * WSLAB + lane * 16;
    const char* dsrc = DS ? static_cast<const char*>(p.ds_w) + (int64_t)cb * nchunks * SLAB_TAP + lane * 16 : nullptr;
    constexpr int PPC = WTOT / 1024;   // 1 KiB pieces per chunk: 36 of the 3x3 slab (+ 4 of the downsample slab)
    for (int i = wave; i < nchunks * PPC; i += WAVES) {
      const int ch = i / PPC, r = i % PPC;
      const char* src = (!DS || r < WSLAB / 1024) ? wsrc + (ch * (WSLAB / 1024) + r) * 1024
                                                  : dsrc + (ch * (SLAB_TAP / 1024) + r - WSLAB / 1024) * 1024;
      lds_dma<16>(src, __builtin_amdgcn_readfirstlane(lds_addr_of(smem) + i * 1024));
    }
  }
#pragma unroll
  for (int q = 0; q < NP; ++q) dma_piece(L_valid, 0, 0, q);
  bool C_valid = L_valid;
  C_ok = N_ok;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) { C_off[nt] = N_off[nt]; C_roff[nt] = N_roff[nt]; }
  int C_ch = 0, C_par = 0, D_par = 0;
  bool pending = false;  // a finished tile (D_*) still owes its epilogue
  stage_barrier();       // stage 0 is in LDS
  stamp(4);              // prologue: geometry, first tile decode, first DMA
  for (int s = 0; s < S; ++s) {
    // (1) load cursor -> stage s+1
    if (L_ch + 1 < nchunks) {
      L_winbase += p.in_chunk_bytes;   // (HALF: the input is in 16-channel planes, so a half-chunk stage reads whole lines too)
      ++L_ch; L_wsrc += WSLAB; if constexpr (DS) L_dsw += SLAB_TAP;
      if (L_ch == 1) fetch_mask();
    }
    else { ++L_it; L_ch = 0; enter_tile(L_it); }
    const bool dma_on = (s + 1 < S) && L_valid;
    stamp(0);
    // (2) epilogue of the previous tile (its stores drain under the MFMAs below); residual prefetch
    if (pending) {
      epilogue(D_par);
      zero_acc();
      pending = false;
    }
    if (CLS != 4 && C_ch == 0 && res && C_valid && !(DH_ABL & 64)) prefetch_residual();
    stamp(1);
    if (L_ch == 0) fetch_desc(L_it);   // this iteration's cursor step entered tile L_it: request the next one's descriptor (lands under the MFMAs)
    // (3) MFMAs of stage s, DMA of stage s+1 issued in between
    if (C_valid) {
      compute_stage(s & 1, C_ch, dma_on, (s + 1) & 1, L_it & 1);
    } else {
#pragma unroll
      for (int q = 0; q < NP; ++q) dma_piece(dma_on, (s + 1) & 1, L_it & 1, q);
    }
    stamp(2);
    // (4) compute cursor -> stage s+1
    if (C_ch == nchunks - 1) {
      pending = C_valid; D_ok = C_ok; D_par = C_par;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) D_off[nt] = C_off[nt];
      C_valid = L_valid; C_ok = N_ok; C_par ^= 1; C_ch = 0;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) { C_off[nt] = N_off[nt]; C_roff[nt] = N_roff[nt]; }
    } else {
      ++C_ch;
    }
#ifdef DH_STAMP_SPLIT   /* diagnostic build only: "barr" = this wave's own vmcnt / lgkmcnt wait; the s_barrier (skew between waves) goes to "cursor" */
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    stamp(3);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    stamp(0);
#else
    stage_barrier();  // retires this wave's DMA of stage s+1 and publishes everyone's
    stamp(3);
#endif
  }
  if (pending) epilogue(D_par);
  stamp(5);
  if constexpr (STAMP) {
    if (tid == 0 && p.stamps) {
      for (int i = 0; i < 6; ++i) atomicAdd(p.stamps + i, tacc[i]);
      atomicAdd(p.stamps + 6, 1ull);
      atomicAdd(p.stamps + 7, (unsigned long long)(__builtin_amdgcn_s_memrealtime() - rt_entry));
    }
  }
}

template <typename T, int STRIDE, int NT, int WAVES, bool STAMP, bool DS, int MT, bool WRES = false, int CLS = -1, bool HALF = false, bool M16 = false>
__global__ __launch_bounds__(WAVES * 64, WAVES / 4) void conv3x3_kernel(const Conv3Params p) {
  conv3x3_body<T, STRIDE, NT, WAVES, STAMP, DS, MT, WRES, CLS, HALF, M16>(p, (int)blockIdx.x, (int)gridDim.x, p.iters, p.lane_tab, p.tile_tab, p.mask_tab);
}

// All four parity classes of a stride-2 data gradient in ONE launch: workgroups [first[k], first[k + 1]) run class order[k] = {3, 1, 2, 0}[k]
// over that class's own schedule.  As four launches each class fills a fraction of the chip at batch 64 (a 7 x 7 class of 64 images is 48-64
// tiles) and the launches run one after the other: 1 + 2 + 2 + 4 = 9 tap-units of time; side by side the 4-tap class sets the time: 4 units.
// The host gives every class the share of the workgroups that evens out (tiles per workgroup) x (taps).
struct S2ClassSched { int first[5]; int iters[4]; const int* lane[4]; const int4* tile[4]; const unsigned* mask[4]; };
template <typename T, int NT, int WAVES, int MT>
__global__ __launch_bounds__(WAVES * 64, WAVES / 4) void conv3x3_s2dgrad_kernel(const Conv3Params p, const S2ClassSched s) {
  const int b = (int)blockIdx.x;
  if (b < s.first[1]) conv3x3_body<T, 1, NT, WAVES, false, false, MT, false, 3>(p, b - s.first[0], s.first[1] - s.first[0], s.iters[0], s.lane[0], s.tile[0], s.mask[0]);
  else if (b < s.first[2]) conv3x3_body<T, 1, NT, WAVES, false, false, MT, false, 1>(p, b - s.first[1], s.first[2] - s.first[1], s.iters[1], s.lane[1], s.tile[1], s.mask[1]);
  else if (b < s.first[3]) conv3x3_body<T, 1, NT, WAVES, false, false, MT, false, 2>(p, b - s.first[2], s.first[3] - s.first[2], s.iters[2], s.lane[2], s.tile[2], s.mask[2]);
  else conv3x3_body<T, 1, NT, WAVES, false, false, MT, false, 0>(p, b - s.first[3], s.first[4] - s.first[3], s.iters[3], s.lane[3], s.tile[3], s.mask[3]);
}
