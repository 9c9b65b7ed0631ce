// stem_pool.inc -- fused stem for bf16 inference: conv 7x7/2 (3->64) + BN + ReLU + maxpool 3x3/2.
// Included inside the anonymous namespace of resnet_kernels.hip.
//
// The unfused pair (stem_kernel + maxpool_kernel) writes the 128x128x64 stem activation to HBM
// and reads it back (536 MB per 128 tiles in bf16) and re-stages the weight image for
// every 256 output pixels.  Here a PERSISTENT 4-wave workgroup keeps the weights in LDS for its
// whole life and sweeps column strips of (image, PC pooled columns) from top to bottom, 4 pooled rows
// (= 8 conv rows) per step (PC = 15 or 16, chosen per geometry by the launcher: see the end of this comment):
//   * the 21 x 69-pixel input window of the step's 8 x 32 conv tile is staged in LDS as normalised bf16
//     (straight from the uint8 slide: 4-byte loads, prefetched into registers one step ahead);
//   * MFMA 32x32x16: a window row holds (pixel, channel) pairs interleaved, so the 21 taps of one kernel row are 21
//     consecutive elements from element 6*tx of the row.  They sit in 24 k-slots (3 groups of 8; slot 0 and slots
//     22, 23 carry zero weights), and TWO kernel rows share three k-steps: [row a: g0 g1] [row a: g2 | row a+1: g0]
//     [row a+1: g1 g2]; row 6 alone takes two.  11 k-steps in all (one 32-slot pair per kernel row would be 14);
//     wave w computes conv rows 2w and 2w+1 of the step, operand fragments double-buffered in registers;
//   * pooled row w = max over conv rows 2w-1, 2w, 2w+1: the wave has the last two in registers and takes row
//     2w-1 -- the second row of wave w-1, or for wave 0 the last row of the PREVIOUS step of the sweep --
//     from a 4 KiB LDS slot, as packed bf16 BEFORE the horizontal pooling: the three rows are combined first and
//     one horizontal pass (two DPP wave shifts per dword) serves the pooled row (an earlier version pooled every
//     row horizontally before the exchange: twice the DPP work; one before that let every wave compute three
//     conv rows: +50 % MFMA work);
//   * bf16 values order like signed 16-bit integers within a sign and every negative is below +0, so max_i16
//     against 0 at the end is the ReLU (bf16(relu(x)) == relu(bf16(x))).  Even lanes hold the pooled pixels of
//     the row and store them with 16-byte stores (half-waves trade halves, permlane32 swap).
// Strip width.  A 32-column conv tile holds the three conv columns 2c-1 .. 2c+1 of 15 pooled columns c.
//   PC = 15: lane 0 is conv column 2*px0 - 1; even lane 2j pools lanes 2j .. 2j+2.  Strips are independent.
//   PC = 16: lane 0 is conv column 2*px0 (the aligned tile: 128 conv columns are 4 strips, not 5); even lane 2j pools
//     lanes 2j-1 .. 2j+1.  Pooled column px0 of a strip s >= 1 lacks conv column 2*px0 - 1, the LAST lane of strip s-1:
//     that strip writes the column's vertical 3-row max (lanes 31 and 63 of the row-combined registers, after the ReLU)
//     to the seam scratch [image][seam][Hp][64 couts in lane order], and stem_seam_kernel, next on the stream, folds it into the output with
//     max_i16.  Max is exact and order-free and every value is a non-negative bf16: the same nine values, the same bits.
// Conv rows/cols outside the image contribute 0, which is neutral for a max that ends in a ReLU.
// The kernel is bound by vector-ALU issue, not by the matrix pipe (ablations in profiles/): everything per conv
// output that is not the MFMA is kept to a handful of instructions.
// Three 4-wave workgroups per CU (52 KiB of LDS, <= 168 VGPRs each) run with independent barriers; two barriers per
// step order (a) the row exchange and the reuse of the single window buffer, (b) the next step's window.
#ifndef SP_ABL
#define SP_ABL 0   /* timing-only ablations (tools/build_variant.sh): 1 no MFMA, 2 no window loads, 4 no window conversion, 8 no pooling math, 16 no output stores, 32 no LDS operand reads */
#endif
constexpr int SP_W = 4;
constexpr int SP_T = SP_W * 64;
constexpr int SP_CR = 2 * SP_W, SP_CC = 32;        // conv tile of a step: wave w computes rows {2w, 2w+1}
constexpr int SP_PR = SP_W;                        // pooled rows of a step (pooled columns: the template parameter PC)
constexpr int SP_WR = 2 * SP_CR + 5;               // window rows (21)
constexpr int SP_WE = 224;                         // elements per window row (slot 0 dummy, 1..207 data)
#ifndef SP_PF
#define SP_PF 3
#endif
constexpr int SP_KS = 11;                          // k-steps (see above)
constexpr int SP_WBYTES = SP_KS * 2 * FRAG_BYTES;  // 22 KiB packed weights (bf16): [k-step][cout half][lane][8]
constexpr int SP_WINB = ((SP_WR * SP_WE * 2 + 255) / 256) * 256;
constexpr int SP_XCH = 4096;                       // one exchanged conv row: 64 lanes x 16 dwords
constexpr int SP_LDS = SP_WBYTES + SP_WINB + (SP_W + 1) * SP_XCH + 512;
constexpr int SP_DW = 52;                          // dwords per window row (207 bytes)
constexpr int SP_NLOAD = (SP_WR * SP_DW + SP_T - 1) / SP_T;
static_assert(3 * ((SP_LDS + 511) / 512 * 512) <= 160 * 1024, "three workgroups per CU");

// k-slot -> (kernel row, element of the 24-slot row image) of the stem_pool weight layout; -1: zero weight
inline void sp_kslot(int ks, int hh, int j, int* kh, int* s) {
  *kh = -1; *s = 0;
  if (ks < 9) {
    const int pz = ks / 3, u = ks % 3;
    if (u == 0) { *kh = 2 * pz; *s = 8 * hh + j; }
    else if (u == 1) { *kh = 2 * pz + hh; *s = hh ? j : 16 + j; }
    else { *kh = 2 * pz + 1; *s = 8 + 8 * hh + j; }
  } else if (ks == 9) { *kh = 6; *s = 8 * hh + j; }
  else if (hh == 0) { *kh = 6; *s = 16 + j; }
}

struct StemPoolParams {
  const float* x_nchw; const uint8_t* slide; const int32_t* yx; int64_t row_bytes, slide_bytes;
  const void* w; const float* scale; const float* shift; void* out;
  void* seam;   // PC = 16: [B][tiles_x - 1][Hp][64] bf16, the last conv column of every strip but an image's last
  int B, P, Hc, Wc, Hp, Wp, tiles_y, tiles_x, nstrips, iters;   // strips = (image, tile column); iters = strips per workgroup x tiles_y
  unsigned long long* stamps;
};

typedef unsigned short sp_u16x2 __attribute__((ext_vector_type(2)));

template <bool SRC_U8, bool STAMP, int PC>
__global__ __launch_bounds__(SP_T, 3) void stem_pool_kernel(const StemPoolParams p) {
  static_assert(PC == 15 || PC == 16, "strips of 15 or 16 pooled columns");
  constexpr int CX = 16 - PC;   // lane 0 is conv column 2*px0 - CX
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* w_lds = smem;
  char* win_lds = smem + SP_WBYTES;
  char* xch_lds = win_lds + SP_WINB;   // slots 0..2: second row of waves 0..2; slots 3, 4: wave 3's, by step parity (the carry)
  float* ss_lds = reinterpret_cast<float*>(xch_lds + (SP_W + 1) * SP_XCH);
  const int tid = threadIdx.x, lane = tid & 63, tx = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // one-time: weights (linear LDS-DMA), scale/shift, zeroed window buffers
  for (int i = wave; i < SP_WBYTES / 1024; i += SP_W)
    lds_dma<16>(static_cast<const char*>(p.w) + i * 1024 + lane * 16, __builtin_amdgcn_readfirstlane(lds_addr_of(w_lds + i * 1024)));
  if (tid < 128) ss_lds[tid] = tid < 64 ? p.scale[tid] : p.shift[tid - 64];
  for (int i = tid * 16; i < SP_WINB; i += SP_T * 16) *reinterpret_cast<uint4*>(win_lds + i) = make_uint4(0, 0, 0, 0);

  struct Tile { int valid, b, py0, px0, ty0, tx0, first; };
  // steps of this workgroup: strip k * gridDim + blockIdx (k = 0, 1, ...), tile rows top to bottom.  The cursor below
  // walks them incrementally (one division per strip, not per step); the tile's slide origin (ty0, tx0) is loaded in
  // next_tile(), an iteration before load_window needs it.
  int cur_sid = (int)blockIdx.x, cur_ty = 0, cur_b = cur_sid / p.tiles_x, cur_px0 = (cur_sid % p.tiles_x) * PC, cur_it = 0;
  auto next_tile = [&]() __attribute__((always_inline)) {
    Tile t;
    t.valid = cur_sid < p.nstrips && cur_it < p.iters;
    t.b = cur_b; t.py0 = cur_ty * SP_PR; t.px0 = cur_px0; t.first = cur_ty == 0;
    t.ty0 = 0; t.tx0 = 0;
    if constexpr (SRC_U8) {
      if (t.valid) { t.ty0 = p.yx[2 * t.b]; t.tx0 = p.yx[2 * t.b + 1]; }
    }
    ++cur_it;
    if (++cur_ty == p.tiles_y) {
      cur_ty = 0; cur_sid += (int)gridDim.x;
      cur_b = cur_sid / p.tiles_x; cur_px0 = (cur_sid % p.tiles_x) * PC;
    }
    return t;
  };

  // window pieces of this thread: piece k = dword d of row r, (r, d) = divmod(tid + k * SP_T, SP_DW); all but the last k exist
  // for every thread.  Source bytes q = 4d-1 .. 4d+2 of the row (an unaligned dword; the window origin is not aligned anyway)
  // are exactly the elements e = 4d .. 4d+3 the thread then writes with one aligned 8-byte LDS store.
  constexpr int SP_TAIL = SP_WR * SP_DW - (SP_NLOAD - 1) * SP_T;   // threads that own a piece in the last round
  uint32_t wr[SP_NLOAD], wr2[SP_NLOAD];   // window pieces of the next tile (staged this step) / of the one after (in flight)
  uint32_t woff[SP_NLOAD];  // byte offset of the piece from (window origin - 1)
  uint32_t wdst[SP_NLOAD];  // byte offset of the piece in the window buffer: (r * SP_WE + 4 * d) * 2
  uint32_t colm[SP_NLOAD];  // byte mask of the piece: columns of the current strip that lie inside the tile
#pragma unroll
  for (int k = 0; k < SP_NLOAD; ++k) {
    wr[k] = 0; wr2[k] = 0; colm[k] = 0;
    const int idx = tid + k * SP_T;
    const bool own = idx < SP_WR * SP_DW;
    const int r = own ? idx / SP_DW : 0, d = own ? idx % SP_DW : 0;
    woff[k] = (uint32_t)(r * (int)p.row_bytes + 4 * d);
    wdst[k] = (uint32_t)((r * SP_WE + 4 * d) * 2);
  }
  // (r, d) of piece k for the masks of edge windows.  Recomputed where it is used: the opaque copy keeps the compiler from hoisting r,
  // d and what is derived from them out of the sweep, where they would hold registers through every step for the sake of a few
  auto piece_rd = [&](int k, int* r, int* d) __attribute__((always_inline)) {
    uint32_t w = wdst[k];
    asm volatile("" : "+v"(w));
    *r = (int)(w / (uint32_t)(SP_WE * 2)); *d = (int)(w % (uint32_t)(SP_WE * 2)) >> 3;
  };
  struct __attribute__((packed, aligned(1))) U32 { uint32_t v; };
  // window of tile t: input rows iy0 + r (r < 21), bytes 3*ix0 + q (q < 207), iy0 = 4*py0 - 3, ix0 = 2*(2*px0 - CX) - 3
  auto load_window = [&](const Tile& t, uint32_t (&wr)[SP_NLOAD]) __attribute__((always_inline)) {
    if constexpr (SRC_U8) {
      const int iy0 = 4 * t.py0 - 3, ix0 = 4 * t.px0 - 2 * CX - 3;
      const int64_t worg = (int64_t)(t.ty0 + iy0) * p.row_bytes + (int64_t)(t.tx0 + ix0) * 3 - 1;   // byte before the window
      const int64_t wend = worg + (int64_t)(SP_WR - 1) * p.row_bytes + 4 * SP_DW;                    // one past its last dword
      if constexpr (SP_ABL & 2) return;
      if (worg >= 0 && wend <= p.slide_bytes) {   // workgroup-uniform: the whole window lies inside the allocation
        const uint8_t* base = p.slide + worg;      // (bytes of other rows / other tiles are masked when the window is staged)
#pragma unroll
        for (int k = 0; k < SP_NLOAD; ++k) wr[k] = reinterpret_cast<const U32*>(base + ((SP_ABL & 64) ? (woff[k] & 1023u) : woff[k]))->v;
      } else {                                     // a tile in the first or last rows of the slide: byte by byte
#pragma unroll
        for (int k = 0; k < SP_NLOAD; ++k) {
          const int64_t a = worg + woff[k];
          uint32_t v = 0;
          for (int i = 0; i < 4; ++i)
            if (a + i >= 0 && a + i < p.slide_bytes) v |= (uint32_t)p.slide[a + i] << (8 * i);
          wr[k] = v;
        }
      }
    }
  };
  auto store_window = [&](const Tile& t, uint32_t (&wr)[SP_NLOAD]) __attribute__((always_inline)) {
    uint16_t* win = reinterpret_cast<uint16_t*>(win_lds);
    const int iy0 = 4 * t.py0 - 3, ix0 = 4 * t.px0 - 2 * CX - 3;
    if constexpr (SRC_U8) {
      if constexpr (SP_ABL & 4) {   // consume the loads, convert nothing
#pragma unroll
        for (int k = 0; k < SP_NLOAD; ++k) if (wr[k] == 0x12345678u) win[k] = 1;
        return;
      }
      // pixels outside the tile count as zero padding: their BYTES are cleared before the conversion.  The column part of
      // the mask depends on the strip only and is rebuilt at its first step; interior windows skip both parts
      // (workgroup-uniform branches).
      if (t.first) {
        const int q_lo = max(0, -ix0) * 3, q_hi = min(207, (p.P - ix0) * 3);   // bytes of pixels inside the tile
#pragma unroll
        for (int k = 0; k < SP_NLOAD; ++k) {
          int r, d;
          piece_rd(k, &r, &d);
          const int q0 = 4 * d - 1;
          const int lo = min(max(q_lo - q0, 0), 4), hi = min(max(q_hi - q0, 0), 4);   // bytes [lo, hi) of the dword stay
          colm[k] = (lo < 4 ? 0xFFFFFFFFu << (8 * lo) : 0u) & (hi > 0 ? 0xFFFFFFFFu >> (32 - 8 * hi) : 0u);
        }
      }
      if (!(ix0 >= 0 && ix0 + 69 <= p.P)) {
#pragma unroll
        for (int k = 0; k < SP_NLOAD; ++k) wr[k] &= colm[k];
      }
      if (!(iy0 >= 0 && iy0 + SP_WR <= p.P)) {
        const int r_lo = max(0, -iy0), r_hi = min(SP_WR, p.P - iy0);
#pragma unroll
        for (int k = 0; k < SP_NLOAD; ++k) {
          int r, d;
          piece_rd(k, &r, &d);
          if (r < r_lo || r >= r_hi) wr[k] = 0u;
        }
      }
#pragma unroll
      for (int k = 0; k < SP_NLOAD; ++k) {
        if (k < SP_NLOAD - 1 || tid < SP_TAIL) {
          // bf16(k * f32(1/255)) == bf16(f32(k)/255) for all 256 byte values (tests/test_div255.py), so one
          // multiply replaces the exact-division sequence here
          const float r255 = 1.0f / 255.0f;
          const uint32_t w = wr[k];
          typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
          const bf16x4_t w4 = {(__bf16)((float)(w & 0xFFu) * r255), (__bf16)((float)((w >> 8) & 0xFFu) * r255),
                               (__bf16)((float)((w >> 16) & 0xFFu) * r255), (__bf16)((float)(w >> 24) * r255)};
          *reinterpret_cast<bf16x4_t*>(win_lds + wdst[k]) = w4;   // element 4d = slot 0 (dummy) when d == 0
        }
      }
    } else {
      for (int idx = tid; idx < SP_WR * 207; idx += SP_T) {
        const int r = idx / 207, q = idx % 207;
        const int iy = iy0 + r, ix = ix0 + q / 3, c = q % 3;
        float v = 0.f;
        if (iy >= 0 && iy < p.P && ix >= 0 && ix < p.P) v = p.x_nchw[(((int64_t)t.b * 3 + c) * p.P + iy) * p.P + ix];
        win[r * SP_WE + 1 + q] = (uint16_t)f32_to_bf16(v);
      }
    }
  };

  Tile cur = next_tile();
  Tile nxt = next_tile();
  Tile nn = next_tile();
#ifdef SP_STAGGER
  {  // co-resident workgroups (blockIdx / 256 on a 768-workgroup grid) start a third of a step apart
    const int ph = (int)(blockIdx.x / 256u) % 3;
    for (int i = 0; i < ph * SP_STAGGER; ++i) __builtin_amdgcn_s_sleep(32);
  }
#endif
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                     // weights, scale/shift, zeroed window
  if (cur.valid) { load_window(cur, wr); store_window(cur, wr); }
  if (nxt.valid) load_window(nxt, wr);
  __syncthreads();

  unsigned long long tacc[6] = {0, 0, 0, 0, 0, 0};
  unsigned long long tprev = STAMP ? __builtin_readcyclecounter() : 0ull;
  auto stamp = [&](int slot) __attribute__((always_inline)) {
    if constexpr (STAMP) {
      __builtin_amdgcn_sched_barrier(0);
      const unsigned long long now = __builtin_readcyclecounter();
      __builtin_amdgcn_sched_barrier(0);
      tacc[slot] += now - tprev;
      tprev = now;
    }
  };
  typedef short sp_i16x2 __attribute__((ext_vector_type(2)));
  auto max16 = [](uint32_t a, uint32_t b) __attribute__((always_inline)) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(sp_i16x2, a), __builtin_bit_cast(sp_i16x2, b)));
  };
  // horizontal 3-max and the ReLU.  PC = 15: lanes tx, tx+1, tx+2; PC = 16: lanes tx-1, tx, tx+1 of values that have the ReLU behind them
  auto hmax3 = [&](uint32_t v0) __attribute__((always_inline)) {
    // wave_shl:1 / wave_shr:1 with bound_ctrl: lane 63 / lane 0 reads 0 and no lane keeps its old value, so the destination needs
    // no initialisation
    const uint32_t v1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v0, 0x130, 0xF, 0xF, true);  // lane+1
    if constexpr (PC == 16) {
      const uint32_t vl = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v0, 0x138, 0xF, 0xF, true);  // lane-1
      return max16(max16(v0, v1), tx == 0 ? 0u : vl);   // lane 32's left neighbour is the other half-wave's last column: the seam
    } else {
      const uint32_t v2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v1, 0x130, 0xF, 0xF, true);  // lane+2
      return max16(max16(max16(v0, v1), v2), 0u);
    }
  };
  // exchange slot addressing: [lane][4 quads of 16 B], quad mt*2 + pr holds the groups g = 2pr, 2pr+1 of cout half mt;
  // quads are XOR-swizzled with lane bits 2..3 (8 consecutive lanes of a ds_*_b128 pass hit 8 different bank groups)
  const int xlane = lane * 64, xsw = (lane >> 2) & 3;
  const bool even = !(tx & 1);
  // MFMA operand addresses.  A: [k-step][cout half][lane][16 B].  B, in bytes from window row 4w (the first tap row of
  // the wave's conv row 2w) and element 6*tx: see sp_kslot; the lane-varying part takes three values.
  // The wave's two conv rows read window rows 4w + kh and 4w + 2 + kh: the B fragment of a row pair serves conv row
  // 2w with the weights of kernel rows (a, a+1) and conv row 2w+1 with those of (a-2, a-1).  14 B fragments feed the
  // 44 MFMAs of a step (22 if each conv row read its own); a weight fragment is read once and kept for its second
  // use three fragments later.
  const char* a_base = w_lds + lane * 16;
  const int b_base = ((4 * wave) * SP_WE + 6 * tx) * 2;
  int b_off[3];
  b_off[0] = 16 * h;                       // [row a: g0 g1], [row a+1: g1 g2] (+16), [single row: g0 g1]
  b_off[1] = h ? SP_WE * 2 : 32;           // [row a: g2 | row a+1: g0]
  b_off[2] = h ? 16 : 32;                  // [single row: g2 | zero weights: any finite elements]
  // schedule of a step: B fragment f = (window row offset in rows, 16-byte shift, lane-varying select), the k-step whose
  // weights conv row 2w (ka) and conv row 2w+1 (kb) multiply it with (-1: none)
  struct SpStep { int row, shift, sel, ka, kb; };
  constexpr SpStep SCHED[14] = {
      {0, 0, 0, 0, -1}, {0, 0, 1, 1, -1}, {1, 16, 0, 2, -1},
      {2, 0, 0, 3, 0},  {2, 0, 1, 4, 1},  {3, 16, 0, 5, 2},
      {4, 0, 0, 6, 3},  {4, 0, 1, 7, 4},  {5, 16, 0, 8, 5},
      {6, 0, 0, 9, 6},  {6, 0, 1, 10, 7}, {7, 16, 0, -1, 8},
      {8, 0, 0, -1, 9}, {8, 0, 2, -1, 10}};
  auto read_a = [&](int ks, int mt) __attribute__((always_inline)) {
    return (SP_ABL & 32) ? make_uint4(lane, tid, lane, lane) : *reinterpret_cast<const uint4*>(a_base + (ks * 2 + mt) * FRAG_BYTES);
  };
  auto read_b = [&](int f) __attribute__((always_inline)) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(win_lds + b_base + b_off[SCHED[f].sel] + SCHED[f].row * SP_WE * 2 + SCHED[f].shift);
    return (SP_ABL & 32) ? make_uint4(tid, tid, lane, tid) : make_uint4(src[0], src[1], src[2], src[3]);
  };
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // One step.  The slide bytes of step it+2 are requested now (into wfly) and converted during step it+1: a full step covers
  // the HBM latency; wnow holds the bytes of step it+1, requested a step ago.  The two register sets trade roles every step
  // (the loop below is unrolled by two: a copy between them would wait for the loads it copies).
  auto step = [&](int it, uint32_t (&wnow)[SP_NLOAD], uint32_t (&wfly)[SP_NLOAD]) __attribute__((always_inline)) {
    if (nn.valid) load_window(nn, wfly);
    const Tile n3 = next_tile();       // step it + 3: its origin load is consumed an iteration from now
    stamp(0);
    uint32_t vm[2][4][2];   // max over this wave's two conv rows: [cout half][group of 8 couts][bf16 pairs]
    if (cur.valid) {
      f32x16 acc[2][2];
      uint4 wa[SP_KS][2];          // weight fragments (live from their first use to their second)
      uint4 bq[SP_PF + 1];         // window fragments, SP_PF steps ahead of the MFMAs (LDS latency under load is several MFMAs long)
      auto fetch = [&](int f) __attribute__((always_inline)) {
        bq[f % (SP_PF + 1)] = read_b(f);
        if (SCHED[f].ka >= 0) { wa[SCHED[f].ka][0] = read_a(SCHED[f].ka, 0); wa[SCHED[f].ka][1] = read_a(SCHED[f].ka, 1); }
      };
#pragma unroll
      for (int f = 0; f < SP_PF; ++f) fetch(f);
#pragma unroll
      for (int f = 0; f < 14; ++f) {
        if (f + SP_PF < 14) fetch(f + SP_PF);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          const int ks = nt == 0 ? SCHED[f].ka : SCHED[f].kb;
          if (ks < 0) continue;
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) {
            if constexpr (SP_ABL & 1) {
              if (ks == 0) acc[mt][nt] = zero16;
              asm volatile("" :: "v"(wa[ks][mt].x), "v"(wa[ks][mt].y), "v"(wa[ks][mt].z), "v"(wa[ks][mt].w), "v"(bq[f % (SP_PF + 1)].x), "v"(bq[f % (SP_PF + 1)].y), "v"(bq[f % (SP_PF + 1)].z), "v"(bq[f % (SP_PF + 1)].w));
            } else {
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wa[ks][mt]), __builtin_bit_cast(bf16x8, bq[f % (SP_PF + 1)]),
                                                                    ks == 0 ? zero16 : acc[mt][nt], 0, 0, 0);
            }
          }
        }
      }
      stamp(1);
      // BN + pack.  Row b (the wave's second conv row) goes to the neighbour through LDS as it is.
      const int r0 = 2 * cur.py0, c0 = 2 * cur.px0 - CX;
      const bool interior = r0 + SP_CR <= p.Hc && c0 >= 0 && c0 + SP_CC <= p.Wc;   // workgroup-uniform
      char* slot = xch_lds + (wave < SP_W - 1 ? wave : SP_W - 1 + (it & 1)) * SP_XCH + xlane;
      auto bn_pack = [&](auto inside) __attribute__((always_inline)) {
        constexpr bool INSIDE = decltype(inside)::value;
        uint32_t okm[2] = {~0u, ~0u};
        if constexpr (!INSIDE) {   // conv rows / columns outside the image count as 0
          const bool col_ok = (c0 + tx) >= 0 && (c0 + tx) < p.Wc;
          okm[0] = col_ok && (r0 + 2 * wave) < p.Hc ? ~0u : 0u;
          okm[1] = col_ok && (r0 + 2 * wave + 1) < p.Hc ? ~0u : 0u;
        }
        typedef float f32x2_t __attribute__((ext_vector_type(2)));
        typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int pr = 0; pr < 2; ++pr) {
            uint32_t rb[2][2];
#pragma unroll
            for (int gg = 0; gg < 2; ++gg) {
              const int g = 2 * pr + gg;
              const float4 sc = *reinterpret_cast<const float4*>(ss_lds + (mt * 4 + g) * 8 + 4 * h);        // BN scale / shift of this lane's
              const float4 sh = *reinterpret_cast<const float4*>(ss_lds + 64 + (mt * 4 + g) * 8 + 4 * h);   // 4 couts (LDS: keeps 64 VGPRs free)
              uint32_t row[2][2];
#pragma unroll
              for (int nt = 0; nt < 2; ++nt) {
                const f32x2_t lo = __builtin_elementwise_fma(f32x2_t{acc[mt][nt][4 * g + 0], acc[mt][nt][4 * g + 1]}, f32x2_t{sc.x, sc.y}, f32x2_t{sh.x, sh.y});
                const f32x2_t hi = __builtin_elementwise_fma(f32x2_t{acc[mt][nt][4 * g + 2], acc[mt][nt][4 * g + 3]}, f32x2_t{sc.z, sc.w}, f32x2_t{sh.z, sh.w});
                row[nt][0] = __builtin_bit_cast(uint32_t, __builtin_convertvector(lo, bf16x2_t));   // v_cvt_pk_bf16_f32 (RNE)
                row[nt][1] = __builtin_bit_cast(uint32_t, __builtin_convertvector(hi, bf16x2_t));
                if constexpr (!INSIDE) { row[nt][0] &= okm[nt]; row[nt][1] &= okm[nt]; }
              }
              rb[gg][0] = row[1][0]; rb[gg][1] = row[1][1];
              vm[mt][g][0] = max16(row[0][0], row[1][0]);
              vm[mt][g][1] = max16(row[0][1], row[1][1]);
            }
            *reinterpret_cast<uint4*>(slot + (((mt * 2 + pr) ^ xsw) << 4)) = make_uint4(rb[0][0], rb[0][1], rb[1][0], rb[1][1]);
          }
      };
      if (interior) bn_pack(std::true_type{});   // workgroup-uniform branch: two copies of the block
      else bn_pack(std::false_type{});
      stamp(2);
    }
    // barrier 1: the exchanged rows are visible and every wave is done reading the window
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    stamp(5);
    // the prefetched window is converted BEFORE this tile's pooled stores are issued: its vmcnt wait then covers
    // only loads that are an iteration old, not the stores
    if (nxt.valid) store_window(nxt, wnow);
    stamp(4);
    if (cur.valid) {
      // conv row 2w-1: the second row of wave w-1; for wave 0 the last row of the previous step (none at the top: 0)
      const char* prev = xch_lds + (wave > 0 ? wave - 1 : SP_W - 1 + ((it + 1) & 1)) * SP_XCH + xlane;
      const bool have_prev = wave > 0 || !cur.first;   // wave-uniform
      // even lanes hold pooled pixel (py0 + wave, px0 + tx/2); 16-byte stores after the half-wave swap
      const int py = cur.py0 + wave, px = cur.px0 + (tx >> 1);
      const bool st_ok = even && (tx >> 1) < PC && py < p.Hp && px < p.Wp;
      // channel-blocked output [image][2 chunks of 32 couts][Hp][Wp][32] (the layout the 3x3 kernels read)
      const int plane = p.Hp * p.Wp * 32;
      __bf16* out = static_cast<__bf16*>(p.out) + (int64_t)cur.b * 2 * plane + (py * p.Wp + px) * 32;
      // PC = 16: lanes 31 and 63 hold conv column 2*px0 + 31, which the next strip's first pooled column needs
      const bool seam_ok = PC == 16 && tx == 31 && py < p.Hp && cur.px0 + PC < p.Wp;
      // the seam pixel's 64 channels as the two lanes hold them, [half-wave][cout half][group][4 couts]: one 16-byte store per
      // (cout half, group pair).  Wave-uniform; the lane's part is added at the store
      __bf16* seam = nullptr;
      if constexpr (PC == 16)
        seam = static_cast<__bf16*>(p.seam) + (((int64_t)cur.b * (p.tiles_x - 1) + cur.px0 / PC) * p.Hp + py) * 64;
      uint4 pvq[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) pvq[q] = make_uint4(0u, 0u, 0u, 0u);
      if (have_prev) {
#pragma unroll
        for (int q = 0; q < 4; ++q) pvq[q] = *reinterpret_cast<const uint4*>(prev + ((q ^ xsw) << 4));
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
          const uint4 pv = pvq[mt * 2 + pr];
          uint32_t v[4] = {max16(vm[mt][2 * pr][0], pv.x), max16(vm[mt][2 * pr][1], pv.y),
                           max16(vm[mt][2 * pr + 1][0], pv.z), max16(vm[mt][2 * pr + 1][1], pv.w)};
          if constexpr (PC == 16) {   // the ReLU first (max commutes with it): the seam column goes out with it applied
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = max16(v[i], 0u);
            if constexpr (!(SP_ABL & 16)) {
              if (seam_ok) *reinterpret_cast<uint4*>(seam + h * 32 + mt * 16 + pr * 8) = make_uint4(v[0], v[1], v[2], v[3]);
            }
          }
          if constexpr (!(SP_ABL & 8)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = hmax3(v[i]);   // horizontal 3-max ... and the ReLU
          }
          uint32_t a0 = v[0], a1 = v[1], b0 = v[2], b1 = v[3];
          { const auto r = __builtin_amdgcn_permlane32_swap(a0, b0, false, false); a0 = r[0]; b0 = r[1]; }
          { const auto r = __builtin_amdgcn_permlane32_swap(a1, b1, false, false); a1 = r[0]; b1 = r[1]; }
          if constexpr (SP_ABL & 16) asm volatile("" :: "v"(a0), "v"(a1), "v"(b0), "v"(b1));
          else if (st_ok) *reinterpret_cast<uint4*>(out + mt * plane + (2 * pr + h) * 8) = make_uint4(a0, a1, b0, b1);
        }
      stamp(3);
    }
    // barrier 2: the next window is staged; the exchange slots may be rewritten.  Raw barrier: LDS traffic only
    // (__syncthreads() would also drain vmcnt(0), i.e. wait for this tile's pooled global stores).
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    stamp(5);
    cur = nxt;
    nxt = nn;
    nn = n3;
  };
  for (int it = 0; it < p.iters; it += 2) {   // a step past the end finds no valid tile and only keeps the barriers paired
    step(it, wr, wr2);
    step(it + 1, wr2, wr);
  }
  if constexpr (STAMP) {
    if (tid == 0 && p.stamps) {
      for (int i = 0; i < 6; ++i) atomicAdd(p.stamps + i, tacc[i]);
      atomicAdd(p.stamps + 6, 1ull);
    }
  }
}

// PC = 16: out[b][:][py][16(s+1)] = max(out, seam[b][s][py]) for every seam pixel, 16 bytes (8 channels) per thread.
// Non-negative bf16 order like 16-bit integers.
__global__ __launch_bounds__(256) void stem_seam_kernel(const void* __restrict__ seam, __bf16* __restrict__ out, int64_t total,
                                                        int nseam, int Hp, int Wp) {
  typedef short sp_i16x8 __attribute__((ext_vector_type(8)));
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // [b][s][py][8 pieces]
  if (i >= total) return;
  const int c8 = (int)(i & 7);   // channels 8*c8 ..: cout half c8 >> 2, group c8 & 3; its couts 0..3 / 4..7 come from half-wave 0 / 1
  const int64_t px = i >> 3;
  const int py = (int)(px % Hp), s = (int)((px / Hp) % nseam);
  const int64_t b = px / Hp / nseam;
  uint4* o = reinterpret_cast<uint4*>(out + (((b * 2 + (c8 >> 2)) * Hp + py) * Wp + 16 * (s + 1)) * 32 + (c8 & 3) * 8);
  const uint2* row = reinterpret_cast<const uint2*>(seam) + px * 16 + c8;   // seam row: [half-wave][cout half][group][4 couts]
  const uint2 lo = row[0], hi = row[8];
  *o = __builtin_bit_cast(uint4, __builtin_elementwise_max(__builtin_bit_cast(sp_i16x8, *o), __builtin_bit_cast(sp_i16x8, make_uint4(lo.x, lo.y, hi.x, hi.y))));
}
