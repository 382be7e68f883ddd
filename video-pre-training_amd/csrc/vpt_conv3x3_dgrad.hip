// 3x3 / pad-1 convolution of the IMPALA residual CNN, dgrad: vpt_conv3x3_dgrad_kernel.  Layout, tile and what it shares with the forward
// kernel (vpt_conv3x3_fwd.hip): vpt_conv3x3_tile.h.
// Dgrad modes (2, 3, 6): v_mfma_f32_32x32x16 main loop (4x2 accumulators of 32x32 per wave; the 32 rows of an M-subtile map to pixels
//   by sub_row() so that every hardware 16-lane ds_read_b128 group covers 16 consecutive pixels of ONE image row), epilogue through
//   v_permlane32_swap / v_permlane16_swap into whole 128-byte lines.
#include "vpt_conv3x3_tile.h"
#include <type_traits>
// Template parameters of vpt_conv3x3_dgrad_kernel:
// TRACE (tools/conv_trace.py): phase timestamps.  Compile time because s_memrealtime is a scalar-memory operation: one of them
// in flight makes lgkmcnt out of order and every LDS wait of the epilogue degenerates to lgkmcnt(0).
// MODE (compile time, so the epilogue carries no runtime branches; the numbers are the ones of the launch function, 0, 1, 4, 5, 7 being the
// forward kernel's): 2 dgrad (+ c0 + c1 * xin), 3 dgrad + skip connection, 6: see the kernel's first lines.
template <bool TRACE, int MODE>
__global__ __launch_bounds__(256, 2) void vpt_conv3x3_dgrad_kernel(VptConv3x3Args a) {
  static_assert(MODE == 2 || MODE == 3 || MODE == 6, "dgrad modes");
  constexpr int NWAVE = 4, NTHR = 64 * NWAVE;
  constexpr int HPIX = 18 * 18;                                  // halo pixels
  constexpr int NA = (HPIX * 4 + NTHR - 1) / NTHR;               // 16-byte halo chunks per thread and channel block: 6
  constexpr int NDMA = 24 / NWAVE;                               // 1 KB weight-DMA pieces per wave and step: 6
  constexpr int A_SZ = A_BYTES, KK_O = KK_OFF, SMEM_SZ = SMEM_BYTES;
  // 6 dgrad of a block's conv1 that hands the block's conv0 its backward operand directly (round 5):  dy = conv^T + c0 + c1 * xin is the
  // gradient w.r.t. conv0's output y = xin, conv0 has no residual, so its ReLU gate is [xin > 0] and its operand dacc0 = rstd0 * dy * [xin > 0]
  // (rstd0: the statistics of conv0's INPUT, gate_stats) is written instead of dy -- vpt_conv_bwd_prep_kernel's pass over (dy, y) -> dacc
  // shrinks to a reduction over dacc0 alone; gate_u[f] += sum rstd0 * dy * xin (= rstd0 * sum dz v: T1's data term; closed gates add 0).
  constexpr bool GATE = MODE == 6;
  constexpr bool HAS_RES = MODE == 3;
  constexpr bool DEFER_STORES = MODE != 3;   // mode 3 holds skip + xin pieces as well: no registers left for the packed results
  __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM_SZ];
  const int tid = threadIdx.x, lane = tid & 63;
  // profiling (vpt_conv3x3_set_trace): CU id + 100 MHz timestamps of the tile's phases
  int cu_key = -1;
  long long t_trace[3];
  if (TRACE && tid == 0) {
    t_trace[0] = wall_clock64();
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID: cu_id[11:8] sh_id[12] se_id[15:13]
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);   // HW_REG_XCC_ID[3:0]
    cu_key = (int)(((xcc & 15u) << 8) | ((hw >> 8) & 0xffu));
  }
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int hi = lane >> 5, l31 = lane & 31;
  const VptConvTile tile = conv_tile_decode(a.NT, a.W >> 4, a.H / 16);
  const int nt = tile.nt, f = tile.f;
  const int tx0 = tile.tx * 16, ty0 = tile.ty * 16;
  const int NCB = a.Cin >> 5;
  const int HW = a.H * a.W;

  // ---- halo staging map: chunk q -> (pixel P = 8*(q>>5) + (q&7), part = (q>>3)&3) ----
  int a_loff[NA];            // LDS byte offset, -1: no chunk (beyond the 324 halo pixels)
  unsigned a_gbyte[NA];      // byte offset inside one channel-block plane (clamped to 0 outside the image)
  unsigned a_inside = 0;    // bit m: chunk m lies inside the image (else literal zeros: the conv pads the NORMALISED tensor)
#pragma unroll
  for (int m = 0; m < NA; ++m) {
    const int q = tid + NTHR * m;
    const int P = ((q >> 5) << 3) + (q & 7);
    const int part = (q >> 3) & 3;
    a_loff[m] = -1;
    a_gbyte[m] = 0u;
    if (P < HPIX) {
      const int hy = P / 18, hx = P - hy * 18;
      const int y = ty0 - 1 + hy, x = tx0 - 1 + hx;
      a_loff[m] = P * A_RS + part * 16;
      if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
        a_gbyte[m] = (unsigned)((y * a.W + x) * 32 + part * 8) * 2u;
        a_inside |= 1u << m;
      }
    }
  }
  const op16_t* xplane = a.x + (size_t)f * NCB * HW * 32;
  // weight DMA: wave w moves pieces (NWAVE*m + w), m = 0..NDMA-1, of the 24 KB step tile; lane = 16-byte chunk
  const op16_t* wbase = a.wpk + (size_t)nt * NCB * 9 * 4096 + (size_t)(w * 64 + lane) * 8;
  unsigned char* bdst = smem + A_SZ + w * 1024;
  // ====================================================================================================================
  // Macros of the DGRAD loop (modes 2, 3, 6): v_mfma_f32_32x32x16, wave tile 128 px x 64 couts = acc[4][2], lane-swap epilogue.
  // One K step = one kernel row (3 taps) of one 32-channel block = 6 groups (tap dx, 16-channel half ks) of 8 MFMAs per wave.  The schedule
  // is explicit, one instruction pair at a time, pinned with sched_barrier (left alone, the scheduler sinks every fragment read next to its
  // first use to save registers, and the matrix pipe drains for one LDS round trip per group):
  //   - two fragment register sets; while group g's MFMAs issue, the fragments of group g+1 are requested, one pair of ds_read_b128 behind
  //     each of the first three MFMAs, in the order the next group consumes them;
  //   - the two remaining slots of each group carry the step's global traffic: the weight DMA of the next step (6 x global_load_lds, groups
  //     0-2) and the halo of the next channel block / the residual (groups 3-4), so no MFMA ever queues behind a burst of memory instructions;
  //   - the step's barrier sits in front of the LAST group's MFMAs: every wave then holds its last fragments of the step in registers, the
  //     next step's weights (requested >= 24 MFMAs earlier) have landed, so the next step's first fragments are requested behind the barrier
  //     and arrive under group 5's MFMAs.
  // ====================================================================================================================
#define WRITE_HALO()                                                                                      \
  _Pragma("unroll") for (int m_ = 0; m_ < NA; ++m_)                                                       \
    if (a_loff[m_] >= 0) *(u32x4*)(smem + a_loff[m_]) = ((a_inside >> m_) & 1u) ? areg[m_] : zero4
#define MM(set_, m_, n_) acc[m_][n_] = VPT_MFMA_32X32X16(fb[set_][n_], fa[set_][m_], acc[m_][n_], 0, 0, 0)
#define MMZ(set_, m_, n_) acc[m_][n_] = VPT_MFMA_32X32X16(fb[set_][n_], fa[set_][m_], zero16, 0, 0, 0)   /* C = 0: no zero-initialised accumulators */
#define FA_LD(set_, dy_, g_, m_) \
  fa[set_][m_] = *(const op16x8*)(aL + ((dy_) * 18 + ((g_) >> 1)) * A_RS + (m_) * (2 * 18 * A_RS) + ((g_) & 1) * 32)
#define FB_LD(set_, g_, n_, boff_) \
  fb[set_][n_] = *(const op16x8*)((((g_) & 1) ? bL1 : bL0) + (boff_) + ((g_) >> 1) * (128 * 64) + (n_) * (32 * 64))
  // MFMAs of register set `set_`; fragments of group (ndy_, ng_) go to the other set; X0 / X1: the two free slots
#define GROUP_(MM_, set_, ndy_, ng_, nboff_, X0, X1)                                                      \
  do {                                                                                                    \
    MM_(set_, 0, 0); FB_LD(1 - (set_), ng_, 0, nboff_); FA_LD(1 - (set_), ndy_, ng_, 0); SB();            \
    MM_(set_, 0, 1); FB_LD(1 - (set_), ng_, 1, nboff_); FA_LD(1 - (set_), ndy_, ng_, 1); SB();            \
    MM_(set_, 1, 0); FA_LD(1 - (set_), ndy_, ng_, 2); FA_LD(1 - (set_), ndy_, ng_, 3); SB();              \
    MM_(set_, 1, 1); SB();                                                                                \
    MM_(set_, 2, 0); X0; SB();                                                                            \
    MM_(set_, 2, 1); SB();                                                                                \
    MM_(set_, 3, 0); X1; SB();                                                                            \
    MM_(set_, 3, 1); SB();                                                                                \
  } while (0)
#define GROUP(set_, ndy_, ng_, nboff_, X0, X1) GROUP_(MM, set_, ndy_, ng_, nboff_, X0, X1)
#define GROUP_Z(set_, ndy_, ng_, nboff_, X0, X1) GROUP_(MMZ, set_, ndy_, ng_, nboff_, X0, X1)   /* the tile's first 8 MFMAs */
#define GROUP_TAIL(set_)                                                                                  \
  do {                                                                                                    \
    _Pragma("unroll") for (int m_ = 0; m_ < 4; ++m_) { MM(set_, m_, 0); MM(set_, m_, 1); }                \
  } while (0)
  // residual (mode 3: the skip connection) in the accumulators' own layout, 8-byte loads; xin and the output as whole 128-byte lines (EPI_LD)
#define EPI_LD(ptr_, m_, n2_, p_) (*(const u32x4*)((const char*)((ptr_) + cbase[n2_]) + (svoff[p_] + (unsigned)(m_) * gm_b)))
#define EPI_LDN(ptr_, m_, n2_, g_) (*(const u32x2*)((const char*)((ptr_) + cbase[n2_]) + (nvoff + (unsigned)(m_) * gm_b + 16u * (unsigned)(g_))))
#define LOAD_RES(m_)                                                                                      \
  _Pragma("unroll") for (int n2_ = 0; n2_ < 2; ++n2_)                                                     \
    _Pragma("unroll") for (int g_ = 0; g_ < 4; ++g_) rq[m_][n2_][g_] = EPI_LDN(a.res, m_, n2_, g_)
#define XR(m_, n2_, p_) do { rq[m_][n2_][2 * (p_)] = EPI_LDN(resp, m_, n2_, 2 * (p_)); rq[m_][n2_][2 * (p_) + 1] = EPI_LDN(resp, m_, n2_, 2 * (p_) + 1); } while (0)
#define CONV_STEP(cb_, dy_, NEXT_DY, PRE_A, WR_A, PRE_R, LAST, FIRST)                                            \
  do {                                                                                                    \
    const int s_ = (cb_) * 3 + (dy_);                                                                     \
    const int boff_ = (s_ & 1) * B_BYTES, noff_ = B_BYTES - boff_;                                        \
    const op16_t* wp_ = wbase + (size_t)(s_ + 1) * 12288;                                                 \
    unsigned char* bd_ = bdst + noff_;                                                                    \
    const unsigned cbo_ = (unsigned)((cb_) + 1) * (unsigned)HW * 64u; /* bytes; uniform */                \
    if (FIRST) {                                                                                          \
      GROUP_Z(0, dy_, 1, boff_, GLDS(0), GLDS(1));                                                        \
      GROUP(1, dy_, 2, boff_, GLDS(2), GLDS(3));                                                          \
      GROUP(0, dy_, 3, boff_, GLDS(4), GLDS(5));                                                          \
    } else if (LAST) {                                                                                    \
      GROUP(0, dy_, 1, boff_, NOP_(), NOP_());                                                            \
      GROUP(1, dy_, 2, boff_, NOP_(), NOP_());                                                            \
      GROUP(0, dy_, 3, boff_, NOP_(), NOP_());                                                            \
    } else {                                                                                              \
      GROUP(0, dy_, 1, boff_, GLDS(0), GLDS(1));                                                          \
      GROUP(1, dy_, 2, boff_, GLDS(2), GLDS(3));                                                          \
      GROUP(0, dy_, 3, boff_, GLDS(4), GLDS(5));                                                          \
    }                                                                                                     \
    if (PRE_A) {                                                                                          \
      GROUP(1, dy_, 4, boff_, do { XA(0); XA(1); } while (0), do { XA(2); } while (0));                   \
      GROUP(0, dy_, 5, boff_, do { XA(3); XA(4); } while (0), do { XA(5); } while (0));                   \
      if (NA == 6) WAIT_BARRIER(6); else WAIT_BARRIER(5);                                                 \
    } else if ((PRE_R) && HAS_RES) { /* compile-time: without a residual the loads would be dead code and the count wrong */ \
      GROUP(1, dy_, 4, boff_, do { XR(0, 0, 0); XR(0, 0, 1); } while (0), do { XR(0, 1, 0); XR(0, 1, 1); } while (0)); \
      GROUP(0, dy_, 5, boff_, do { XR(1, 0, 0); XR(1, 0, 1); } while (0), do { XR(1, 1, 0); XR(1, 1, 1); } while (0)); \
      WAIT_BARRIER(16);   /* (two 8-byte loads per XR) */                                                \
    } else {                                                                                              \
      GROUP(1, dy_, 4, boff_, NOP_(), NOP_());                                                            \
      GROUP(0, dy_, 5, boff_, NOP_(), NOP_());                                                            \
      WAIT_BARRIER(0);                                                                                    \
    }                                                                                                     \
    if (WR_A) {   /* the halo of the next channel block replaces the current one: second barrier before its first read */ \
      _Pragma("unroll") for (int m_ = 0; m_ < 4; ++m_) {                                                  \
        if (a_loff[m_] >= 0) *(u32x4*)(smem + a_loff[m_]) = ((a_inside >> m_) & 1u) ? areg[m_] : zero4; \
        if (m_ + 4 < NA && a_loff[m_ + 4] >= 0) *(u32x4*)(smem + a_loff[m_ + 4]) = ((a_inside >> (m_ + 4)) & 1u) ? areg[m_ + 4] : zero4; \
        SB(); MM(1, m_, 0); SB();                                                                         \
      }                                                                                                   \
      WAIT_BARRIER(0);                                                                                    \
      MM(1, 0, 1); FB_LD(0, 0, 0, noff_); SB();                                                           \
      MM(1, 1, 1); FA_LD(0, 0, 0, 0); SB();                                                               \
      MM(1, 2, 1); FB_LD(0, 0, 1, noff_); FA_LD(0, 0, 0, 1); SB();                                        \
      MM(1, 3, 1); FA_LD(0, 0, 0, 2); FA_LD(0, 0, 0, 3); SB();                                            \
    } else if (LAST) {                                                                                    \
      GROUP_TAIL(1);                                                                                      \
    } else {                                                                                              \
      GROUP(1, NEXT_DY, 0, noff_, NOP_(), NOP_());                                                        \
    }                                                                                                     \
  } while (0)
  // epilogue: the forward layer's input one subtile ahead, and the lane exchanges between "whole pixel rows" and the accumulator layout
#define LOAD_XIN(m_)                                                                                      \
  _Pragma("unroll") for (int n2_ = 0; n2_ < 2; ++n2_)                                                     \
    _Pragma("unroll") for (int p_ = 0; p_ < 2; ++p_) xq[(m_) & 1][n2_][p_] = EPI_LD(a.xin, m_, n2_, p_)
  // rows arrive per instruction j as the pixels of lanes (l31 & 15) + 16 j; the exchange gives every lane the two 16-byte pieces (p = 0, 1) of its own pixel
#define ROWS_TO_PIECES(src_, dst_)                                                                        \
  _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) {                                                      \
    const auto sw_ = __builtin_amdgcn_permlane16_swap((src_)[0][j_], (src_)[1][j_], false, false);        \
    (dst_)[0][j_] = sw_[0]; (dst_)[1][j_] = sw_[1];                                                       \
  }
  // 16-byte piece {first half x, y | second half z, w} of a lane pair -> this lane's own 8 bytes of group 2p (e) and 2p + 1 (o)
#define UNSWAP(v_, e_, o_)                                                                                \
  do {                                                                                                    \
    const auto s0_ = __builtin_amdgcn_permlane32_swap((v_).x, (v_).z, false, false);                      \
    const auto s1_ = __builtin_amdgcn_permlane32_swap((v_).y, (v_).w, false, false);                      \
    (e_).x = s0_[0]; (o_).x = s0_[1]; (e_).y = s1_[0]; (o_).y = s1_[1];                                   \
  } while (0)
  u32x4 areg[NA];
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  // ---- prologue: weights of step 0 (DMA), halo of channel block 0, epilogue constant table ----
  ISSUE_B(0, 0);
#pragma unroll
  for (int m = 0; m < NA; ++m) areg[m] = *(const u32x4*)((const char*)xplane + a_gbyte[m]);
  float c0f = 0.f, c1f = 0.f;
  if (a.coef) {
    c0f = a.coef[2 * f];
    c1f = a.coef[2 * f + 1];
  }
  float rgate = 1.f;
  if (GATE) {      // everything the epilogue adds is linear in the scale: fold rstd0 into the coefficients
    float mg;
    frame_mean_rstd(a.gate_stats, f, a.inv_count_gate, mg, rgate);
    c0f *= rgate;
    c1f *= rgate;
  }
  {   // the forward kernel's epilogue-table area: the dgrad modes read none of it and store the zeros they always did (no instruction appears or
      // disappears in the split; the block statistics' slots behind it serve gate_u)
    float* kk = (float*)(smem + KK_O);
    constexpr int NKK = (9 * 128 + NTHR - 1) / NTHR;
#pragma unroll
    for (int k = 0; k < NKK; ++k) {
      const int idx = tid + NTHR * k;
      if (idx < 9 * 128) kk[idx] = 0.f;
    }
  }
  WRITE_HALO();
  __syncthreads();

  f32x16 acc[4][2];
  f32x16 zero16;
#pragma unroll
  for (int r = 0; r < 16; ++r) zero16[r] = 0.f;

  // fragment base addresses
  const unsigned char* aL = smem + ((wm * 8 + sub_row(l31)) * 18 + (l31 & 15)) * A_RS + hi * 16;
  const int bsw = (l31 >> 2) & 3;
  const unsigned char* bL0 = smem + A_SZ + (wn * 64 + l31) * 64 + (((0 + hi) ^ bsw) << 4);  // ks = 0
  const unsigned char* bL1 = smem + A_SZ + (wn * 64 + l31) * 64 + (((2 + hi) ^ bsw) << 4);  // ks = 1
  // epilogue addressing (needed early: the residual is requested during the last channel block)
  // Dgrad epilogue: operands are SWAPPED in the MFMA (weights = A rows, pixels = B columns): a lane holds ONE pixel (column l31 of the
  // 2x16-pixel subtile) and, per accumulator, four groups g of 4 consecutive output channels 8g + 4hi .. +3 -- 8 bytes of
  // the pixel's 64-byte channel row per group, the partner lane (l31, 1 - hi) holding the 8 bytes next to them.  One
  // v_permlane32_swap per dword turns the pair (g = 2p, 2p + 1) into 16 CONTIGUOUS bytes per lane (lower half-wave: bytes
  // 32p.., upper: 32p + 16..), and one v_permlane16_swap per dword (lanes l <-> l ^ 16, p = 0 <-> 1) regroups those so that one
  // 16-byte access per lane covers the WHOLE 64-byte channel row of 16 pixels: the residual / xin / output move as complete
  // 128-byte lines, with no LDS staging at all.
  const int CB_out = a.Cout >> 5;
  const int cb0 = nt * 4 + wn * 2;                 // 32-channel block of n2 = 0
  const bool nvalid[2] = {(cb0 + 0) < CB_out, (cb0 + 1) < CB_out};
  // Addresses = wave-uniform base (frame, channel block n2) + a 32-bit per-lane byte offset: global accesses with an SGPR
  // base, no 64-bit vector address arithmetic, no address registers kept across the main loop.
  const unsigned gm_b = (unsigned)(2 * a.W) * 64u;   // + m * gm_b: two image rows further down (bytes)
  // instruction j = 0 / 1 of a pair carries the 64-byte rows of the pixels held by lanes (l31 & 15) + 16 j; this lane supplies
  // (receives) bytes 32 (l31 >> 4) + 16 hi .. + 15 of them
  unsigned svoff[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
    svoff[j] = (unsigned)(((ty0 + wm * 8 + sub_row((l31 & 15) + 16 * j)) * a.W + tx0 + (l31 & 15)) * 32 + 16 * (l31 >> 4) + 8 * hi) * 2u;
  size_t cbase[2];                                  // element offset of channel block n2 of this frame
#pragma unroll
  for (int n2 = 0; n2 < 2; ++n2) cbase[n2] = (size_t)(f * CB_out + (nvalid[n2] ? cb0 + n2 : 0)) * HW * 32;
  // The skip connection of mode 3 does NOT go that way: an 8-byte load per (subtile, channel block, group) puts the lane's own 4 channels where
  // the add needs them, without lane exchanges (43 cycles of latency each, half the issue rate of a plain instruction: tools/ubench/permlane.hip).
  u32x2 rq[4][2][4];                                // residual [subtile m][n2][group g]
  const unsigned nvoff = (unsigned)(((ty0 + wm * 8 + sub_row(l31)) * a.W + tx0 + (l31 & 15)) * 32 + 4 * hi) * 2u;
  // ---- main loop (the schedule is the CONV_STEP macro above) ----
  op16x8 fa[2][4], fb[2][2];   // two fragment register sets
  const op16_t* resp = a.res;
  if (TRACE && tid == 0) t_trace[1] = wall_clock64();
  if (CONV_ABLATE != 2) {
    FB_LD(0, 0, 0, 0); FA_LD(0, 0, 0, 0); FB_LD(0, 0, 1, 0); FA_LD(0, 0, 0, 1); FA_LD(0, 0, 0, 2); FA_LD(0, 0, 0, 3);
    SB();
    if (NCB > 1) {   // first channel block peeled: its first eight MFMAs take C = 0 instead of 128 zeroed registers
      CONV_STEP(0, 0, 1, true, false, false, false, true);
      CONV_STEP(0, 1, 2, false, false, false, false, false);
      CONV_STEP(0, 2, 0, false, true, false, false, false);
    } else {
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
    }
    for (int cb = 1; cb + 1 < NCB; ++cb) {
      CONV_STEP(cb, 0, 1, true, false, false, false, false);
      CONV_STEP(cb, 1, 2, false, false, false, false, false);
      CONV_STEP(cb, 2, 0, false, true, false, false, false);
    }
    // last channel block: no further halo -> kernel row 0 requests the residual of the first two subtiles instead (mode 3).  Row 1's barrier forces it
    // home, 56 MFMAs later; requesting it in row 1 was measured and bought nothing on the step (profiles/r04_experiments.md section 15).
    CONV_STEP(NCB - 1, 0, 1, false, false, true, false, false);
    CONV_STEP(NCB - 1, 1, 2, false, false, false, false, false);
    CONV_STEP(NCB - 1, 2, 0, false, false, false, true, false);
  } else {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
    __syncthreads();
  }

  // ---------------- epilogue ----------------
  if (TRACE && tid == 0) t_trace[2] = wall_clock64();
  if (CONV_ABLATE == 1) {  // profiling: keep the accumulators live, skip the epilogue
    float t = 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) t += acc[m][n][r];
    if (t == 12345.678f) a.y[0] = (vpt_op16)t;
    return;
  }
  if (HAS_RES && CONV_ABLATE == 2) { LOAD_RES(0); LOAD_RES(1); }
  SB();

  f32x2 s_sum2 = {0.f, 0.f}, s_sq2 = {0.f, 0.f};   // packed fp32 (v_pk_add_f32 / v_pk_fma_f32): two values per VALU issue
  // The epilogue body is instantiated for NV = 2 and NV = 1 valid 32-channel blocks of this wave (Cout / 32 odd) and selected by one
  // uniform branch: with no control flow inside, the waits on the prefetched table / residual pieces stay counted.
  // ---- dgrad epilogue (32x32 accumulators, lane-swap layout: see "epilogue addressing" above):  dy = acc + c0 + c1 * xin (+ skip connection, mode 3;
  // gated and scaled for conv0, mode 6) ----
  auto epilogue = [&](auto nv_) __attribute__((always_inline)) {
  constexpr int NV = decltype(nv_)::value;
  const int row_l = sub_row(l31); (void)row_l;   // unused, and it stays: without this evaluation inside the lambda the dgrad kernels' prologue instructions come out in another order
  u32x4 xq[2][2][2];          // the forward layer's input, [parity of m][n2][pair], one subtile ahead
  u32x4 outv[4][2][2];        // packed results: ALL stores are issued after the last load has been consumed.  gfx950 has one
                              // counter (vmcnt) for loads and stores, which may retire out of order relative to each other, so a
                              // wait for a load issued among stores degenerates to vmcnt(0) = "every store has reached L2" --
                              // the round-2 trace showed the first subtile waiting 4-14 us that way.
  LOAD_XIN(0);
  SB();
  const f32x2 c0f2 = {c0f, c0f}, c1f2 = {c1f, c1f}, rgate2 = {rgate, rgate};

#pragma unroll
  for (int m = 0; m < 4; ++m) {
    if (HAS_RES && m < 2) LOAD_RES(m + 2);   // rolling prefetch, two subtiles ahead (0 / 1 were requested during the last channel block)
    if (m < 3) LOAD_XIN(m + 1);   // next subtile's xin: in flight while this one is processed
    SB();
#pragma unroll
    for (int n2 = 0; n2 < 2; ++n2) {
      if (n2 >= NV) continue;
      u32x4 ovp[2], xp[2];
      // xin arrives as whole pixel rows: the same exchanges as for the stores, run backwards
      ROWS_TO_PIECES(xq[m & 1][n2], xp);
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        u32x2 r2[2] = {{0u, 0u}, {0u, 0u}}, x2[2], pk[2];
        if (HAS_RES) { r2[0] = rq[m][n2][2 * p]; r2[1] = rq[m][n2][2 * p + 1]; }
        UNSWAP(xp[p], x2[0], x2[1]);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int g = 2 * p + q;
          f32x2 v01 = {acc[m][n2][4 * g + 0], acc[m][n2][4 * g + 1]}, v23 = {acc[m][n2][4 * g + 2], acc[m][n2][4 * g + 3]};
          {  // + d(mu, rstd)/dx terms of the GroupNorm statistics (c0 + c1 * xin)
            const f32x2 x01 = {op16_lo_to_f32(x2[q].x), op16_hi_to_f32(x2[q].x)}, x23 = {op16_lo_to_f32(x2[q].y), op16_hi_to_f32(x2[q].y)};
            if (GATE) {
              v01 = rgate2 * v01 + (c1f2 * x01 + c0f2);     // rstd0 * dy  (c0, c1 carry rstd0 already)
              v23 = rgate2 * v23 + (c1f2 * x23 + c0f2);
              s_sum2 = v01 * x01 + s_sum2;                  // sum rstd0 dy xin: where the gate is closed xin = 0 contributes nothing
              s_sq2 = v23 * x23 + s_sq2;
              v01.x = x01.x > 0.f ? v01.x : 0.f; v01.y = x01.y > 0.f ? v01.y : 0.f;
              v23.x = x23.x > 0.f ? v23.x : 0.f; v23.y = x23.y > 0.f ? v23.y : 0.f;
            } else {
              v01 += c1f2 * x01 + c0f2;
              v23 += c1f2 * x23 + c0f2;
            }
          }
          if (HAS_RES) {
            const f32x2 r01 = {op16_lo_to_f32(r2[q].x), op16_hi_to_f32(r2[q].x)}, r23 = {op16_lo_to_f32(r2[q].y), op16_hi_to_f32(r2[q].y)};
            v01 += r01;   // mode 3: the block's skip connection
            v23 += r23;
          }
          pk[q].x = pack_op16x2(v01.x, v01.y);
          pk[q].y = pack_op16x2(v23.x, v23.y);
        }
        // back to 16 contiguous bytes per lane (the swap is an involution) and out
        const auto o0 = __builtin_amdgcn_permlane32_swap(pk[0].x, pk[1].x, false, false);
        const auto o1 = __builtin_amdgcn_permlane32_swap(pk[0].y, pk[1].y, false, false);
        ovp[p] = u32x4{o0[0], o1[0], o0[1], o1[1]};
      }
      // One more exchange, between lanes l and l ^ 16 (v_permlane16_swap), so that each store instruction writes all 64 bytes of
      // 16 pixels -- whole 128-byte lines -- instead of one 32-byte half of 32 pixels' rows (every line was then written by two
      // instructions: twice the write requests on the CU's path to L2).
      {
        u32x4 oa, ob;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const auto sw = __builtin_amdgcn_permlane16_swap(ovp[0][j], ovp[1][j], false, false);
          oa[j] = sw[0]; ob[j] = sw[1];
        }
        if (DEFER_STORES) { outv[m][n2][0] = oa; outv[m][n2][1] = ob; }
        else {
          *(u32x4*)((char*)(a.y + cbase[n2]) + (svoff[0] + (unsigned)m * gm_b)) = oa;
          *(u32x4*)((char*)(a.y + cbase[n2]) + (svoff[1] + (unsigned)m * gm_b)) = ob;
        }
      }
    }
  }
  if (DEFER_STORES)
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n2 = 0; n2 < NV; ++n2) {
#pragma unroll
      for (int p = 0; p < 2; ++p)
        *(u32x4*)((char*)(a.y + cbase[n2]) + (svoff[p] + (unsigned)m * gm_b)) = outv[m][n2][p];
    }
  };
  // An opaque copy of the lane id, unused -- like row_l above it stays: the kernel this one was split from made one here for its forward epilogue, and
  // with it the compiler emits the dgrad kernels instruction for instruction as before (tools/isa_diff.py, profiles/conv3x3_split.md).  Without it the
  // register allocation is renumbered, the code outside the main loop comes out in another order and mode 3's loop loses two s_nop.
  int lane_l = lane;
  asm volatile("" : "+v"(lane_l));
  if (nvalid[1]) epilogue(std::integral_constant<int, 2>{});
  else if (nvalid[0]) epilogue(std::integral_constant<int, 1>{});
#undef WRITE_HALO
#undef MM
#undef MMZ
#undef FA_LD
#undef FB_LD
#undef GROUP_
#undef GROUP
#undef GROUP_Z
#undef GROUP_TAIL
#undef EPI_LD
#undef EPI_LDN
#undef LOAD_RES
#undef XR
#undef CONV_STEP
#undef LOAD_XIN
#undef ROWS_TO_PIECES
#undef UNSWAP
  float s_sum = s_sum2.x + s_sum2.y, s_sq = s_sq2.x + s_sq2.y;
  if (GATE) {      // one fp64 atomic per tile: this tile's share of sum rstd0 dy xin
    float* red = (float*)(smem + KK_O + KK_BYTES);
    s_sum = wave_sum(s_sum + s_sq);
    if (lane == 0) red[w] = s_sum;
    __syncthreads();
    if (tid == 0) atomicAdd(a.gate_u + f, (double)((red[0] + red[1]) + (red[2] + red[3])));
  }
  if (TRACE && tid == 0) {
    long long* t = a.trace + (size_t)blockIdx.x * 12;
    t[0] = t_trace[0]; t[1] = t_trace[1]; t[2] = t_trace[2]; t[3] = wall_clock64(); t[4] = cu_key; t[5] = 0;
    for (int k = 0; k < 5; ++k) t[6 + k] = 0;   // (slots of the former per-subtile stamps: they perturbed the epilogue's waits)
  }
}

// Called by vpt_conv3x3_launch (vpt_conv3x3.hip) with validated arguments; mode 2, 3 or 6, a->trace set: the tracing instantiation (modes 2, 3).
void vpt_conv3x3_dgrad_launch(const VptConv3x3Args* a, int mode, long grid, int extra_lds, hipStream_t stream) {
#define LAUNCH_(T_, M_) hipLaunchKernelGGL((vpt_conv3x3_dgrad_kernel<T_, M_>), dim3((unsigned)grid), dim3(256), extra_lds, stream, *a)
  if (mode == 6) LAUNCH_(false, 6);
  else if (a->trace) { if (mode == 2) LAUNCH_(true, 2); else LAUNCH_(true, 3); }
  else { if (mode == 2) LAUNCH_(false, 2); else LAUNCH_(false, 3); }
#undef LAUNCH_
}
