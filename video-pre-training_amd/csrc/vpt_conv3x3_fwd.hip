// 3x3 / pad-1 convolution of the IMPALA residual CNN, forward: vpt_conv3x3_kernel (modes 0, 1, 4, 5, 7) and the pool-fused modes' seam pass.
// Layout, GroupNorm fold, tile, LDS plan and what it shares with the dgrad kernel (vpt_conv3x3_dgrad.hip): vpt_conv3x3_tile.h.
// Halo DMA (template parameter HDMA: modes 0, 1, 4, 5 with 16-row tiles on an even count of 32-channel blocks -- what the launch function picks
//   wherever it can; the plan of vpt_conv3x3_tile.h stays for every other case and is the bitwise reference of tests/test_gpu_conv_halo_dma.py):
//   - LDS plan: [ring of four 8 KB one-tap weight slots 32 768][two dense, swizzled halo images of 324 pixels x 64 bytes 41 472][table, statistics,
//     residual bias 5 184] = 79 424 bytes; the pool-fused mode's 69 632-byte output tile still fits below the table.
//   - the halo of the NEXT channel block goes global -> LDS by buffer loads (21 pieces of 1 KB; out-of-image chunks carry an offset beyond the
//     resource and arrive as zeros) into the image the current block does not read: no staging registers, no zero-fill selects, no ds_write and
//     no second barrier per channel block.
//   - K step = TWO taps (64 MFMAs per wave) of the global tap index t = 9 cb + 3 dy + dx, one barrier each; behind the barrier the pieces of taps
//     t + 2 and t + 3 go into the slots of taps t - 2 and t - 1.  The loop body is two channel blocks; its vector-memory operations are counted.
//   K order, accumulators, epilogue: unchanged, so every output bit is.  profiles/conv3x3_halo_dma.md has the measurements.
// Forward modes (0, 1, 4, 5, 7): v_mfma_f32_16x16x32 main loop (8 pixel rows x 4 cout groups of 16x16 accumulators per wave), epilogue
//   in the accumulators' own layout -- 16-byte loads and stores per lane, no lane exchange.  Halo records of odd pixels are shifted by
//   16 bytes so that fragment reads and halo writes are bank-conflict-free (see "Main loop" in the kernel).
#include "vpt_conv3x3_tile.h"
#include <type_traits>
#ifndef VPT_EPI_NO_CLAMP_RELU
#define VPT_EPI_NO_CLAMP_RELU 0   // A/B builds: 1 = residual modes with the fp32 v_max ReLU of rounds 1-4 (bit-identical outputs)
#endif
// Timing-only ablations of the FORWARD main loop (wrong results; -DVPT_CONV_PROFILE builds only, chosen at compile time so that the unablated
// loop carries no branch): -DVPT_CONV_FWD_ABLATE=1 no weight DMA inside the loop (stale weights), 2 no halo reloads (block 0's halo serves every
// channel block), 4 both (MFMAs, fragment reads, waits and barriers only).  profiles/conv3x3_cycles.md has the table they gave.  In the halo-DMA
// instantiations the same switches drop the in-loop weight pieces (HWP: all four ring slots are filled once, in the prologue) and the in-loop halo
// pieces (HXP: both images are filled once, with blocks 0 and 1); the counted waits then find fewer operations in flight and return at once.
#if defined(VPT_CONV_PROFILE) && defined(VPT_CONV_FWD_ABLATE)
#define FWD_NO_DMA (VPT_CONV_FWD_ABLATE == 1 || VPT_CONV_FWD_ABLATE == 4)
#define FWD_NO_HALO (VPT_CONV_FWD_ABLATE == 2 || VPT_CONV_FWD_ABLATE == 4)
#else
#define FWD_NO_DMA 0
#define FWD_NO_HALO 0
#endif
// Template parameters of vpt_conv3x3_kernel:
// TRACE (tools/conv_trace.py): phase timestamps.  Compile time because s_memrealtime is a scalar-memory operation: one of them
// in flight makes lgkmcnt out of order and every LDS wait of the epilogue degenerates to lgkmcnt(0).
// MODE (compile time, so the epilogue carries no runtime branches): 0 forward, 1 forward + residual,
// (2, 3, 6: the dgrad kernel's, vpt_conv3x3_dgrad.hip), 4 forward + the stack's 3x3 / stride-2 max-pool (CnnDownStack.forward,
// lib/impala_cnn.py:114-117: firstconv -> max_pool2d): the 16 x 16 output tile goes to LDS instead of HBM, its 8 x 8 pooled pixels are
// written -- complete where the 3 x 3 window lies inside the tile, the in-tile part of the maximum on the tile's first pooled row /
// column otherwise -- together with the tile's last row and column (the "seams"); vpt_pool_seam_kernel finishes the seam pixels.
// The pre-pool tensor (2 MB per frame in stack 1) never reaches HBM.  Modes 5, 7: see the kernel's first lines.
// TR (compile time, forward modes): pixel rows of the workgroup's tile.  16: four waves, two workgroups per CU.
// 32: EIGHT waves (4 row groups x 2 channel halves) on a 32 x 16-pixel tile, one workgroup per CU -- the same waves per SIMD, the same
// per-wave program, but the step's 24 KB weight tile is fetched ONCE for 512 pixels instead of once per co-resident workgroup: half
// the weight DMA and 11 % less halo (34 x 18 instead of 2 x 18 x 18 pixels).  Measured at parity (see the launch function).
//
// Forward accumulators: the four 16x16 accumulators (cout groups u) of one pixel row live in ONE 16-register tuple, so the register allocator
// places them like the 32x32 accumulators (whole aligned blocks, no fragmentation between 4-register tuples)
template <int U> __device__ __forceinline__ f32x4 ac_get(const f32x16& v) {
  return __builtin_shufflevector(v, v, 4 * U, 4 * U + 1, 4 * U + 2, 4 * U + 3);
}
template <int U> __device__ __forceinline__ void ac_set(f32x16& v, const f32x4 c) {
  const f32x16 w = __builtin_shufflevector(c, c, 0, 1, 2, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1);
  if constexpr (U == 0) v = __builtin_shufflevector(v, w, 16, 17, 18, 19, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
  else if constexpr (U == 1) v = __builtin_shufflevector(v, w, 0, 1, 2, 3, 16, 17, 18, 19, 8, 9, 10, 11, 12, 13, 14, 15);
  else if constexpr (U == 2) v = __builtin_shufflevector(v, w, 0, 1, 2, 3, 4, 5, 6, 7, 16, 17, 18, 19, 12, 13, 14, 15);
  else v = __builtin_shufflevector(v, w, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19);
}

template <bool TRACE, int MODE, int TR = 16, bool HDMA = false>
__global__ __launch_bounds__(TR * 16, 2) void vpt_conv3x3_kernel(VptConv3x3Args a) {
  static_assert(TR == 16 || TR == 32, "tile rows");
  static_assert(MODE == 0 || MODE == 1 || MODE == 4 || MODE == 5 || MODE == 7, "forward modes");
  static_assert(!HDMA || (TR == 16 && !TRACE && (MODE == 0 || MODE == 1 || MODE == 4 || MODE == 5)), "halo DMA: the 16-row forward modes but the arg-max one");
  static_assert(!HDMA || 256 * PT_RS <= H_RING + 2 * H_BUF, "the pooled mode's output tile must fit below the epilogue table");
  constexpr int NWAVE = TR / 4, NTHR = 64 * NWAVE;
  constexpr int HPIX = (TR + 2) * 18;                            // halo pixels
  constexpr int NA = (HPIX * 4 + NTHR - 1) / NTHR;               // 16-byte halo chunks per thread and channel block: 6 / 5
  constexpr int NDMA = 24 / NWAVE;                               // 1 KB weight-DMA pieces per wave and step: 6 / 3
  constexpr int A_SZ = HPIX * A_RS, KK_O = HDMA ? H_RING + 2 * H_BUF : A_SZ + 2 * B_BYTES, BT_O = KK_O + KK_BYTES + 64, SMEM_SZ = BT_O + 512;
  static_assert(TR != 16 || HDMA || (A_SZ == A_BYTES && KK_O == KK_OFF && SMEM_SZ <= SMEM_BYTES), "16-row layout");
  static_assert(!HDMA || (SMEM_SZ == 79424 && 2 * SMEM_SZ <= 163840), "halo-DMA layout: two workgroups per CU");
  static_assert((MODE != 4 && MODE != 7) || TR == 16, "the pool-fused epilogue is written for 16 x 16 tiles");
  // 5 forward + residual through a per-frame affine:  out = relu(...) + res_scale[f] * res + res_bias[f][channel]  -- the block that
  // follows a stack's GroupNorm `n` reads the pooled tensor itself (already multiplied by n's gain) instead of a normalised copy
  // (lib/impala_cnn.py:118-121 with the `n` pass folded away).
  // 7 = mode 4 for the TRAINING forward (round 5): the pooled tensor plus, per pooled value, which window positions hold the maximum -- a 9-bit
  // "differs from the maximum" mask per 16-bit lane (bit 8 - k for scan position k = 3 (dy + 1) + (dx + 1); positions outside the tile or the
  // image: 1), pool_mask [F][Cout/32][H/2][W/2][32] uint16.  The backward routes the pooled gradient to the FIRST zero bit (torch's tie rule)
  // and needs neither the pre-pool tensor nor vpt_pool_kernel (vpt_conv_bwd_prep_pooled_kernel).  Measured cost of the masks: +5 % of the
  // K = 1152 pool-fused launch, +2.5 % of the K = 2304 one (profiles/r05_experiments.md).
  constexpr bool PMASK = MODE == 7;
  constexpr bool PACKED_RELU = MODE == 0;    // forward without residual: ReLU + statistics on the packed 16-bit pairs (see the epilogue)
  // Forward WITH residual (modes 1, 5): the ReLU must precede the residual add in fp32, and gfx950 has no packed fp32 maximum -- but every VALU
  // instruction has a clamp-to-[0, 1] result modifier.  The epilogue's affine step runs SCALED by 2^-40 (rstd and the constant table carry the
  // factor: exact, a power of two commutes with the rounding of the FMA) with the clamp set, which is 2^-40 * ReLU for every value below 2^40, and
  // the residual add that follows is an FMA with 2^40 -- exact product, ONE rounding, bit for bit `ReLU(v) + r`: two packed instructions per value
  // pair where there were a packed FMA, two v_max_f32 and a packed add (192 of the mode's 1121 vector instructions per wave and tile).  Outside
  // [2^-86, 2^40] the result would differ from an unscaled ReLU (denormal / saturated): no GroupNorm-fed convolution output lives there.
  constexpr bool CLAMP_RELU = (MODE == 1 || MODE == 5) && !VPT_EPI_NO_CLAMP_RELU;
  constexpr float RELU_S = CLAMP_RELU ? 0x1p-40f : 1.f, RELU_INV = 0x1p40f;
  constexpr bool HAS_RES = (MODE == 1 || MODE == 5), POOL = (MODE == 4 || MODE == 7), RES_AFF = MODE == 5;
  // Main loop on v_mfma_f32_16x16x32.  Wave tile 8 pixel rows x 64 couts = 8 x 4 accumulators of 16 pixels x 16 couts;
  // weights are the A operand, pixels the B operand, one ds_read_b128 per fragment carries the whole K = 32 of a tap.
  //   - halo image: the 64-byte record of halo pixel P starts at 80 P + 16 (P & 1) -- odd pixels use the pitch's pad chunk in FRONT -- and MFMA
  //     column c holds pixel pcol(c) of the row: the even pixels on lanes {0-3, 12-15}, the odd ones on {4-11}.  The hardware serves a
  //     ds_read_b128 in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ...: lanes that read chunk q of even (odd) pixels together
  //     with lanes that read chunk q + 1 of odd (even) pixels.  16-byte slot mod 16 = 5 P + q + (P & 1): the even pixels of 16 consecutive
  //     ones give the 8 even (odd) slots, the odd pixels the other 8, for every tap offset dx -- conflict-free.  (With the plain 80 P image
  //     three of the sixteen slots of every group are hit twice.)
  //   - weight fragment of cout group u = 2 blk + b: MFMA row r <-> cout 32 blk + 8 (r >> 2) + 4 b + (r & 3), so the two accumulators of a
  //     32-cout block give lane (c, q) couts 8 q .. 8 q + 7: 16 contiguous bytes of its pixel's record.  Under the packed image's swizzle
  //     ((cout >> 2) & 3) the four rows of one bank class (r & 3) read chunk positions q0 ^ s, (q0 + 1) ^ (s + 2), (q0 + 1) ^ s, q0 ^ (s + 2)
  //     (s = b) in a hardware lane group: all four, conflict-free, the swizzle stays as it is.
  __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM_SZ];
  const int tid = threadIdx.x, lane = tid & 63;
  // profiling (vpt_conv3x3_set_trace): CU id + 100 MHz timestamps of the tile's phases
  int cu_key = -1;
  long long t_trace[3];
  if (TRACE) {   // (wave-uniform, so the stamps stay in scalar registers across the main loop)
    t_trace[0] = wall_clock64();
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID: cu_id[11:8] sh_id[12] se_id[15:13]
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);   // HW_REG_XCC_ID[3:0]
    cu_key = (int)(((xcc & 15u) << 8) | ((hw >> 8) & 0xffu));
  }
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int tilesX = a.W >> 4, tilesY = a.H / TR;
  const VptConvTile tile = conv_tile_decode(a.NT, tilesX, tilesY);
  const int nt = tile.nt, tx = tile.tx, ty = tile.ty, f = tile.f;
  const int tx0 = tx * 16, ty0 = ty * TR;
  const int NCB = a.Cin >> 5;
  const int HW = a.H * a.W;

  // ---- halo staging map of the register-staged instantiations ----
  int a_loff[NA];            // LDS byte offset, -1: no chunk (beyond the 324 halo pixels)
  unsigned a_gbyte[NA];      // byte offset inside one channel-block plane (clamped to 0 outside the image)
  unsigned a_inside = 0;    // bit m: chunk m lies inside the image (else literal zeros: the conv pads the NORMALISED tensor)
#pragma unroll
  for (int m = 0; m < NA; ++m) {
    const int q = tid + NTHR * m;
    // the 8 lanes of a ds_write_b128 group carry 4 pixels of one parity x 2 parts (slots 2 k + part + const mod 8: all eight)
    const int P = ((q >> 5) << 3) + 2 * (q & 3) + ((q >> 4) & 1);
    const int part = 2 * ((q >> 3) & 1) + ((q >> 2) & 1);
    a_loff[m] = -1;
    a_gbyte[m] = 0u;
    if (P < HPIX) {
      const int hy = P / 18, hx = P - hy * 18;
      const int y = ty0 - 1 + hy, x = tx0 - 1 + hx;
      a_loff[m] = P * A_RS + part * 16 + 16 * (P & 1);
      if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
        a_gbyte[m] = (unsigned)((y * a.W + x) * 32 + part * 8) * 2u;
        a_inside |= 1u << m;
      }
    }
  }
  const op16_t* xplane = a.x + (size_t)f * NCB * HW * 32;
  // chunk m of a thread lies NTHR / 4 halo pixels behind chunk m - 1 (same parity, same part): ONE address register and constant
  // offsets; only the last chunk can fall beyond the halo
  constexpr int H16_STR = (NTHR / 4) * A_RS;
  static_assert(((NA - 2) * NTHR + NTHR - 1) / 32 * 8 + 7 < HPIX, "all chunks but a thread's last are inside the halo");
  const int a_l0 = a_loff[0];
  const bool a_lastok = a_loff[NA - 1] >= 0;
  // weight DMA: wave w moves pieces (NWAVE*m + w), m = 0..NDMA-1, of the 24 KB step tile; lane = 16-byte chunk
  const op16_t* wbase = a.wpk + (size_t)nt * NCB * 9 * 4096 + (size_t)(w * 64 + lane) * 8;
  unsigned char* bdst = smem + A_SZ + w * 1024;
  // HDMA (forward modes 0, 1, 4, 5 on an even channel-block count): the halo is no longer register-staged.  Two DENSE halo images (64 bytes per
  // pixel) are filled alternately by buffer loads to LDS -- no staging registers, no zero-fill selects, no ds_write, no second barrier -- and
  // the weight double buffer is a ring of four one-tap slots.  Schedule: HSTEP below.
  //   - image: the 16-byte slot 4 P + (q ^ ((hx >> 2) & 3)) holds chunk q of halo pixel P = 18 hy + hx.  The swizzle is a function of the
  //     COLUMN only, so a fragment read is one of three per-lane bases (tap column dx) + an immediate (row, buffer).  A hardware
  //     ds_read_b128 group reads 16 consecutive pixels of one halo row, chunk q of one pixel parity and q + 1 of the other: slot mod 16 =
  //     4 (P & 3) + (q' ^ ((hx >> 2) & 3)); the four pixels of a class P & 3 share q' and are 4 columns apart, so (hx >> 2) & 3 separates
  //     them -- 16 distinct slots for every tap offset.
  //   - fill: 21 pieces of 1 KB (64 lanes x 16 bytes, destination contiguous, source per lane).  Wave w moves pieces 4 n + w, n = 0..4; the
  //     last 1 KB of the image (n = 5: it overlaps piece 19, so no lane points beyond pixel 323) is written by every wave with the same data,
  //     which keeps the number of vector-memory operations per wave fixed.  A chunk outside the image carries the offset H_OOB, beyond the
  //     frame's resource: the range check delivers zeros (tests/test_gpu_conv_halo_dma.py: NaN surround).
  unsigned hv[6] = {0u, 0u, 0u, 0u, 0u, 0u};       // per-lane source offset of the wave's six pieces inside one channel-block plane
  if constexpr (HDMA) {
#pragma unroll
    for (int n = 0; n < 6; ++n) {
      const int s = (n < 5 ? (4 * n + w) * 64 : (H_BUF - 1024) / 16) + lane;
      const int P = s >> 2, hy = P / 18, hx = P - 18 * hy;
      const int q = (s & 3) ^ ((hx >> 2) & 3);
      const int y = ty0 - 1 + hy, x = tx0 - 1 + hx;
      hv[n] = (y >= 0 && y < a.H && x >= 0 && x < a.W) ? (unsigned)((y * a.W + x) * 64 + q * 16) : H_OOB;
    }
  }
  // resources (scalar registers): this channel tile's packed weights, this frame's input planes -- exact sizes.  The *_n copies of the loop have
  // num_records 0 in the last pass: what the schedule requests beyond the last channel block touches no memory and arrives as zeros.
  const unsigned h_wbytes = (unsigned)NCB * 9u * (unsigned)H_SLOT, h_xbytes = (unsigned)NCB * (unsigned)HW * 64u;
  const op16_t* const h_wptr = a.wpk + (size_t)nt * NCB * 9 * 4096;
  const __amdgpu_buffer_rsrc_t hwrs = __builtin_amdgcn_make_buffer_rsrc((void*)h_wptr, 0, HDMA ? h_wbytes : 0u, 0x00020000);
  const __amdgpu_buffer_rsrc_t hxrs = __builtin_amdgcn_make_buffer_rsrc((void*)xplane, 0, HDMA ? h_xbytes : 0u, 0x00020000);
  const int h_wvoff = (w * 64 + lane) * 16;
  unsigned char* const rdst = smem + w * 1024;     // ring slot s, piece 4 m + w: rdst + s * H_SLOT + m * 4096
  int h_wso = 0, h_rpi = 0;                        // loop-carried: byte offset of the pass's first tap in the packed weights; 16384 in odd passes

  // ====================================================================================================================
  // (All macros of the kernel -- these and the shared ones of vpt_conv3x3_tile.h -- expand where they are used, so the names they mention are
  // declared further down; the kernel's own are undefined together behind the epilogue dispatch.)
  // Macros of the FORWARD loop (modes 0, 1, 4, 5, 7): v_mfma_f32_16x16x32, wave tile 8 pixel rows x 4 cout groups = ac[8], epilogue in the
  // accumulators' own layout.  One K step = 3 taps x 4 cout groups x 8 pixel rows = 96 MFMAs per wave, in 12 groups of 8 (one cout group
  // over the 8 pixel rows).  Registers: the 8 pixel fragments of the CURRENT tap (32) + a double-buffered weight fragment (8) = 40.  A group
  // requests the weight fragment of the next group behind its first MFMA; the tap's last group also refills each pixel fragment for the next
  // tap right behind the MFMA that used it last.  Vector-memory operations keep the order and count of the dgrad loop (weight DMA, then halo /
  // residual), one slot per group; the step's barrier sits in front of its LAST group, which holds every fragment it needs and requests the
  // next step's first ones behind the barrier.
  // ====================================================================================================================
  // Weight DMA piece of the forward loop: a BUFFER load to LDS (resource wrs over this channel tile's packed weights, the lane's 32-bit offset,
  // step and piece in the scalar offset).  global_load_lds is a FLAT-encoded operation that the compiler's wait-count model books as a possible
  // LDS access with out-of-order return: behind each piece every fragment wait of the loop degenerated to lgkmcnt(0), so the first MFMA of a
  // group also waited for the fragment requested one instruction earlier, and each piece carried two 64-bit vector adds for its address.  The
  // buffer form is counted in vmcnt alone: the loop's fragment waits stay COUNTED (lgkmcnt(7) .. (1)) and a piece costs scalar adds only.
#define GLDS16(m_)                                                                                        \
  do { if (POOL) { if (!FWD_NO_DMA) GLDS(m_); } else if ((m_) < NDMA && !FWD_NO_DMA)                      \
  __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (__attribute__((address_space(3))) void*)(bd_ + (m_) * (NWAVE * 1024)), 16, wvoff, \
                                           (s_ + 1) * B_BYTES + (m_) * (NWAVE * 1024), 0, 0); } while (0)
#define XA16(m_) do { if (!FWD_NO_HALO) XA(m_); } while (0)
#define HALO_WR16(m_) do { if ((m_) < NA - 1 || a_lastok) *(u32x4*)(smem + a_l0 + (m_) * H16_STR) = ((a_inside >> (m_)) & 1u) ? areg[m_] : zero4; } while (0)
#define PA(j_, dy_, dx_) fp[j_] = *(const __attribute__((address_space(3))) op16x8*)((((dx_) & 1) ? aLo : aLe) + (((j_) + (dy_)) * 18 + (dx_)) * A_RS)
#define WB(tap_, u_, boff_) fw[(u_) & 1] = *(const __attribute__((address_space(3))) op16x8*)((((u_) & 1) ? bW1 : bW0) + (boff_) + (tap_) * (128 * 64) + ((u_) >> 1) * (32 * 64))
#define M16A(j_, u_) ac_set<(u_)>(ac[j_], VPT_MFMA_16X16X32(fw[(u_) & 1], fp[j_], ac_get<(u_)>(ac[j_]), 0, 0, 0))
  // cout group u_ < 3 of a tap: WLD = the next group's weight fragment, X = the group's vector-memory slot
#define G16(MM_, u_, WLD, X)                                                                              \
  do {                                                                                                    \
    MM_(0, u_); WLD; SB();                                                                                \
    MM_(1, u_); SB();                                                                                     \
    MM_(2, u_); SB();                                                                                     \
    MM_(3, u_); X; SB();                                                                                  \
    MM_(4, u_); SB();                                                                                     \
    MM_(5, u_); SB();                                                                                     \
    MM_(6, u_); SB();                                                                                     \
    MM_(7, u_); SB();                                                                                     \
  } while (0)
  // cout group 3: every pixel fragment is refilled for tap (ndy_, ndx_) behind its last use
#define G16R(MM_, WLD, X, ndy_, ndx_)                                                                     \
  do {                                                                                                    \
    MM_(0, 3); SB(); WLD; PA(0, ndy_, ndx_); SB();                                                              \
    MM_(1, 3); SB(); PA(1, ndy_, ndx_); SB();                                                                   \
    MM_(2, 3); SB(); PA(2, ndy_, ndx_); SB();                                                                   \
    MM_(3, 3); SB(); PA(3, ndy_, ndx_); X; SB();                                                                \
    MM_(4, 3); SB(); PA(4, ndy_, ndx_); SB();                                                                   \
    MM_(5, 3); SB(); PA(5, ndy_, ndx_); SB();                                                                   \
    MM_(6, 3); SB(); PA(6, ndy_, ndx_); SB();                                                                   \
    MM_(7, 3); SB(); PA(7, ndy_, ndx_); SB();                                                                   \
  } while (0)
#define TAP16(MM_, dy_, dx_, X0, X1, X2, X3)                                                              \
  do {                                                                                                    \
    G16(MM_, 0, WB(dx_, 1, boff_), X0);                                                                   \
    G16(MM_, 1, WB(dx_, 2, boff_), X1);                                                                   \
    G16(MM_, 2, WB(dx_, 3, boff_), X2);                                                                   \
    G16R(MM_, WB((dx_) + 1, 0, boff_), X3, dy_, (dx_) + 1);                                               \
  } while (0)
  // residual row j_ x 2 channel blocks: XR16 inside the main loop, XR16L (addresses re-derived behind the loop, see voff16_l) in the epilogue
#define EPI_LD16(ptr_, j_, n2_) (*(const u32x4*)((const char*)((ptr_) + cbase[n2_]) + (voff16 + (unsigned)(j_) * gj_b)))
#define XR16(j_) do { rq16[j_][0] = EPI_LD16(resp, j_, 0); rq16[j_][1] = EPI_LD16(resp, j_, 1); } while (0)
#define XR16L(j_) do { rq16[j_][0] = *(const u32x4*)((const char*)(resp + cbase[0]) + (voff16_l + (unsigned)(j_) * gj_b)); rq16[j_][1] = *(const u32x4*)((const char*)(resp + cbase[1]) + (voff16_l + (unsigned)(j_) * gj_b)); } while (0)
#define CONV_STEP16(cb_, dy_, NEXT_DY, PRE_A, WR_A, PRE_R, LAST)                                          \
  do {                                                                                                    \
    const int s_ = (cb_) * 3 + (dy_);                                                                     \
    const int boff_ = (s_ & 1) * B_BYTES, noff_ = B_BYTES - boff_;                                        \
    const op16_t* wp_ = wbase + (size_t)(s_ + 1) * 12288;     /* (the pool-fused modes' global_load_lds) */ \
    unsigned char* bd_ = bdst + noff_;                                                                    \
    const unsigned cbo_ = (unsigned)((cb_) + 1) * (unsigned)HW * 64u; /* bytes; uniform */                \
    if (LAST) {                                                                                           \
      TAP16(M16A, dy_, 0, NOP_(), NOP_(), NOP_(), NOP_());                                                \
    } else {                                                                                              \
      TAP16(M16A, dy_, 0, GLDS16(0), GLDS16(1), GLDS16(2), GLDS16(3));                                          \
    }                                                                                                     \
    if (PRE_A) {                                                                                          \
      TAP16(M16A, dy_, 1, GLDS16(4), GLDS16(5), do { XA16(0); XA16(1); } while (0), XA16(2));             \
      G16(M16A, 0, WB(2, 1, boff_), do { XA16(3); XA16(4); } while (0));                                  \
      G16(M16A, 1, WB(2, 2, boff_), XA16(5));                                                             \
      G16(M16A, 2, WB(2, 3, boff_), NOP_());                                                              \
      if (NA == 6) WAIT_BARRIER(6); else WAIT_BARRIER(5);                                                 \
    } else if ((PRE_R) && HAS_RES) {                                                                      \
      TAP16(M16A, dy_, 1, GLDS16(4), GLDS16(5), XR16(0), NOP_());                                           \
      G16(M16A, 0, WB(2, 1, boff_), NOP_());                                                              \
      G16(M16A, 1, WB(2, 2, boff_), NOP_());                                                              \
      G16(M16A, 2, WB(2, 3, boff_), NOP_());                                                              \
      WAIT_BARRIER(2);   /* row 0 x 2 blocks */                                                                                      \
    } else {                                                                                              \
      if (LAST) TAP16(M16A, dy_, 1, NOP_(), NOP_(), NOP_(), NOP_());                                      \
      else TAP16(M16A, dy_, 1, GLDS16(4), GLDS16(5), NOP_(), NOP_());                                       \
      G16(M16A, 0, WB(2, 1, boff_), NOP_());                                                              \
      G16(M16A, 1, WB(2, 2, boff_), NOP_());                                                              \
      G16(M16A, 2, WB(2, 3, boff_), NOP_());                                                              \
      WAIT_BARRIER(0);                                                                                    \
    }                                                                                                     \
    if (WR_A) {   /* the halo of the next channel block replaces the current one: second barrier before its first read */ \
      _Pragma("unroll") for (int m_ = 0; m_ < 4; ++m_) {                                                  \
        if (!FWD_NO_HALO) HALO_WR16(m_); SB();                                                            \
        if (m_ + 4 < NA && !FWD_NO_HALO) HALO_WR16(m_ + 4);                                                         \
        SB(); if (m_ == 0) M16A(0, 3); else if (m_ == 1) M16A(1, 3); else if (m_ == 2) M16A(2, 3); else M16A(3, 3); SB();                                                                        \
      }                                                                                                   \
      WAIT_BARRIER(0);                                                                                    \
      WB(0, 0, noff_); PA(0, 0, 0); PA(1, 0, 0); PA(2, 0, 0); PA(3, 0, 0); SB();                          \
      M16A(4, 3); SB(); PA(4, 0, 0); SB();                                                                      \
      M16A(5, 3); SB(); PA(5, 0, 0); SB();                                                                      \
      M16A(6, 3); SB(); PA(6, 0, 0); SB();                                                                      \
      M16A(7, 3); SB(); PA(7, 0, 0); SB();                                                                      \
    } else if (LAST) {                                                                                    \
      M16A(0, 3); M16A(1, 3); M16A(2, 3); M16A(3, 3); M16A(4, 3); M16A(5, 3); M16A(6, 3); M16A(7, 3);                                    \
    } else {                                                                                              \
      G16R(M16A, WB(0, 0, noff_), NOP_(), NEXT_DY, 0);                                                    \
    }                                                                                                     \
  } while (0)
  // ---- HDMA schedule (modes 0, 1, 4, 5; even channel-block count).  K order unchanged: (channel block, kernel row, tap) -- every accumulator sees
  // the MFMA sequence of CONV_STEP16.  One PASS of the loop = two channel blocks = local taps l = 0 .. 17 (block A: 0 .. 8 reads halo image 0,
  // block B: 9 .. 17 image 1); tap l of pass i is global tap t = 18 i + l and lives in ring slot t & 3 = (l + 2 i) & 3: bases bWl* serve the taps
  // with l & 2 == 0, bWh* the others, and both pairs swap slots {0, 1} <-> {2, 3} behind every pass.
  // A STEP is two taps (2 k, 2 k + 1), 64 MFMAs per wave; its barrier sits in front of the LAST group of tap 2 k + 1, where every wave holds that
  // group's fragments in registers and has finished taps 2 k - 1 and 2 k with all their LDS reads.  The counted wait in front of the barrier
  // retires the weights of taps 2 k + 2 and 2 k + 3 (requested behind the previous barrier); behind it the pieces of taps 2 k + 4 and 2 k + 5 go
  // into the slots of taps 2 k and 2 k + 1, one per group.  The groups' other slots carry the next block's halo: image 1 is requested behind the
  // barrier of step 0 (the last reads of image 1 lie in front of the barrier of step 8 of the previous pass) and is counted home at the barrier of
  // step 3, the last one before tap 8's refills read it; image 0 likewise behind the barrier of step 4, home at the barrier of step 8.  Modes 1 / 5
  // request the residual's first row in step 7 of every pass (one instruction, always live; the last pass's value is the one the epilogue uses).
  // Vector-memory operations per wave and pass, in order: see the X arguments of HSTEP in the loop; the n_late_ of a barrier counts those behind
  // the step's last weight piece.
#define HWP(lp_, m_, rs_)                                                                                 \
  do { if (!FWD_NO_DMA) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_, (__attribute__((address_space(3))) void*)(rdst + ((((lp_) & 3) * H_SLOT) ^ h_rpi) + (m_) * 4096), \
                                           16, h_wvoff, h_wso + (lp_) * H_SLOT + (m_) * 4096, 0, 0); } while (0)
#define HXP_(n_, img_, rs_, cbo_)                                                                         \
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_, (__attribute__((address_space(3))) void*)(smem + H_RING + (img_) * H_BUF + ((n_) < 5 ? w * 1024 + (n_) * 4096 : H_BUF - 1024)), \
                                           16, hv[n_], cbo_, 0, 0)
#define HXP(n_, img_, rs_, cbo_) do { if (!FWD_NO_HALO) HXP_(n_, img_, rs_, cbo_); } while (0)
#define HPA(j_, l_) fp[j_] = *(const __attribute__((address_space(3))) op16x8*)(((l_) % 3 == 0 ? aH0 : ((l_) % 3 == 1 ? aH1 : aH2)) + (((l_) % 18) >= 9 ? H_BUF : 0) + ((j_) + ((l_) % 9) / 3) * (18 * 64))
#define HWB(l_, u_) fw[(u_) & 1] = *(const __attribute__((address_space(3))) op16x8*)((((l_) & 2) ? (((u_) & 1) ? bWh1 : bWh0) : (((u_) & 1) ? bWl1 : bWl0)) + ((l_) & 1) * H_SLOT + ((u_) >> 1) * (32 * 64))
#define HG(l_, u_, X) G16(M16A, u_, HWB(l_, (u_) + 1), X)
#define HGR(l_, X)                                                                                        \
  do {                                                                                                    \
    M16A(0, 3); SB(); HWB((l_) + 1, 0); HPA(0, (l_) + 1); SB();                                           \
    M16A(1, 3); SB(); HPA(1, (l_) + 1); SB();                                                             \
    M16A(2, 3); SB(); HPA(2, (l_) + 1); SB();                                                             \
    M16A(3, 3); SB(); HPA(3, (l_) + 1); X; SB();                                                          \
    M16A(4, 3); SB(); HPA(4, (l_) + 1); SB();                                                             \
    M16A(5, 3); SB(); HPA(5, (l_) + 1); SB();                                                             \
    M16A(6, 3); SB(); HPA(6, (l_) + 1); SB();                                                             \
    M16A(7, 3); SB(); HPA(7, (l_) + 1); SB();                                                             \
  } while (0)
  // step k_: X1 .. X3 = the weight pieces left of taps 2 k + 2, 2 k + 3; X4 .. X7 = halo / residual; WAITB; X0N = first piece of tap 2 k + 4
#define HSTEP(k_, X1, X2, X3, X4, X5, X6, X7, WAITB, X0N)                                                 \
  do {                                                                                                    \
    HG(2 * (k_), 0, X1); HG(2 * (k_), 1, X2); HG(2 * (k_), 2, X3); HGR(2 * (k_), X4);                     \
    HG(2 * (k_) + 1, 0, X5); HG(2 * (k_) + 1, 1, X6); HG(2 * (k_) + 1, 2, X7);                            \
    WAITB;                                                                                                \
    HGR(2 * (k_) + 1, X0N);                                                                               \
  } while (0)
  // epilogue: edge class of pixel row j_ (only the wave's first / last row can touch the image border) and the constant-table prefetch
#define EO16(j_) ((j_) == 0 ? eo_top : ((j_) == 7 ? eo_bot : 3 * 128))
#define LOAD_KK16(c_)                                                                                     \
  do {                                                                                                    \
    const float* kp_ = kk16 + EO16((c_) >> 1) + ((c_) & 1) * 32;                                          \
    kq[(c_) & 1][0] = *(const f32x4*)kp_; kq[(c_) & 1][1] = *(const f32x4*)(kp_ + 4);                     \
  } while (0)
  // ====================================================================================================================

  u32x4 areg[NA];
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  // ---- prologue: weights of step 0 (DMA), halo of channel block 0, epilogue constant table ----
  if constexpr (HDMA) {   // taps 0 and 1 into ring slots 0 and 1, channel block 0 into halo image 0: retired by the __syncthreads() below
    if (!FWD_NO_DMA) { HWP(0, 0, hwrs); HWP(0, 1, hwrs); HWP(1, 0, hwrs); HWP(1, 1, hwrs); }
    else { for (int t_ = 0; t_ < 4; ++t_) { __builtin_amdgcn_raw_ptr_buffer_load_lds(hwrs, (__attribute__((address_space(3))) void*)(rdst + t_ * H_SLOT), 16, h_wvoff, t_ * H_SLOT, 0, 0);
                                            __builtin_amdgcn_raw_ptr_buffer_load_lds(hwrs, (__attribute__((address_space(3))) void*)(rdst + t_ * H_SLOT + 4096), 16, h_wvoff, t_ * H_SLOT + 4096, 0, 0); } }
    HXP_(0, 0, hxrs, 0); HXP_(1, 0, hxrs, 0); HXP_(2, 0, hxrs, 0); HXP_(3, 0, hxrs, 0); HXP_(4, 0, hxrs, 0); HXP_(5, 0, hxrs, 0);
    if (FWD_NO_HALO) {   // (timing-only ablation: both images are filled once, here)
      const unsigned cb1_ = (unsigned)HW * 64u;
      HXP_(0, 1, hxrs, cb1_); HXP_(1, 1, hxrs, cb1_); HXP_(2, 1, hxrs, cb1_); HXP_(3, 1, hxrs, cb1_); HXP_(4, 1, hxrs, cb1_); HXP_(5, 1, hxrs, cb1_);
    }
  } else {
  ISSUE_B(0, 0);
#pragma unroll
  for (int m = 0; m < NA; ++m) areg[m] = *(const u32x4*)((const char*)xplane + a_gbyte[m]);
  }
  float mean = 0.f, rstd = 1.f;
  const float* esa = a.edge_sa;
  if (a.kk_frame) {   // the epilogue table of THIS frame was prepared by vpt_nfold_coef_kernel (the input is a pooled tensor whose GroupNorm `n`
    rstd = a.rs_frame[f];                               // is folded into this layer): out = relu(rs * acc + kk_frame[f][e][o])
    esa = a.kk_frame + (size_t)f * 9 * a.CoutPad;
  } else {
    frame_mean_rstd(a.stats_in, f, a.inv_count_in, mean, rstd);
  }
  // wave-uniform, but computed by vector instructions: held in a scalar register across the main loop
  rstd = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, rstd)));
  mean = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, mean)));
  {   // epilogue constant table [9 edge classes][128 couts] of this channel tile
    float* kk = (float*)(smem + KK_O);
    constexpr int NKK = (9 * 128 + NTHR - 1) / NTHR;
    float ksa[NKK], ksg[NKK];
#pragma unroll
    for (int k = 0; k < NKK; ++k) {  // 9*128 = 4.5 * 256 entries: all the loads in flight together
      const int idx = tid + NTHR * k;
      const int o = (idx >> 7) * a.CoutPad + nt * 128 + (idx & 127);
      ksa[k] = (idx < 9 * 128) ? esa[o] : 0.f;
      ksg[k] = (idx < 9 * 128) ? a.edge_sg[o] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < NKK; ++k) {
      const int idx = tid + NTHR * k;
      if (idx < 9 * 128) kk[idx] = (ksa[k] - rstd * mean * ksg[k]) * RELU_S;
    }
  }
  float res_s = 1.f;
  if (RES_AFF) {
    res_s = a.res_scale[f];
    if (tid < 128) ((float*)(smem + BT_O))[tid] = (nt * 128 + tid < a.Cout) ? a.res_bias[(size_t)f * a.Cout + nt * 128 + tid] : 0.f;
  }
  if constexpr (HDMA) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the prologue's pieces are home before the barrier, whatever the fence below waits for
  } else {
#pragma unroll
    for (int m = 0; m < NA; ++m) HALO_WR16(m);
  }
  __syncthreads();

  f32x16 ac[8];              // [pixel row j of the wave's 8], elements 4 u .. 4 u + 3 = cout group u (ac_get / ac_set)
  f32x16 zero16;
#pragma unroll
  for (int r = 0; r < 16; ++r) zero16[r] = 0.f;

  // Unused, and they stay (like row_l in the dgrad kernel): the fragment bases of the 32x32 loop, which the kernel this one was split from computed at
  // this point in every instantiation.  With them the compiler emits all 14 forward kernels instruction for instruction as before the split; without
  // them 7 differ in the prologue (halo-DMA 0, 4 and register-staged 4, 7: one instruction in another place; halo-DMA 1, 5 and register-staged 0: scalar
  // registers renamed) -- tools/isa_diff.py, profiles/conv3x3_split.md.  Removing them is a change to time on its own.
  const int hi = lane >> 5, l31 = lane & 31;
  const unsigned char* aL = smem + ((wm * 8 + sub_row(l31)) * 18 + (l31 & 15)) * A_RS + hi * 16;
  const int bsw = (l31 >> 2) & 3;
  const unsigned char* bL0 = smem + A_SZ + (wn * 64 + l31) * 64 + (((0 + hi) ^ bsw) << 4);
  const unsigned char* bL1 = smem + A_SZ + (wn * 64 + l31) * 64 + (((2 + hi) ^ bsw) << 4);
  (void)aL; (void)bL0; (void)bL1;

  // fragment bases: lane = (MFMA column / row c16, K chunk q16)
  const int c16 = lane & 15, q16 = lane >> 4;
  const int pcol = (c16 < 4) ? 2 * c16 : ((c16 < 12) ? 2 * (c16 - 4) + 1 : 2 * (c16 - 8));   // pixel column of MFMA column c16
  // (LDS pointers the compiler cannot see behind: every fragment read is base + a 16-bit immediate; folded into the array's address the larger
  // offsets no longer fit the instruction and each costs an address register)
  typedef const __attribute__((address_space(3))) unsigned char* lds_cptr;
  lds_cptr aLe = (lds_cptr)smem + ((wm * 8) * 18 + pcol) * A_RS + q16 * 16 + 16 * (pcol & 1);        // taps dx = 0, 2: halo pixel parity = pcol's
  lds_cptr aLo = (lds_cptr)smem + ((wm * 8) * 18 + pcol) * A_RS + q16 * 16 + 16 * (1 - (pcol & 1));  // tap dx = 1
  // cout group u = 2 blk + b: row 32 blk + 8 (c16 >> 2) + 4 b + (c16 & 3), swizzle ((row >> 2) & 3) = (2 (c16 >> 2) + b) & 3
  lds_cptr bW0 = (lds_cptr)smem + A_SZ + (wn * 64 + 8 * (c16 >> 2) + (c16 & 3)) * 64 + ((q16 ^ ((2 * (c16 >> 2)) & 3)) << 4);
  lds_cptr bW1 = (lds_cptr)smem + A_SZ + (wn * 64 + 8 * (c16 >> 2) + 4 + (c16 & 3)) * 64 + ((q16 ^ ((2 * (c16 >> 2) + 1) & 3)) << 4);
  if constexpr (!HDMA) { asm volatile("" : "+v"(aLe), "+v"(aLo), "+v"(bW0), "+v"(bW1)); }
  // HDMA fragment bases: one per tap column dx (the image's swizzle is a function of the halo column pcol + dx), the weight rows in ring slot 0 / 2
#define HA_BASE(dx_) ((lds_cptr)smem + H_RING + ((wm * 8) * 18 + pcol + (dx_)) * 64 + ((q16 ^ (((pcol + (dx_)) >> 2) & 3)) << 4))
  lds_cptr aH0 = HA_BASE(0), aH1 = HA_BASE(1), aH2 = HA_BASE(2);
#undef HA_BASE
  lds_cptr bWl0 = (lds_cptr)smem + (wn * 64 + 8 * (c16 >> 2) + (c16 & 3)) * 64 + ((q16 ^ ((2 * (c16 >> 2)) & 3)) << 4);
  lds_cptr bWl1 = (lds_cptr)smem + (wn * 64 + 8 * (c16 >> 2) + 4 + (c16 & 3)) * 64 + ((q16 ^ ((2 * (c16 >> 2) + 1) & 3)) << 4);
  lds_cptr bWh0 = bWl0 + 2 * H_SLOT, bWh1 = bWl1 + 2 * H_SLOT;
  int h_swap = 2 * H_SLOT;
  if constexpr (HDMA) { asm volatile("" : "+v"(aH0), "+v"(aH1), "+v"(aH2), "+v"(bWl0), "+v"(bWl1), "+v"(bWh0), "+v"(bWh1)); }

  // epilogue addressing (needed early: the residual is requested during the last channel block)
  const int CB_out = a.Cout >> 5;
  const int cb0 = nt * 4 + wn * 2;                 // 32-channel block of n2 = 0
  const bool nvalid[2] = {(cb0 + 0) < CB_out, (cb0 + 1) < CB_out};
  // Addresses = wave-uniform base (frame, channel block n2) + a 32-bit per-lane byte offset: global accesses with an SGPR
  // base, no 64-bit vector address arithmetic, no address registers kept across the main loop.
  size_t cbase[2];                                  // element offset of channel block n2 of this frame
#pragma unroll
  for (int n2 = 0; n2 < 2; ++n2) cbase[n2] = (size_t)(f * CB_out + (nvalid[n2] ? cb0 + n2 : 0)) * HW * 32;
  // Forward epilogue: lane (c16, q16) owns bytes 16 q16 .. + 15 of pixel pcol(c16)'s 64-byte record in every (pixel row j, 32-cout block n2): residual and
  // output move as ONE 16-byte access per lane, 1024 contiguous bytes per instruction, in the accumulators' own layout.
  const unsigned voff16 = (unsigned)(((ty0 + wm * 8) * a.W + tx0 + pcol) * 32 + 8 * q16) * 2u;
  const unsigned gj_b = (unsigned)a.W * 64u;           // + j * gj_b: one image row further down (bytes)
  u32x4 rq16[8][2];                                    // residual [pixel row j][n2]

  // ---- main loop (the schedules are the CONV_STEP16 / HSTEP macros above) ----
  const op16_t* resp = a.res;
  op16x8 fp[8], fw[2];         // the current tap's 8 pixel fragments, a double-buffered weight fragment
  // forward weight DMA (GLDS16): resource over this channel tile's NCB * 9 packed tap tiles of 8 KB -- built from kernel arguments and the block index
  // only, so it lives in scalar registers; reads beyond it would return zeros (none: step s + 1 <= 3 NCB - 1 ends at the resource's last byte)
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.wpk + (size_t)nt * NCB * 9 * 4096), 0, NCB * 9 * 8192, 0x00020000);
  const int wvoff = (w * 64 + lane) * 16;

  if (TRACE) t_trace[1] = wall_clock64();
  if constexpr (HDMA) {
    if (CONV_ABLATE != 2) {
      HWP(2, 0, hwrs);          // (the piece the last group of a pass requests for the next one)
      HWB(0, 0);
#pragma unroll
      for (int j = 0; j < 8; ++j) HPA(j, 0);
      SB();
#pragma unroll
      for (int j = 0; j < 8; ++j) ac[j] = zero16;
      const int NPASS = NCB >> 1;
#pragma unroll 1
      for (int ps = 0; ps < NPASS; ++ps) {
        const bool more = ps + 1 < NPASS;
        const __amdgpu_buffer_rsrc_t hwrs_n = __builtin_amdgcn_make_buffer_rsrc((void*)h_wptr, 0, more ? h_wbytes : 0u, 0x00020000);
        const __amdgpu_buffer_rsrc_t hxrs_n = __builtin_amdgcn_make_buffer_rsrc((void*)xplane, 0, more ? h_xbytes : 0u, 0x00020000);
        const unsigned cbB = (unsigned)(2 * ps + 1) * (unsigned)HW * 64u, cbA = cbB + (unsigned)HW * 64u;   // bytes; uniform
        HSTEP(0, HWP(2, 1, hwrs), HWP(3, 0, hwrs), HWP(3, 1, hwrs), NOP_(), NOP_(), NOP_(), NOP_(), WAIT_BARRIER(0), HWP(4, 0, hwrs));
        HSTEP(1, HWP(4, 1, hwrs), HWP(5, 0, hwrs), HWP(5, 1, hwrs), HXP(0, 1, hxrs, cbB), HXP(1, 1, hxrs, cbB), HXP(2, 1, hxrs, cbB), HXP(3, 1, hxrs, cbB), WAIT_BARRIER(4), HWP(6, 0, hwrs));
        HSTEP(2, HWP(6, 1, hwrs), HWP(7, 0, hwrs), HWP(7, 1, hwrs), HXP(4, 1, hxrs, cbB), HXP(5, 1, hxrs, cbB), NOP_(), NOP_(), WAIT_BARRIER(2), HWP(8, 0, hwrs));
        HSTEP(3, HWP(8, 1, hwrs), HWP(9, 0, hwrs), HWP(9, 1, hwrs), NOP_(), NOP_(), NOP_(), NOP_(), WAIT_BARRIER(0), HWP(10, 0, hwrs));
        HSTEP(4, HWP(10, 1, hwrs), HWP(11, 0, hwrs), HWP(11, 1, hwrs), NOP_(), NOP_(), NOP_(), NOP_(), WAIT_BARRIER(0), HWP(12, 0, hwrs));
        HSTEP(5, HWP(12, 1, hwrs), HWP(13, 0, hwrs), HWP(13, 1, hwrs), HXP(0, 0, hxrs_n, cbA), HXP(1, 0, hxrs_n, cbA), HXP(2, 0, hxrs_n, cbA), HXP(3, 0, hxrs_n, cbA), WAIT_BARRIER(4), HWP(14, 0, hwrs));
        HSTEP(6, HWP(14, 1, hwrs), HWP(15, 0, hwrs), HWP(15, 1, hwrs), HXP(4, 0, hxrs_n, cbA), HXP(5, 0, hxrs_n, cbA), NOP_(), NOP_(), WAIT_BARRIER(2), HWP(16, 0, hwrs));
        if constexpr (HAS_RES) {   // compile-time: without a residual the loads would be dead code and the count wrong
          HSTEP(7, HWP(16, 1, hwrs), HWP(17, 0, hwrs), HWP(17, 1, hwrs), XR16(0), NOP_(), NOP_(), NOP_(), WAIT_BARRIER(2), HWP(18, 0, hwrs_n));
        } else {
          HSTEP(7, HWP(16, 1, hwrs), HWP(17, 0, hwrs), HWP(17, 1, hwrs), NOP_(), NOP_(), NOP_(), NOP_(), WAIT_BARRIER(0), HWP(18, 0, hwrs_n));
        }
        HSTEP(8, HWP(18, 1, hwrs_n), HWP(19, 0, hwrs_n), HWP(19, 1, hwrs_n), NOP_(), NOP_(), NOP_(), NOP_(), WAIT_BARRIER(0), HWP(20, 0, hwrs_n));
        h_wso += 18 * H_SLOT;
        h_rpi ^= 2 * H_SLOT;
        bWl0 += h_swap; bWl1 += h_swap; bWh0 -= h_swap; bWh1 -= h_swap;
        h_swap = -h_swap;
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the (empty) pieces of the last pass are retired before the workgroup's LDS is given up
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) ac[j] = zero16;
      __syncthreads();
    }
  } else {
    if (CONV_ABLATE != 2) {
      WB(0, 0, 0);
#pragma unroll
      for (int j = 0; j < 8; ++j) PA(j, 0, 0);
      SB();
      // The accumulators start from zero: a peeled first channel block whose first tap takes C = 0 (as the dgrad loop does) cost 27 spilled registers.
#pragma unroll
      for (int j = 0; j < 8; ++j) ac[j] = zero16;
#pragma unroll 1
      for (int cb = 0; cb + 1 < NCB; ++cb) {
        CONV_STEP16(cb, 0, 1, true, false, false, false);
        CONV_STEP16(cb, 1, 2, false, false, false, false);
        CONV_STEP16(cb, 2, 0, false, true, false, false);
      }
      // (the tracing instantiations hold the phase stamps as well: no residual request inside their main loop)
      CONV_STEP16(NCB - 1, 0, 1, false, false, !TRACE, false);
      CONV_STEP16(NCB - 1, 1, 2, false, false, false, false);
      CONV_STEP16(NCB - 1, 2, 0, false, false, false, true);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) ac[j] = zero16;
      __syncthreads();
    }
  }

  // ---------------- epilogue ----------------
  if (TRACE) t_trace[2] = wall_clock64();
  if (CONV_ABLATE == 1) {  // profiling: keep the accumulators live, skip the epilogue
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) t += ac[j][r];
    if (t == 12345.678f) a.y[0] = (vpt_op16)t;
    return;
  }
  if (HAS_RES && (TRACE || CONV_ABLATE == 2)) XR16(0);
  SB();

  f32x2 s_sum2 = {0.f, 0.f}, s_sq2 = {0.f, 0.f};   // packed fp32 (v_pk_add_f32 / v_pk_fma_f32): two values per VALU issue
  // The epilogue body is instantiated for NV = 2 and NV = 1 valid 32-channel blocks of this wave (Cout / 32 odd) and selected by one
  // uniform branch: with no control flow inside, the waits on the prefetched table / residual pieces stay counted.
  // ---- forward epilogue: everything in the 16x16 accumulators' own layout.  Lane (c16, q16) holds, per pixel row j and 32-cout block n2, the 8 values
  // of couts 8 q16 .. + 7 of pixel pcol (accumulator elements 8 n2 .. 8 n2 + 7 of ac[j]): two f32x4 of the constant table, ONE 16-byte residual load
  // and ONE 16-byte store per lane -- whole 128-byte lines, no lane exchange anywhere.  Per value: GroupNorm fold, ReLU (packed / clamp, see PACKED_RELU
  // and CLAMP_RELU), residual FMA, rounding, frame statistics of the STORED tensor by v_dot2 (products of two 16-bit operands are exact in fp32) -- what
  // the next layer's GroupNorm normalises.  The edge class of a row differs from "interior" only on the wave's first row (image top) and last row (bottom).
  // (derived from a copy of the lane id the compiler cannot see through: computed HERE, not held in registers across the main loop)
  int lane_l = lane;
  asm volatile("" : "+v"(lane_l));
  const int c16_l = lane_l & 15, q16_l = lane_l >> 4;
  const int pcol_l = (c16_l < 4) ? 2 * c16_l : ((c16_l < 12) ? 2 * (c16_l - 4) + 1 : 2 * (c16_l - 8));
  const unsigned voff16_l = (unsigned)(((ty0 + wm * 8) * a.W + tx0 + pcol_l) * 32 + 8 * q16_l) * 2u;
  const int x16_ = tx0 + pcol_l;
  const int ex16 = (x16_ == 0) ? 0 : ((x16_ == a.W - 1) ? 2 : 1);
  const int eo_top = (ty0 + wm * 8 == 0) ? 0 : 3 * 128, eo_bot = (ty0 + wm * 8 + 7 == a.H - 1) ? 6 * 128 : 3 * 128;
  const float* kk16 = (const float*)(smem + KK_O) + ex16 * 128 + wn * 64 + 8 * q16_l;
  auto epilogue16 = [&](auto nv_) __attribute__((always_inline)) {
    constexpr int NV = decltype(nv_)::value;
    u32x4 outv[8][2];          // packed results: all stores are issued after the last load has been consumed: gfx950 has one counter (vmcnt)
                               // for loads and stores, and a wait for a load issued among stores degenerates to vmcnt(0)
    f32x4 kq[2][2];            // constant table [parity of chunk c = 2 j + n2][half h], one chunk AHEAD: read at the point of use every chunk paid a full
                               // LDS round trip behind the co-resident workgroup's fragment reads
    LOAD_KK16(0);
    SB();
    const f32x2 zero2 = {0.f, 0.f};
    const f32x2 rstd2 = {rstd * RELU_S, rstd * RELU_S}, ress2 = {res_s, res_s};
    const f32x2 relu_inv2 = {RELU_INV, RELU_INV};
    const float* btab = (const float*)(smem + BT_O) + wn * 64 + 8 * q16_l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (HAS_RES && j == 0) XR16L(1);
      if (HAS_RES && j < 6) XR16L(j + 2);   // rolling prefetch, two rows ahead (row 0 was requested during the last channel block)
      SB();
#pragma unroll
      for (int n2 = 0; n2 < 2; ++n2) {
        if (2 * j + n2 < 15) { LOAD_KK16(2 * j + n2 + 1); SB(); }
        if (n2 >= NV) continue;
        f32x4 bq[2];
        if (RES_AFF) {
          bq[0] = *(const f32x4*)(btab + n2 * 32); bq[1] = *(const f32x4*)(btab + n2 * 32 + 4);
          SB();
        }
        u32x2 pk[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          f32x2 v01 = {ac[j][8 * n2 + 4 * h + 0], ac[j][8 * n2 + 4 * h + 1]}, v23 = {ac[j][8 * n2 + 4 * h + 2], ac[j][8 * n2 + 4 * h + 3]};
          const f32x4 k4 = kq[n2][h];
          const f32x2 k01 = {k4.x, k4.y}, k23 = {k4.z, k4.w};
          if (PACKED_RELU) {
            v01 = rstd2 * v01 + k01;
            v23 = rstd2 * v23 + k23;
          } else if (CLAMP_RELU) {
            v01 = pk_fma_clamp01(rstd2, v01, k01);
            v23 = pk_fma_clamp01(rstd2, v23, k23);
          } else {
            v01 = __builtin_elementwise_max(rstd2 * v01 + k01, zero2);
            v23 = __builtin_elementwise_max(rstd2 * v23 + k23, zero2);
          }
          if (HAS_RES) {
            const uint32_t ra = h ? rq16[j][n2].z : rq16[j][n2].x, rb = h ? rq16[j][n2].w : rq16[j][n2].y;
            const f32x2 r01 = {op16_lo_to_f32(ra), op16_hi_to_f32(ra)}, r23 = {op16_lo_to_f32(rb), op16_hi_to_f32(rb)};
            if (RES_AFF) {
              const f32x4 b4 = bq[h];
              const f32x2 b01 = {b4.x, b4.y}, b23 = {b4.z, b4.w};
              if (CLAMP_RELU) {
                v01 = ress2 * r01 + __builtin_elementwise_fma(v01, relu_inv2, b01);
                v23 = ress2 * r23 + __builtin_elementwise_fma(v23, relu_inv2, b23);
              } else {
                v01 = ress2 * r01 + (v01 + b01);
                v23 = ress2 * r23 + (v23 + b23);
              }
            } else if (CLAMP_RELU) {
              v01 = __builtin_elementwise_fma(v01, relu_inv2, r01);
              v23 = __builtin_elementwise_fma(v23, relu_inv2, r23);
            } else {
              v01 += r01;
              v23 += r23;
            }
          }
          pk[h].x = pack_op16x2(v01.x, v01.y);
          pk[h].y = pack_op16x2(v23.x, v23.y);
          if (PACKED_RELU) {   // ReLU as ONE packed signed-16-bit maximum per pair on the ROUNDED bit patterns: positive 16-bit floats order like integers,
                               // negative ones (and -0) are negative integers, rounding is monotone, so max(round(v), 0) == round(max(v, 0)) bit for bit
            pk[h].x = relu_op16x2(pk[h].x);
            pk[h].y = relu_op16x2(pk[h].y);
          }
          s_sum2.x = dot2_op16(pk[h].x, OP16_ONE2, s_sum2.x);   // frame statistics of the STORED tensor
          s_sum2.y = dot2_op16(pk[h].y, OP16_ONE2, s_sum2.y);
          s_sq2.x = dot2_op16(pk[h].x, pk[h].x, s_sq2.x);
          s_sq2.y = dot2_op16(pk[h].y, pk[h].y, s_sq2.y);
        }
        outv[j][n2] = u32x4{pk[0].x, pk[0].y, pk[1].x, pk[1].y};
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int n2 = 0; n2 < NV; ++n2)
        *(u32x4*)((char*)(a.y + cbase[n2]) + (voff16_l + (unsigned)j * gj_b)) = outv[j][n2];
  };
  if constexpr (POOL) {
    // The four pointers only this epilogue uses are read from the kernarg segment HERE, through a pointer the compiler cannot see behind: taken from
    // `a` they are loaded with the rest of the arguments at kernel entry and sit in eight scalar registers through the whole main loop -- in the
    // arg-max mode (7) that was the eight registers too many (8 SGPRs spilled to VGPR lanes around the loop).
    const __attribute__((address_space(4))) VptConv3x3Args* late = (const __attribute__((address_space(4))) VptConv3x3Args*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(late));
    int tid_p = threadIdx.x;   // the thread-indexed addressing of phase 2 is derived HERE, not held across the main loop
    asm volatile("" : "+v"(tid_p));
    const int tid = tid_p, lane = tid_p & 63;
    vpt_op16* const seam_r_p = late->seam_r;
    vpt_op16* const seam_c_p = late->seam_c;
    vpt_op16* const pool_mask_p = late->pool_mask;
    double* const chs_out_p = late->chs_out;
    // ---- phase 1: GroupNorm fold + ReLU, rounded to 16 bits, into the LDS tile [16 x 16 pixels][128 channels] (pixel pitch PT_RS: the
    // 16 extra bytes spread a column of pixels over the banks).  The tile reuses the halo / weight buffers: every wave must be past
    // its last fragment read first.
    __syncthreads();
    {   // one ds_write_b128 per lane and (pixel row, 32-cout block): couts 8 q16 .. + 7 of pixel (wm 8 + j, pcol)
      const f32x2 zero2 = {0.f, 0.f};
      const f32x2 rstd2 = {rstd, rstd};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float* ke = kk16 + EO16(j);
        unsigned char* dst = smem + ((wm * 8 + j) * 16 + pcol_l) * PT_RS + (wn * 64 + 8 * q16_l) * 2;
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2) {
          if (!nvalid[n2]) continue;
          u32x2 pk[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const f32x4 k4 = *(const f32x4*)(ke + n2 * 32 + 4 * h);
            const f32x2 k01 = {k4.x, k4.y}, k23 = {k4.z, k4.w};
            f32x2 v01 = {ac[j][8 * n2 + 4 * h + 0], ac[j][8 * n2 + 4 * h + 1]}, v23 = {ac[j][8 * n2 + 4 * h + 2], ac[j][8 * n2 + 4 * h + 3]};
            if (PMASK) {      // (the masks compare post-ReLU values: a window of negatives must read as a window of zeros)
              v01 = __builtin_elementwise_max(rstd2 * v01 + k01, zero2);
              v23 = __builtin_elementwise_max(rstd2 * v23 + k23, zero2);
            } else {          // inference: the pool's packed maximum starts from 0 and the seam kernel's from a pooled value >= 0 -- that IS the ReLU
              v01 = rstd2 * v01 + k01;
              v23 = rstd2 * v23 + k23;
            }
            pk[h].x = pack_op16x2(v01.x, v01.y);
            pk[h].y = pack_op16x2(v23.x, v23.y);
          }
          *(u32x4*)(dst + n2 * 64) = u32x4{pk[0].x, pk[0].y, pk[1].x, pk[1].y};
        }
      }
    }
    __syncthreads();
    // ---- phase 2: pooled pixel (j, i) of the tile = max over conv rows 2j-1 .. 2j+1, columns 2i-1 .. 2i+1 that lie INSIDE the tile (j = 0
    // / i = 0 miss the row / column above / left of the tile: image border -> the pool's padding, nothing is missing; otherwise the seam
    // kernel adds it).  Packed signed 16-bit max from 0 on the raw bit patterns (post-ReLU values are >= +0; a -0.0 stays below 0).
    // item = (pooled pixel, channel octet): the 16 lanes of a ds_read_b128 group read the 256 contiguous bytes of one pixel.
    typedef short i16x8 __attribute__((ext_vector_type(8)));
    const int PH = a.H >> 1, PW = a.W >> 1;
    const bool top_open = ty0 > 0, left_open = tx0 > 0;      // the tile's first pooled row / column is incomplete
    float p_sum = 0.f, p_sq = 0.f;
    float c1[8], c2[8];      // per-channel sums of the STORED (scaled, rounded) complete pixels: a thread's four items share the octet tid & 15
#pragma unroll
    for (int k = 0; k < 8; ++k) { c1[k] = 0.f; c2[k] = 0.f; }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int item = tid + 256 * it;
      const int oct = item & 15, pi = (item >> 4) & 7, pj = item >> 7;
      const int cg = nt * 128 + oct * 8;
      const unsigned char* src = smem + oct * 16;
      i16x8 mx = {0, 0, 0, 0, 0, 0, 0, 0};
      i16x8 vv[PMASK ? 9 : 1];
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        const int r = 2 * pj + dy;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int c = 2 * pi + dx;
          const i16x8 v = *(const i16x8*)(src + (max(r, 0) * 16 + max(c, 0)) * PT_RS);     // (clamped: the duplicate does not change a maximum)
          mx = __builtin_elementwise_max(mx, v);
          if (PMASK) vv[PMASK ? (dy + 1) * 3 + dx + 1 : 0] = v;
        }
      }
      if constexpr (PMASK) {
        // which positions hold the maximum: per position and channel pair xor, packed min with 1 (0: equal), m = 2 m + b -- three packed
        // instructions (inline asm: left to the compiler the 16-bit lanes are scalarised into v_cmp_ne_u16 + v_cndmask pairs, 930 instructions
        // per thread instead of 430).  Positions outside the tile (clamped reads above: duplicates) or the image count as "differs"; the seam
        // kernel fills in the bits of the neighbouring tiles' row / column for the pixels it finishes.
        const u32x4 mxu = __builtin_bit_cast(u32x4, mx);
        u32x4 mk = {0u, 0u, 0u, 0u};
        const uint32_t one2 = 0x00010001u, two2 = 0x00020002u;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const u32x4 vk = __builtin_bit_cast(u32x4, vv[k]);
          const bool inside = (2 * pj + k / 3 - 1 >= 0) && (2 * pi + k % 3 - 1 >= 0);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            uint32_t t = inside ? (vk[j] ^ mxu[j]) : 0xffffffffu, b, m2;
            asm("v_pk_min_u16 %0, %1, %2" : "=v"(b) : "v"(t), "s"(one2));
            asm("v_pk_mad_u16 %0, %1, %2, %3" : "=v"(m2) : "v"(mk[j]), "s"(two2), "v"(b));
            mk[j] = m2;
          }
        }
        if (cg < a.Cout) {
          const size_t moff = ((size_t)(f * CB_out + (cg >> 5)) * PH * PW + (size_t)(((ty0 >> 1) + pj) * PW + (tx0 >> 1) + pi)) * 32 + (cg & 31);
          *(u32x4*)(pool_mask_p + moff) = mk;
        }
      }
      if (cg < a.Cout) {
        u32x4 mv = __builtin_bit_cast(u32x4, mx);
        const size_t off = ((size_t)(f * CB_out + (cg >> 5)) * PH * PW + (size_t)(((ty0 >> 1) + pj) * PW + (tx0 >> 1) + pi)) * 32 + (cg & 31);
        const bool complete = (pj > 0 || !top_open) && (pi > 0 || !left_open);
        if (complete) {      // the seam kernel accounts for the others once they are final
#pragma unroll
          for (int k = 0; k < 4; ++k) {     // packed pairs: one v_dot2 per two values and moment (products of 16-bit operands are exact in fp32)
            p_sum = dot2_op16(mv[k], OP16_ONE2, p_sum);
            p_sq = dot2_op16(mv[k], mv[k], p_sq);
          }
          if (a.out_gain) {  // GroupNorm `n`'s gain folded into the stored tensor (a thread's items share the channel octet: 8 cached loads)
            float vals[8];
            unpack8(mv, vals);
            const f32x4 g0 = *(const f32x4*)(a.out_gain + cg), g1 = *(const f32x4*)(a.out_gain + cg + 4);
            vals[0] *= g0.x; vals[1] *= g0.y; vals[2] *= g0.z; vals[3] *= g0.w; vals[4] *= g1.x; vals[5] *= g1.y; vals[6] *= g1.z; vals[7] *= g1.w;
            mv = pack8(vals);
          }
          if (chs_out_p) {
            float q[8];
            unpack8(mv, q);
#pragma unroll
            for (int k = 0; k < 8; ++k) { c1[k] += q[k]; c2[k] = fmaf(q[k], q[k], c2[k]); }
          }
        }
        *(u32x4*)(a.y + off) = mv;
      }
    }
    // ---- seams: the tile's last row (-> the pooled row below) and last column (-> the pooled column to the right), one 16-byte piece per
    // thread each: seam_r [f][C/32][H/16][W][32], seam_c [f][C/32][W/16][H][32] (whole image rows / columns, so the corner pixel needs no case)
    {
      const int oct = tid & 15, q = tid >> 4;     // q = position along the seam
      const int cg = nt * 128 + oct * 8;
      if (cg < a.Cout) {
        if (ty0 + 16 < a.H) {
          const u32x4 v = *(const u32x4*)(smem + (15 * 16 + q) * PT_RS + oct * 16);
          *(u32x4*)(seam_r_p + ((size_t)((f * CB_out + (cg >> 5)) * tilesY + ty) * a.W + tx0 + q) * 32 + (cg & 31)) = v;
        }
        if (tx0 + 16 < a.W) {
          const u32x4 v = *(const u32x4*)(smem + (q * 16 + 15) * PT_RS + oct * 16);
          *(u32x4*)(seam_c_p + ((size_t)((f * CB_out + (cg >> 5)) * tilesX + tx) * a.H + ty0 + q) * 32 + (cg & 31)) = v;
        }
      }
    }
    s_sum2.x = p_sum; s_sum2.y = 0.f; s_sq2.x = p_sq; s_sq2.y = 0.f;
    if (chs_out_p) {
      // threads tid = octet + 16 q share an octet: lanes octet + 16 {0..3} of each wave (two exchanges), then the four waves through the
      // epilogue-table area of the LDS (dead since phase 1), then one fp64 atomic per (channel, moment): 256 per tile
      float* scr = (float*)(smem + KK_O);          // [4 waves][16 octets][16]
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        c1[k] += __shfl_xor(c1[k], 16, 64); c1[k] += __shfl_xor(c1[k], 32, 64);
        c2[k] += __shfl_xor(c2[k], 16, 64); c2[k] += __shfl_xor(c2[k], 32, 64);
      }
      if (lane < 16) {
#pragma unroll
        for (int k = 0; k < 8; ++k) { scr[(w * 16 + lane) * 16 + k] = c1[k]; scr[(w * 16 + lane) * 16 + 8 + k] = c2[k]; }
      }
      __syncthreads();
      {
        const int o = tid >> 4, k = tid & 15;
        const float t = (scr[(0 * 16 + o) * 16 + k] + scr[(1 * 16 + o) * 16 + k]) + (scr[(2 * 16 + o) * 16 + k] + scr[(3 * 16 + o) * 16 + k]);
        const int ch = nt * 128 + o * 8 + (k & 7);
        if (ch < a.Cout) atomicAdd(chs_out_p + ((size_t)f * a.Cout + ch) * 2 + (k >> 3), (double)t);
      }
    }
  } else {
    if (nvalid[1]) epilogue16(std::integral_constant<int, 2>{});
    else if (nvalid[0]) epilogue16(std::integral_constant<int, 1>{});
  }
#undef GLDS16
#undef XA16
#undef HALO_WR16
#undef PA
#undef WB
#undef M16A
#undef G16
#undef G16R
#undef TAP16
#undef EPI_LD16
#undef XR16
#undef XR16L
#undef CONV_STEP16
#undef HWP
#undef HXP_
#undef HXP
#undef HPA
#undef HWB
#undef HG
#undef HGR
#undef HSTEP
#undef EO16
#undef LOAD_KK16
  float s_sum = s_sum2.x + s_sum2.y, s_sq = s_sq2.x + s_sq2.y;
  if (a.stats_out) {
    float* red = (float*)(smem + KK_O + KK_BYTES);
    s_sum = wave_sum(s_sum);
    s_sq = wave_sum(s_sq);
    if (lane == 0) { red[w] = s_sum; red[NWAVE + w] = s_sq; }
    __syncthreads();
    if (tid == 0) {
      float t1 = (red[0] + red[1]) + (red[2] + red[3]), t2 = (red[NWAVE] + red[NWAVE + 1]) + (red[NWAVE + 2] + red[NWAVE + 3]);
      if (NWAVE == 8) {
        t1 += (red[4] + red[5]) + (red[6] + red[7]);
        t2 += (red[12] + red[13]) + (red[14] + red[15]);
      }
      atomicAdd(a.stats_out + 2 * f, (double)t1);
      atomicAdd(a.stats_out + 2 * f + 1, (double)t2);
    }
  }
  if (TRACE && tid == 0) {
    long long* t = a.trace + (size_t)blockIdx.x * 12;
    t[0] = t_trace[0]; t[1] = t_trace[1]; t[2] = t_trace[2]; t[3] = wall_clock64(); t[4] = cu_key; t[5] = 0;
    for (int k = 0; k < 5; ++k) t[6 + k] = 0;   // (slots of the former per-subtile stamps: they perturbed the epilogue's waits)
  }
}

// Called by vpt_conv3x3_launch (vpt_conv3x3.hip) with validated arguments and its choice of instantiation: mode 0, 1, 4, 5 or 7; variant 0 = 16-row
// register-staged tiles (a->trace set: the tracing instantiation, modes 0, 1), 1 = 32-row tiles (modes 0, 1, 5; grid = half the 16-row grid),
// 2 = halo DMA (modes 0, 1, 4, 5).
void vpt_conv3x3_fwd_launch(const VptConv3x3Args* a, int mode, int variant, long grid, int extra_lds, hipStream_t stream) {
#ifdef VPT_CONV_PROFILE
  static bool lds_attr_set = false;
  if (extra_lds > 0 && !lds_attr_set) {
    (void)hipFuncSetAttribute((const void*)vpt_conv3x3_kernel<false, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, extra_lds);
    (void)hipFuncSetAttribute((const void*)vpt_conv3x3_kernel<false, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, extra_lds);
    lds_attr_set = true;
  }
#endif
#define LAUNCH_(T_, M_) hipLaunchKernelGGL((vpt_conv3x3_kernel<T_, M_>), dim3((unsigned)grid), dim3(256), extra_lds, stream, *a)
#define LAUNCH32_(M_) hipLaunchKernelGGL((vpt_conv3x3_kernel<false, M_, 32>), dim3((unsigned)grid), dim3(512), 0, stream, *a)
#define LAUNCHH_(M_) hipLaunchKernelGGL((vpt_conv3x3_kernel<false, M_, 16, true>), dim3((unsigned)grid), dim3(256), 0, stream, *a)
  if (variant == 1) { if (mode == 0) LAUNCH32_(0); else if (mode == 1) LAUNCH32_(1); else LAUNCH32_(5); }
  else if (variant == 2) { if (mode == 0) LAUNCHH_(0); else if (mode == 1) LAUNCHH_(1); else if (mode == 4) LAUNCHH_(4); else LAUNCHH_(5); }
  else if (a->trace) { if (mode == 0) LAUNCH_(true, 0); else LAUNCH_(true, 1); }
  else if (mode == 0) LAUNCH_(false, 0); else if (mode == 1) LAUNCH_(false, 1); else if (mode == 4) LAUNCH_(false, 4); else if (mode == 5) LAUNCH_(false, 5); else LAUNCH_(false, 7);
#undef LAUNCH_
#undef LAUNCH32_
#undef LAUNCHH_
}

// ---------------------------------------------------------------------------------------------------------------------------
// Seam pass of the pool-fused convolution (mode 4 above): the pooled pixels on a tile's first pooled row / column got the in-tile part of
// their 3 x 3 window only.  Pooled pixel (J, I), J % 8 == 0, J > 0: conv row 2J - 1 is row 15 of the tile row above = seam_r[J / 8 - 1],
// columns 2I - 1 .. 2I + 1 (whole image rows: the corner needs no case); I % 8 == 0, I > 0: conv column 2I - 1 = seam_c[I / 8 - 1], rows
// 2J - 1 .. 2J + 1.  A pixel on both kinds of seam is handled once, by its row item.  Adds these pixels' share of the frame statistics.
// Work per frame: ((H/16 - 1) * W/2 + (W/16 - 1) * (H/2 - (H/16 - 1))) pixels x C/8 sixteen-byte items -- 18 % of the pooled tensor at
// 64 x 64, instead of the whole pre-pool tensor written and read back.
template <bool MASK>      // MASK: the training forward's arg-max masks are finished too (the inference instantiation carries none of that code)
__global__ __launch_bounds__(256) void vpt_pool_seam_kernel(VptPoolSeamArgs a) {
  // one workgroup per (frame, 32-channel block): thread = (seam pixel slot tid >> 2, channel octet tid & 3), a slot walks the seam pixels in steps of 64
  typedef short i16x8 __attribute__((ext_vector_type(8)));
  __shared__ float red[4][4][18];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int PH = a.H >> 1, PW = a.W >> 1, TY = a.H >> 4, TX = a.W >> 4;
  const int n_row = (TY - 1) * PW;                   // pixels on row seams
  const int col_len = PH - (TY - 1);                 // pixels of one column seam that are not on a row seam
  const int n_pix = n_row + (TX - 1) * col_len;
  const int cb = blockIdx.x % a.CB, f = blockIdx.x / a.CB;
  const int oct = tid & 3;
  const size_t plane = (size_t)(f * a.CB + cb);
  float s_sum = 0.f, s_sq = 0.f;                     // statistics of the UNscaled finished pixels (the frame statistics of P)
  float c1[8], c2[8];                                // per-channel sums of the STORED pixels
  float gv[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { c1[k] = 0.f; c2[k] = 0.f; gv[k] = a.gain ? a.gain[cb * 32 + oct * 8 + k] : 1.f; }
  for (int pix = tid >> 2; pix < n_pix; pix += 64) {
    int J, I;
    if (pix < n_row) { J = (pix / PW + 1) * 8; I = pix % PW; }
    else {
      const int q = pix - n_row, t = q / col_len, k = q - t * col_len;   // k-th pooled row that is not a multiple of 8 (row 0 counts: it is not a seam)
      I = (t + 1) * 8;
      J = (k == 0) ? 0 : (k - 1) / 7 * 8 + (k - 1) % 7 + 1;
    }
    vpt_op16* yp = a.y + (plane * PH * PW + (size_t)(J * PW + I)) * 32 + oct * 8;
    i16x8 m = *(const i16x8*)yp;
    const i16x8 m_in = m;                      // the in-tile part of the maximum (what the convolution's epilogue stored)
    i16x8 sv[6];                               // the window positions outside the tile: row above (k = 0, 1, 2), column to the left (k = 0, 3, 6)
    bool have[6] = {false, false, false, false, false, false};
    if ((J & 7) == 0 && J > 0) {
      const vpt_op16* sr = a.seam_r + ((plane * TY + (J >> 3) - 1) * a.W) * 32 + oct * 8;
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int x = 2 * I + dx;
        if (x >= 0) {
          const i16x8 v = *(const i16x8*)(sr + (size_t)x * 32);
          m = __builtin_elementwise_max(m, v);
          if (MASK) { sv[dx + 1] = v; have[dx + 1] = true; }
        }
      }
    }
    if ((I & 7) == 0 && I > 0) {
      const vpt_op16* sc = a.seam_c + ((plane * TX + (I >> 3) - 1) * a.H) * 32 + oct * 8;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        const int y = 2 * J + dy;
        if (y >= 0) {
          const i16x8 v = *(const i16x8*)(sc + (size_t)y * 32);
          m = __builtin_elementwise_max(m, v);
          if (MASK) { sv[3 + dy + 1] = v; have[3 + dy + 1] = true; }
        }
      }
    }
    if constexpr (MASK) {
      // arg-max masks of the training forward (vpt_conv3x3_kernel mode 7: bit 8 - k set = position k differs from the maximum): the in-tile bits
      // stay valid only where the in-tile maximum IS the window's maximum; the positions this kernel adds get their bits here
      typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
      unsigned short* mp = (unsigned short*)a.mask + (plane * PH * PW + (size_t)(J * PW + I)) * 32 + oct * 8;
      u16x8 mk = *(const u16x8*)mp;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        unsigned bits = (m_in[c] == m[c]) ? (unsigned)mk[c] : 0x1ffu;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          const int k = q < 3 ? q : 3 * (q - 3);            // scan position of seam value q
          if (have[q] && sv[q][c] == m[c]) bits &= ~(1u << (8 - k));
        }
        mk[c] = (unsigned short)bits;
      }
      *(u16x8*)mp = mk;
    }
    float vals[8];
    u32x4 mv = __builtin_bit_cast(u32x4, m);
    unpack8(mv, vals);
#pragma unroll
    for (int k = 0; k < 8; ++k) { s_sum += vals[k]; s_sq = fmaf(vals[k], vals[k], s_sq); }
    if (a.gain) {
#pragma unroll
      for (int k = 0; k < 8; ++k) vals[k] *= gv[k];
      mv = pack8(vals);
      unpack8(mv, vals);
    }
    *(u32x4*)yp = mv;
#pragma unroll
    for (int k = 0; k < 8; ++k) { c1[k] += vals[k]; c2[k] = fmaf(vals[k], vals[k], c2[k]); }
  }
  // reduce: lanes with the same octet (lane & 3), then the four waves
#pragma unroll
  for (int off = 4; off < 64; off <<= 1) {
#pragma unroll
    for (int k = 0; k < 8; ++k) { c1[k] += __shfl_xor(c1[k], off, 64); c2[k] += __shfl_xor(c2[k], off, 64); }
    s_sum += __shfl_xor(s_sum, off, 64); s_sq += __shfl_xor(s_sq, off, 64);
  }
  if (lane < 4) {
#pragma unroll
    for (int k = 0; k < 8; ++k) { red[w][lane][k] = c1[k]; red[w][lane][8 + k] = c2[k]; }
    red[w][lane][16] = s_sum; red[w][lane][17] = s_sq;
  }
  __syncthreads();
  if (tid < 64 && a.chs_out) {
    const int o = tid >> 4, k = tid & 15;
    const float t = (red[0][o][k] + red[1][o][k]) + (red[2][o][k] + red[3][o][k]);
    atomicAdd(a.chs_out + ((size_t)f * a.CB * 32 + cb * 32 + o * 8 + (k & 7)) * 2 + (k >> 3), (double)t);
  }
  if (tid >= 64 && tid < 66 && a.stats_out) {        // the frame totals: four octets x four waves
    const int k = 16 + (tid - 64);
    float t = 0.f;
#pragma unroll
    for (int o = 0; o < 4; ++o) t += (red[0][o][k] + red[1][o][k]) + (red[2][o][k] + red[3][o][k]);
    atomicAdd(a.stats_out + 2 * f + (tid - 64), (double)t);
  }
}

extern "C" int vpt_pool_seam_launch(const VptPoolSeamArgs* a, hipStream_t stream) {
  if ((a->H & 15) || (a->W & 15) || a->frames <= 0 || a->CB <= 0) return -1;
  const int PH = a->H >> 1, PW = a->W >> 1, TY = a->H >> 4, TX = a->W >> 4;
  const int n_pix = (TY - 1) * PW + (TX - 1) * (PH - (TY - 1));
  if (n_pix == 0) return 0;                          // a single tile per frame: every window is inside it
  const long grid = (long)a->frames * a->CB;
  if (grid > 0x7fffffffL) return -2;
  if (a->mask) hipLaunchKernelGGL(vpt_pool_seam_kernel<true>, dim3((unsigned)grid), dim3(256), 0, stream, *a);
  else hipLaunchKernelGGL(vpt_pool_seam_kernel<false>, dim3((unsigned)grid), dim3(256), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
