// 3x3 / pad-1 convolution of the IMPALA residual CNN as an implicit GEMM on 16-bit MFMA (gfx950): forward and dgrad.
//
// Replaces, per call:  FanInInitReLULayer.forward (lib/util.py:75-82) with GroupNorm(1,C) -> Conv2d(3x3,
// pad 1, no bias) -> ReLU, as used by CnnBasicBlock.conv0/conv1 (lib/impala_cnn.py:30-52) and by the
// firstconv of stacks 1..2 (lib/impala_cnn.py:86-97), plus the residual add of CnnBasicBlock.forward.
//
// Layout in HBM: activations are channel-blocked NHWC, [frame][C/32][H][W][32] 16-bit, so that the 18-pixel
// halo row of one 32-channel block is one contiguous 1152-byte run.  Weights are pre-packed (host side)
// as [ntile][C_in/32][tap][128 couts][32 cin] with the GroupNorm gain folded in and the four 16-byte
// chunks of every 64-byte row XOR-swizzled by ((cout >> 2) & 3), i.e. already in their LDS image.
//
// GroupNorm fold: conv(W, (x-mu)*rstd*g + b) with zero padding applied AFTER the norm equals
//     rstd * conv(W*g, x)  -  rstd*mu * SG[e][o]  +  SA[e][o]
// where SG/SA sum W*g / W*b over the taps that are inside the image for the pixel's edge class e
// (3 row classes x 3 column classes).  The main loop therefore streams raw 16-bit activations; the
// per-frame statistics (sum, sum of squares; produced by the previous kernel's epilogue) enter only
// in the epilogue.
//
// What every mode of vpt_conv3x3_kernel shares:
//   - Tile: one workgroup (4 waves: 2 row groups x 2 channel halves) = 16x16 output pixels x 128 output channels of one frame; a wave
//     owns 128 pixels x 64 couts.  Two workgroups per CU (78.6 KB LDS each, <= 256 VGPRs) hide each other's barriers and epilogues.
//   - LDS plan: [halo 18x18 pixels x 80-byte pitch][2 x 24 KB weight buffers][epilogue constant table 9 edge classes x 128 couts]
//     [block statistics][mode 5's residual bias].  Per 32-channel block the halo tile is register-staged into LDS once (zero-filled
//     outside the image) and reused by all nine taps.
//   - K step = one kernel row (3 taps) of one 32-channel block.  Its 24 KB weight tile is DMA'd global -> LDS (global_load_lds: no
//     VGPRs, no ds_write) into the double buffer one step ahead, so a step costs ONE barrier; the wait in front of the barrier is a
//     counted s_waitcnt that retires the DMA only and leaves the younger halo / residual loads in flight.
//   - The instruction order of a step is written out and pinned with sched_barrier (macros CONV_STEP / CONV_STEP16).
// Halo DMA (template parameter HDMA: modes 0, 1, 4, 5 with 16-row tiles on an even count of 32-channel blocks -- what the launch function picks
//   wherever it can; the plan above stays for every other case and is the bitwise reference of tests/test_gpu_conv_halo_dma.py):
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
//   16 bytes so that fragment reads and halo writes are bank-conflict-free (see FWD16 in the kernel).
// Dgrad modes (2, 3, 6): v_mfma_f32_32x32x16 main loop (4x2 accumulators of 32x32 per wave; the 32 rows of an M-subtile map to pixels
//   by sub_row() so that every hardware 16-lane ds_read_b128 group covers 16 consecutive pixels of ONE image row), epilogue through
//   v_permlane32_swap / v_permlane16_swap into whole 128-byte lines.
// How the kernel got here (the measurements behind each of these choices): DESIGN.md section 4, docs/history/, profiles/.
#include "vpt_common.h"
#include "vpt_kernels.h"
#include <stdlib.h>
#include <type_traits>
#ifndef VPT_EPI_NO_CLAMP_RELU
#define VPT_EPI_NO_CLAMP_RELU 0   // A/B builds: 1 = residual modes with the fp32 v_max ReLU of rounds 1-4 (bit-identical outputs)
#endif
// Profiling switches (VPT_CONV_ABLATE = 1: skip the epilogue, 2: skip the main loop; VPT_CONV_EXTRA_LDS: dynamic LDS to force one
// workgroup per CU) exist ONLY in builds made with -DVPT_CONV_PROFILE (tools/build_variant.sh): the shipped library reads no
// environment variable and its kernel carries no ablation branch -- a stray variable cannot change results.
#ifdef VPT_CONV_PROFILE
#define CONV_ABLATE (a.ablate)
#else
#define CONV_ABLATE 0
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
#define A_RS 80
#define A_BYTES (324 * A_RS)            // 25920
#define B_BYTES (3 * 128 * 64)          // 24576 per buffer (unpadded, swizzled)
#define KK_OFF (A_BYTES + 2 * B_BYTES)  // 75072
#define KK_BYTES (9 * 128 * 4)          // 4608
#define BT_OFF (KK_OFF + KK_BYTES + 64)  // 79744: per-channel residual bias of mode 5 (128 floats), after the block statistics' 64 bytes
#define SMEM_BYTES (BT_OFF + 512)       // 80256: two workgroups per CU = 160512 of 163840 bytes
// LDS plan of the halo-DMA instantiations (HDMA, see the kernel): [ring of four 8 KB tap slots][two dense halo images of 324 x 64 bytes][table ...]
#define H_SLOT (128 * 64)               // one tap's weights: 128 couts x 32 cin
#define H_RING (4 * H_SLOT)             // 32768
#define H_BUF (324 * 64)                // 20736
#define H_OOB 0x40000000u               // buffer offset of a halo chunk outside the image: beyond every resource, reads as zeros
#define PT_RS 272                       // pixel pitch of the 16 x 16 x 128-channel output tile of the pool-fused mode (256 + 16 bytes)
static_assert(256 * PT_RS <= KK_OFF, "the pooled mode's output tile must fit below the epilogue table");

// MFMA M-subtile row i (0..31) -> pixel (row 0/1, col 0..15) of a 2x16 patch.  Rows are swapped for columns
// 4..11 so that each 16-lane ds_read_b128 group {0-3,12-15,20-27} / {4-11,16-19,28-31} stays in one image row.
__device__ __forceinline__ int sub_row(int i) { return ((i >> 4) ^ (i >> 2) ^ (i >> 3)) & 1; }

// Template parameters of vpt_conv3x3_kernel:
// TRACE (tools/conv_trace.py): phase timestamps.  Compile time because s_memrealtime is a scalar-memory operation: one of them
// in flight makes lgkmcnt out of order and every LDS wait of the epilogue degenerates to lgkmcnt(0).
// MODE (compile time, so the epilogue carries no runtime branches): 0 forward, 1 forward + residual,
// 2 dgrad (+ c0 + c1 * xin), 3 dgrad + skip connection, 4 forward + the stack's 3x3 / stride-2 max-pool (CnnDownStack.forward,
// lib/impala_cnn.py:114-117: firstconv -> max_pool2d): the 16 x 16 output tile goes to LDS instead of HBM, its 8 x 8 pooled pixels are
// written -- complete where the 3 x 3 window lies inside the tile, the in-tile part of the maximum on the tile's first pooled row /
// column otherwise -- together with the tile's last row and column (the "seams"); vpt_pool_seam_kernel finishes the seam pixels.
// The pre-pool tensor (2 MB per frame in stack 1) never reaches HBM.  Modes 5, 6, 7: see the kernel's first lines.
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
  static_assert(!HDMA || (TR == 16 && !TRACE && (MODE == 0 || MODE == 1 || MODE == 4 || MODE == 5)), "halo DMA: the 16-row forward modes but the arg-max one");
  static_assert(!HDMA || 256 * PT_RS <= H_RING + 2 * H_BUF, "the pooled mode's output tile must fit below the epilogue table");
  constexpr int NWAVE = TR / 4, NTHR = 64 * NWAVE;
  constexpr int HPIX = (TR + 2) * 18;                            // halo pixels
  constexpr int NA = (HPIX * 4 + NTHR - 1) / NTHR;               // 16-byte halo chunks per thread and channel block: 6 / 5
  constexpr int NDMA = 24 / NWAVE;                               // 1 KB weight-DMA pieces per wave and step: 6 / 3
  constexpr int A_SZ = HPIX * A_RS, KK_O = HDMA ? H_RING + 2 * H_BUF : A_SZ + 2 * B_BYTES, BT_O = KK_O + KK_BYTES + 64, SMEM_SZ = BT_O + 512;
  constexpr int NKK = (9 * 128 + NTHR - 1) / NTHR;
  static_assert(TR != 16 || HDMA || (A_SZ == A_BYTES && KK_O == KK_OFF && SMEM_SZ <= SMEM_BYTES), "16-row layout");
  static_assert(!HDMA || (SMEM_SZ == 79424 && 2 * SMEM_SZ <= 163840), "halo-DMA layout: two workgroups per CU");
  static_assert((MODE != 4 && MODE != 7) || TR == 16, "the pool-fused epilogue is written for 16 x 16 tiles");
  // 5 forward + residual through a per-frame affine:  out = relu(...) + res_scale[f] * res + res_bias[f][channel]  -- the block that
  // follows a stack's GroupNorm `n` reads the pooled tensor itself (already multiplied by n's gain) instead of a normalised copy
  // (lib/impala_cnn.py:118-121 with the `n` pass folded away).
  // 6 dgrad of a block's conv1 that hands the block's conv0 its backward operand directly (round 5):  dy = conv^T + c0 + c1 * xin is the
  // gradient w.r.t. conv0's output y = xin, conv0 has no residual, so its ReLU gate is [xin > 0] and its operand dacc0 = rstd0 * dy * [xin > 0]
  // (rstd0: the statistics of conv0's INPUT, gate_stats) is written instead of dy -- vpt_conv_bwd_prep_kernel's pass over (dy, y) -> dacc
  // shrinks to a reduction over dacc0 alone; gate_u[f] += sum rstd0 * dy * xin (= rstd0 * sum dz v: T1's data term; closed gates add 0).
  constexpr bool GATE = MODE == 6;
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
  constexpr bool BWD = (MODE == 2 || MODE == 3 || MODE == 6), HAS_RES = (MODE == 1 || MODE == 3 || MODE == 5), POOL = (MODE == 4 || MODE == 7), RES_AFF = MODE == 5;
  // FWD16 (forward modes): main loop on v_mfma_f32_16x16x32.  Wave tile 8 pixel rows x 64 couts = 8 x 4 accumulators of 16 pixels x 16 couts;
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
  constexpr bool FWD16 = (MODE == 0 || MODE == 1 || MODE == 4 || MODE == 5 || MODE == 7);
  static_assert(FWD16 == !BWD, "forward modes: 16x16x32 loop and native-layout epilogue; dgrad modes: 32x32x16 loop and lane-swap epilogue");
  static_assert(!POOL || FWD16, "the pool-fused epilogue reads the 16x16 accumulators");
  constexpr bool DEFER_STORES = MODE != 3;   // mode 3 holds skip + xin pieces as well: no registers left for the packed results
  __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM_SZ];
  const int tid = threadIdx.x, lane = tid & 63;
  // profiling (vpt_conv3x3_set_trace): CU id + 100 MHz timestamps of the tile's phases
  int cu_key = -1;
  long long t_trace[3];
  if (TRACE && (FWD16 || tid == 0)) {   // (FWD16: wave-uniform, so the stamps stay in scalar registers across the main loop)
    t_trace[0] = wall_clock64();
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID: cu_id[11:8] sh_id[12] se_id[15:13]
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);   // HW_REG_XCC_ID[3:0]
    cu_key = (int)(((xcc & 15u) << 8) | ((hw >> 8) & 0xffu));
  }
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int hi = lane >> 5, l31 = lane & 31;
  const int tilesX = a.W >> 4, tilesY = a.H / TR;
  int L = xcd_remap(blockIdx.x, gridDim.x);
  const int nt = L % a.NT; L /= a.NT;
  const int tx = L % tilesX; L /= tilesX;
  const int ty = L % tilesY;
  const int f = L / tilesY;
  const int tx0 = tx * 16, ty0 = ty * TR;
  const int NCB = a.Cin >> 5;
  const int HW = a.H * a.W;

  // ---- halo staging map: chunk q -> (pixel P = 8*(q>>5) + (q&7), part = (q>>3)&3) ----
  int a_loff[NA];            // LDS byte offset, -1: no chunk (beyond the 324 halo pixels)
  unsigned a_gbyte[NA];      // byte offset inside one channel-block plane (clamped to 0 outside the image)
  unsigned a_inside = 0;    // bit m: chunk m lies inside the image (else literal zeros: the conv pads the NORMALISED tensor)
#pragma unroll
  for (int m = 0; m < NA; ++m) {
    const int q = tid + NTHR * m;
    // FWD16: the 8 lanes of a ds_write_b128 group carry 4 pixels of one parity x 2 parts (slots 2 k + part + const mod 8: all eight)
    const int P = FWD16 ? ((q >> 5) << 3) + 2 * (q & 3) + ((q >> 4) & 1) : ((q >> 5) << 3) + (q & 7);
    const int part = FWD16 ? 2 * ((q >> 3) & 1) + ((q >> 2) & 1) : (q >> 3) & 3;
    a_loff[m] = -1;
    a_gbyte[m] = 0u;
    if (P < HPIX) {
      const int hy = P / 18, hx = P - hy * 18;
      const int y = ty0 - 1 + hy, x = tx0 - 1 + hx;
      a_loff[m] = P * A_RS + part * 16 + (FWD16 ? 16 * (P & 1) : 0);
      if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
        a_gbyte[m] = (unsigned)((y * a.W + x) * 32 + part * 8) * 2u;
        a_inside |= 1u << m;
      }
    }
  }
  const op16_t* xplane = a.x + (size_t)f * NCB * HW * 32;
  // FWD16: chunk m of a thread lies NTHR / 4 halo pixels behind chunk m - 1 (same parity, same part): ONE address register and constant
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
  // Macros of BOTH main loops.  (All macros of the kernel are defined here, in three sections, and undefined together behind the epilogue
  // dispatch; they expand where they are used, so the names they mention are declared further down.)
  // ====================================================================================================================
#define SB() __builtin_amdgcn_sched_barrier(0)
#define NOP_() ((void)0)
  // weight DMA of one step (global -> LDS, no registers): ISSUE_B = all of a wave's pieces at once (prologue), GLDS = one piece in a slot of the loop
#define ISSUE_B(step_, buf_)                                                                              \
  do {                                                                                                    \
    const op16_t* wp_ = wbase + (size_t)(step_) * 12288;                                                  \
    _Pragma("unroll") for (int m_ = 0; m_ < NDMA; ++m_)                                                   \
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wp_ + m_ * (NWAVE * 512)),  \
                                       (__attribute__((address_space(3))) void*)(bdst + (buf_) * B_BYTES + m_ * (NWAVE * 1024)), \
                                       16, 0, 0);                                                         \
  } while (0)
#define GLDS(m_)                                                                                          \
  do { if ((m_) < NDMA)                                                                                   \
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wp_ + (m_) * (NWAVE * 512)),    \
                                   (__attribute__((address_space(3))) void*)(bd_ + (m_) * (NWAVE * 1024)), 16, 0, 0); } while (0)
  // halo chunk m_ of the next channel block, into its staging register
#define XA(m_) do { if ((m_) < NA) areg[m_] = *(const u32x4*)((const char*)xplane + (cbo_ + a_gbyte[m_])); } while (0)
  // The wait in front of a step's barrier is a COUNTED s_waitcnt: it retires the weight DMA and leaves the younger halo / residual loads in
  // flight across the barrier (a plain __syncthreads() drains vmcnt to 0 because an LDS-DMA is pending).  Memory operations are therefore
  // issued in a FIXED order and count per wave -- weight DMA (NDMA), then either the halo of the next block (NA, PRE_A) or, in the modes with
  // a residual, the first pieces of it (PRE_R).  Every counted load must be LIVE (a load whose result is unused is deleted by the compiler and
  // the count would then release the barrier early -- this bit once: the residual prefetch of a residual-free instantiation), hence the
  // compile-time HAS_RES in the steps.
#define WAIT_BARRIER(n_late_)                                                                             \
  do {                                                                                                    \
    asm volatile("s_waitcnt vmcnt(" #n_late_ ") lgkmcnt(0)" ::: "memory");                                \
    __builtin_amdgcn_s_barrier();                                                                         \
    asm volatile("" ::: "memory");                                                                        \
    SB();                                                                                                 \
  } while (0)

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

  // ====================================================================================================================
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
  float mean = 0.f, rstd = 1.f, c0f = 0.f, c1f = 0.f;
  const float* esa = a.edge_sa;
  if (!BWD) {
    if (a.kk_frame) {   // the epilogue table of THIS frame was prepared by vpt_nfold_coef_kernel (the input is a pooled tensor whose GroupNorm `n`
      rstd = a.rs_frame[f];                               // is folded into this layer): out = relu(rs * acc + kk_frame[f][e][o])
      esa = a.kk_frame + (size_t)f * 9 * a.CoutPad;
    } else {
      frame_mean_rstd(a.stats_in, f, a.inv_count_in, mean, rstd);
    }
  } else if (a.coef) {
    c0f = a.coef[2 * f];
    c1f = a.coef[2 * f + 1];
  }
  if constexpr (FWD16) {   // wave-uniform, but computed by vector instructions: held in a scalar register across the main loop
    rstd = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, rstd)));
    mean = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, mean)));
  }
  float rgate = 1.f;
  if (GATE) {      // everything the epilogue adds is linear in the scale: fold rstd0 into the coefficients
    float mg;
    frame_mean_rstd(a.gate_stats, f, a.inv_count_gate, mg, rgate);
    c0f *= rgate;
    c1f *= rgate;
  }
  {
    float* kk = (float*)(smem + KK_O);
    float ksa[NKK], ksg[NKK];
#pragma unroll
    for (int k = 0; k < NKK; ++k) {  // 9*128 = 4.5 * 256 entries: all the loads in flight together
      const int idx = tid + NTHR * k;
      const int o = (idx >> 7) * a.CoutPad + nt * 128 + (idx & 127);
      ksa[k] = (idx < 9 * 128 && !BWD) ? esa[o] : 0.f;
      ksg[k] = (idx < 9 * 128 && !BWD) ? a.edge_sg[o] : 0.f;
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
  } else if constexpr (FWD16) {
#pragma unroll
    for (int m = 0; m < NA; ++m) HALO_WR16(m);
  } else {
    WRITE_HALO();
  }
  __syncthreads();

  f32x16 acc[4][2];
  f32x16 ac[8];              // FWD16: [pixel row j of the wave's 8], elements 4 u .. 4 u + 3 = cout group u (ac_get / ac_set)
  f32x16 zero16;
#pragma unroll
  for (int r = 0; r < 16; ++r) zero16[r] = 0.f;

  // fragment base addresses
  const unsigned char* aL = smem + ((wm * 8 + sub_row(l31)) * 18 + (l31 & 15)) * A_RS + hi * 16;
  const int bsw = (l31 >> 2) & 3;
  const unsigned char* bL0 = smem + A_SZ + (wn * 64 + l31) * 64 + (((0 + hi) ^ bsw) << 4);  // ks = 0
  const unsigned char* bL1 = smem + A_SZ + (wn * 64 + l31) * 64 + (((2 + hi) ^ bsw) << 4);  // ks = 1

  // FWD16 fragment bases: lane = (MFMA column / row c16, K chunk q16)
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
  if constexpr (FWD16 && !HDMA) { asm volatile("" : "+v"(aLe), "+v"(aLo), "+v"(bW0), "+v"(bW1)); }
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
  // Forward epilogue: lane (c16, q16) owns bytes 16 q16 .. + 15 of pixel pcol(c16)'s 64-byte record in every (pixel row j, 32-cout block n2): residual and
  // output move as ONE 16-byte access per lane, 1024 contiguous bytes per instruction, in the accumulators' own layout.
  const unsigned voff16 = (unsigned)(((ty0 + wm * 8) * a.W + tx0 + pcol) * 32 + 8 * q16) * 2u;
  const unsigned gj_b = (unsigned)a.W * 64u;           // + j * gj_b: one image row further down (bytes)
  u32x4 rq16[8][2];                                    // residual [pixel row j][n2]

  // ---- main loop (the schedules are the CONV_STEP / CONV_STEP16 macros above) ----
  op16x8 fa[2][4], fb[2][2];   // dgrad: two fragment register sets
  const op16_t* resp = a.res;
  op16x8 fp[8], fw[2];         // forward: the current tap's 8 pixel fragments, a double-buffered weight fragment
  // forward weight DMA (GLDS16): resource over this channel tile's NCB * 9 packed tap tiles of 8 KB -- built from kernel arguments and the block index
  // only, so it lives in scalar registers; reads beyond it would return zeros (none: step s + 1 <= 3 NCB - 1 ends at the resource's last byte)
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.wpk + (size_t)nt * NCB * 9 * 4096), 0, NCB * 9 * 8192, 0x00020000);
  const int wvoff = (w * 64 + lane) * 16;

  if (TRACE && (FWD16 || tid == 0)) t_trace[1] = wall_clock64();
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
  } else if constexpr (FWD16) {
    if (CONV_ABLATE != 2) {
      WB(0, 0, 0);
#pragma unroll
      for (int j = 0; j < 8; ++j) PA(j, 0, 0);
      SB();
      // The accumulators start from zero: a peeled first channel block whose first tap takes C = 0 (as the 32x32 loop does) cost 27 spilled registers.
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
  } else if (CONV_ABLATE != 2) {
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
  if (TRACE && (FWD16 || tid == 0)) t_trace[2] = wall_clock64();
  if (CONV_ABLATE == 1) {  // profiling: keep the accumulators live, skip the epilogue
    float t = 0.f;
    if constexpr (FWD16) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) t += ac[j][r];
    } else {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) t += acc[m][n][r];
    }
    if (t == 12345.678f) a.y[0] = (vpt_op16)t;
    return;
  }
  if constexpr (FWD16) {
    if (HAS_RES && (TRACE || CONV_ABLATE == 2)) XR16(0);
  } else {
    if (HAS_RES && CONV_ABLATE == 2) { LOAD_RES(0); LOAD_RES(1); }
  }
  SB();

  f32x2 s_sum2 = {0.f, 0.f}, s_sq2 = {0.f, 0.f};   // packed fp32 (v_pk_add_f32 / v_pk_fma_f32): two values per VALU issue
  // Both epilogue bodies are instantiated for NV = 2 and NV = 1 valid 32-channel blocks of this wave (Cout / 32 odd) and selected by one
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
    u32x4 outv[8][2];          // packed results: all stores are issued after the last load has been consumed (see the dgrad epilogue)
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
  } else if constexpr (FWD16) {
    if (nvalid[1]) epilogue16(std::integral_constant<int, 2>{});
    else if (nvalid[0]) epilogue16(std::integral_constant<int, 1>{});
  } else {
    static_assert(BWD, "the 32x32 epilogue is written for the dgrad modes only");
    if (nvalid[1]) epilogue(std::integral_constant<int, 2>{});
    else if (nvalid[0]) epilogue(std::integral_constant<int, 1>{});
  }
  // both loops' macros
#undef SB
#undef NOP_
#undef ISSUE_B
#undef GLDS
#undef XA
#undef WAIT_BARRIER
  // the dgrad loop's
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
  // the forward loop's
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
  if (GATE) {      // one fp64 atomic per tile: this tile's share of sum rstd0 dy xin
    float* red = (float*)(smem + KK_O + KK_BYTES);
    s_sum = wave_sum(s_sum + s_sq);
    if (lane == 0) red[w] = s_sum;
    __syncthreads();
    if (tid == 0) atomicAdd(a.gate_u + f, (double)((red[0] + red[1]) + (red[2] + red[3])));
  }
  if (!BWD && a.stats_out) {
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

// ---------------------------------------------------------------------------------------------------------------------------
// Small-batch (acting path, agent.py:190-206: B = 1 .. 8 frames) instantiation: the SAME convolution, layouts and arithmetic, tiled
// for LATENCY.  One frame of the 2x model gives the throughput kernel above 16 / 8 / 2 workgroups per layer, each walking the whole
// K = 1152 ... 2304 chain alone (26-28 us per launch on 2-32 of 256 CUs: profiles/r02_t1_step_kernel_stats.csv).  Here a workgroup
// takes 16 x 16 pixels x 32 output channels (4x the workgroups) with EIGHT waves -- wave w = pixel rows 2w, 2w+1 = one 2 x 16-pixel
// subtile, 18 MFMAs per wave and channel block: an eighth of the throughput kernel's serial chain, and two waves per SIMD to hide
// each other's LDS round trips.  Halo and the 18 KB weight slice of a channel block
// are double-buffered in LDS (one workgroup per CU is plenty), one barrier per channel block, plain epilogue.  Same K order
// (channel block, kernel row, kernel column, 16-channel half) as the throughput kernel.
#define S_W_BYTES (9 * 32 * 64)                       // 18432: 9 taps x 32 couts x 32 cin
#define S_NBUF 3                                      // stages in LDS: the loads of channel block cb + 2 are in flight while cb computes
#define S_KK_OFF (S_NBUF * (A_BYTES + S_W_BYTES))     // 133056
#define S_BYTES (S_KK_OFF + 9 * 32 * 4 + 64)

template <bool HAS_RES>
__global__ __launch_bounds__(512, 1) void vpt_conv3x3_small_kernel(VptConv3x3Args a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[S_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  const int tilesX = a.W >> 4, tilesY = a.H >> 4;
  const int CB_out = a.Cout >> 5;
  int L = blockIdx.x;
  const int cbo = L % CB_out; L /= CB_out;
  const int tx = L % tilesX; L /= tilesX;
  const int ty = L % tilesY;
  const int f = L / tilesY;
  const int nt = cbo >> 2, qo = cbo & 3;
  const int tx0 = tx * 16, ty0 = ty * 16;
  const int NCB = a.Cin >> 5;
  const int HW = a.H * a.W;

  int a_loff[3];
  unsigned a_gbyte[3];
  unsigned a_inside = 0;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const int q = tid + 512 * m;
    const int P = ((q >> 5) << 3) + (q & 7), part = (q >> 3) & 3;
    a_loff[m] = -1;
    a_gbyte[m] = 0u;
    if (P < 324) {
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
  // weight slice of one channel block: 18 pieces of 1 KB (tap, 16-row half); wave w moves pieces w, w + 8, w + 16 (3 for waves 0 / 1,
  // 2 for the others).  A stage = those pieces by LDS-DMA + the halo's three 16-byte loads per lane into one of two register sets.
  const op16_t* wbase = a.wpk + (size_t)nt * NCB * 9 * 4096 + (size_t)(qo * 32) * 32 + (size_t)lane * 8;
  u32x4 areg[2][3];
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  unsigned char* const wlds = smem + S_NBUF * A_BYTES;
#define S_ISSUE(cb_, SET_)                                                                                \
  do {                                                                                                    \
    unsigned char* wd_ = wlds + ((cb_) % S_NBUF) * S_W_BYTES;                                             \
    _Pragma("unroll") for (int p_ = w; p_ < 18; p_ += 8)                                                  \
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wbase + ((size_t)(cb_) * 9 + (p_ >> 1)) * 4096 + (p_ & 1) * 512), \
                                       (__attribute__((address_space(3))) void*)(wd_ + (p_ >> 1) * 2048 + (p_ & 1) * 1024), 16, 0, 0); \
    _Pragma("unroll") for (int m_ = 0; m_ < 3; ++m_)                                                      \
      areg[SET_][m_] = *(const u32x4*)((const char*)xplane + ((size_t)(cb_) * HW * 64 + a_gbyte[m_]));    \
  } while (0)
#define S_WRITE_A(cb_, SET_)                                                                              \
  _Pragma("unroll") for (int m_ = 0; m_ < 3; ++m_)                                                        \
    if (a_loff[m_] >= 0) *(u32x4*)(smem + ((cb_) % S_NBUF) * A_BYTES + a_loff[m_]) = ((a_inside >> m_) & 1u) ? areg[SET_][m_] : zero4
  // counted wait: everything up to and including stage `older` has landed, the stage issued after it (if any) stays in flight.
  // Loads retire in issue order; a stage is 6 vector-memory instructions for waves 0 / 1 and 5 for the others.
#define S_WAIT_OLDER(YOUNGER_ISSUED)                                                                      \
  do {                                                                                                    \
    if (!(YOUNGER_ISSUED)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                               \
    else if (w < 2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");                                      \
    else asm volatile("s_waitcnt vmcnt(5)" ::: "memory");                                                 \
  } while (0)

  S_ISSUE(0, 0);
  if (NCB > 1) S_ISSUE(1, 1);
  float mean, rstd;
  frame_mean_rstd(a.stats_in, f, a.inv_count_in, mean, rstd);
  {
    float* kk = (float*)(smem + S_KK_OFF);
    for (int idx = tid; idx < 9 * 32; idx += 512) {
      const int o = (idx >> 5) * a.CoutPad + cbo * 32 + (idx & 31);
      kk[idx] = a.edge_sa[o] - rstd * mean * a.edge_sg[o];
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (the statistics / table loads above were issued after the stages: drain once)
  S_WRITE_A(0, 0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int bsw = (l31 >> 2) & 3;
  // iteration cb: issue stage cb + 2 (its halo into the register set stage cb used), compute stage cb, then move the halo of stage
  // cb + 1 -- issued one iteration EARLIER, so it has had two compute phases to land; the counted wait leaves stage cb + 2 in flight
  // -- from its registers into LDS for the next iteration.  One barrier per channel block.
  op16x8 sfb[3], sfa[3];
#define SB() __builtin_amdgcn_sched_barrier(0)
#define S_LOADG(g__)                                                                                      \
  do {                                                                                                    \
    const int gg_ = (g__);   /* a constant after unrolling: the register-set index gg_ % 3 must fold */ \
    const int tap_ = gg_ >> 1, ks_ = gg_ & 1, dy_ = tap_ / 3, dx_ = tap_ - 3 * dy_;                       \
    sfb[gg_ % 3] = *(const op16x8*)(bL + tap_ * 2048 + (((2 * ks_ + hi) ^ bsw) << 4));                    \
    sfa[gg_ % 3] = *(const op16x8*)(aL + (dy_ * 18 + dx_) * A_RS + ks_ * 32);                             \
  } while (0)
#define S_ITER(cb_, SET_)                                                                                 \
  do {                                                                                                    \
    const bool more_ = (cb_) + 2 < NCB;                                                                   \
    if (more_) S_ISSUE((cb_) + 2, SET_);                                                                  \
    const unsigned char* aL = smem + ((cb_) % S_NBUF) * A_BYTES + ((w * 2 + sub_row(l31)) * 18 + (l31 & 15)) * A_RS + hi * 16; \
    const unsigned char* bL = wlds + ((cb_) % S_NBUF) * S_W_BYTES + l31 * 64;                             \
    /* 18 groups (kernel row, kernel column, 16-channel half) of one weight fragment, one pixel fragment, one MFMA: the fragments \
       of group g + 2 are requested before the MFMA of group g issues (three register sets, order pinned; left alone the compiler \
       reads each group right before its use and waits for it). */ \
    S_LOADG(0); S_LOADG(1); SB();                                                                         \
    _Pragma("unroll") for (int g_ = 0; g_ < 18; ++g_) {                                                   \
      if (g_ + 2 < 18) { S_LOADG(g_ + 2); }                                                               \
      /* LDS reads return in order: group g_ has landed once at most the two younger groups' four reads are outstanding */ \
      if (g_ < 16) asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");                                     \
      else if (g_ == 16) asm volatile("s_waitcnt lgkmcnt(2)" ::: "memory");                               \
      else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                             \
      SB();                                                                                               \
      acc = VPT_MFMA_32X32X16(sfb[g_ % 3], sfa[g_ % 3], acc, 0, 0, 0);                                    \
      SB();                                                                                               \
    }                                                                                                     \
    if ((cb_) + 1 < NCB) {                                                                                \
      S_WAIT_OLDER(more_);                                                                                \
      S_WRITE_A((cb_) + 1, 1 - (SET_));                                                                   \
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                  \
    }                                                                                                     \
    __builtin_amdgcn_s_barrier();                                                                         \
    asm volatile("" ::: "memory");                                                                        \
  } while (0)
  for (int cb = 0; cb < NCB; cb += 2) {
    S_ITER(cb, 0);
    if (cb + 1 < NCB) S_ITER(cb + 1, 1);
  }
#undef S_ITER
#undef S_LOADG
#undef SB
#undef S_ISSUE
#undef S_WRITE_A
#undef S_WAIT_OLDER

  // ---- epilogue: GroupNorm fold + ReLU (+ residual), 8-byte pieces (4 consecutive output channels of one pixel), statistics ----
  const float* kk = (const float*)(smem + S_KK_OFF);
  float s_sum = 0.f, s_sq = 0.f;
  const size_t obase = (size_t)(f * CB_out + cbo) * HW * 32;
  {
    const int y = ty0 + w * 2 + sub_row(l31);
    const int x = tx0 + (l31 & 15);
    const int ey = (y == 0) ? 0 : ((y == a.H - 1) ? 2 : 1);
    const int ex = (x == 0) ? 0 : ((x == a.W - 1) ? 2 : 1);
    const float* ke = kk + (ey * 3 + ex) * 32 + 4 * hi;
    const size_t poff = obase + (size_t)(y * a.W + x) * 32 + 4 * hi;
    u32x2 r2[4];
    if (HAS_RES) {
#pragma unroll
      for (int g = 0; g < 4; ++g) r2[g] = *(const u32x2*)(a.res + poff + 8 * g);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 k4 = *(const f32x4*)(ke + 8 * g);
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = fmaxf(fmaf(rstd, acc[4 * g + j], k4[j]), 0.f);
      if (HAS_RES) {
        v[0] += op16_lo_to_f32(r2[g].x); v[1] += op16_hi_to_f32(r2[g].x);
        v[2] += op16_lo_to_f32(r2[g].y); v[3] += op16_hi_to_f32(r2[g].y);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) { s_sum += v[j]; s_sq = fmaf(v[j], v[j], s_sq); }
      const u32x2 pk = {pack_op16x2(v[0], v[1]), pack_op16x2(v[2], v[3])};
      *(u32x2*)(a.y + poff + 8 * g) = pk;
    }
  }
  if (a.stats_out) {
    float* red = (float*)(smem + S_KK_OFF + 9 * 32 * 4);
    s_sum = wave_sum(s_sum);
    s_sq = wave_sum(s_sq);
    if (lane == 0) { red[w] = s_sum; red[8 + w] = s_sq; }
    __syncthreads();
    if (tid == 0) {
      atomicAdd(a.stats_out + 2 * f, (double)(((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]))));
      atomicAdd(a.stats_out + 2 * f + 1, (double)(((red[8] + red[9]) + (red[10] + red[11])) + ((red[12] + red[13]) + (red[14] + red[15]))));
    }
  }
}

static long long* g_conv_trace = nullptr;
extern "C" void vpt_conv3x3_set_trace(void* buf) { g_conv_trace = (long long*)buf; }  // profiling: [grid][12] int64, or null

// which forward modes take the halo-DMA instantiation where the shape allows it: bit 0 = modes 0, 1, 5; bit 1 = the pool-fused mode 4
#define HALO_DMA_DEFAULT 3
static int g_conv_halo_dma = HALO_DMA_DEFAULT;
// tests and A/B measurements: 0 = the register-staged path everywhere, a negative value = the shipped selection; returns the previous mask
extern "C" int vpt_conv3x3_set_halo_dma(int mask) { const int was = g_conv_halo_dma; g_conv_halo_dma = mask < 0 ? HALO_DMA_DEFAULT : (mask & 3); return was; }

extern "C" int vpt_conv3x3_launch(const VptConv3x3Args* a_in, hipStream_t stream) {
  int ablate = 0, extra_lds = 0;
#ifdef VPT_CONV_PROFILE
  static int ablate_env = -1, extra_lds_env = 0;
  if (ablate_env < 0) {
    const char* e = getenv("VPT_CONV_ABLATE");
    ablate_env = e ? atoi(e) : 0;
    const char* xl = getenv("VPT_CONV_EXTRA_LDS");  // dynamic LDS bytes (> 2 KB forces one workgroup per CU)
    extra_lds_env = xl ? atoi(xl) : 0;
    if (extra_lds_env > 0) {
      (void)hipFuncSetAttribute((const void*)vpt_conv3x3_kernel<false, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, extra_lds_env);
      (void)hipFuncSetAttribute((const void*)vpt_conv3x3_kernel<false, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, extra_lds_env);
    }
  }
  ablate = ablate_env; extra_lds = extra_lds_env;
#endif
  VptConv3x3Args a_copy = *a_in;
  a_copy.ablate = ablate;
  a_copy.trace = g_conv_trace;
  const VptConv3x3Args* a = &a_copy;
  if ((a->H & 15) || (a->W & 15) || (a->Cin & 31) || (a->Cout & 31) || a->frames <= 0) return -1;
  const long grid = (long)a->frames * (a->H >> 4) * (a->W >> 4) * a->NT;
  if (grid > 0x7fffffffL) return -2;
  const int mode = a->bwd ? (a->res ? 3 : (a->gate_stats ? 6 : 2)) : (a->pool ? (a->pool_mask ? 7 : 4) : (a->res ? (a->res_bias ? 5 : 1) : 0));
  if (a->pool_mask && !a->pool) return -1;
  if (a->gate_stats && (!a->bwd || a->res || !a->gate_u || a->trace)) return -1;   // the gated dgrad: no skip connection (a block's conv1 -> conv0)
  if ((a->res_bias != nullptr) != (a->res_scale != nullptr) || (a->res_bias && (a->bwd || !a->res))) return -1;
  if ((a->kk_frame != nullptr) != (a->rs_frame != nullptr) || (a->kk_frame && a->bwd)) return -1;
  if (a->bwd && (!a->xin || !a->coef)) return -1;   // dgrad always carries the GroupNorm-statistics terms (c0 + c1 * xin)
  if (a->pool && (a->bwd || a->res || (a->tiling != 1 && a->tiling != 3) || a->trace || !a->seam_r || !a->seam_c)) return -1;
  // the latency tiling (32 output channels per workgroup) is the CALLER's choice, never the grid size's: a frame's result must not
  // depend on how many frames share the launch (the two tilings sum a tile's statistics in different orders)
  if (!a->bwd && a->tiling != 1 && a->tiling != 2 && a->tiling != 3) return -1;
  if (!a->bwd && !a->trace && a->tiling == 2) {
    const long sgrid = (long)a->frames * (a->H >> 4) * (a->W >> 4) * (a->Cout >> 5);
    if (a->res) hipLaunchKernelGGL((vpt_conv3x3_small_kernel<true>), dim3((unsigned)sgrid), dim3(512), 0, stream, *a);
    else hipLaunchKernelGGL((vpt_conv3x3_small_kernel<false>), dim3((unsigned)sgrid), dim3(512), 0, stream, *a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
  }
#define LAUNCH_(T_, M_) hipLaunchKernelGGL((vpt_conv3x3_kernel<T_, M_>), dim3((unsigned)grid), dim3(256), extra_lds, stream, *a)
  if (a->trace && mode > 3) return -1;
  if (mode == 6) { LAUNCH_(false, 6); return hipGetLastError() == hipSuccess ? 0 : -3; }
  // Halo DMA (HDMA): the 16-row forward modes on an even count of 32-channel blocks (a pass of its loop is two blocks) whose frame fits the
  // 2^30-byte offset range below H_OOB.  Everything else -- odd counts, tracing, profile builds with extra LDS -- runs the register-staged
  // instantiation, which is also the bitwise reference of tests/test_gpu_conv_halo_dma.py (vpt_conv3x3_set_halo_dma(0) sends every launch there).
  const bool hdma_shape = !a->bwd && !a->trace && !extra_lds && ((a->Cin >> 5) & 1) == 0 && (long long)(a->Cin >> 5) * a->H * a->W * 64 < (long long)H_OOB;
#define LAUNCHH_(M_) hipLaunchKernelGGL((vpt_conv3x3_kernel<false, M_, 16, true>), dim3((unsigned)grid), dim3(256), 0, stream, *a)
  // (mode 7, the pool-fused training forward with arg-max masks, lost 4 % on the K = 1152 layer under the new schedule and won 2.5 % on the K = 2304
  // one -- profiles/conv3x3_halo_dma.md -- so it keeps the register-staged instantiation)
  if (mode == 7) { LAUNCH_(false, 7); return hipGetLastError() == hipSuccess ? 0 : -3; }
  // tiling 3 (forward) = the 32-row, eight-wave tiles wherever the image has whole 32-row bands.  Measured at parity with the 16-row tiles on
  // every layer shape (profiles/r04_experiments.md section 7: halving the weight DMA buys nothing on a power-limited chip), so the shipped
  // choice stays the 16-row kernel; the variant is kept selectable because it is bit-identical per pixel and covered by the same tests.
  if (!a->trace && !a->bwd && mode != 4 && (a->H & 31) == 0 && a->tiling == 3 && !extra_lds) {
    const long g32 = grid >> 1;
#define LAUNCH32_(M_) hipLaunchKernelGGL((vpt_conv3x3_kernel<false, M_, 32>), dim3((unsigned)g32), dim3(512), 0, stream, *a)
    if (mode == 0) LAUNCH32_(0); else if (mode == 1) LAUNCH32_(1); else LAUNCH32_(5);
#undef LAUNCH32_
    return hipGetLastError() == hipSuccess ? 0 : -3;
  }
  if (hdma_shape && (((g_conv_halo_dma & 1) && (mode == 0 || mode == 1 || mode == 5)) || ((g_conv_halo_dma & 2) && mode == 4))) {
    if (mode == 0) LAUNCHH_(0); else if (mode == 1) LAUNCHH_(1); else if (mode == 4) LAUNCHH_(4); else LAUNCHH_(5);
    return hipGetLastError() == hipSuccess ? 0 : -3;
  }
#undef LAUNCHH_
  if (a->trace) { if (mode == 0) LAUNCH_(true, 0); else if (mode == 1) LAUNCH_(true, 1); else if (mode == 2) LAUNCH_(true, 2); else LAUNCH_(true, 3); }
  else { if (mode == 0) LAUNCH_(false, 0); else if (mode == 1) LAUNCH_(false, 1); else if (mode == 2) LAUNCH_(false, 2); else if (mode == 3) LAUNCH_(false, 3); else if (mode == 4) LAUNCH_(false, 4); else LAUNCH_(false, 5); }
#undef LAUNCH_
  return hipGetLastError() == hipSuccess ? 0 : -3;
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
