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
// What every mode of vpt_conv3x3_kernel (forward: vpt_conv3x3_fwd.hip) and vpt_conv3x3_dgrad_kernel (vpt_conv3x3_dgrad.hip) shares:
//   - Tile: one workgroup (4 waves: 2 row groups x 2 channel halves) = 16x16 output pixels x 128 output channels of one frame; a wave
//     owns 128 pixels x 64 couts.  Two workgroups per CU (78.6 KB LDS each, <= 256 VGPRs) hide each other's barriers and epilogues.
//   - LDS plan: [halo 18x18 pixels x 80-byte pitch][2 x 24 KB weight buffers][epilogue constant table 9 edge classes x 128 couts]
//     [block statistics][mode 5's residual bias].  Per 32-channel block the halo tile is register-staged into LDS once (zero-filled
//     outside the image) and reused by all nine taps.
//   - K step = one kernel row (3 taps) of one 32-channel block.  Its 24 KB weight tile is DMA'd global -> LDS (global_load_lds: no
//     VGPRs, no ds_write) into the double buffer one step ahead, so a step costs ONE barrier; the wait in front of the barrier is a
//     counted s_waitcnt that retires the DMA only and leaves the younger halo / residual loads in flight.
//   - The instruction order of a step is written out and pinned with sched_barrier (macros CONV_STEP / CONV_STEP16).
// How the kernel got here (the measurements behind each of these choices): DESIGN.md section 4, docs/history/, profiles/.
#pragma once
#include "vpt_common.h"
#include "vpt_kernels.h"
// Profiling switches (VPT_CONV_ABLATE = 1: skip the epilogue, 2: skip the main loop; VPT_CONV_EXTRA_LDS: dynamic LDS to force one
// workgroup per CU) exist ONLY in builds made with -DVPT_CONV_PROFILE (tools/build_variant.sh): the shipped library reads no
// environment variable and its kernel carries no ablation branch -- a stray variable cannot change results.
#ifdef VPT_CONV_PROFILE
#define CONV_ABLATE (a.ablate)
#else
#define CONV_ABLATE 0
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

// Tile decode: block index -> (channel tile nt, tile column tx, tile row ty, frame f), channel tiles fastest
struct VptConvTile { int nt, tx, ty, f; };
__device__ __forceinline__ VptConvTile conv_tile_decode(int NT, int tilesX, int tilesY) {
  int L = xcd_remap(blockIdx.x, gridDim.x);
  VptConvTile t;
  t.nt = L % NT; L /= NT;
  t.tx = L % tilesX; L /= tilesX;
  t.ty = L % tilesY;
  t.f = L / tilesY;
  return t;
}

// ====================================================================================================================
// Macros of BOTH main loops.  They expand where they are used, inside the kernels, so the names they mention (wbase, bdst, NDMA, NWAVE, NA, areg,
// xplane, a_gbyte, and the step's wp_, bd_, cbo_) are the kernel's own.
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
