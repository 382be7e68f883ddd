// Sequence-consistent image augmentation on the device (gfx950): a chunk of uint8 frames [F][H][W][3] -> augmented uint8 frames in one
// launch -- colour (hue, saturation, brightness, contrast about the frame's mean luma) and a small affine warp with bilinear taps and zero fill.  The
// transform of a frame is a 16-float table (vpt_augment_pixel.h) that the host side builds from nine uniforms per frame (augment.py: torch ops in float64;
// no double-precision sin / cos in a kernel, whose argument reduction may bring a private array, i.e. scratch).  vpt_augment_uniforms_kernel draws those
// uniforms from Philox4x32-10 keyed by (seed; draw group, recording key, epoch): frames of one recording get one transform by construction, also across
// chunk edges.
//
// vpt_augment_frames_kernel: one workgroup of 256 threads per frame.
//   1. the frame is staged whole in LDS (H*W*3 <= 65536 bytes; 48 KB at the policy's 128 x 128: three workgroups per CU) with 16-byte loads over the
//      16-byte-aligned middle of the frame and byte loads for the unaligned head and tail (a 5 x 7 frame is 105 bytes: frame 1 of a batch starts
//      unaligned).  The LDS copy starts at the global address's offset within 16 bytes, so an aligned global chunk is an aligned LDS chunk.
//   2. the integer luma sum 77 R + 150 G + 29 B is taken from the loaded registers (v_dot4_u32_u8 against the weight pattern of the chunk's phase mod 3),
//      reduced per wave and through four LDS partials: integer, hence exact and order-free; no atomics.
//   3. after the barrier each thread produces 16 consecutive output bytes at a 16-byte-aligned address -- the six pixels that hold them, from LDS taps,
//      packed and shifted to the vector's phase within a pixel -- and stores them as one vector; the unaligned head and the tail go through a byte path.
// The kernel is bound by its vector arithmetic, not by HBM or LDS: 782 VALU instructions per loop pass of six pixel evaluations (per pixel: the range
// tests, twelve byte-to-float conversions and selects, the bilinear and colour sums), four cycles each for a wave of 64, account for the measured time --
// 3.25 x a copy of the same frames at 64 x 128 frames (profiles/augment.md).  A variant with one output dword per lane (taps of neighbouring lanes on
// neighbouring LDS banks, two pixel evaluations per 4 bytes instead of six per 16) was slower in the proportion of its pixel evaluations, 8 : 6.
// HBM traffic: one read and one write of the frame.  The whole frame is in LDS before the first store, and a workgroup touches its own frame only, so
// `dst` may be `src` itself (in place); partially overlapping buffers are not supported.
// Plain HIP: no MFMA, no inline assembly.  All floating-point arithmetic is in vpt_augment_pixel.h, under `fp contract(off)`.
#include "vpt_common.h"
#include "vpt_kernels.h"
#include "vpt_augment_pixel.h"

#pragma clang fp contract(off)

#define AUG_THREADS 256
// The thread-strided loops below are neither vectorised nor unrolled by the compiler: a byte path of at most 30 bytes gains nothing, and the vectorised
// form of the pixel function brought packed fp32 adds across register halves (build.py: EXTRA_FLAGS) and SGPR spills.
#define AUG_LDS_EXTRA (16 + 16)                       // the frame's offset within 16 bytes; the four wave partials
#define AUG_LDS_MAX (VPT_AUG_MAX_FRAME_BYTES + AUG_LDS_EXTRA)

// luma weights of the four bytes of a dword whose first byte is channel p of a pixel: w[p], w[p+1], w[p+2], w[p] (indices mod 3)
__device__ __forceinline__ uint32_t aug_luma_weights(int p) {
  const uint32_t r = VPT_AUG_LUMA_R, g = VPT_AUG_LUMA_G, b = VPT_AUG_LUMA_B;
  const uint32_t w0 = r | (g << 8) | (b << 16) | (r << 24), w1 = g | (b << 8) | (r << 16) | (g << 24), w2 = b | (r << 8) | (g << 16) | (b << 24);
  return p == 0 ? w0 : (p == 1 ? w1 : w2);
}
__device__ __forceinline__ int aug_mod3_next(int p) { return p == 2 ? 0 : p + 1; }

__global__ __launch_bounds__(AUG_THREADS) void vpt_augment_frames_kernel(const uint8_t* src, const float* __restrict__ tables, uint8_t* dst, int nb, int H,
                                                                         int W, float inv) {
  extern __shared__ __attribute__((aligned(16))) uint8_t aug_lds_[];
  const int tid = threadIdx.x;
  const size_t f = blockIdx.x;
  const uint8_t* g = src + f * (size_t)nb;
  const int sh = (int)((uintptr_t)g & 15);
  uint8_t* lf = aug_lds_ + sh;                                          // LDS copy of the frame: lf[i] = g[i], same alignment within 16 bytes
  int* partial = (int*)(aug_lds_ + ((nb + 15 + 15) & ~15));              // behind the frame, 16-byte aligned: offset <= 65536 + 16

  // the frame's table: a workgroup-uniform address, i.e. scalar loads into SGPRs
  float tb[VPT_AUG_TABLE_FLOATS];
#pragma unroll
  for (int i = 0; i < VPT_AUG_TABLE_FLOATS; ++i) tb[i] = tables[f * VPT_AUG_TABLE_FLOATS + i];

  // ---- 1 + 2: stage the frame, sum its luma -------------------------------------------------------------------------------------------------
  const int head = min(nb, (16 - sh) & 15);
  const int nvec = (nb - head) >> 4;
  const int tail0 = head + (nvec << 4);                                 // first byte behind the vector part
  uint32_t lum = 0;
#pragma clang loop vectorize(disable) unroll(disable)
  for (int j = tid; j < nvec; j += AUG_THREADS) {
    const int o = head + (j << 4);
    const u32x4 d = *(const u32x4*)(g + o);
    *(u32x4*)(lf + o) = d;
    const int p0 = o % 3, p1 = aug_mod3_next(p0), p2 = aug_mod3_next(p1);      // a dword is 4 = 1 (mod 3) bytes on
    lum = __builtin_amdgcn_udot4(d.x, aug_luma_weights(p0), lum, false);
    lum = __builtin_amdgcn_udot4(d.y, aug_luma_weights(p1), lum, false);
    lum = __builtin_amdgcn_udot4(d.z, aug_luma_weights(p2), lum, false);
    lum = __builtin_amdgcn_udot4(d.w, aug_luma_weights(p0), lum, false);
  }
#pragma clang loop vectorize(disable) unroll(disable)
  for (int i = tid; i < head + (nb - tail0); i += AUG_THREADS) {
    const int o = i < head ? i : tail0 + (i - head);
    const uint32_t b = g[o];
    lf[o] = (uint8_t)b;
    lum += b * (aug_luma_weights(o % 3) & 0xffu);
  }
  int s = (int)lum;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((tid & 63) == 0) partial[tid >> 6] = s;
  __syncthreads();                                                      // the frame is whole in LDS: from here on `dst` may be written, also when it is `src`
  const float mu = vpt_augment_mean((partial[0] + partial[1]) + (partial[2] + partial[3]), inv);

  // ---- 3: output ------------------------------------------------------------------------------------------------------------------------------
  uint8_t* gd = dst + f * (size_t)nb;
  const int dh = min(nb, (16 - (int)((uintptr_t)gd & 15)) & 15);        // bytes before the first 16-byte-aligned output address
  const int nout = (nb - dh) >> 4;
  const int dt0 = dh + (nout << 4);
#pragma clang loop vectorize(disable) unroll(disable)
  for (int j = tid; j < nout; j += AUG_THREADS) {
    // output bytes [o, o + 16) lie in the six pixels q0 .. q0 + 5 (18 bytes from byte 3 q0 = o - pa on; pa + 16 <= 18), all of them inside the frame
    const int o = dh + (j << 4);
    const int q0 = o / 3, pa = o - 3 * q0;
    int y = q0 / W, x = q0 - y * W;
    uint32_t S[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      uint8_t px[3];
      vpt_augment_pixel(lf, H, W, tb, mu, x, y, px);
#pragma unroll
      for (int c = 0; c < 3; ++c) S[(3 * i + c) >> 2] |= (uint32_t)px[c] << (8 * ((3 * i + c) & 3));
      if (++x == W) { x = 0; ++y; }
    }
    u32x4 d;                                                            // the 20 bytes shifted down by pa
    d.x = __builtin_amdgcn_alignbyte(S[1], S[0], (uint32_t)pa);
    d.y = __builtin_amdgcn_alignbyte(S[2], S[1], (uint32_t)pa);
    d.z = __builtin_amdgcn_alignbyte(S[3], S[2], (uint32_t)pa);
    d.w = __builtin_amdgcn_alignbyte(S[4], S[3], (uint32_t)pa);
    *(u32x4*)(gd + o) = d;
  }
#pragma clang loop vectorize(disable) unroll(disable)
  for (int i = tid; i < dh + (nb - dt0); i += AUG_THREADS) {           // byte path: at most 15 + 15 bytes
    const int o = i < dh ? i : dt0 + (i - dh);
    const int q = o / 3, c = o - 3 * q;
    const int y = q / W, x = q - y * W;
    uint8_t px[3];
    vpt_augment_pixel(lf, H, W, tb, mu, x, y, px);
    gd[o] = c == 0 ? px[0] : (c == 1 ? px[1] : px[2]);
  }
}

// out[f][d], d = 0..8: uniform d of the frame with key keys[f]: Philox4x32-10, key (seed lo, seed hi), counter (d >> 2, key lo, key hi, epoch), word d & 3,
// u = (word >> 8) * 2^-24.  One thread per (frame, group of four draws).
__global__ __launch_bounds__(256) void vpt_augment_uniforms_kernel(const int64_t* __restrict__ keys, float* __restrict__ out, long frames, uint64_t seed,
                                                                   uint32_t epoch) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= frames * 3) return;
  const long f = i / 3;
  const int grp = (int)(i - f * 3);
  const uint64_t k = (uint64_t)keys[f];
  uint32_t w[4];
  philox4x32_10((uint32_t)grp, (uint32_t)k, (uint32_t)(k >> 32), epoch, (uint32_t)seed, (uint32_t)(seed >> 32), w);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (4 * grp + j < 9) out[f * 9 + 4 * grp + j] = (float)(w[j] >> 8) * (1.0f / 16777216.0f);
}

extern "C" int vpt_augment_uniforms_launch(const int64_t* keys, float* out, long frames, uint64_t seed, uint32_t epoch, hipStream_t stream) {
  if (frames <= 0 || !keys || !out) return -1;
  const long grid = (frames * 3 + 255) / 256;
  if (grid > 0x7fffffffL) return -2;
  hipLaunchKernelGGL(vpt_augment_uniforms_kernel, dim3((unsigned)grid), dim3(256), 0, stream, keys, out, frames, seed, epoch);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int vpt_augment_frames_launch(const uint8_t* src, const float* tables, uint8_t* dst, long frames, int H, int W, hipStream_t stream) {
  if (frames <= 0 || H <= 0 || W <= 0 || !src || !tables || !dst) return -1;
  if ((long)H * W * 3 > VPT_AUG_MAX_FRAME_BYTES) return -5;           // the frame does not fit the LDS staging
  if (frames > 0x7fffffffL) return -2;
  const int nb = H * W * 3;
  static unsigned long long optin_done = 0;
  if (!vpt_lds_optin((const void*)vpt_augment_frames_kernel, AUG_LDS_MAX, &optin_done)) return -4;
  const int lds = ((nb + 15 + 15) & ~15) + 16;
  const float inv = (float)(1.0 / (256.0 * (double)H * (double)W));
  hipLaunchKernelGGL(vpt_augment_frames_kernel, dim3((unsigned)frames), dim3(AUG_THREADS), lds, stream, src, tables, dst, nb, H, W, inv);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
