// One output pixel of the sequence-consistent frame augmentation: the arithmetic of vpt_augment_frames_kernel, in one
// function that the device kernel (vpt_augment.hip) and a plain host program (tools/augment_host_check.cpp, built with the address and undefined-behaviour
// sanitizers) both compile.  tests/augment_ref.py restates it element-wise in float32 numpy; the three agree bit for bit.
//
// Table of a frame, 16 fp32: colour matrix C[3][3] row-major (0..8), mean gain k (9), inverse map G[2][3] (10..15).  G takes an OUTPUT pixel index
// (x, y) to a SOURCE pixel index; every centre convention is folded into it by the table builder (augment.py), this code knows none.
//     sx = (G00 x + G01 y) + G02,  sy = (G10 x + G11 y) + G12;  x0 = floor(sx), fx = sx - x0 (y alike)
//     v_c = ((1-fy)(1-fx) t00 + (1-fy) fx t01) + (fy (1-fx) t10 + fy fx t11)        taps outside the frame are 0 ("zeros" padding, in source space)
//     o_c = ((C[c][0] v_0 + C[c][1] v_1) + C[c][2] v_2) + k mu;   out = (uint8) rint(min(max(o_c, 0), 255))   (round half to even)
// Every product and sum is rounded on its own (no fused multiply-add) in exactly this association.
//
// The range test of a tap is made on the FLOAT coordinate, before any conversion to an integer: NaN, +-Inf and huge finite coordinates fail it and
// the tap is 0, so no table contents can make this function read outside [frame, frame + H*W*3).  A NaN result clamps to 0.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__)           // compiled as HIP (the library); a plain C++ compile (the host check) takes the other branch
#define VPT_AUG_HD __host__ __device__ __forceinline__
#else
#define VPT_AUG_HD static inline
#endif

#define VPT_AUG_TABLE_FLOATS 16
#define VPT_AUG_MAX_FRAME_BYTES 65536      // the frame is staged whole in LDS; the integer luma sum fits int32 up to here

#pragma clang fp contract(off)

// luma weights of the frame mean: (77 R + 150 G + 29 B) / 256
#define VPT_AUG_LUMA_R 77
#define VPT_AUG_LUMA_G 150
#define VPT_AUG_LUMA_B 29

// mean luma of a frame from its exact integer sum; inv = (float)(1.0 / (256.0 * H * W))
VPT_AUG_HD float vpt_augment_mean(int lum, float inv) { return (float)lum * inv; }

// index products (row * W, pixel * 3): the factors are non-negative and the product is below 2^16, so the 24-bit multiply -- full rate on the device,
// where the 32-bit one is not -- is exact
#if defined(__HIP_DEVICE_COMPILE__)
#define VPT_AUG_MUL24(a, b) __mul24((a), (b))
#else
#define VPT_AUG_MUL24(a, b) ((a) * (b))
#endif

// a coordinate's range test, on the float: NaN compares false
VPT_AUG_HD bool vpt_augment_inside(float v, int n) { return v >= 0.0f && v < (float)n; }
// the index of an in-range coordinate; 0 for one that failed the test: only in-range values are converted to integers
VPT_AUG_HD int vpt_augment_index(float v, bool ok) { return (int)(ok ? v : 0.0f); }

// The three channels of the source pixel `pixel` (row * W + column, both clamped into the frame), or the fill when the tap failed its range test.
// Branch-free: a failed tap still reads a pixel inside the frame and is then replaced.  (With a branch around the loads the four taps of a pixel
// become four dependent regions on the device, each waiting for its own LDS loads.)
VPT_AUG_HD void vpt_augment_tap(const uint8_t* frame, int pixel, bool ok, float* t) {
  const uint8_t* p = frame + VPT_AUG_MUL24(pixel, 3);
  const float a = (float)p[0], b = (float)p[1], c = (float)p[2];
  t[0] = ok ? a : 0.0f; t[1] = ok ? b : 0.0f; t[2] = ok ? c : 0.0f;
}

VPT_AUG_HD uint8_t vpt_augment_quantize(float o) {
  float m = o > 0.0f ? o : 0.0f;        // NaN -> 0
  m = m < 255.0f ? m : 255.0f;
  return (uint8_t)(int)rintf(m);
}

VPT_AUG_HD void vpt_augment_pixel(const uint8_t* frame, int H, int W, const float* tbl, float mu, int x, int y, uint8_t* out3) {
  const float xf = (float)x, yf = (float)y;
  const float off = tbl[9] * mu;
  const float sx = (tbl[10] * xf + tbl[11] * yf) + tbl[12];
  const float sy = (tbl[13] * xf + tbl[14] * yf) + tbl[15];
  const float xl = floorf(sx), yl = floorf(sy);
  const float fx = sx - xl, fy = sy - yl;
  const float xh = xl + 1.0f, yh = yl + 1.0f;
  const float gy = 1.0f - fy, gx = 1.0f - fx;
  const float w00 = gy * gx, w01 = gy * fx, w10 = fy * gx, w11 = fy * fx;
  float t00[3], t01[3], t10[3], t11[3], v[3];
  const bool oxl = vpt_augment_inside(xl, W), oxh = vpt_augment_inside(xh, W), oyl = vpt_augment_inside(yl, H), oyh = vpt_augment_inside(yh, H);
  const int cl = vpt_augment_index(xl, oxl), ch = vpt_augment_index(xh, oxh);
  const int rl = VPT_AUG_MUL24(vpt_augment_index(yl, oyl), W), rh = VPT_AUG_MUL24(vpt_augment_index(yh, oyh), W);
  vpt_augment_tap(frame, rl + cl, oyl && oxl, t00);
  vpt_augment_tap(frame, rl + ch, oyl && oxh, t01);
  vpt_augment_tap(frame, rh + cl, oyh && oxl, t10);
  vpt_augment_tap(frame, rh + ch, oyh && oxh, t11);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = (w00 * t00[c] + w01 * t01[c]) + (w10 * t10[c] + w11 * t11[c]);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float o = ((tbl[3 * c] * v[0] + tbl[3 * c + 1] * v[1]) + tbl[3 * c + 2] * v[2]) + off;
    out3[c] = vpt_augment_quantize(o);
  }
}
