// Merge of a low-rank update into an fp32 master weight (gfx950):
//     out[i][k] = W[i][k] + s * sum_j B[i][j] * A[j][k]        W, out fp32 [n][K],  B fp32 [n][r],  A fp32 [r][K],  1 <= r <= 64
// in fp32, j ascending, as a FIXED sequence of single roundings: p_j = B[i][j] * A[j][k] (one rounding), acc = acc + p_j from acc = 0 (one
// rounding each), then W + (s * acc) (two roundings).  Contraction is off for the whole file, so no multiply is ever fused into the add that
// follows it and a float32 numpy restatement of these lines (tests/lowrank_ref.merge_f32) equals the kernel bit for bit.
// LowRankAdapters.merge_ / merged_state_dict use it instead of an addmm, whose summation order nobody pins.
// One thread per output element, k fastest: W, A's row j and out are read / written as consecutive dwords by consecutive lanes; a workgroup
// stays inside one row i (blockIdx.y), so B[i][j] is one address per wave.  No LDS, no atomics.  out may be W itself: an element is read and
// written by the same thread only.
#include "vpt_common.h"
#include "vpt_kernels.h"

#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void vpt_lowrank_merge_kernel(const float* W, const float* __restrict__ A, const float* __restrict__ B, float* out,
                                                                int n, int K, int r, float s) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  for (int i = blockIdx.y; i < n; i += gridDim.y) {
    const float* b = B + (size_t)i * r;
    float acc = 0.f;
    for (int j = 0; j < r; ++j) {
      const float p = b[j] * A[(size_t)j * K + k];
      acc = acc + p;
    }
    const float u = s * acc;
    out[(size_t)i * K + k] = W[(size_t)i * K + k] + u;
  }
}

extern "C" int vpt_lowrank_merge_launch(const float* W, const float* A, const float* B, float* out, int n, int K, int r, float s, hipStream_t stream) {
  if (!W || !A || !B || !out || n <= 0 || K <= 0 || r < 1 || r > 64) return -1;
  if (A == out || B == out) return -1;
  const unsigned gy = n < 65535 ? (unsigned)n : 65535u;
  hipLaunchKernelGGL(vpt_lowrank_merge_kernel, dim3((unsigned)((K + 255) / 256), gy), dim3(256), 0, stream, W, A, B, out, n, K, r, s);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
