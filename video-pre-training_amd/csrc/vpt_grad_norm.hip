// Global l2 norm of all gradients and the clip coefficient, on the device (gfx950).
//
// Replaces th.nn.utils.clip_grad_norm_(params, MAX_GRAD_NORM) of behavioural_cloning.py:121 -- as the script MEANT it (upstream hands the call an
// exhausted generator, so it does nothing there; the trainers' default max_grad_norm=None reproduces that).  torch's route is a dozen foreach
// launches, a host synchronisation and a read-modify-write of every gradient; here the norm is ONE more read of the gradients over the table the
// Adam launch uses anyway, and the coefficient is one multiply inside that launch (vpt_adam_multi_kernel<true>): no scaling pass, no host round trip.
//
//   x = g * grad_scale;  q = x * x                                  fp32, no contraction
//   partial[b]   = sum of the 1024 squares of table block b          fp32, fixed tree: thread (4 sequential) -> xor butterfly -> (w0 + w1) + (w2 + w3)
//   tsum[t]      = sum of tensor t's partials                        fp64, fixed order (stage one, one workgroup per tensor)
//   total        = sum of tsum                                       fp64, fixed order (stage two, one workgroup)
//   norm_out[0]  = (float)sqrt(total)
//   norm_out[1]  = min((1 / (norm + 1e-6)) * max_norm, 1)            fp32, the operations of torch's clip_coef_clamped (max_norm / tensor is
//                                                                    reciprocal x scalar there); 1 when max_norm <= 0, 0 when total is not finite
//   norm_out[2]  = total not finite
// No float atomics, no "last workgroup" counters: every launch computes the same bits.  tests/grad_norm_ref.py restates all of it in numpy.
//
// Below the norm kernels, over the same table walk: vpt_grad_accumulate_kernel, the one-launch sum of a micro-batch's gradients into the window's
// accumulators (gradient accumulation).
#include "vpt_common.h"
#include "vpt_kernels.h"

#define VPT_GN_BLOCKS_PER_WG 4      // consecutive table blocks one workgroup walks: four independent 16-byte loads per lane in flight

__device__ __forceinline__ double gn_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the workgroup's 256 lanes in the fixed order butterfly -> (w0 + w1) + (w2 + w3); valid in thread 0
__device__ __forceinline__ double gn_block_sum_f64(double v, double* red) {
  v = gn_wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- the read of the gradients: one fp32 partial per 1024-element table block (same table and block mapping as vpt_adam_multi_kernel)
__global__ __launch_bounds__(256) void vpt_grad_norm_partial_kernel(const VptAdamTensor* __restrict__ table, int ntensors, long total_blocks,
                                                                    float grad_scale, float* __restrict__ partial, int* flag) {
#pragma clang fp contract(off)
  __shared__ float red[VPT_GN_BLOCKS_PER_WG][4];
  const long b0 = (long)blockIdx.x * VPT_GN_BLOCKS_PER_WG;
  const int tid = threadIdx.x;
  float g[VPT_GN_BLOCKS_PER_WG][4];
#pragma unroll
  for (int k = 0; k < VPT_GN_BLOCKS_PER_WG; ++k) {
    g[k][0] = g[k][1] = g[k][2] = g[k][3] = 0.f;
    const long b = b0 + k;
    if (b >= total_blocks) continue;       // uniform
    int lo = 0, hi = ntensors - 1;
    while (lo < hi) {   // last descriptor with first_block <= b
      const int mid = (lo + hi + 1) >> 1;
      if (table[mid].first_block <= b) lo = mid; else hi = mid - 1;
    }
    const float* tg = table[lo].g;
    const size_t n = table[lo].n;
    const size_t i0 = ((size_t)(b - table[lo].first_block) * 256 + tid) * 4;
    if (i0 + 4 <= n) {   // views may start at any element: unaligned dwordx4 is legal on gfx950 (vpt_adam_multi_kernel)
      const f32x4 v = *(const f32x4*)(tg + i0);
      g[k][0] = v.x; g[k][1] = v.y; g[k][2] = v.z; g[k][3] = v.w;
    } else {             // the tensor's last (partial) group of four, and the lanes past n: exact zeros
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + j < n) g[k][j] = tg[i0 + j];
    }
  }
  bool bad = false;
  float s[VPT_GN_BLOCKS_PER_WG];
#pragma unroll
  for (int k = 0; k < VPT_GN_BLOCKS_PER_WG; ++k) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float r = g[k][j];
      bad |= !((r - r) == 0.f);            // x - x is 0 for finite x and nan for inf / nan (vpt_grads_nonfinite_kernel)
      const float x = r * grad_scale;
      const float q = x * x;
      acc = (j == 0) ? q : acc + q;        // the thread's four squares, sequentially
    }
    s[k] = wave_sum(acc);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < VPT_GN_BLOCKS_PER_WG; ++k) red[k][tid >> 6] = s[k];
  }
  if (flag && __any(bad) && (tid & 63) == 0) *flag = 1;      // only ever set (the caller zeroes it)
  __syncthreads();
  if (tid < VPT_GN_BLOCKS_PER_WG && b0 + tid < total_blocks)
    partial[b0 + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// ---- finish, stage one: tensor t's partials in fp64 -- thread i adds partials i, i + 256, ... in that order, then the fixed tree
__global__ __launch_bounds__(256) void vpt_grad_norm_tensor_kernel(const VptAdamTensor* __restrict__ table, const float* __restrict__ partial,
                                                                   double* __restrict__ tsum, float* per_tensor) {
  __shared__ double red[4];
  const VptAdamTensor t = table[blockIdx.x];
  const long nb = (long)((t.n + 1023) >> 10);
  const float* p = partial + t.first_block;
  double acc = 0.0;
  for (long i = threadIdx.x; i < nb; i += 256) acc += (double)p[i];
  const double tot = gn_block_sum_f64(acc, red);
  if (threadIdx.x == 0) {
    tsum[blockIdx.x] = tot;
    if (per_tensor) per_tensor[blockIdx.x] = (float)sqrt(tot);
  }
}

// ---- finish, stage two: the tensors' sums in table order per thread, the fixed tree, the norm and the coefficient
__global__ __launch_bounds__(256) void vpt_grad_norm_finish_kernel(const double* __restrict__ tsum, int ntensors, float max_norm, float* norm_out, int* flag) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < ntensors; i += 256) acc += tsum[i];
  const double tot = gn_block_sum_f64(acc, red);
  if (threadIdx.x != 0) return;
  const bool finite = (tot - tot) == 0.0;
  const float norm = (float)sqrt(tot);
  float coef = 1.0f;
  if (max_norm > 0.f) coef = fminf((1.0f / (norm + 1e-6f)) * max_norm, 1.0f);
  norm_out[0] = norm;
  norm_out[1] = finite ? coef : 0.0f;      // nothing downstream ever multiplies by nan
  norm_out[2] = finite ? 0.0f : 1.0f;
  norm_out[3] = 0.0f;
  if (flag && !finite) *flag = 1;
}

// ---- gradient accumulation over micro-batches: p[i] = p[i] + g[i] for every tensor of the table in ONE launch (p: the fp32 accumulator, g: the
// addend; m and v are not read).  The table walk and block mapping of the norm kernel above: VPT_GN_BLOCKS_PER_WG consecutive 1024-element blocks per
// workgroup, all their 16-byte loads issued before the first store.  One fp32 add per element, no reductions, no atomics: the same inputs give the
// same bits, inf / nan go through the sum (the norm launch / overflow check in front of the Adam launch sees them).  Only [p, p + n) is written.
__global__ __launch_bounds__(256) void vpt_grad_accumulate_kernel(const VptAdamTensor* __restrict__ table, int ntensors, long total_blocks) {
  const long b0 = (long)blockIdx.x * VPT_GN_BLOCKS_PER_WG;
  const int tid = threadIdx.x;
  float* tp[VPT_GN_BLOCKS_PER_WG];
  size_t rem[VPT_GN_BLOCKS_PER_WG];        // elements of the tensor from this lane's first one on (0: nothing to do)
  float a[VPT_GN_BLOCKS_PER_WG][4], g[VPT_GN_BLOCKS_PER_WG][4];
#pragma unroll
  for (int k = 0; k < VPT_GN_BLOCKS_PER_WG; ++k) {
    tp[k] = nullptr; rem[k] = 0;
    a[k][0] = a[k][1] = a[k][2] = a[k][3] = 0.f;
    g[k][0] = g[k][1] = g[k][2] = g[k][3] = 0.f;
    const long b = b0 + k;
    if (b >= total_blocks) continue;       // uniform
    int lo = 0, hi = ntensors - 1;
    while (lo < hi) {   // last descriptor with first_block <= b
      const int mid = (lo + hi + 1) >> 1;
      if (table[mid].first_block <= b) lo = mid; else hi = mid - 1;
    }
    const size_t n = table[lo].n;
    const size_t i0 = ((size_t)(b - table[lo].first_block) * 256 + tid) * 4;
    if (i0 >= n) continue;
    tp[k] = table[lo].p + i0;
    rem[k] = n - i0;
    const float* tg = table[lo].g + i0;
    if (rem[k] >= 4) {   // views may start at any element: unaligned dwordx4 is legal on gfx950 (vpt_adam_multi_kernel)
      const f32x4 va = *(const f32x4*)tp[k], vg = *(const f32x4*)tg;
      a[k][0] = va.x; a[k][1] = va.y; a[k][2] = va.z; a[k][3] = va.w;
      g[k][0] = vg.x; g[k][1] = vg.y; g[k][2] = vg.z; g[k][3] = vg.w;
    } else {             // the tensor's last (partial) group of four
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if ((size_t)j < rem[k]) { a[k][j] = tp[k][j]; g[k][j] = tg[j]; }
    }
  }
#pragma unroll
  for (int k = 0; k < VPT_GN_BLOCKS_PER_WG; ++k) {
    if (rem[k] >= 4) {
      f32x4 s;
      s.x = a[k][0] + g[k][0]; s.y = a[k][1] + g[k][1]; s.z = a[k][2] + g[k][2]; s.w = a[k][3] + g[k][3];
      *(f32x4*)tp[k] = s;
    } else {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if ((size_t)j < rem[k]) tp[k][j] = a[k][j] + g[k][j];
    }
  }
}

extern "C" int vpt_grad_accumulate_launch(const VptAdamTensor* table_dev, int ntensors, long total_blocks, hipStream_t stream) {
  if (ntensors <= 0 || total_blocks <= 0) return 0;
  const long wgs = (total_blocks + VPT_GN_BLOCKS_PER_WG - 1) / VPT_GN_BLOCKS_PER_WG;
  if (wgs > 0x7fffffffL) return -2;
  hipLaunchKernelGGL(vpt_grad_accumulate_kernel, dim3((unsigned)wgs), dim3(256), 0, stream, table_dev, ntensors, total_blocks);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" long vpt_grad_norm_workspace_floats(int ntensors, long total_blocks) {
  if (ntensors < 0 || total_blocks < 0) return -1;
  return 2L * ntensors + total_blocks;      // [ntensors] fp64 tensor sums first (8-byte aligned), then [total_blocks] fp32 partials
}

extern "C" int vpt_grad_norm_launch(const VptAdamTensor* table_dev, int ntensors, long total_blocks, float grad_scale, float max_norm,
                                    float* workspace, float* norm_out, float* per_tensor, int* flag, hipStream_t stream) {
  if (ntensors <= 0 || total_blocks < 0) return -1;
  const long wgs = (total_blocks + VPT_GN_BLOCKS_PER_WG - 1) / VPT_GN_BLOCKS_PER_WG;
  if (wgs > 0x7fffffffL) return -2;
  double* tsum = (double*)workspace;
  float* partial = workspace + 2L * ntensors;
  if (wgs > 0)
    hipLaunchKernelGGL(vpt_grad_norm_partial_kernel, dim3((unsigned)wgs), dim3(256), 0, stream, table_dev, ntensors, total_blocks, grad_scale, partial, flag);
  hipLaunchKernelGGL(vpt_grad_norm_tensor_kernel, dim3((unsigned)ntensors), dim3(256), 0, stream, table_dev, (const float*)partial, tsum, per_tensor);
  hipLaunchKernelGGL(vpt_grad_norm_finish_kernel, dim3(1), dim3(256), 0, stream, (const double*)tsum, ntensors, max_norm, norm_out, flag);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
