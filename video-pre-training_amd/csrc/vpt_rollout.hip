// On-device rollout collection for RL fine-tuning (gfx950): what MinecraftAgentPolicy.act() hands out at one environment step goes into column t of
// [B][T] buffers that PPOTrainer reads as they are (rollout.py: RolloutBuffer).  No reference counterpart: the reference ships no RL loop.  No 16-bit
// operands: both operand formats build this file identically.
//
//  vpt_rollout_record_kernel : one acting step of B environments -> column t.  grid (ceil(frame_bytes / 4096), B) x 256 threads: every thread moves one
//                              16-byte vector of frame b (a 128 x 128 x 3 frame is 3072 of them: 12 workgroups per environment), no LDS; thread 0 of the
//                              workgroups with blockIdx.x == 0 writes environment b's five scalars.  The scalar inputs are read through element strides,
//                              so the views of vpt_act_epilogue's packed record (stride 4 int64 / 8 floats) go in without a copy.  A NaN log-prob stores 1
//                              to a one-byte sticky flag: a plain byte store, every writer writes the same value, nobody clears it here.
//  vpt_rollout_reward_kernel : after the environment has stepped, one lane per environment: the reward into column t, the running episode return and
//                              length advanced by ONE fp32 add / one integer increment, and -- where the next frame starts an episode -- the finished
//                              episode's totals into column t and the accumulators back to 0.  No cross-lane reduction: a float32 host loop
//                              (tests/rollout_ref.py) reproduces every value bit for bit; totals over a rollout are the caller's sums over done_*.
#include "vpt_common.h"
#include "vpt_kernels.h"

__global__ __launch_bounds__(256) void vpt_rollout_record_kernel(VptRolloutRecordArgs a) {
  const int b = blockIdx.y;
  const size_t col = (size_t)b * a.T + a.t;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < a.frame_vec) {
    const uint4* src = reinterpret_cast<const uint4*>(a.img) + (size_t)b * a.frame_vec;
    uint4* dst = reinterpret_cast<uint4*>(a.img_buf) + col * a.frame_vec;
    dst[i] = src[i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const float lp = a.log_prob[(size_t)b * a.stride_log_prob];
    a.first_buf[col] = a.first[b] ? 1 : 0;
    a.act_buttons_buf[col] = a.act_buttons[(size_t)b * a.stride_buttons];
    a.act_camera_buf[col] = a.act_camera[(size_t)b * a.stride_camera];
    a.old_log_prob_buf[col] = lp;
    a.vpred_buf[col] = a.vpred[(size_t)b * a.stride_vpred];
    if (lp != lp) *a.nan_flag = 1;
  }
}

extern "C" int vpt_rollout_record_launch(const VptRolloutRecordArgs* a, hipStream_t stream) {
  if (a->B <= 0 || a->T <= 0 || a->t < 0 || a->t >= a->T || a->frame_vec <= 0) return -1;
  const long gx = (a->frame_vec + 255) / 256;
  if (gx > 0x7fffffffL || a->B > 65535) return -2;
  hipLaunchKernelGGL(vpt_rollout_record_kernel, dim3((unsigned)gx, (unsigned)a->B), dim3(256), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

__global__ __launch_bounds__(256) void vpt_rollout_reward_kernel(VptRolloutRewardArgs a) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.B) return;
  const size_t col = (size_t)b * a.T + a.t;
  const float r = a.reward[b];
  const float ret = a.ep_return[b] + r;
  const int len = a.ep_length[b] + 1;
  const bool done = a.done[b] != 0;
  a.reward_buf[col] = r;
  a.done_return[col] = done ? ret : 0.f;
  a.done_length[col] = done ? len : 0;
  a.ep_return[b] = done ? 0.f : ret;
  a.ep_length[b] = done ? 0 : len;
}

extern "C" int vpt_rollout_reward_launch(const VptRolloutRewardArgs* a, hipStream_t stream) {
  if (a->B <= 0 || a->T <= 0 || a->t < 0 || a->t >= a->T) return -1;
  hipLaunchKernelGGL(vpt_rollout_reward_kernel, dim3((a->B + 255) / 256), dim3(256), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
