// Reinforcement-learning fine-tuning of the cloned policy (gfx950), fp32: the third stage of the VPT method (the reference ships no RL training
// script; the pieces it does ship are the heads' logprob / entropy / kl_divergence, lib/action_head.py:176-203,252-275, and the value head's loss in
// normalised space, lib/scaled_mse_head.py:37-43 with lib/normalize_ewma.py:33-55).
//
//  vpt_rl_loss_kernel : clipped policy gradient + KL to a frozen prior + entropy bonus + value loss of one frame per workgroup, in vpt_bc_loss_kernel's
//                       form: the gradient dz w.r.t. the fused head logits, a per-frame record, and the weighted records' totals through a slab row per
//                       frame + vpt_slab_sum (no float atomics: the same inputs give the same bits).
//  vpt_gae_kernel     : generalised advantage estimation, one lane per sequence walking back over t (one launch in place of ~5 T tiny ones).
//
// With l_j, q_j the log-probs of the policy and of the prior, p_j = exp(l_j), per head K = sum p_j (l_j - q_j) and H = -sum p_j l_j (p_j = 0 counts 0):
//   lp = l_b[a_b] + l_c[a_c],  rho = expf(lp - old_lp),  t^ = (value_target - mean) / std
//   L_r  = -min(rho A, clamp(rho, 1 - eps, 1 + eps) A) + kappa (K_b + K_c) - beta (H_b + H_c) + c_v (v - t^)^2,   loss = sum w_r L_r / sum w_r
//   c    = -A rho, except 0 where (A > 0 and rho > 1 + eps) or (A < 0 and rho < 1 - eps)          (torch.min / clamp's gradient, boundaries inclusive)
//   dz_j = rs [ c (onehot_j - p_j) + kappa p_j ((l_j - q_j) - K) + beta p_j (l_j + H) ] / T        per head, K and H that head's
//   dz_value = rs 2 c_v (v - t^),   rs = scale w_r
// THE KL IS KL(pi || prior): the expectation runs over the CURRENT policy (the direction of lib/action_head.py:198-203 called as
// pi.kl_divergence(pi_logits, prior_logits)); it penalises the policy for putting mass where the prior has none.
//
// K and H of a head are needed before any of its dz_j can be written, so a row takes two phases.  Phase 2 RE-READS the row's log-probs (70 KB per
// frame at 8641 + 121 classes with a prior: it was read a moment ago by the same workgroup and sits in L2) instead of holding up to 34 (l, q) pairs per
// thread in registers: the register version needs a compile-time bound on the head width and ~70 live VGPRs more, the re-read needs neither.
// A term whose coefficient is 0 is skipped (not multiplied by 0), so that with kappa = beta = c_v = 0, A = 1 and rho = 1 a row's policy columns are
// vpt_bc_loss_kernel's, bit for bit: c (onehot - p) with c = -1 is exactly p - onehot.
#include "vpt_common.h"
#include "vpt_kernels.h"

// One element of dz, in a fixed order of operations (no contraction): ((c (onehot - p) + kappa p ((l - q) - K)) + beta p (l + H)) * rst.
__device__ __forceinline__ float rl_loss_grad(float l, float q, float p, bool is_label, float c, bool has_kl, float kl_coef, float K, bool has_ent,
                                              float ent_coef, float H, float rst) {
#pragma clang fp contract(off)
  float g = c * ((is_label ? 1.f : 0.f) - p);
  if (p != 0.f) {                    // p = 0 (l = -inf): both terms are 0 (0 x -inf would be NaN)
    if (has_kl) g = g + (kl_coef * p) * ((l - q) - K);
    if (has_ent) g = g + (ent_coef * p) * (l + H);
  }
  return g * rst;
}

__global__ __launch_bounds__(256) void vpt_rl_loss_kernel(VptRlLossArgs a) {
#pragma clang fp contract(off)
  __shared__ float red[4][6];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* lb = a.lp_buttons + (size_t)row * a.nb;
  const float* lc = a.lp_camera + (size_t)row * a.nc;
  const bool prior = a.prior_buttons != nullptr;                    // (the launcher takes both or neither)
  const float* qb = prior ? a.prior_buttons + (size_t)row * a.nb : nullptr;
  const float* qc = prior ? a.prior_camera + (size_t)row * a.nc : nullptr;
  const float w = a.weight ? a.weight[row] : 1.f;
  const bool live = w != 0.f;
  const float rs = a.scale * w;
  const long ab64 = a.act_buttons[row], ac64 = a.act_camera[row];
  const int ab = (ab64 >= 0 && ab64 < a.nb) ? (int)ab64 : -1, ac = (ac64 >= 0 && ac64 < a.nc) ? (int)ac64 : -1;   // out of range: matches no element
  const int nbc = a.nb + a.nc;
  // ---- phase 1: per head sum p (l - q), sum p l and the label's log-prob ----
  float kb = 0.f, kc = 0.f, eb = 0.f, ec = 0.f, pb = 0.f, pc = 0.f;
  for (int i = tid; i < nbc; i += 256) {
    if (i < a.nb) {
      const float l = lb[i], p = expf(l);
      eb += (p == 0.f) ? 0.f : p * l;
      if (prior) kb += (p == 0.f) ? 0.f : p * (l - qb[i]);
      if (i == ab) pb += l;
    } else {
      const int j = i - a.nb;
      const float l = lc[j], p = expf(l);
      ec += (p == 0.f) ? 0.f : p * l;
      if (prior) kc += (p == 0.f) ? 0.f : p * (l - qc[j]);
      if (j == ac) pc += l;
    }
  }
  kb = wave_sum(kb); kc = wave_sum(kc); eb = wave_sum(eb); ec = wave_sum(ec); pb = wave_sum(pb); pc = wave_sum(pc);
  const int wv = tid >> 6;
  if ((tid & 63) == 0) { red[wv][0] = kb; red[wv][1] = kc; red[wv][2] = eb; red[wv][3] = ec; red[wv][4] = pb; red[wv][5] = pc; }
  __syncthreads();
  float s[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) s[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  // ---- the frame's scalars (every thread: phase 2 needs c, K, H) ----
  const float Kb = s[0], Kc = s[1], Hb = -s[2], Hc = -s[3];
  const float lp = s[4] + s[5];
  const float old_lp = a.old_log_prob[row], A = a.advantage[row];
  const float rho = expf(lp - old_lp);
  const float lo = 1.f - a.clip, hi = 1.f + a.clip;
  const bool clipped = (A > 0.f && rho > hi) || (A < 0.f && rho < lo);
  const float c = clipped ? 0.f : -(A * rho);
  float vd = 0.f;                                                    // v - t^ (normalised space)
  if (a.value) {
    const float that = (a.value_target[row] - a.vnorm[0]) / a.vnorm[1];
    vd = a.value[(size_t)row * a.value_stride] - that;
  }
  // ---- phase 2: dz ----
  if (a.dz) {
    vpt_op16* dz = a.dz + (size_t)row * a.ldz;
    const bool has_kl = prior && a.kl_coef != 0.f, has_ent = a.entropy_coef != 0.f;
    const float rst = rs * a.inv_temp;
    for (int i = tid; i < a.ldz; i += 256) {
      float g = 0.f;
      if (i < a.nb) {
        const float l = lb[i];
        g = rl_loss_grad(l, has_kl ? qb[i] : 0.f, expf(l), i == ab, c, has_kl, a.kl_coef, Kb, has_ent, a.entropy_coef, Hb, rst);
      } else if (i < nbc) {
        const int j = i - a.nb;
        const float l = lc[j];
        g = rl_loss_grad(l, has_kl ? qc[j] : 0.f, expf(l), j == ac, c, has_kl, a.kl_coef, Kc, has_ent, a.entropy_coef, Hc, rst);
      } else if (i == nbc && a.value && a.value_coef != 0.f) {
        g = ((2.f * a.value_coef) * vd) * rs;
      }
      dz[i] = (vpt_op16)(live ? g : 0.f);
    }
  }
  if (tid != 0 || (!a.frame_out && !a.slab)) return;
  const float rA = rho * A, cA = fminf(fmaxf(rho, lo), hi) * A;
  // [surrogate, K_b, K_c, H_b, H_c, (v - t^)^2, rho, clipped, lp, old_lp - lp, w, w > 0, 0, 0, 0, 0]: the frame's own (unweighted) values
  const float rec[12] = {-fminf(rA, cA), Kb, Kc, Hb, Hc, vd * vd, rho, clipped ? 1.f : 0.f, lp, old_lp - lp, w, (w > 0.f) ? 1.f : 0.f};
  if (a.frame_out) {
#pragma unroll
    for (int k = 0; k < 12; ++k) a.frame_out[(size_t)row * 16 + k] = rec[k];
#pragma unroll
    for (int k = 12; k < 16; ++k) a.frame_out[(size_t)row * 16 + k] = 0.f;
  }
  if (a.slab) {    // the weighted record: row `row` of the [M][16] slab vpt_slab_sum adds in its fixed order (slot 10: w, slot 11: one per row with w > 0)
#pragma unroll
    for (int k = 0; k < 10; ++k) a.slab[(size_t)row * 16 + k] = live ? w * rec[k] : 0.f;
    a.slab[(size_t)row * 16 + 10] = live ? w : 0.f;
    a.slab[(size_t)row * 16 + 11] = (w > 0.f) ? 1.f : 0.f;
#pragma unroll
    for (int k = 12; k < 16; ++k) a.slab[(size_t)row * 16 + k] = 0.f;
  }
}

extern "C" long vpt_rl_loss_workspace_floats(int M) { return M > 0 ? 16L * M + vpt_slab_sum_scratch_floats(M, 16) : 0; }

extern "C" int vpt_rl_loss_launch(const VptRlLossArgs* a, float* totals, float* workspace, hipStream_t stream) {
  if (a->M <= 0 || a->nb <= 0 || a->nc <= 0) return -1;
  if (a->dz && a->ldz < a->nb + a->nc + 1) return -1;
  if ((a->prior_buttons == nullptr) != (a->prior_camera == nullptr)) return -1;
  if (a->value && (!a->value_target || !a->vnorm || a->value_stride < 1)) return -1;
  if (totals && !workspace) return -1;
  if (totals && a->M > 65536) return -2;        // vpt_slab_sum: at most 256 slices of 256 rows
  VptRlLossArgs k = *a;
  k.slab = totals ? workspace : nullptr;
  hipLaunchKernelGGL(vpt_rl_loss_kernel, dim3(a->M), dim3(256), 0, stream, k);
  if (hipGetLastError() != hipSuccess) return -3;
  if (!totals) return 0;
  return vpt_slab_sum_launch(workspace, a->M, 16, 16L, totals, 16, nullptr, 0, workspace + 16L * a->M, stream);
}

// ------------------------------------------------------------------------------------------------
// Generalised advantage estimation over [B][T] rollouts, one lane per sequence, t = T-1 .. 0:
//   nt = !first[t+1] (t = T-1: !next_first),  delta = r + (nt ? gamma V_{t+1} : 0) - V,  A = delta + (nt ? (gamma lambda) A_{t+1} : 0),  ret = A + V
// in exactly this order of fp32 operations, no contraction: a float32 host twin reproduces it bit for bit.  A frame that starts an episode cuts
// the recursion (nothing of the next episode flows back, NaN included: a select, not a multiplication by 0).
__global__ __launch_bounds__(256) void vpt_gae_kernel(VptGaeArgs a) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.B) return;
  const size_t o = (size_t)b * a.T;
  const float gl = a.gamma * a.lam;
  float vnext = a.last_value[b], anext = 0.f;
  bool nt = !a.next_first[b];
  for (int t = a.T - 1; t >= 0; --t) {
    const float v = a.value[o + t];
    const float delta = (a.reward[o + t] + (nt ? a.gamma * vnext : 0.f)) - v;
    const float adv = delta + (nt ? gl * anext : 0.f);
    a.adv[o + t] = adv;
    a.ret[o + t] = adv + v;
    vnext = v; anext = adv;
    nt = !a.first[o + t];
  }
}

extern "C" int vpt_gae_launch(const VptGaeArgs* a, hipStream_t stream) {
  if (a->B <= 0 || a->T <= 0) return -1;
  hipLaunchKernelGGL(vpt_gae_kernel, dim3((a->B + 255) / 256), dim3(256), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
