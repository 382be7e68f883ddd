// The auxiliary ("sleep") phase of phasic policy gradient, the form of RL fine-tuning the VPT method uses (gfx950), fp32.  The released models have one
// network with one value head, so the single-network variant applies: the phase keeps fitting the value head on the stored returns through the whole
// shared trunk while a cloning term holds the policy at a snapshot pi_old taken just before the phase.
//
//  vpt_ppg_aux_loss_kernel : clone_coef x KL(pi_old || pi) + value_coef x (v - t^)^2 of one frame per workgroup, in vpt_bc_loss_kernel's form: the
//                            gradient dz w.r.t. the fused head logits, a per-frame record, and the weighted records' totals through a slab row per
//                            frame + vpt_slab_sum (no float atomics: the same inputs give the same bits).
//
// With l_j, m_j the log-probs of the policy and of the snapshot, p_j = expf(l_j), o_j = expf(m_j), per head
//   D = sum_j o_j (m_j - l_j)  (o_j = 0 counts 0),   S = sum_j o_j  (the teacher's mass, a diagnostic),   t^ = (value_target - mean) / std,  vd = v - t^
//   loss     = sum_r w_r [ beta (D_b + D_c) + c_v vd^2 ] / sum_r w_r
//   dz_j     = (beta (p_j - o_j)) rst,   rst = (scale w_r) inv_temp          per head
//   dz_value = ((2 c_v) vd) (scale w_r)
// THE KL IS KL(pi_old || pi): the expectation runs over the STORED TEACHER, the opposite direction of vpt_rl_loss_kernel's KL(pi || prior).  It is the
// cross-entropy to a soft label minus the label's own entropy; with a one-hot teacher it is vpt_bc_loss_kernel's NLL and its gradient, bit for bit.
// p - o IS THE GRADIENT OF D FOR A TEACHER WHOSE MASS IS EXACTLY 1.  The exact gradient w.r.t. the logits is p S - o; the record carries S_b and S_c so
// that a caller sees how far a teacher is from 1 (a snapshot rounded to fp32 is within a few 1e-7 per class).
//
// Nothing of a row has to be reduced before its dz can be written (vpt_rl_loss_kernel needs K and H first and sweeps twice): ONE sweep, every (l_j, m_j)
// pair loaded once, dz_j written at once, D and S accumulated on the side -- vpt_bc_loss_kernel's structure with a second input row.
// A term whose coefficient is 0 is skipped (not multiplied by 0).  A class with o_j > 0 and l_j = -inf (live at the snapshot, masked now) gives
// D = +inf with a finite dz: the snapshot must be taken under the same logit masks as the forward; this is not guarded.
#include "vpt_common.h"
#include "vpt_kernels.h"

// One element of dz, in a fixed order of operations (no contraction): (beta (p - o)) * rst.  With beta = 1 and a one-hot teacher this is
// vpt_rl_loss_kernel's (c (onehot - p)) * rst at c = -1, and vpt_bc_loss_kernel's (p - onehot) * row_scale.
__device__ __forceinline__ float ppg_aux_grad(float p, float o, float beta, float rst) {
#pragma clang fp contract(off)
  return (beta * (p - o)) * rst;
}

__global__ __launch_bounds__(256) void vpt_ppg_aux_loss_kernel(VptPpgAuxLossArgs a) {
#pragma clang fp contract(off)
  __shared__ float red[4][4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* lb = a.lp_buttons + (size_t)row * a.nb;
  const float* lc = a.lp_camera + (size_t)row * a.nc;
  const float* mb = a.old_buttons + (size_t)row * a.nb;
  const float* mc = a.old_camera + (size_t)row * a.nc;
  const float w = a.weight ? a.weight[row] : 1.f;
  const bool live = w != 0.f;
  const float rs = a.scale * w;
  const float rst = rs * a.inv_temp;
  const bool clone = a.clone_coef != 0.f;
  const bool stats = a.frame_out || a.slab;
  vpt_op16* dz = a.dz ? a.dz + (size_t)row * a.ldz : nullptr;
  const int nbc = a.nb + a.nc, n = dz ? a.ldz : nbc;
  float vd = 0.f;                                                    // v - t^ (normalised space)
  if (a.value) {
    const float that = (a.value_target[row] - a.vnorm[0]) / a.vnorm[1];
    vd = a.value[(size_t)row * a.value_stride] - that;
  }
  float db = 0.f, dc = 0.f, sb = 0.f, sc = 0.f;           // sum o (m - l) and sum o, per head
  for (int i = tid; i < n; i += 256) {
    float g = 0.f;
    if (i < a.nb) {
      const float l = lb[i], m = mb[i], o = expf(m);
      if (clone) g = ppg_aux_grad(expf(l), o, a.clone_coef, rst);
      db += (o == 0.f) ? 0.f : o * (m - l);
      sb += o;
    } else if (i < nbc) {
      const int j = i - a.nb;
      const float l = lc[j], m = mc[j], o = expf(m);
      if (clone) g = ppg_aux_grad(expf(l), o, a.clone_coef, rst);
      dc += (o == 0.f) ? 0.f : o * (m - l);
      sc += o;
    } else if (i == nbc && a.value && a.value_coef != 0.f) {
      g = ((2.f * a.value_coef) * vd) * rs;
    }
    if (dz) dz[i] = (vpt_op16)(live ? g : 0.f);
  }
  if (!stats) return;
  db = wave_sum(db); dc = wave_sum(dc); sb = wave_sum(sb); sc = wave_sum(sc);
  const int wv = tid >> 6;
  if ((tid & 63) == 0) { red[wv][0] = db; red[wv][1] = dc; red[wv][2] = sb; red[wv][3] = sc; }
  __syncthreads();
  if (tid != 0) return;
  float s[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  // [D_b, D_c, (v - t^)^2, S_b, S_c, w, w > 0, 0]: the frame's own (unweighted) values
  const float rec[8] = {s[0], s[1], vd * vd, s[2], s[3], w, (w > 0.f) ? 1.f : 0.f, 0.f};
  if (a.frame_out) {
#pragma unroll
    for (int k = 0; k < 8; ++k) a.frame_out[(size_t)row * 8 + k] = rec[k];
  }
  if (a.slab) {    // the weighted record: row `row` of the [M][8] slab vpt_slab_sum adds in its fixed order (slot 5: w, slot 6: one per row with w > 0)
#pragma unroll
    for (int k = 0; k < 5; ++k) a.slab[(size_t)row * 8 + k] = live ? w * rec[k] : 0.f;
    a.slab[(size_t)row * 8 + 5] = live ? w : 0.f;
    a.slab[(size_t)row * 8 + 6] = (w > 0.f) ? 1.f : 0.f;
    a.slab[(size_t)row * 8 + 7] = 0.f;
  }
}

extern "C" long vpt_ppg_aux_loss_workspace_floats(int M) { return M > 0 ? 8L * M + vpt_slab_sum_scratch_floats(M, 8) : 0; }

extern "C" int vpt_ppg_aux_loss_launch(const VptPpgAuxLossArgs* a, float* totals, float* workspace, hipStream_t stream) {
  if (a->M <= 0 || a->nb <= 0 || a->nc <= 0) return -1;
  if (!a->lp_buttons || !a->lp_camera || !a->old_buttons || !a->old_camera) return -1;
  if (a->dz && a->ldz < a->nb + a->nc + 1) return -1;
  if (a->value && (!a->value_target || !a->vnorm || a->value_stride < 1)) return -1;
  if (totals && !workspace) return -1;
  if (totals && a->M > 65536) return -2;        // vpt_slab_sum: at most 256 slices of 256 rows
  VptPpgAuxLossArgs k = *a;
  k.slab = totals ? workspace : nullptr;
  hipLaunchKernelGGL(vpt_ppg_aux_loss_kernel, dim3(a->M), dim3(256), 0, stream, k);
  if (hipGetLastError() != hipSuccess) return -3;
  if (!totals) return 0;
  return vpt_slab_sum_launch(workspace, a->M, 8, 8L, totals, 8, nullptr, 0, workspace + 8L * a->M, stream);
}
