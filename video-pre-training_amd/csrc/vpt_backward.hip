// Backward kernels of the behavioural-cloning step for the heads and the trunk (gfx950), fp32.
//
// The BC loss is  L = -mean_{b,t}[ log pi_buttons(a_bt) + log pi_camera(a_bt) ]  (behavioural_cloning.py:107-119,
// lib/action_head.py:176-184,252-253); the reference obtains its gradient from torch autograd.  Linear layers
// reuse vpt_gemm_kernel (dgrad with W^T packed, wgrad with A = dY^T); this file holds the rest:
//
//  vpt_nll_bwd_kernel    : d/dz of -(log_softmax(z/T)[a]) summed over the two heads -> bf16 dz (GEMM operand).
//  vpt_bc_loss_kernel    : the same gradient with per-frame weights, plus per-head NLL / entropy / arg-max hit per frame and their weighted
//                          totals (one sweep; the totals through a slab row per frame + vpt_slab_sum: bit-reproducible).
//  vpt_ln_bwd_kernel     : nn.LayerNorm backward (optionally through a ReLU on its input), dgain/dbias by
//                          per-workgroup register partials -> the workgroup's row of a partial slab -> vpt_ln_bwd_finish_kernel
//                          (fixed summation order: bit-reproducible).
//  vpt_colsum_kernel     : bias gradients (column sums of a bf16 matrix).
// The attention backward kernels have a source of their own, vpt_attn_bwd.hip.
#include "vpt_common.h"
#include "vpt_kernels.h"

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vpt_nll_bwd_kernel(VptNllBwdArgs a) {
  const int row = blockIdx.x, tid = threadIdx.x;
  vpt_op16* dz = a.dz + (size_t)row * a.ldz;
  const float* lb = a.lp_buttons + (size_t)row * a.nb;
  const float* lc = a.lp_camera + (size_t)row * a.nc;
  const long ab = a.act_buttons[row], ac = a.act_camera[row];
  for (int i = tid; i < a.ldz; i += 256) {
    float g = 0.f;
    if (i < a.nb) g = (expf(lb[i]) - (i == ab ? 1.f : 0.f)) * a.scale;
    else if (i < a.nb + a.nc) g = (expf(lc[i - a.nb]) - ((i - a.nb) == ac ? 1.f : 0.f)) * a.scale;
    dz[i] = (vpt_op16)g;
  }
}

extern "C" int vpt_nll_bwd_launch(const VptNllBwdArgs* a, hipStream_t stream) {
  if (a->M <= 0 || a->ldz < a->nb + a->nc) return -1;
  hipLaunchKernelGGL(vpt_nll_bwd_kernel, dim3(a->M), dim3(256), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ------------------------------------------------------------------------------------------------
// The BC loss with per-frame weights and its metrics in ONE sweep over a frame's nb + nc log-probs (behavioural_cloning.py:107,
// lib/action_head.py:176-193): every element is loaded once and feeds the loss gradient dz, the label's log-prob, the entropy sum and the arg-max.
//   loss = sum_rows w (nll_b + nll_c) / sum_rows w;  the caller folds 1 / (sum w x temperature) into `scale`, the row's factor is scale * w.
// A row with w == 0 (padding, a frame left out of the loss) stores exact zeros in dz and in its slab record whatever its log-probs hold, and its
// labels are only ever COMPARED with the sweep index (the label's log-prob is picked up where i == label), never used as one.
// One element of dz, in vpt_nll_bwd_kernel's order of operations -- (exp(lp) - onehot) * row_scale, no contraction -- so that a weighted row equals,
// bit for bit, that kernel's row at scale' = scale * w.
__device__ __forceinline__ float bc_loss_grad(float p, bool is_label, float row_scale) {
#pragma clang fp contract(off)
  const float d = p - (is_label ? 1.f : 0.f);
  return d * row_scale;
}

__global__ __launch_bounds__(256) void vpt_bc_loss_kernel(VptBcLossArgs a) {
  __shared__ float red[4][6];
  __shared__ int redi[4][2];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* lb = a.lp_buttons + (size_t)row * a.nb;
  const float* lc = a.lp_camera + (size_t)row * a.nc;
  const float w = a.weight ? a.weight[row] : 1.f;
  const bool live = w != 0.f;
  const float rs = a.scale * w;
  const long ab64 = a.act_buttons[row], ac64 = a.act_camera[row];
  const int ab = (ab64 >= 0 && ab64 < a.nb) ? (int)ab64 : -1, ac = (ac64 >= 0 && ac64 < a.nc) ? (int)ac64 : -1;   // out of range: matches no element
  const bool stats = a.frame_out || a.slab;
  vpt_op16* dz = a.dz ? a.dz + (size_t)row * a.ldz : nullptr;
  const int nbc = a.nb + a.nc, n = dz ? a.ldz : nbc;
  float eb = 0.f, ec = 0.f, pb = 0.f, pc = 0.f;            // sum p lp and the label's lp, per head
  float mb = -INFINITY, mc = -INFINITY;                    // running arg-max, per head
  int ib = 0x7fffffff, ic = 0x7fffffff;
  for (int i = tid; i < n; i += 256) {
    float g = 0.f;
    if (i < a.nb) {
      const float l = lb[i], p = expf(l);
      g = bc_loss_grad(p, i == ab, rs);
      eb += (p == 0.f) ? 0.f : p * l;
      if (i == ab) pb += l;
      argmax_take(mb, ib, l, i);
    } else if (i < nbc) {
      const int j = i - a.nb;
      const float l = lc[j], p = expf(l);
      g = bc_loss_grad(p, j == ac, rs);
      ec += (p == 0.f) ? 0.f : p * l;
      if (j == ac) pc += l;
      argmax_take(mc, ic, l, j);
    }
    if (dz) dz[i] = (vpt_op16)(live ? g : 0.f);
  }
  if (!stats) return;
  eb = wave_sum(eb); ec = wave_sum(ec); pb = wave_sum(pb); pc = wave_sum(pc);
  wave_argmax(mb, ib); wave_argmax(mc, ic);
  const int wv = tid >> 6;
  if ((tid & 63) == 0) {
    red[wv][0] = eb; red[wv][1] = ec; red[wv][2] = pb; red[wv][3] = pc; red[wv][4] = mb; red[wv][5] = mc;
    redi[wv][0] = ib; redi[wv][1] = ic;
  }
  __syncthreads();
  if (tid != 0) return;
  float s[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  int best[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float v01 = red[0][4 + h], v23 = red[2][4 + h];
    int i01 = redi[0][h], i23 = redi[2][h];
    argmax_take(v01, i01, red[1][4 + h], redi[1][h]);
    argmax_take(v23, i23, red[3][4 + h], redi[3][h]);
    argmax_take(v01, i01, v23, i23);
    best[h] = i01;
  }
  // [nll_b, nll_c, ent_b, ent_c, hit_b, hit_c, w, 0]: the frame's own (unweighted) values
  const float rec[8] = {-s[2], -s[3], -s[0], -s[1], (ab >= 0 && best[0] == ab) ? 1.f : 0.f, (ac >= 0 && best[1] == ac) ? 1.f : 0.f, w, 0.f};
  if (a.frame_out) {
#pragma unroll
    for (int k = 0; k < 8; ++k) a.frame_out[(size_t)row * 8 + k] = rec[k];
  }
  if (a.slab) {    // the weighted record: row `row` of the [M][8] slab vpt_slab_sum adds in its fixed order (slot 6: w, slot 7: one per row with w > 0)
#pragma unroll
    for (int k = 0; k < 6; ++k) a.slab[(size_t)row * 8 + k] = live ? w * rec[k] : 0.f;
    a.slab[(size_t)row * 8 + 6] = live ? w : 0.f;
    a.slab[(size_t)row * 8 + 7] = (w > 0.f) ? 1.f : 0.f;
  }
}

extern "C" long vpt_bc_loss_workspace_floats(int M) { return M > 0 ? 8L * M + vpt_slab_sum_scratch_floats(M, 8) : 0; }

extern "C" int vpt_bc_loss_launch(const VptBcLossArgs* a, float* totals, float* workspace, hipStream_t stream) {
  if (a->M <= 0 || a->nb <= 0 || a->nc <= 0) return -1;
  if (a->dz && a->ldz < a->nb + a->nc) return -1;
  if (totals && !workspace) return -1;
  if (totals && a->M > 65536) return -2;        // vpt_slab_sum: at most 256 slices of 256 rows
  VptBcLossArgs k = *a;
  k.slab = totals ? workspace : nullptr;
  hipLaunchKernelGGL(vpt_bc_loss_kernel, dim3(a->M), dim3(256), 0, stream, k);
  if (hipGetLastError() != hipSuccess) return -3;
  if (!totals) return 0;
  return vpt_slab_sum_launch(workspace, a->M, 8, 8L, totals, 8, nullptr, 0, workspace + 8L * a->M, stream);
}

// ------------------------------------------------------------------------------------------------
// The inverse-dynamics model's loss: gb independent nb-way button groups and gc nc-way camera groups per frame (20 x 2 and 2 x 11 in the released
// model), loss = sum_rows w (nll_b + nll_c) / sum_rows w with nll_* summed over the head's groups -- the negative of DictActionHead.logprob
// (lib/action_head.py:176-184,252-253).  One wavefront per frame: the elementwise pass writes dz in the column order of the two head matrices
// concatenated ([group][class], buttons first; vpt_bc_loss_kernel's element arithmetic), then lane g takes group g -- its label's log-prob, its
// entropy, its arg-max -- and the head sums are wave reductions (a fixed shuffle tree).  The record layout, the zero-weight rule and the totals
// (slab row per frame + vpt_slab_sum) are vpt_bc_loss_kernel's.
__global__ __launch_bounds__(256) void vpt_idm_loss_kernel(VptIdmLossArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.M) return;                                    // (wave-uniform: the shuffles below see whole waves)
  const int nbt = a.gb * a.nb, nct = a.gc * a.nc;
  const float* lb = a.lp_buttons + (size_t)row * nbt;
  const float* lc = a.lp_camera + (size_t)row * nct;
  const long* ab = a.act_buttons + (size_t)row * a.gb;
  const long* ac = a.act_camera + (size_t)row * a.gc;
  const float w = a.weight ? a.weight[row] : 1.f;
  const bool live = w != 0.f;
  const float rs = a.scale * w;
  if (a.dz) {
    vpt_op16* dz = a.dz + (size_t)row * a.ldz;
    for (int i = lane; i < a.ldz; i += 64) {
      float g = 0.f;
      if (i < nbt) {
        const int grp = i / a.nb, c = i - grp * a.nb;
        g = bc_loss_grad(expf(lb[i]), (long)c == ab[grp], rs);
      } else if (i < nbt + nct) {
        const int j = i - nbt, grp = j / a.nc, c = j - grp * a.nc;
        g = bc_loss_grad(expf(lc[j]), (long)c == ac[grp], rs);
      }
      dz[i] = (vpt_op16)(live ? g : 0.f);
    }
  }
  if (!a.frame_out && !a.slab) return;
  float pb = 0.f, pc = 0.f, eb = 0.f, ec = 0.f, hb = 0.f, hc = 0.f;      // the label's lp, sum p lp and the hits, per head
  for (int grp = lane; grp < a.gb + a.gc; grp += 64) {
    const bool cam = grp >= a.gb;
    const int gi = cam ? grp - a.gb : grp, n = cam ? a.nc : a.nb;
    const float* l = cam ? lc + gi * a.nc : lb + gi * a.nb;
    const long lab = cam ? ac[gi] : ab[gi];
    float e = 0.f, pick = 0.f, mv = -INFINITY;
    int mi = 0x7fffffff;
    for (int c = 0; c < n; ++c) {
      const float lv = l[c], p = expf(lv);
      e += (p == 0.f) ? 0.f : p * lv;
      if ((long)c == lab) pick += lv;
      argmax_take(mv, mi, lv, c);
    }
    const float hit = (lab >= 0 && lab < n && (long)mi == lab) ? 1.f : 0.f;
    if (cam) { pc += pick; ec += e; hc += hit; }
    else { pb += pick; eb += e; hb += hit; }
  }
  pb = wave_sum(pb); pc = wave_sum(pc); eb = wave_sum(eb); ec = wave_sum(ec); hb = wave_sum(hb); hc = wave_sum(hc);
  if (lane != 0) return;
  // [nll_b, nll_c, ent_b, ent_c, hit_b, hit_c, w, 0]: the frame's own (unweighted) values; a hit is the fraction of the head's groups
  const float rec[8] = {-pb, -pc, -eb, -ec, hb / (float)a.gb, hc / (float)a.gc, w, 0.f};
  if (a.frame_out) {
#pragma unroll
    for (int k = 0; k < 8; ++k) a.frame_out[(size_t)row * 8 + k] = rec[k];
  }
  if (a.slab) {
#pragma unroll
    for (int k = 0; k < 6; ++k) a.slab[(size_t)row * 8 + k] = live ? w * rec[k] : 0.f;
    a.slab[(size_t)row * 8 + 6] = live ? w : 0.f;
    a.slab[(size_t)row * 8 + 7] = (w > 0.f) ? 1.f : 0.f;
  }
}

extern "C" int vpt_idm_loss_launch(const VptIdmLossArgs* a, float* totals, float* workspace, hipStream_t stream) {
  if (a->M <= 0 || a->gb <= 0 || a->nb <= 0 || a->gc <= 0 || a->nc <= 0) return -1;
  if (a->dz && a->ldz < a->gb * a->nb + a->gc * a->nc) return -1;
  if (totals && !workspace) return -1;
  if (totals && a->M > 65536) return -2;        // vpt_slab_sum: at most 256 slices of 256 rows
  VptIdmLossArgs k = *a;
  k.slab = totals ? workspace : nullptr;
  hipLaunchKernelGGL(vpt_idm_loss_kernel, dim3((a->M + 3) / 4), dim3(256), 0, stream, k);
  if (hipGetLastError() != hipSuccess) return -3;
  if (!totals) return 0;
  return vpt_slab_sum_launch(workspace, a->M, 8, 8L, totals, 8, nullptr, 0, workspace + 8L * a->M, stream);
}

// ------------------------------------------------------------------------------------------------
// Backward of lp = log_softmax(z / T) for an ARBITRARY incoming gradient g = dL/dlp (what torch autograd hands to the
// policy's outputs, lib/policy.py:271-305): dz = (g - exp(lp) * sum_j g_j) / T per head; the value column passes through.
// One workgroup per row; the row sums by wave shuffles + LDS.
__global__ __launch_bounds__(256) void vpt_heads_bwd_kernel(VptHeadsBwdArgs a) {
  __shared__ float red[8];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* lb = a.lp_buttons + (size_t)row * a.nb;
  const float* lc = a.lp_camera + (size_t)row * a.nc;
  const float* gb = a.g_buttons ? a.g_buttons + (size_t)row * a.nb : nullptr;
  const float* gc = a.g_camera ? a.g_camera + (size_t)row * a.nc : nullptr;
  float sb = 0.f, sc = 0.f;
  if (gb) for (int i = tid; i < a.nb; i += 256) sb += gb[i];
  if (gc) for (int i = tid; i < a.nc; i += 256) sc += gc[i];
  sb = wave_sum(sb); sc = wave_sum(sc);
  if ((tid & 63) == 0) { red[tid >> 6] = sb; red[4 + (tid >> 6)] = sc; }
  __syncthreads();
  sb = (red[0] + red[1]) + (red[2] + red[3]);
  sc = (red[4] + red[5]) + (red[6] + red[7]);
  vpt_op16* dz = a.dz + (size_t)row * a.ldz;
  for (int i = tid; i < a.ldz; i += 256) {
    float g = 0.f;
    if (i < a.nb) {
      if (gb && !(a.mask_buttons && !a.mask_buttons[(size_t)row * a.nb + i])) g = (gb[i] - expf(lb[i]) * sb) * a.inv_temp * a.grad_scale;
    } else if (i < a.nb + a.nc) {
      const int j = i - a.nb;
      if (gc && !(a.mask_camera && !a.mask_camera[(size_t)row * a.nc + j])) g = (gc[j] - expf(lc[j]) * sc) * a.inv_temp * a.grad_scale;
    }
    else if (i == a.nb + a.nc && a.g_value) g = a.g_value[row] * a.grad_scale;
    dz[i] = (vpt_op16)g;
  }
}

extern "C" int vpt_heads_bwd_launch(const VptHeadsBwdArgs* a, hipStream_t stream) {
  if (a->M <= 0 || a->ldz < a->nb + a->nc + 1) return -1;
  hipLaunchKernelGGL(vpt_heads_bwd_kernel, dim3(a->M), dim3(256), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ------------------------------------------------------------------------------------------------
// The same backward for the inverse-dynamics model's heads (lib/action_head.py:136-184: a CategoricalActionHead of shape (groups, classes) is
// `groups` independent log-softmaxes): gb nb-way button groups and gc nc-way camera groups per frame, an ARBITRARY incoming gradient g = dL/dlp
// (what torch autograd hands to InverseActionPolicy.forward's outputs).  One element, with l, g the group's n log-probs and incoming gradients:
//   s = ((g_0 + g_1) + ...) + g_{n-1}     p_j = expf(l_j)     dz_j = ((g_j - p_j s) * (1 / T)) * grad_scale     (fp32, no contraction)
// rounded once to the operand format; a masked element (its logit was the constant LOG0) stores 0 -- its g still counts in s, as in autograd.
// Shaped like vpt_idm_loss_kernel: one wavefront per frame, lane c owns columns c, c + 64, ... of the two head matrices concatenated ([group][class],
// buttons first) and sums its own group serially (n <= 11 in the released heads: the g values come from L1).  No LDS, no barrier, no cross-lane
// traffic, no atomics: the same inputs give the same bits.
__device__ __forceinline__ float grouped_lp_bwd_elem(const float* l, const float* g, const uint8_t* mask, int i, int n, float inv_temp, float grad_scale) {
#pragma clang fp contract(off)
  const int base = (i / n) * n;
  float s = g[base];
  for (int c = 1; c < n; ++c) s = s + g[base + c];
  if (mask && !mask[i]) return 0.f;
  const float p = expf(l[i]);
  const float d = g[i] - p * s;
  return (d * inv_temp) * grad_scale;
}

__global__ __launch_bounds__(256) void vpt_grouped_lp_bwd_kernel(VptGroupedLpBwdArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.M) return;
  const int nbt = a.gb * a.nb, nct = a.gc * a.nc;
  const float* lb = a.lp_buttons + (size_t)row * nbt;
  const float* lc = a.lp_camera + (size_t)row * nct;
  const float* gb = a.g_buttons ? a.g_buttons + (size_t)row * nbt : nullptr;
  const float* gc = a.g_camera ? a.g_camera + (size_t)row * nct : nullptr;
  const uint8_t* mb = a.mask_buttons ? a.mask_buttons + (size_t)row * nbt : nullptr;
  const uint8_t* mc = a.mask_camera ? a.mask_camera + (size_t)row * nct : nullptr;
  vpt_op16* dz = a.dz + (size_t)row * a.ldz;
  for (int i = lane; i < a.ldz; i += 64) {
    float v = 0.f;
    if (i < nbt) {
      if (gb) v = grouped_lp_bwd_elem(lb, gb, mb, i, a.nb, a.inv_temp, a.grad_scale);
    } else if (i < nbt + nct) {
      if (gc) v = grouped_lp_bwd_elem(lc, gc, mc, i - nbt, a.nc, a.inv_temp, a.grad_scale);
    }
    dz[i] = (vpt_op16)v;
  }
}

extern "C" int vpt_grouped_lp_bwd_launch(const VptGroupedLpBwdArgs* a, hipStream_t stream) {
  if (a->M <= 0 || a->gb <= 0 || a->nb <= 0 || a->gc <= 0 || a->nc <= 0) return -1;
  if (a->ldz < a->gb * a->nb + a->gc * a->nc) return -1;
  hipLaunchKernelGGL(vpt_grouped_lp_bwd_kernel, dim3((a->M + 3) / 4), dim3(256), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ------------------------------------------------------------------------------------------------
// out_bf16[M][ldo] = (mask > 0 ? x : 0), columns >= N zero: ReLU gate + cast + K-padding of a GEMM A operand
__global__ __launch_bounds__(256) void vpt_gate_cast_kernel(VptGateCastArgs a) {
  const size_t total = (size_t)a.M * a.ldo;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int row = (int)(i / a.ldo), col = (int)(i - (size_t)row * a.ldo);
    float v = 0.f;
    if (col < a.N) {
      v = a.x[(size_t)row * a.ldx + col];
      if (a.mask && !((float)a.mask[(size_t)row * a.ldm + col] > 0.f)) v = 0.f;
    }
    a.out[i] = (vpt_op16)v;
  }
}

extern "C" int vpt_gate_cast_launch(const VptGateCastArgs* a, hipStream_t stream) {
  if (a->M <= 0 || a->ldo < a->N) return -1;
  size_t blocks = ((size_t)a->M * a->ldo + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(vpt_gate_cast_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ------------------------------------------------------------------------------------------------
#define LNB_ROWS 32  // rows per workgroup (8 per wave)
#define LNB_MAXD4 16 // D <= 4096

// ND4 = float4 slots per lane (D <= 256 ND4), a compile-time bound: the row lives in registers (x always, dy too when
// ND4 <= 8) for its four passes, and the per-lane column partials pg / pb are indexed statically.
template <int ND4>
__global__ __launch_bounds__(256) void vpt_ln_bwd_kernel(VptLnBwdArgs a) {
  constexpr bool KEEP_DY = ND4 <= 8;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n4 = a.D >> 2;            // float4 per row
  f32x4 pg[ND4], pb[ND4];
#pragma unroll
  for (int q = 0; q < ND4; ++q) { pg[q] = (f32x4){0.f, 0.f, 0.f, 0.f}; pb[q] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
  const float invD = 1.0f / (float)a.D;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int rr = 0; rr < LNB_ROWS / 4; ++rr) {
    const int row = blockIdx.x * LNB_ROWS + w * (LNB_ROWS / 4) + rr;
    if (row >= a.M) break;
    const float* x = a.x + (size_t)row * a.D;
    const float* dy = a.dy + (size_t)row * a.D;
    f32x4 xv[ND4], dv[KEEP_DY ? ND4 : 1];
#pragma unroll
    for (int q = 0; q < ND4; ++q) {
      const int i = lane + 64 * q;
      xv[q] = (i < n4) ? *(const f32x4*)(x + 4 * i) : zero;
      if (KEEP_DY) dv[q] = (i < n4) ? *(const f32x4*)(dy + 4 * i) : zero;
    }
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < ND4; ++q) {
      if (a.relu_in) { xv[q].x = fmaxf(xv[q].x, 0.f); xv[q].y = fmaxf(xv[q].y, 0.f); xv[q].z = fmaxf(xv[q].z, 0.f); xv[q].w = fmaxf(xv[q].w, 0.f); }
      s += (xv[q].x + xv[q].y) + (xv[q].z + xv[q].w);     // (slots past the row hold zeros)
    }
    const float mean = wave_sum(s) * invD;
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < ND4; ++q) {
      if (lane + 64 * q < n4) {
        const float d0 = xv[q].x - mean, d1 = xv[q].y - mean, d2 = xv[q].z - mean, d3 = xv[q].w - mean;
        ss += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
      }
    }
    const float rstd = rsqrtf(wave_sum(ss) * invD + VPT_NORM_EPS);
    // sums of dy*g and dy*g*xhat over the row
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int q = 0; q < ND4; ++q) {
      const int i = lane + 64 * q;
      if (i < n4) {
        const f32x4 g = *(const f32x4*)(a.gain + 4 * i), d = KEEP_DY ? dv[q] : *(const f32x4*)(dy + 4 * i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float xh = (xv[q][k] - mean) * rstd, dg = d[k] * g[k];
          s1 += dg;
          s2 = fmaf(dg, xh, s2);
        }
      }
    }
#ifdef VPT_LN_DEBUG   // diagnostics build (tools/ubench/pk_hazard): every lane's partial sums and the reduced values of every row, [M][64][4]
    if (a.debug) { a.debug[((size_t)row * 64 + lane) * 4 + 0] = s1; a.debug[((size_t)row * 64 + lane) * 4 + 1] = s2; }
#endif
    s1 = wave_sum(s1) * invD;
    s2 = wave_sum(s2) * invD;
#ifdef VPT_LN_DEBUG
    if (a.debug) { a.debug[((size_t)row * 64 + lane) * 4 + 2] = s1; a.debug[((size_t)row * 64 + lane) * 4 + 3] = s2; }
#endif
#pragma unroll
    for (int q = 0; q < ND4; ++q) {
      const int i = lane + 64 * q;
      if (i < n4) {
        const f32x4 g = *(const f32x4*)(a.gain + 4 * i), d = KEEP_DY ? dv[q] : *(const f32x4*)(dy + 4 * i);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float xh = (xv[q][k] - mean) * rstd;
          float dxk = rstd * (d[k] * g[k] - s1 - xh * s2);
          if (a.relu_in && !(xv[q][k] > 0.f)) dxk = 0.f;     // max(x, 0) > 0  <=>  x > 0
          o[k] = dxk;
          pg[q][k] = fmaf(d[k], xh, pg[q][k]);
          pb[q][k] += d[k];
        }
        if (a.dx_add) {
          const f32x4 e = *(const f32x4*)(a.dx_add + (size_t)row * a.D + 4 * i);
          o.x += e.x; o.y += e.y; o.z += e.z; o.w += e.w;
        }
        *(f32x4*)(a.dx + (size_t)row * a.D + 4 * i) = o;
      }
    }
  }
  // column partials: every WAVE writes its sums to its own row of the partial slab (row = 4 x workgroup + wave; float4 per lane, coalesced) and
  // vpt_ln_bwd_finish_kernel adds the rows in row order -- no LDS table, no barrier, nothing that depends on the order in which waves or
  // workgroups run.  (Until round 5: LDS float atomics across the waves + one global fp32 atomic per column per workgroup.)
  float* part = a.partials + ((size_t)blockIdx.x * 4 + w) * 2 * a.D;
#pragma unroll
  for (int q = 0; q < ND4; ++q) {
    const int i = lane + 64 * q;
    if (i < n4) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {      // (element stores: as 16-byte stores the partials would have to sit in aligned register quadruples -- 600 spills at ND4 = 8)
        part[4 * i + k] = pg[q][k];
        part[a.D + 4 * i + k] = pb[q][k];
      }
    }
  }
}

// dgain[c] += sum_b partials[b][0][c], dbias[c] += sum_b partials[b][1][c] over the nblocks = 4 x workgroups rows: a workgroup takes 16 columns x 16 contiguous
// row segments (b ascending inside a segment), the segments are combined by a fixed binary tree -- one summation order per column, a function of
// (nblocks, D) alone, whatever the order the workgroups above ran in.  (16 segments: 64 dependent-free loads per thread at M = 8192 instead of 256.)
__global__ __launch_bounds__(256) void vpt_ln_bwd_finish_kernel(const float* __restrict__ partials, int nblocks, int D, float* dgain, float* dbias) {
  __shared__ float seg_[16][16];
  const int lc = threadIdx.x & 15, sg = threadIdx.x >> 4;
  const int col = blockIdx.x * 16 + lc;                                   // col indexes the 2 D columns [dgain ; dbias]
  const int per = (nblocks + 15) >> 4, b0 = sg * per, b1 = min(b0 + per, nblocks);
  float s = 0.f;
  if (col < 2 * D) {
#pragma unroll 8
    for (int b = b0; b < b1; ++b) s += partials[(size_t)b * 2 * D + col];
  }
  seg_[sg][lc] = s;
  __syncthreads();
  if (sg == 0 && col < 2 * D) {
    float t[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = seg_[i][lc];
#pragma unroll
    for (int w = 1; w < 16; w <<= 1)
#pragma unroll
      for (int i = 0; i < 16; i += 2 * w) t[i] += t[i + w];
    if (col < D) dgain[col] += t[0];
    else dbias[col - D] += t[0];
  }
}

extern "C" int vpt_ln_bwd_launch(const VptLnBwdArgs* a, hipStream_t stream) {
  if (a->M <= 0 || (a->D & 3) || a->D > 4 * 64 * LNB_MAXD4 || !a->partials) return -1;
  const dim3 g((a->M + LNB_ROWS - 1) / LNB_ROWS), b(256);
  const int nd4 = ((a->D >> 2) + 63) >> 6;
  if (nd4 <= 4) hipLaunchKernelGGL(vpt_ln_bwd_kernel<4>, g, b, 0, stream, *a);
  else if (nd4 <= 8) hipLaunchKernelGGL(vpt_ln_bwd_kernel<8>, g, b, 0, stream, *a);
  else if (nd4 <= 12) hipLaunchKernelGGL(vpt_ln_bwd_kernel<12>, g, b, 0, stream, *a);
  else hipLaunchKernelGGL(vpt_ln_bwd_kernel<16>, g, b, 0, stream, *a);
  hipLaunchKernelGGL(vpt_ln_bwd_finish_kernel, dim3((2 * a->D + 15) / 16), b, 0, stream, (const float*)a->partials, 4 * (int)g.x, a->D, a->dgain, a->dbias);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ------------------------------------------------------------------------------------------------
// out[col] += sum_r x[r][col]: the rows are cut into gridDim.y slices, slice sums go to the slab partials[slice][col] and
// vpt_colsum_finish_kernel adds them in slice order (bit-reproducible; until round 5 one fp32 atomic per slice).
__global__ __launch_bounds__(256) void vpt_colsum_kernel(VptColsumArgs a) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  const int rows_per = (a.M + gridDim.y - 1) / gridDim.y;
  const int r0 = blockIdx.y * rows_per, r1 = min(r0 + rows_per, a.M);
  if (col >= a.N) return;
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s += (float)a.x[(size_t)r * a.ld + col];
  if (gridDim.y == 1) a.out[col] += s;
  else a.partials[(size_t)blockIdx.y * a.N + col] = s;
}

__global__ __launch_bounds__(256) void vpt_colsum_finish_kernel(VptColsumArgs a, int slices) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= a.N) return;
  float s = 0.f;
  for (int y = 0; y < slices; ++y) s += a.partials[(size_t)y * a.N + col];
  a.out[col] += s;
}

static int colsum_slices(int M) { return M >= 4096 ? 64 : (M >= 256 ? 16 : 1); }
extern "C" long vpt_colsum_partial_floats(int M, int N) { const int gy = colsum_slices(M); return gy > 1 ? (long)gy * N : 0; }

extern "C" int vpt_colsum_launch(const VptColsumArgs* a, hipStream_t stream) {
  if (a->M <= 0 || a->N <= 0) return -1;
  const int gy = colsum_slices(a->M);
  if (gy > 1 && !a->partials) return -1;
  hipLaunchKernelGGL(vpt_colsum_kernel, dim3((a->N + 255) / 256, gy), dim3(256), 0, stream, *a);
  if (gy > 1) hipLaunchKernelGGL(vpt_colsum_finish_kernel, dim3((a->N + 255) / 256), dim3(256), 0, stream, *a, gy);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
