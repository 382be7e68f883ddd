// Backward kernels of the two attentions (gfx950), fp32, on the 32-query tile whose constants and shared bodies are in vpt_attn_tile.h.
//
//  vpt_attn_bwd_kernel      : backward of vpt_attn_kernel (banded attention with KV memory + rel-pos bias): per
//                             (sequence, head, 32-query tile) recompute P, then dV = P^T dO, dP = dO V^T,
//                             dS = P (dP - rowsum(P dP)), dQ = dS K / d, dK = dS^T Q / d, dR = dS B, db_nd = R^T dS.
//                             Keys are shared by up to five query tiles -> each tile's dK / dV piece goes to its own slab slot, db_nd to
//                             the workgroup's slab row; vpt_attn_bwd_finish_kernel / vpt_slab_sum add them in a fixed order (bit-reproducible);
//                             memory keys (detached state, behavioural_cloning.py:111) receive no gradient.
//  vpt_full_attn_bwd_kernel : the same for mask "none" (the inverse-dynamics model): no memory, no bias, every query sees its whole window.
//
// Round 2: every contraction runs on the fp32 matrix cores with its operands taken straight from global memory or from the 32 x 160 score tiles in
// LDS; 65 KB of LDS -> two workgroups per CU.  The first version staged Q, dO and the K / V slab in 151 KB of LDS and did the five contractions on
// the vector ALU.
#include "vpt_common.h"
#include "vpt_kernels.h"
#include "vpt_attn_tile.h"

// ------------------------------------------------------------------------------------------------
#define AB_P_OFF 0                                        // P  [32][ATT_SS]
#define AB_D_OFF (AB_P_OFF + ATT_QT * ATT_SS)             // dP, then dS  [32][ATT_SS]
#define AB_R_OFF (AB_D_OFF + ATT_QT * ATT_SS)
#define AB_B_OFF (AB_R_OFF + ATT_QT * 10)
#define AB_BP 133                                         // pitch of a b_nd row in LDS: odd, so that ten lanes reading one offset of ten DIFFERENT rows (the
                                                          // dR loop) hit ten banks -- at pitch maxlen = 128 they all hit one (47 % of this kernel's LDS cycles
                                                          // were bank conflicts in the round-3 PMC survey)
#define AB_QL_OFF (AB_B_OFF + 10 * AB_BP)                 // the tile's 32 qlo values (ints)
#define AB_PT_OFF ((AB_QL_OFF + ATT_QT + 3) & ~3)         // partial tiles of key tile 4: [wave][16][64]
#define AB_FLOATS (AB_PT_OFF + 4 * 16 * 64)

__global__ __launch_bounds__(256, 2) void vpt_attn_bwd_kernel(VptAttnBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* Ps = sm + AB_P_OFF;
  float* Ds = sm + AB_D_OFF;
  float* Rs = sm + AB_R_OFF;
  float* Bs = sm + AB_B_OFF;
  float* Pt = sm + AB_PT_OFF;
  int* Ql = (int*)(sm + AB_QL_OFF);

  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const int b = blockIdx.y / a.heads, h = blockIdx.y - b * a.heads;
  const int q0 = blockIdx.x * ATT_QT;
  const int maxlen = a.maxlen, t = a.t, hid = a.hid;
  const size_t tok0 = (size_t)b * t;
  const float inv_dh = 1.0f / ATT_DH;
  const int jbase = q0 + 1;             // key kk of the band = row jbase + kk of [memory ; chunk]
  float* dbnd_row = a.dbnd_slab + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (10 * a.maxlen);

  for (int idx = tid; idx < ATT_QT * 10; idx += 256) {
    const int r = idx / 10, n = idx - r * 10;
    Rs[idx] = (q0 + r < t) ? a.qkvr[(tok0 + q0 + r) * a.ld + 3 * hid + h * 10 + n] : 0.f;
  }
  for (int idx = tid; idx < 10 * maxlen; idx += 256) { const int n = idx / maxlen; Bs[n * AB_BP + (idx - n * maxlen)] = a.b_nd[idx]; }
  if (tid < ATT_QT) Ql[tid] = (a.qlo && q0 + tid < t) ? a.qlo[tok0 + q0 + tid] : 0;      // as the forward kernel: rows below Ql[qi] are invisible
  __syncthreads();

  // row j of [memory ; chunk] -> its K (which = 1) / V (which = 2) row of this head, or null beyond the chunk
  auto kv_row = [&](int j, int which) -> const float* {
    if (j < maxlen) return (which == 1 ? a.kmem : a.vmem) + ((size_t)b * maxlen + j) * hid + h * ATT_DH;
    if (j - maxlen < t) return a.qkvr + (tok0 + j - maxlen) * a.ld + which * hid + h * ATT_DH;
    return nullptr;
  };
  // query-indexed rows as (wave-uniform base pointer, 32-bit element offset or -1): one scalar register per row instead of a 64-bit pointer
  // (the pointer-returning form kept 8 pointers x several unrolled iterations alive: 163 spilled SGPRs)
  const float* qbase = a.qkvr + (tok0 + q0) * a.ld + h * ATT_DH;
  const float* dobase = a.dout + (tok0 + q0) * hid + h * ATT_DH;
  const int nq_valid = t - q0;                            // queries q0 + qi with qi < nq_valid exist
  auto q_row = [&](int qi) -> const float* { return (qi < nq_valid) ? qbase + qi * a.ld : nullptr; };
  auto do_row = [&](int qi) -> const float* { return (qi < nq_valid) ? dobase + qi * hid : nullptr; };
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  const uint8_t* memv = a.memvalid + (size_t)b * maxlen;

  // QK-like contraction: key tiles 0..3 belong to waves 0..3 (acc), tile 4 (keys 128..159) is split over the waves by d
  // (four groups each, acc4) and summed through Pt, so every wave issues 80 MFMAs.  emit(key, r, value) receives the tile.
  // The contractions and the dS pass stay inline here: on vpt_attn_tile.h's helpers this kernel took 0.8962 ms against 0.8931 at the BC shape.
  auto qk_like = [&](const float* arow, int which, auto emit) __attribute__((always_inline)) {
    f32x16 acc, acc4;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[r] = 0.f; acc4[r] = 0.f; }
    const float* qa = arow ? arow + 4 * hi : nullptr;
    const float* kr = kv_row(jbase + w * 32 + l31, which);
    const float* kr4 = kv_row(jbase + 128 + l31, which);
    const float* kb = kr ? kr + 4 * hi : nullptr;
    const float* kb4 = kr4 ? kr4 + 4 * hi : nullptr;
#pragma unroll 8
    for (int g = 0; g < 16; ++g) {
      const f32x4 q4 = qa ? *(const f32x4*)(qa + 8 * g) : z4, k4 = kb ? *(const f32x4*)(kb + 8 * g) : z4;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.x, k4.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.y, k4.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.z, k4.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.w, k4.w, acc, 0, 0, 0);
    }
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int g = 4 * w + g4;
      const f32x4 q4 = qa ? *(const f32x4*)(qa + 8 * g) : z4, k4 = kb4 ? *(const f32x4*)(kb4 + 8 * g) : z4;
      acc4 = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.x, k4.x, acc4, 0, 0, 0);
      acc4 = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.y, k4.y, acc4, 0, 0, 0);
      acc4 = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.z, k4.z, acc4, 0, 0, 0);
      acc4 = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.w, k4.w, acc4, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) Pt[(w * 16 + r) * 64 + lane] = acc4[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) emit(w * 32 + l31, r, acc[r]);
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {   // key tile 4: this wave finishes accumulator registers 4 w .. 4 w + 3
      const int r = 4 * w + r4;
      emit(128 + l31, r, (Pt[(0 * 16 + r) * 64 + lane] + Pt[(1 * 16 + r) * 64 + lane]) + (Pt[(2 * 16 + r) * 64 + lane] + Pt[(3 * 16 + r) * 64 + lane]));
    }
    __syncthreads();
  };

  // ---- 1. logits (as the forward kernel) -> Ps ----
  qk_like(q_row(l31), 1, [&](int kk, int r, float dot) {
    const int qi = attn_acc_row(r, hi);
    const int off = maxlen - 1 + qi - kk;  // 0 = the query itself, maxlen-1 = oldest key in the band
    const int j = jbase + kk;
    bool vis = (q0 + qi) < t && off >= 0 && off < maxlen;
    if (vis && j < maxlen) vis = memv[j] != 0;
    vis = vis && j >= Ql[qi];
    float sc = -3.0e38f;
    if (vis) {
      float rb = 0.f;
#pragma unroll
      for (int n = 0; n < 10; ++n) rb = fmaf(Rs[qi * 10 + n], Bs[n * AB_BP + off], rb);
      sc = dot * inv_dh + rb;
    }
    Ps[qi * ATT_SS + kk] = sc;
  });
  // ---- softmax -> normalised P in Ps (8 rows per wave) ----
  attn_softmax_rows(Ps, w, lane);
  // ---- 2. dP = dO V^T -> Ds (its trailing barrier also publishes P) ----
  qk_like(do_row(l31), 2, [&](int kk, int r, float dot) { Ds[attn_acc_row(r, hi) * ATT_SS + kk] = dot; });
  // ---- 3. D_i = sum_k P dP;  dS = P (dP - D_i) -> Ds (0 where masked since P = 0) ----
  for (int r = w * 8; r < w * 8 + 8; ++r) {
    const float* prow = Ps + r * ATT_SS;
    float* drow = Ds + r * ATT_SS;
    const float p0 = prow[lane], p1 = prow[lane + 64], p2 = (lane + 128 < ATT_NK) ? prow[lane + 128] : 0.f;
    const float d0 = drow[lane], d1 = drow[lane + 64], d2 = (lane + 128 < ATT_NK) ? drow[lane + 128] : 0.f;
    const float Di = wave_sum(fmaf(p0, d0, fmaf(p1, d1, p2 * d2)));
    drow[lane] = p0 * (d0 - Di);
    drow[lane + 64] = p1 * (d1 - Di);
    if (lane + 128 < ATT_NK) drow[lane + 128] = p2 * (d2 - Di);
  }
  __syncthreads();

  const int dcol = w * 32 + l31;        // wave w owns d_head slice 32 w .. 32 w + 31 from here on
  const float* kmem_h = a.kmem + (size_t)b * maxlen * hid + h * ATT_DH;        // K rows of the memory / of the chunk, this head
  const float* kchunk_h = a.qkvr + tok0 * a.ld + hid + h * ATT_DH;
  // dV-like contraction: out[key][d] = scale * sum_query X[query][key] Y[query][d]; accumulated into the K / V columns of the
  // chunk's keys (memory keys are detached state: no gradient)
  auto dv_like = [&](const float* X, const float* ybase, int ystride, int which, float scale) __attribute__((always_inline)) {
    f32x16 acc[5];
#pragma unroll
    for (int kt = 0; kt < 5; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[kt][r] = 0.f;
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {   // not unrolled: eight wave-uniform row pointers per iteration live in scalar registers
      float y[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int qi = 8 * g + 4 * hi + e;          // this lane's query row of the k step
        y[e] = (qi < nq_valid) ? ybase[qi * ystride + dcol] : 0.f;
      }
#pragma unroll
      for (int kt = 0; kt < 5; ++kt) {
        const float* xc = X + (8 * g + 4 * hi) * ATT_SS + kt * 32 + l31;     // A: row = key, k = queries 8 g + 4 hi + e
        acc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xc[0], y[0], acc[kt], 0, 0, 0);
        acc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xc[ATT_SS], y[1], acc[kt], 0, 0, 0);
        acc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xc[2 * ATT_SS], y[2], acc[kt], 0, 0, 0);
        acc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xc[3 * ATT_SS], y[3], acc[kt], 0, 0, 0);
      }
    }
    // A key of the chunk is reached by up to five query tiles (its own and the four behind it).  Each writes its piece into a slab slot of its own --
    // slot = (this query tile) - (the key's 32-row tile), 0..4 -- and vpt_attn_bwd_finish_kernel adds the slots in slot order: bit-reproducible
    // (until round 5: fp32 atomics into dqkvr, i.e. sums in arrival order).  Rows beyond q0 + 31 lie outside the band (their pieces are exact
    // zeros) and are not written; the finish kernel knows which (row, slot) pairs exist from the same arithmetic.
    // wave-uniform base + one 32-bit per-lane index per element (80 64-bit vector addresses would not fit the register file)
    float* colbase = a.dkv_slab + tok0 * (2 * hid) + (which - 1) * hid + h * ATT_DH;
    const int slot_stride = a.B * t * 2 * hid;        // (the launcher checks 5 x this fits 31 bits)
    const int jr0 = jbase - maxlen + 4 * hi;          // chunk row of accumulator register 0 of key tile 0
#pragma unroll
    for (int kt = 0; kt < 5; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int jr = jr0 + kt * 32 + (r & 3) + 8 * (r >> 2);
        asm volatile("" : "+v"(jr));     // keep the validity test next to its store: hoisted and shared between the two calls, the 80 lane masks
                                         // were 160 scalar registers, all spilled
        if ((unsigned)jr < (unsigned)t && jr <= q0 + ATT_QT - 1)
          colbase[((int)blockIdx.x - (jr >> 5)) * slot_stride + jr * (2 * hid) + dcol] = acc[kt][r] * scale;
      }
  };
  // ---- 4. dV += P^T dO ;  5. dK += dS^T Q / d_h ----
  dv_like(Ps, dobase, hid, 2, 1.0f);
  dv_like(Ds, qbase, a.ld, 1, inv_dh);
  // ---- 6. dQ = dS K / d_h (PV-like) ----
  {
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    const float* pa = Ds + l31 * ATT_SS + 4 * hi;
#pragma unroll 2
    for (int g = 0; g < ATT_NK / 8; ++g) {
      const f32x4 p4 = *(const f32x4*)(pa + 8 * g);
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {          // per-LANE row arithmetic (32-bit offsets from two uniform bases), no wave-uniform pointer sets
        const int j = jbase + 8 * g + 4 * hi + e;
        const float* rr = (j < maxlen) ? kmem_h + (size_t)j * hid : ((j - maxlen < t) ? kchunk_h + (size_t)(j - maxlen) * a.ld : nullptr);
        v[e] = rr ? rr[dcol] : 0.f;
      }
      o = __builtin_amdgcn_mfma_f32_32x32x2f32(p4.x, v[0], o, 0, 0, 0);
      o = __builtin_amdgcn_mfma_f32_32x32x2f32(p4.y, v[1], o, 0, 0, 0);
      o = __builtin_amdgcn_mfma_f32_32x32x2f32(p4.z, v[2], o, 0, 0, 0);
      o = __builtin_amdgcn_mfma_f32_32x32x2f32(p4.w, v[3], o, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qi = attn_acc_row(r, hi);
      if (q0 + qi < t) a.dqkvr[(tok0 + q0 + qi) * a.ld + h * ATT_DH + dcol] = o[r] * inv_dh;
    }
  }
  // ---- 7. dR[qi][n] = sum_kk dS B[n][off];  db_nd[n][off] += sum_qi dS R[qi][n] ----
  for (int idx = tid; idx < ATT_QT * 10; idx += 256) {
    const int r = idx / 10, n = idx - r * 10;
    float s = 0.f;
    for (int kk = 0; kk < ATT_NK; ++kk) {
      const int off = maxlen - 1 + r - kk;
      if (off >= 0 && off < maxlen) s = fmaf(Ds[r * ATT_SS + kk], Bs[n * AB_BP + off], s);
    }
    if (q0 + r < t) a.dqkvr[(tok0 + q0 + r) * a.ld + 3 * hid + h * 10 + n] = s;
  }
  for (int idx = tid; idx < 10 * maxlen; idx += 256) {
    const int n = idx / maxlen, off = idx - n * maxlen;
    float s = 0.f;
    for (int r = 0; r < ATT_QT; ++r) {
      const int kk = maxlen - 1 + r - off;
      if (kk >= 0 && kk < ATT_NK) s = fmaf(Ds[r * ATT_SS + kk], Rs[r * 10 + n], s);
    }
    dbnd_row[idx] = s;      // this workgroup's row of the slab; vpt_slab_sum adds the rows in row order (until round 5: an fp32 atomic per entry)
  }
}

// dqkvr[token][K and V columns] = sum over the slots that exist for the token's row, in slot order (see dv_like above).  One thread per float4.
__global__ __launch_bounds__(256) void vpt_attn_bwd_finish_kernel(VptAttnBwdArgs a) {
  const int c4n = (2 * a.hid) >> 2;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)a.B * a.t * c4n) return;
  const int tok = (int)(i / c4n), c4 = (int)(i - (long)tok * c4n);
  const int jr = tok % a.t, kt = jr >> 5;
  const size_t slot_stride = (size_t)a.B * a.t * 2 * a.hid;
  const float* p = a.dkv_slab + (size_t)tok * (2 * a.hid) + 4 * c4;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int sl = 0; sl < 5; ++sl) {
    const int q0 = (kt + sl) * ATT_QT;              // the query tile of slot sl
    if (q0 < a.t && jr >= q0 - a.maxlen + 1) {      // it exists and its band reaches back to this row
      const f32x4 v = *(const f32x4*)(p + sl * slot_stride);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  *(f32x4*)(a.dqkvr + (size_t)tok * a.ld + a.hid + 4 * c4) = s;
}

extern "C" long vpt_attn_bwd_dkv_floats(int B, int t, int hid) { return 5L * B * t * 2 * hid; }
// rows of the db_nd slab (one per workgroup) followed by vpt_slab_sum's scratch
extern "C" long vpt_attn_bwd_dbnd_floats(int B, int t, int heads, int maxlen) {
  const long rows = (long)((t + ATT_QT - 1) / ATT_QT) * B * heads;
  return rows * 10 * maxlen + vpt_slab_sum_scratch_floats((int)rows, 10 * maxlen);
}

extern "C" int vpt_attn_bwd_launch(const VptAttnBwdArgs* a, hipStream_t stream) {
  if (a->hid != a->heads * ATT_DH || a->maxlen < 1 || a->maxlen > 129 || !a->dkv_slab || !a->dbnd_slab || (a->ld & 3)) return -1;
  if (vpt_attn_bwd_dkv_floats(a->B, a->t, a->hid) > 0x7fffffffL) return -2;       // 32-bit slab indices in the kernel
  static unsigned long long optin_done = 0;
  const size_t lds = AB_FLOATS * sizeof(float);
  if (!vpt_lds_optin((const void*)vpt_attn_bwd_kernel, (int)lds, &optin_done)) return -4;
  dim3 grid((a->t + ATT_QT - 1) / ATT_QT, a->B * a->heads);
  const long rows = (long)grid.x * grid.y;
  if (rows > 65536) return -2;
  hipLaunchKernelGGL(vpt_attn_bwd_kernel, grid, dim3(256), lds, stream, *a);
  const long n4 = (long)a->B * a->t * ((2 * a->hid) >> 2);
  hipLaunchKernelGGL(vpt_attn_bwd_finish_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, *a);
  if (hipGetLastError() != hipSuccess) return -3;
  return vpt_slab_sum_launch(a->dbnd_slab, (int)rows, 10 * a->maxlen, 10L * a->maxlen, a->db_nd, 10 * a->maxlen, nullptr, 1,
                             a->dbnd_slab + rows * 10 * a->maxlen, stream);
}

// ------------------------------------------------------------------------------------------------
// Backward of vpt_attn_kernel with causal = 0 -- the inverse-dynamics model's attention (mask "none", lib/masked_attention.py:139-141, lib/xf.py
// with maxlen = 0): every query of a window sees all t <= 160 rows of the window, no memory, no relative-position bias.
//   out_i = sum_j P_ij V_j,  P = softmax_j(Q_i . K_j / d_h);  D_i = sum_j P_ij (dO_i . V_j);  dS = P (dP - D);
//   dQ = dS K / d_h;  dK = dS^T Q / d_h;  dV = P^T dO.
// One workgroup per (window, head, 32-query tile), the contractions on the fp32 matrix cores exactly as vpt_attn_bwd_kernel lays them out (same
// lane -> operand maps; P is recomputed from qkv, the forward keeps nothing).  Rows >= t of a partial tile load zeros, their scores are masked,
// so they add exact zeros to every sum.  Every key is reached by all ceil(t / 32) query tiles: tile q writes its piece of dK / dV to slab slot q
// and vpt_full_attn_bwd_finish_kernel adds the slots in slot order -- no atomics, the grid is a function of (B, t, heads) alone and a window's
// workgroups read and write that window's rows only, so a window's result does not depend on its neighbours.
#define FA_P_OFF 0                                        // P  [32][ATT_SS]
#define FA_D_OFF (FA_P_OFF + ATT_QT * ATT_SS)             // dP, then dS  [32][ATT_SS]
#define FA_PT_OFF (FA_D_OFF + ATT_QT * ATT_SS)            // partial tiles of key tile 4: [wave][16][64]
#define FA_FLOATS (FA_PT_OFF + 4 * 16 * 64)               // 58 368 bytes: two workgroups per CU

__global__ __launch_bounds__(256, 2) void vpt_full_attn_bwd_kernel(VptFullAttnBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float sm[FA_FLOATS];
  float* Ps = sm + FA_P_OFF;
  float* Ds = sm + FA_D_OFF;
  float* Pt = sm + FA_PT_OFF;

  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const int b = blockIdx.y / a.heads, h = blockIdx.y - b * a.heads;
  const int q0 = blockIdx.x * ATT_QT;
  const int t = a.t, hid = a.hid;
  const size_t tok0 = (size_t)b * t;
  const float inv_dh = 1.0f / ATT_DH;
  const float* qbase = a.qkv + (tok0 + q0) * a.ld + h * ATT_DH;          // this tile's Q rows / dO rows, this head
  const float* dobase = a.dout + (tok0 + q0) * hid + h * ATT_DH;
  const float* kbase = a.qkv + tok0 * a.ld + hid + h * ATT_DH;           // the window's K rows; V sits hid columns further
  const int nq_valid = t - q0;                                           // queries q0 + qi with qi < nq_valid exist

  // QK-like contraction of this lane's row `arow` with the window's K (voff = 0) / V (voff = hid) rows
  auto qk_like = [&](const float* arow, int voff, auto emit) __attribute__((always_inline)) {
    const int k0 = w * 32 + l31, k4 = 128 + l31;
    attn_qk_tile(arow ? arow + 4 * hi : nullptr, (k0 < t) ? kbase + (size_t)k0 * a.ld + voff + 4 * hi : nullptr,
                 (k4 < t) ? kbase + (size_t)k4 * a.ld + voff + 4 * hi : nullptr, Pt, w, lane, l31, emit);
  };

  // ---- 1. logits (as the forward kernel: dot / d_h where query and key exist) -> Ps ----
  qk_like((l31 < nq_valid) ? qbase + l31 * a.ld : nullptr, 0, [&](int kk, int r, float dot) {
    const int qi = attn_acc_row(r, hi);
    Ps[qi * ATT_SS + kk] = (qi < nq_valid && kk < t) ? dot * inv_dh : -3.0e38f;
  });
  // ---- softmax -> normalised P in Ps (8 rows per wave); a row that does not exist is all zeros ----
  attn_softmax_rows(Ps, w, lane);
  // ---- 2. dP = dO V^T -> Ds (its trailing barrier also publishes P) ----
  qk_like((l31 < nq_valid) ? dobase + l31 * hid : nullptr, hid, [&](int kk, int r, float dot) { Ds[attn_acc_row(r, hi) * ATT_SS + kk] = dot; });
  // ---- 3. D_i = sum_k P dP;  dS = P (dP - D_i) -> Ds (0 where the key or the query does not exist since P = 0) ----
  attn_ds_rows(Ps, Ds, w, lane);
  __syncthreads();

  const int dcol = w * 32 + l31;        // wave w owns d_head slice 32 w .. 32 w + 31 from here on
  // dV-like contraction (M = keys, N = d_head, K = the tile's queries): piece[key][d] = scale * sum_query X[query][key] Y[query][d] -> this query
  // tile's slab slot, column block `cb` (0: dK, 1: dV).  Key tiles beyond the window are skipped (wave-uniform).
  auto dv_like = [&](const float* X, const float* ybase, int ystride, int cb, float scale) __attribute__((always_inline)) {
    f32x16 acc[5];
    attn_dv_tile(acc, X, ybase, ystride, nq_valid, t, dcol, l31, hi);
    // wave-uniform base + one 32-bit per-lane index per element (the launcher checks that the slab fits 31 bits)
    float* colbase = a.dkv_slab + ((size_t)blockIdx.x * a.B * t + tok0) * (2 * hid) + cb * hid + h * ATT_DH;
#pragma unroll
    for (int kt = 0; kt < 5; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int jr = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        asm volatile("" : "+v"(jr));     // keep the row test next to its store (vpt_attn_bwd_kernel: hoisted, the 80 lane masks spill)
        if (jr < t) colbase[jr * (2 * hid) + dcol] = acc[kt][r] * scale;
      }
  };
  // ---- 4. dV piece = P^T dO ;  5. dK piece = dS^T Q / d_h ----
  dv_like(Ps, dobase, hid, 1, 1.0f);
  dv_like(Ds, qbase, a.ld, 0, inv_dh);
  // ---- 6. dQ = dS K / d_h (PV-like: M = queries, N = d_head, K = keys) ----
  {
    const f32x16 o = attn_pv_tile(Ds + l31 * ATT_SS + 4 * hi, [&](int g, int e) {
      const int j = 8 * g + 4 * hi + e;
      return (j < t) ? kbase[(size_t)j * a.ld + dcol] : 0.f;
    });
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qi = attn_acc_row(r, hi);
      if (qi < nq_valid) a.dqkv[(tok0 + q0 + qi) * a.ld + h * ATT_DH + dcol] = o[r] * inv_dh;
    }
  }
}

// dqkv[token][hid .. ld): dK and dV = the sum over the ceil(t / 32) slab slots in slot order, zeros in the columns >= 3 hid.  One thread per float4.
__global__ __launch_bounds__(256) void vpt_full_attn_bwd_finish_kernel(VptFullAttnBwdArgs a) {
  const int c4n = (a.ld - a.hid) >> 2, kv4 = (2 * a.hid) >> 2;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)a.B * a.t * c4n) return;
  const long tok = i / c4n;
  const int c4 = (int)(i - tok * c4n);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (c4 < kv4) {
    const int slots = (a.t + ATT_QT - 1) / ATT_QT;
    const size_t slot_stride = (size_t)a.B * a.t * 2 * a.hid;
    const float* p = a.dkv_slab + (size_t)tok * (2 * a.hid) + 4 * c4;
    for (int sl = 0; sl < slots; ++sl) {
      const f32x4 v = *(const f32x4*)(p + sl * slot_stride);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  *(f32x4*)(a.dqkv + (size_t)tok * a.ld + a.hid + 4 * c4) = s;
}

extern "C" long vpt_full_attn_bwd_dkv_floats(int B, int t, int hid) { return (long)((t + ATT_QT - 1) / ATT_QT) * B * t * 2 * hid; }

extern "C" int vpt_full_attn_bwd_launch(const VptFullAttnBwdArgs* a, hipStream_t stream) {
  if (a->B <= 0 || a->t < 1 || a->t > ATT_NK || a->heads <= 0 || a->hid != a->heads * ATT_DH || a->ld < 3 * a->hid || (a->ld & 3)) return -1;
  if (!a->qkv || !a->dout || !a->dqkv || !a->dkv_slab) return -1;
  if (vpt_full_attn_bwd_dkv_floats(a->B, a->t, a->hid) > 0x7fffffffL || (long)a->B * a->heads > 65535) return -2;       // 32-bit slab indices, grid.y
  dim3 grid((a->t + ATT_QT - 1) / ATT_QT, a->B * a->heads);
  hipLaunchKernelGGL(vpt_full_attn_bwd_kernel, grid, dim3(256), 0, stream, *a);
  const long n4 = (long)a->B * a->t * ((a->ld - a->hid) >> 2);
  hipLaunchKernelGGL(vpt_full_attn_bwd_finish_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
