// The 32-query attention tile of vpt_attn_kernel (vpt_transformer.hip), vpt_attn_bwd_kernel and vpt_full_attn_bwd_kernel (vpt_attn_bwd.hip):
// the tile's constants, the accumulator-row map and the softmax row, which all three use, and one body of each contraction and of the dS row pass,
// which vpt_full_attn_bwd_kernel uses.  The forward and the banded backward keep their own copies of the contractions: on these helpers the compiler
// schedules them differently and they measured 0.4 - 0.6 % slower (profiles/attention_tile.md), so there the helpers are the text to edit the copies against.  256 threads = 4 waves per tile; every
// contraction runs on the fp32 matrix cores (v_mfma_f32_32x32x2_f32) with its operands taken straight from global memory (each element is used by
// exactly one lane) or from the 32 x 160 score tiles in LDS:
//   "QK-like"  (logits, dP):  M = queries, N = keys, K = d_head; A = a query row, B = a key row, both contiguous in d.
//   "PV-like"  (out, dQ):     M = queries, N = d_head, K = keys;  A = a score row (LDS, contiguous in keys), B = key / value rows.
//   "dV-like"  (dV, dK):      M = keys,    N = d_head, K = queries; A = a score column (LDS), B = query rows.
// A lane (l31 = lane & 31, hi = lane >> 5) supplies the k values 8 g + 4 hi + e, e = 0..3, of group g in every case (the k order of an MFMA step is
// free as long as both operands agree).  The LDS layouts and the bias pitch belong to the kernels.  The results of all three kernels are pinned bit
// for bit (tests/test_gpu_attention_bitwise.py): a change here keeps every summation order, parenthesisation, sentinel and rounding point.
#pragma once
#include "vpt_common.h"

#define ATT_DH 128
#define ATT_QT 32
#define ATT_NK 160                      // keys staged per query tile (31 + maxlen, maxlen <= 129)
#define ATT_SS 164                      // padded score row (16-byte aligned: the PV-like A operand is read as float4)

// accumulator register r of a lane = row (r & 3) + 8 (r >> 2) + 4 hi of the 32 x 32 tile, column l31
__device__ __forceinline__ int attn_acc_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// QK-like contraction.  qa / kb / kb4: this lane's query row, its key row of the wave's own tile and of tile 4, each + 4 hi, or null (zeros).
// Key tiles 0..3 belong to waves 0..3, tile 4 (keys 128..159) is split over the waves by d (four groups each) and summed through
// Pt ([wave][16][64] floats of LDS), so every wave issues 80 MFMAs.  emit(key, r, value) receives accumulator register r of the wave's own tile
// and registers 4 w .. 4 w + 3 of tile 4; the trailing barrier publishes what it stored.
template <class Emit>
__device__ __forceinline__ void attn_qk_tile(const float* qa, const float* kb, const float* kb4, float* Pt, int w, int lane, int l31, Emit emit) {
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x16 acc, acc4;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc[r] = 0.f; acc4[r] = 0.f; }
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
}

// One row of the 32 x 164 score tile (a wave's lanes hold keys lane, lane + 64, lane + 128): the exponentials against the row maximum, exact zeros for
// masked keys (score -3.0e38f), and inv = 1 / their sum (0 for a row without a visible key).  The caller stores e (and keeps inv) or e * inv.
struct AttnSoftmaxRow { float e0, e1, e2, inv; };
__device__ __forceinline__ AttnSoftmaxRow attn_softmax_row(const float* srow, int lane) {
  const float s0 = srow[lane], s1 = srow[lane + 64], s2 = (lane + 128 < ATT_NK) ? srow[lane + 128] : -3.0e38f;
  const float m = wave_max(fmaxf(s0, fmaxf(s1, s2)));
  AttnSoftmaxRow x;
  x.e0 = (s0 > -1.0e38f) ? expf(s0 - m) : 0.f;
  x.e1 = (s1 > -1.0e38f) ? expf(s1 - m) : 0.f;
  x.e2 = (s2 > -1.0e38f) ? expf(s2 - m) : 0.f;
  const float tot = wave_sum(x.e0 + x.e1 + x.e2);
  x.inv = (tot > 0.f) ? 1.0f / tot : 0.f;
  return x;
}

// softmax -> normalised P in place, the wave's 8 rows of the tile (the backward kernels; a row without a visible key is all zeros)
__device__ __forceinline__ void attn_softmax_rows(float* Ps, int w, int lane) {
  for (int r = w * 8; r < w * 8 + 8; ++r) {
    float* srow = Ps + r * ATT_SS;
    const AttnSoftmaxRow x = attn_softmax_row(srow, lane);
    srow[lane] = x.e0 * x.inv;
    srow[lane + 64] = x.e1 * x.inv;
    if (lane + 128 < ATT_NK) srow[lane + 128] = x.e2 * x.inv;
  }
}

// D_i = sum_k P dP;  dS = P (dP - D_i) -> Ds, the wave's 8 rows (0 where masked since P = 0)
__device__ __forceinline__ void attn_ds_rows(const float* Ps, float* Ds, int w, int lane) {
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
}

// dV-like contraction: acc[key tile][.] = sum_query X[query][key] Y[query][d] over the tile's 32 queries, for the wave's d_head column dcol.
// X: a score tile in LDS; Y[query] = ybase + query * ystride (query rows >= nq_valid are zeros).  Key tiles at or beyond the window length t
// are skipped (wave-uniform).
__device__ __forceinline__ void attn_dv_tile(f32x16 (&acc)[5], const float* X, const float* ybase, int ystride, int nq_valid, int t, int dcol, int l31, int hi) {
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
      if (kt * 32 < t) {
        const float* xc = X + (8 * g + 4 * hi) * ATT_SS + kt * 32 + l31;     // A: row = key, k = queries 8 g + 4 hi + e
        acc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xc[0], y[0], acc[kt], 0, 0, 0);
        acc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xc[ATT_SS], y[1], acc[kt], 0, 0, 0);
        acc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xc[2 * ATT_SS], y[2], acc[kt], 0, 0, 0);
        acc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xc[3 * ATT_SS], y[3], acc[kt], 0, 0, 0);
      }
    }
  }
}

// PV-like contraction: o[query][d] = sum_key S[query][key] B[key][d] over the 160 staged keys.  pa: this lane's score row + 4 hi (LDS);
// value(g, e) supplies B[key 8 g + 4 hi + e][the lane's d column], zero where the key does not exist -- how it forms the row address (scalar
// pointers with a select on hi, or per-lane offsets) is the kernel's register-pressure choice.
template <class Value>
__device__ __forceinline__ f32x16 attn_pv_tile(const float* pa, Value value) {
  f32x16 o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll 2
  for (int g = 0; g < ATT_NK / 8; ++g) {
    const f32x4 p4 = *(const f32x4*)(pa + 8 * g);
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = value(g, e);
    o = __builtin_amdgcn_mfma_f32_32x32x2f32(p4.x, v[0], o, 0, 0, 0);
    o = __builtin_amdgcn_mfma_f32_32x32x2f32(p4.y, v[1], o, 0, 0, 0);
    o = __builtin_amdgcn_mfma_f32_32x32x2f32(p4.z, v[2], o, 0, 0, 0);
    o = __builtin_amdgcn_mfma_f32_32x32x2f32(p4.w, v[3], o, 0, 0, 0);
  }
  return o;
}
