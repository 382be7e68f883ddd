"""References for the low-rank adapter path: plain torch / numpy, fp64, importable without a GPU.  Instruments and notation are
tests/linear_ref.py's (D, U32, ulp16, ints, reals, linear_ref, wgrad_ref, bound, exact_failure, bound_ratio).

An adapted linear is  y = epi(x W^T (+) u16 (sB)^T),  u16 = rnd16(x A^T):  three GEMMs and the split-K epilogue.  The references read THE OPERANDS
THE KERNELS READ: x, and W, A (stacked, rank padded to R, a multiple of 64) and sB (= s B formed in fp32) each rounded ONCE to the 16-bit format.

1. EXACT INTEGERS.  x, A in {-1, +1}: u is an integer with |u| <= K <= 256, which 8 significant bits hold exactly, so u16 = u in bf16 and in
   fp16 -- the forward's 16-bit rounding between the two stages is the identity.  B, W, dy from linear_ref.ints (|.| <= 8) and s a power of two
   keep sB and every product and partial sum a multiple of s below 2^24: fp32 outputs equal the exact value, 16-bit outputs its one RNE
   rounding.  In the backward du = dy (sB) outgrows 8 bits, so du16 is checked as the ONE rounding of the exact du and the reference carries that
   rounded value on (its products with A = +-1 and x = +-1 are exact again): still bit for bit, no tolerance anywhere.

2. REAL VALUES, THE TWO-STAGE BOUND.  Stage one,  u16 = rnd16(u32),  u32 the GEMM's fp32 result over K terms in S_u slices:
       |u16 - u64| <= du := bound(sum_k |x||A|, K, S_u) + ulp16(u64)                                   (linear_ref.bound16)
   Stage two sums K base products and R low-rank products into S + 1 slices and applies the epilogue; against y64 formed with the EXACT u64:
       |y - y64| <= bound(mag, K + R, S + 1)  +  sum_j |sB_nj| du_mj,        mag = sum_k |x||W| + sum_j (|u64| + du)_mj |sB_nj| + |bias| + |res|
   -- the first term is linear_ref.bound over the total reduction length and slice count (the magnitudes taken with the perturbed u), the second
   carries stage one's error through the second product (sB is an exact operand).  ReLU is 1-Lipschitz and the gate multiplies by 0 or 1, so
   both are taken on pre-activation magnitudes.  A 16-bit output adds ulp16(y64).
   The backward is the same shape:  du16 = rnd16(dy (sB))  is stage one with (dy, (sB)^T);  dx = epi(dy W (+) du16 A)  is stage two with
   (dy, W^T, du, A^T).  The adapter gradients are TN GEMMs over the M rows reading one rounded operand:
       d a_stack = du16^T x:    |.| <= bound((|du64| + ddu)^T |x|, M) + ddu^T |x|
       d sb      = dy^T u16:    |.| <= bound(|dy|^T (|u64| + du), M) + |dy|^T du,      dB = s x its diagonal block: one more rounding, 2^-24 |dB|.

3. THE MERGE (vpt_lowrank_merge):  out = W + s sum_j B_ij A_jk  in fp32, j ascending, no contraction.  merge_f32 restates it in float32 numpy
   (bit-equal to the kernel); against fp64 each product passes through at most 1 (itself) + (r - 1) (adds; the first lands on 0 exactly) + 1 (s)
   + 1 (the add to W) roundings:   |out - out64| <= (r + 2) 2^-24 (|W| + s sum_j |B||A|)."""
import numpy as np
import torch

from tests.linear_ref import D, DT, U32, bound, bound_ratio, exact_failure, ints, linear_ref, reals, ulp16, wgrad_ref  # noqa: F401


def rnd16(t, fmt):
    """One rounding to the 16-bit format, returned in fp64 (the value the kernels' operand holds)."""
    return t.to(torch.float32).to(DT[fmt]).to(D)


def signs(gen, *shape):
    """+-1 (fp32 tensor)."""
    return (torch.randint(0, 2, shape, generator=gen) * 2 - 1).float()


def stage_one(x, a, k_slices, fmt):
    """u64 = x a^T and du, the bound on |u16 - u64| (x [M, K], a [R, K]: operand values)."""
    u64, mag = linear_ref(x, a)
    return u64, bound(mag, x.shape[1], k_slices) + ulp16(u64, fmt)


def adapted_ref(x, w, a, sb, fmt, bias=None, relu=False, mask=None, res=None, slices=1, u_slices=1, out16=False):
    """fp64 adapted linear over operand values x [M, K], w [n, K], a [R, K], sb [n, R] -> (y64, bound [M, n], u64, du).
    slices / u_slices: the K slices of the base GEMM / of the u GEMM (1 unless ops.linear splits K)."""
    x, w, a, sb = x.to(D), w.to(D), a.to(D), sb.to(D)
    u64, du = stage_one(x, a, u_slices, fmt)
    y = x @ w.t() + u64 @ sb.t()
    mag = x.abs() @ w.abs().t() + (u64.abs() + du) @ sb.abs().t()
    if bias is not None:
        y = y + bias.to(D)
        mag = mag + bias.to(D).abs()
    if relu:
        y = torch.relu(y)
    if mask is not None:
        y = torch.where(mask.to(D)[:, :y.shape[1]] > 0, y, torch.zeros_like(y))
    if res is not None:
        y = y + res.to(D)
        mag = mag + res.to(D).abs()
    bnd = bound(mag, x.shape[1] + a.shape[0], slices + 1) + du @ sb.abs().t()
    if out16:
        bnd = bnd + ulp16(y, fmt)
    return y, bnd, u64, du


def da_ref(du64, ddu, x):
    """d a_stack = du16^T x  -> (fp64 [R, K] from the exact du64, bound)."""
    du64, ddu, x = du64.to(D), ddu.to(D), x.to(D)
    return du64.t() @ x, bound((du64.abs() + ddu).t() @ x.abs(), x.shape[0]) + ddu.t() @ x.abs()


def db_ref(dy, u64, du, n, s=1.0):
    """s dy[:, :n]^T u16  -> (fp64 [n, R] from the exact u64, bound); s: the fp32 factor applied to the GEMM's fp32 result (one rounding)."""
    dy, u64, du = dy.to(D)[:, :n], u64.to(D), du.to(D)
    v = dy.t() @ u64
    b = bound(dy.abs().t() @ (u64.abs() + du), dy.shape[0]) + dy.abs().t() @ du
    return s * v, abs(s) * b + U32 * (abs(s) * v).abs()


# ---- the merge ----------------------------------------------------------------------------------------------------------------------------
def merge_f32(w, a, b, s):
    """The kernel's lines in float32 numpy: acc = 0; acc = acc + B[:, j] * A[j, :] for j ascending (each product and each sum rounded to fp32 on
    its own); out = W + s * acc.  w [n, K], a [r, K], b [n, r] float32 arrays -> float32 [n, K]."""
    w, a, b = (np.asarray(t, dtype=np.float32) for t in (w, a, b))
    acc = np.zeros_like(w)
    for j in range(a.shape[0]):
        p = b[:, j:j + 1] * a[j:j + 1, :]
        acc = acc + p
    u = np.float32(s) * acc
    return w + u


def merge_ref(w, a, b, s):
    """-> (out64, bound) = (W + s B A in fp64, (r + 2) 2^-24 (|W| + |s| |B||A|)); s enters as the fp32 value the kernel receives."""
    w, a, b = (torch.as_tensor(np.asarray(t)).to(D) for t in (w, a, b))
    s = float(np.float32(s))
    return w + s * (b @ a), (a.shape[0] + 2) * U32 * (w.abs() + abs(s) * (b.abs() @ a.abs()))
