"""References for the linear-layer kernels (vpt_gemm.hip, vpt_gemv.hip): plain torch, fp64, importable without a GPU.

Two instruments.

1. EXACT INTEGERS (index mapping).  Operands drawn from the nonzero integers -8 .. 8 are exact in bf16 and fp16, every product is exact in
   fp32 and every partial sum stays below 2^24 up to K = 65536 (64 * 65536 = 2^22), so EVERY correct summation order gives the same integer:
   the fp32 output must equal it and the 16-bit output must be its one RNE rounding, bit for bit.  A dropped, duplicated or misplaced product,
   row or column fails on every element it touches, at any K.

2. REAL VALUES UNDER A DERIVED BOUND (rounding points).  randn operands rounded to the 16-bit format, reference in fp64 over the same operands:

       fp32 output:    |y - y64| <= (K + 8 + S) * 2^-24 * (sum_k |a||w| + |bias| + |res|)
       16-bit output:  the same + ulp16(y64)

   K = reduction length (M for the weight gradient), S = number of K slices summed.  Products of two 8-bit or two 11-bit significands are exact
   in fp32; each of the K - 1 additions of the accumulation, the S - 1 of the slice sum and the epilogue's few (bias, residual) costs at most
   2^-24 relative to a partial result that |.|-sums bound.  ReLU is 1-Lipschitz and the gate multiplies by exactly 0 or 1, so the bound is taken
   on the pre-activation magnitudes.  O(K): used at K <= 256 only, where one lost product (~ 1 / sqrt(K) of an output's standard deviation) is still
   ~100 x the bound.

The fold epilogue of the dense layer (vpt_dense_fold_epilogue) has its own bound, derived at dense_fold_ref()."""
import torch

D = torch.float64
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
MANT = {"bf16": 7, "fp16": 10}
EMIN = {"bf16": -126, "fp16": -14}
U32 = 2.0 ** -24          # unit roundoff of fp32


def fmt_of(dt):
    return {v: k for k, v in DT.items()}[dt]


def ulp16(v, fmt):
    """One unit in the last place of the 16-bit format at |v| (the form of tests/test_gpu_conv_mfma16.py)."""
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** EMIN[fmt]))).clamp(min=EMIN[fmt])
    return torch.pow(torch.tensor(2.0, dtype=D), e - MANT[fmt])


def ints(gen, *shape):
    """Nonzero integers -8 .. 8 (fp32 tensor): exact in bf16 and fp16."""
    mag = torch.randint(1, 9, shape, generator=gen)
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (mag * sign).float()


def reals(gen, fmt, *shape, scale=1.0):
    """randn * scale rounded to the 16-bit format (returned in that format)."""
    return (torch.randn(*shape, generator=gen) * scale).to(DT[fmt])


def linear_ref(a, w, bias=None, relu=False, mask=None, res=None):
    """fp64 linear layer with every epilogue stage in the kernels' order: a w^T -> + bias -> ReLU -> gate (zero where mask <= 0) -> + res.
    -> (y64 [M, N], mag [M, N] = sum_k |a||w| + |bias| + |res|, the magnitude the bound scales with).  On integer operands y64 is exact."""
    a, w = a.to(D), w.to(D)
    y = a @ w.t()
    mag = a.abs() @ w.abs().t()
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
    return y, mag


def exact(a, w, bias=None, relu=False, mask=None, res=None):
    """The integer result of the layer (fp64 arithmetic is exact on the integer generator's data)."""
    return linear_ref(a, w, bias, relu, mask, res)[0]


def wgrad_ref(dy, x, n, base=None):
    """dW [n, K] = dy[:, :n]^T x (+ base): the TN GEMM.  -> (dw64, mag); the reduction length is M = dy.shape[0]."""
    dy, x = dy.to(D)[:, :n], x.to(D)
    dw = dy.t() @ x
    mag = dy.abs().t() @ x.abs()
    if base is not None:
        dw = dw + base.to(D)
        mag = mag + base.to(D).abs()
    return dw, mag


def bound(mag, k, s=1):
    """fp32 output: (K + 8 + S) * 2^-24 * mag."""
    return (k + 8 + s) * U32 * mag


def bound16(y64, mag, k, fmt, s=1):
    return bound(mag, k, s) + ulp16(y64, fmt)


def first_bad(bad):
    """(row, col) of the first True of a 2-D mask, or None."""
    nz = bad.nonzero()
    return tuple(nz[0].tolist()) if nz.numel() else None


def exact_failure(out, want64, what=""):
    """None when `out` is `want64` held in out's format after ONE rounding to nearest even (fp32: want64 itself, which is an integer below 2^24),
    compared bit for bit; else a message with the shape, the count and the first failing (row, col)."""
    want = want64.to(out.dtype)
    if tuple(out.shape) != tuple(want.shape):
        return f"{what}: shape {tuple(out.shape)}, expected {tuple(want.shape)}"
    it = torch.int32 if out.dtype == torch.float32 else torch.int16
    bad = out.contiguous().view(it) != want.contiguous().view(it)
    if not bool(bad.any()):
        return None
    idx = first_bad(bad.reshape(-1, bad.shape[-1]))
    return (f"{what}: {int(bad.sum())} of {bad.numel()} elements of the {tuple(out.shape)} {out.dtype} output differ from the exact result; "
            f"first at (row, col) = {idx}: got {out.reshape(-1, out.shape[-1])[idx].item()}, exact {want64.reshape(-1, out.shape[-1])[idx].item()}")


def bound_ratio(out, y64, bnd):
    """-> (worst err / bound over ALL elements, message or None)."""
    err = (out.to(D) - y64).abs()
    ratio = err / bnd
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)       # 0 / 0 (an all-zero row under a zero bound) is no error
    worst = ratio.max().item()
    if worst <= 1.0 and bool(torch.isfinite(out).all()):
        return worst, None
    bad = ~(ratio <= 1.0)
    idx = first_bad(bad)
    return worst, (f"{int(bad.sum())} of {bad.numel()} elements of the {tuple(out.shape)} {out.dtype} output beyond the bound (worst ratio {worst:.3f}); "
                   f"first at (row, col) = {idx}: got {out[idx].item()}, fp64 {y64[idx].item()}, bound {bnd[idx].item():.3e}")


# ---- vpt_dense_fold_epilogue: out[f][n] = rstd_f * sum_s part[s][f][n] - rstd_f * mean_f * sg[n] + sb[n] --------------------------------------------
#
# The kernel takes (mean_f, rstd_f) from the fp64 frame statistics (sum, sum of squares) with var = ss / count - mean^2 in fp64, rounds mean and var to fp32,
# adds eps in fp32 and takes rsqrtf (<= 1 ulp = 2^-23), sums the S partials in fp32, and evaluates fma(rstd, v, fma(-rstd * mean, sg, sb)).  Relative errors, in
# units of u = 2^-24:  rstd: float(var) and (+ eps) one each, halved by the power -1/2 -> 1, rsqrtf 2, together <= 3 (taken as 4);  mean: 1.
#     term rstd * v:         (S - 1) for the slice sum + 4 for rstd + 1 for the outer fma's rounding            = S + 4
#     term rstd * mean * sg: 4 + 1 (mean) + 1 (the product rstd * mean) + 1 (inner fma) + 1 (outer fma)        = 8
#     term sb:               inner + outer fma                                                                  = 2
# each relative to the term's magnitude, so
#     |out - out64| <= (S + 8) * 2^-24 * (rstd * sum_s |part_s| + |rstd * mean * sg| + |sb|)
# holds with room for the second-order terms.  A frame with a large |mean| * rstd makes the second term dominate the result: the case that pins its sign,
# its column index and the fp64 variance.
EPS = 1e-5


def dense_fold_ref(part, stats, count, sg, sb):
    """-> (out64 [M, N], bound [M, N]) from the same partial slices [S, M, N] and frame statistics [M, 2] (fp64) the kernel reads."""
    part, sg, sb = part.to(D), sg.to(D), sb.to(D)
    mean = stats[:, 0] * (1.0 / count)
    var = (stats[:, 1] * (1.0 / count) - mean * mean).clamp(min=0)
    rstd = (1.0 / torch.sqrt(var + EPS)).view(-1, 1)
    mean = mean.view(-1, 1)
    out = rstd * part.sum(0) - rstd * mean * sg.view(1, -1) + sb.view(1, -1)
    mag = rstd * part.abs().sum(0) + (rstd * mean * sg.view(1, -1)).abs() + sb.view(1, -1).abs()
    return out, (part.shape[0] + 8) * U32 * mag
