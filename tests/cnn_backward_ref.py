"""fp64 reference of the CNN backward kernels with the ReLU gates PINNED to the stored tensors, and the per-element error bounds the
kernels are held to.  A plain helper (no test, no fixture): torch on the CPU only, nothing of vpt_amd.

Every backward kernel takes its gate from a stored 16-bit tensor (prepare: y - res > 0; pooled prepare: P > 0; gated dgrad: xin > 0).
The functions below read the SAME stored values (NCHW fp64 tensors holding exactly the 16-bit numbers, packing.blocked_to_nchw(...).double()),
so reference and kernel open exactly the same gates and what is left between them is the kernel's own arithmetic.
tests/test_cnn_backward_ref_cpu.py proves on the CPU that these functions are the true gradient of the layer (fp64 autograd, 1e-9) and that
plain fp32 arithmetic stays inside every bound; tests/test_gpu_cnn_backward_fp64.py holds the kernels to them.

Layer (vpt_conv3x3.hip):  W' = op16(W * gain),  v = rstd conv(W', x) + SA[e,o] - rstd mu SG[e,o],  y = relu(v) (+ res),
e = the pixel's edge class 3 * ey + ex (packing.edge_tap_matrix), SG[e,o] = sum of W' over the taps valid in e and over c, SA likewise of W * bias.

Bounds, u = 2^-24 (fp32 unit roundoff), ulp16 = one unit in the last place of the 16-bit format at the reference value:
  dacc    ulp16 + 4u |dacc|                    one 16-bit rounding; the fp32 rstd (fp32 add of eps, v_rsq_f32: 1 ulp = 2u) and one multiply.
                                               The pooled entries first add the <= 4 routed window gradients in fp32: + 3u rstd sum|routed|
                                               (vpt_cnn_backward.hip, `dy[k] +=` / add_if).
  dx      ulp16 + (9 Cout + 8) u convT(|dacc|, |W'|) + 8u (|skip| + |c0| + |c1 xin|)     fp32 accumulation of K = 9 Cout products in any
                                               order + the epilogue's few operations: the forward test's bound with cin and cout exchanged.
  gated   the same, the fp32 part scaled by rstd0; the zero pattern is that of xin.
  dw_raw  (n + g + 2) u sum|dacc||x|           n = frames * H * W products per element, g frame groups added by the reduce kernel; fp32 output.
  sums    n u sum|terms| + u |value|           any-order fp32 summation of n terms, stored as one fp32 value.  Where every term carries an fp32
                                               factor of its own (d_sg: -rstd mu, vpt_cnn_backward.hip `nrm_`; the reduce kernel's 1 / rstd,
                                               `const float inv = 1.0f / rstd`) that factor's 4u, resp. 8u (rstd and the division), is added to n.
  coef    the T1 / T2 bounds propagated through c1 = -rstd^2 T1 / n, c0 = -rstd T2 / n - c1 mu, plus 2u relative (fp64 arithmetic stored as
          fp32) and the fp32 rstd of vpt_conv_bwd_finish_kernel (4u per factor of rstd)."""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

U = 2.0 ** -24
EPS = 1e-5
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
MANT = {"bf16": 7, "fp16": 10}
EMIN = {"bf16": -126, "fp16": -14}


def ulp16(v, fmt):
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** EMIN[fmt]))).clamp(min=EMIN[fmt])
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT[fmt])


def tiny16(fmt):
    """The format's smallest subnormal."""
    return 2.0 ** (EMIN[fmt] - MANT[fmt])


def op16(v, fmt):
    return v.to(DT[fmt]).double()


def edge_class(h, w):
    ey = torch.ones(h, dtype=torch.long); ey[0] = 0; ey[-1] = 2
    ex = torch.ones(w, dtype=torch.long); ex[0] = 0; ex[-1] = 2
    return ey.view(h, 1) * 3 + ex.view(1, w)          # [h, w]


def class_onehot(h, w):
    """[9, h * w] fp64: row e is 1 at the pixels of edge class e."""
    return F.one_hot(edge_class(h, w).reshape(-1), 9).t().double().contiguous()


def stats_of(x):
    flat = x.double().reshape(x.shape[0], -1)
    return torch.stack([flat.sum(1), (flat * flat).sum(1)], 1).contiguous()


def frame_mean_rstd(stats, n, fp32_stats=False):
    """(mu, rstd) fp64 [F] of a frame's n elements from (sum, sum of squares).  fp32_stats: mean and variance rounded to fp32 where the
    kernels round them (frame_mean_rstd in vpt_common.h), so that only the fp32 add of eps and the reciprocal square root remain."""
    m = stats[:, 0].double() / n
    var = (stats[:, 1].double() / n - m * m).clamp(min=0)
    if fp32_stats:
        m, var = m.float().double(), var.float().double()
    return m, 1.0 / torch.sqrt(var + EPS)


def dgrad_coef(mu, rstd, t1, t2, n):
    """training.conv_dgrad_coef in fp64: dx += c0 + c1 x,  c1 = -rstd^2 T1 / n,  c0 = -rstd T2 / n - c1 mu.  -> [F, 2]"""
    c1 = -(rstd * rstd) * t1 / n
    c0 = -(rstd / n) * t2 - c1 * mu
    return torch.stack([c0, c1], 1)


def maxpool_backward_ref(dpooled, pre):
    """F.max_pool2d(pre, 3, 2, 1) backward with torch's rule: the FIRST maximum of a window in scan order keeps the gradient.  Written out
    (unfold, first arg-max, fold) rather than taken from autograd, which the CPU test compares it with."""
    f, c, h, w = pre.shape
    p = F.pad(pre, (1, 1, 1, 1), value=-math.inf)
    win = F.unfold(p, 3, stride=2).view(f, c, 9, -1)                       # [f, c, 9 window positions, windows]
    idx = win.argmax(dim=2, keepdim=True)                                  # torch.argmax: the first of several maxima
    routed = torch.zeros_like(win).scatter_(2, idx, dpooled.reshape(f, c, 1, -1))
    return F.fold(routed.view(f, c * 9, -1), (h + 2, w + 2), 3, stride=2)[:, :, 1:-1, 1:-1].contiguous()


def _reduce(dz, sum_dzv, abs_dzv, mu, rstd, sa, sg, n):
    """Everything prepare returns besides dacc from dz [F,Cout,H,W], the frame's sum dz v, and the tables."""
    f, cout, h, w = dz.shape
    onehot = class_onehot(h, w)
    s = torch.einsum("fop,ep->feo", dz.reshape(f, cout, h * w), onehot)             # S_f[e, o]
    abs_dz = torch.einsum("fop,ep->feo", dz.abs().reshape(f, cout, h * w), onehot)
    sa, sg = sa.double()[:, :cout], sg.double()[:, :cout]
    nrm = (-rstd * mu).view(f, 1, 1)
    t1 = sum_dzv - (sa * s).sum((1, 2))
    t2 = (sg * s).sum((1, 2))
    return SimpleNamespace(d_sa=s.sum(0), d_sg=(nrm * s).sum(0), T1=t1, T2=t2, coef=dgrad_coef(mu, rstd, t1, t2, n), abs_dz=abs_dz,
                           abs_d_sa=abs_dz.sum(0), abs_d_sg=(nrm.abs() * abs_dz).sum(0),
                           abs_T1=abs_dzv + (sa.abs() * s.abs()).sum((1, 2)), abs_T2=(sg.abs() * abs_dz).sum((1, 2)),
                           mu=mu, rstd=rstd, n_in=n, n_class=onehot.sum(1))


def prepare_ref(dy, y, res, stats_in, sa, sg, cin, dpooled=None, fp32_stats=False):
    """ops.conv_backward_prepare: dz = dy [y - res > 0], dacc = rstd dz, the edge-table sums, T1 / T2 and (c0, c1).
    dy=None with dpooled: dy is the max-pool backward of dpooled on the stored pre-pool tensor y (the pooled entries).
    sa / sg: the layer's fp32 tables [9, >= Cout].  Returns a namespace; abs_* are the sums of magnitudes the bounds need."""
    f, cout, h, w = y.shape
    routed_abs = None
    if dy is None:
        dy, routed_abs = maxpool_backward_ref(dpooled, y), maxpool_backward_ref(dpooled.abs(), y)
    v = y if res is None else y - res
    dz = dy * (v > 0)
    n = cin * h * w
    mu, rstd = frame_mean_rstd(stats_in, n, fp32_stats)
    r = _reduce(dz, (dz * v).sum((1, 2, 3)), (dz * v).abs().sum((1, 2, 3)), mu, rstd, sa, sg, n)
    r.dz, r.dacc, r.v = dz, rstd.view(f, 1, 1, 1) * dz, v
    r.routed_abs = None if routed_abs is None else rstd.view(f, 1, 1, 1) * routed_abs * (v > 0)
    return r


def reduce_ref(dacc, gate_u, stats_in, sa, sg, cin, fp32_stats=False):
    """ops.conv_backward_reduce: the same sums for an operand dacc = rstd dz that the gated dgrad already stored; sum dz v = gate_u / rstd."""
    f, cout, h, w = dacc.shape
    n = cin * h * w
    mu, rstd = frame_mean_rstd(stats_in, n, fp32_stats)
    return _reduce(dacc / rstd.view(f, 1, 1, 1), gate_u / rstd, gate_u.abs() / rstd, mu, rstd, sa, sg, n)


def dgrad_ref(dacc, w16, skip, xin, coef):
    """ops.conv3x3_dgrad: conv^T(dacc, W') + skip + c0 + c1 xin, and conv^T(|dacc|, |W'|).  w16 [Cout, Cin, 3, 3] = op16(W * gain)."""
    conv_t = F.conv_transpose2d(dacc, w16, padding=1)
    conv_abs = F.conv_transpose2d(dacc.abs(), w16.abs(), padding=1)
    f = dacc.shape[0]
    dx = conv_t + coef[:, 0].double().view(f, 1, 1, 1) + coef[:, 1].double().view(f, 1, 1, 1) * xin
    if skip is not None:
        dx = dx + skip
    return dx, conv_abs


def dgrad_gated_ref(dacc, w16, xin, coef, gate_stats, gate_cin, fp32_stats=False):
    """ops.conv3x3_dgrad_gated: (rstd0 (conv^T + c0 + c1 xin) [xin > 0],  gate_u_f = sum rstd0 (conv^T + c0 + c1 xin) xin over the frame
    (the unrounded values), conv^T(|dacc|, |W'|), rstd0)."""
    u, conv_abs = dgrad_ref(dacc, w16, None, xin, coef)
    f, _, h, w = xin.shape
    _, rstd0 = frame_mean_rstd(gate_stats, gate_cin * h * w, fp32_stats)
    u = rstd0.view(f, 1, 1, 1) * u
    return u * (xin > 0), (u * xin).sum((1, 2, 3)), conv_abs, rstd0, (u * xin).abs().sum((1, 2, 3))


def wgrad_ref(dacc, x):
    """ops.conv3x3_wgrad: dw[o, tap, c] = sum over frames and pixels of dacc[f, o, p] x[f, c, p + tap] (zero outside the image), and the same
    sum over |dacc|, |x|."""
    h, w = x.shape[2:]
    out = []
    for d, xx in ((dacc, x), (dacc.abs(), x.abs())):
        xp = F.pad(xx, (1, 1, 1, 1))
        out.append(torch.stack([torch.einsum("foyx,fcyx->oc", d, xp[:, :, t // 3:t // 3 + h, t % 3:t % 3 + w]) for t in range(9)], 1))
    return out[0], out[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# bounds (module docstring)

def bound_dacc(r, fmt):
    b = ulp16(r.dacc, fmt) + 4 * U * r.dacc.abs()
    return b if r.routed_abs is None else b + 3 * U * r.routed_abs


def bound_dx(dx64, fmt, cout, conv_abs, skip, coef, xin, scale=None):
    f = dx64.shape[0]
    c = coef.double().abs()
    fp32 = (9 * cout + 8) * U * conv_abs + 8 * U * ((0 if skip is None else skip.abs()) + c[:, 0].view(f, 1, 1, 1) + c[:, 1].view(f, 1, 1, 1) * xin.abs())
    return ulp16(dx64, fmt) + (fp32 if scale is None else scale.view(f, 1, 1, 1) * fp32)


def bound_dw(n, groups, dw_abs):
    return (n + groups + 2) * U * dw_abs


def bound_sum(n, abs_terms, value, factor_u=0):
    return (n + factor_u) * U * abs_terms + U * value.abs()


def bounds_tables(r, frames, hw_cout, factor_u=0):
    """Bounds of (d_sa, d_sg, T1, T2, coef) of a prepare / reduce namespace.  n of a table entry = frames * pixels of its class; of T1 / T2 =
    all the frame's Cout * H * W terms.  factor_u: 0 for prepare, 8 for the reduce kernel (its sums are scaled by an fp32 1 / rstd)."""
    n_e = (frames * r.n_class).view(9, 1)
    b = SimpleNamespace()
    b.d_sa = (n_e + factor_u) * U * r.abs_d_sa + U * r.d_sa.abs()
    b.d_sg = (n_e + factor_u + 4) * U * r.abs_d_sg + U * r.d_sg.abs()
    b.T1 = bound_sum(hw_cout, r.abs_T1, r.T1, factor_u)
    b.T2 = bound_sum(hw_cout, r.abs_T2, r.T2, factor_u)
    c1 = r.coef[:, 1].abs()
    b1 = r.rstd ** 2 / r.n_in * b.T1 + (2 + 8) * U * c1
    t2_part = (r.rstd / r.n_in * r.T2).abs()
    b0 = r.rstd / r.n_in * b.T2 + r.mu.abs() * b1 + (2 + 4) * U * (t2_part + c1 * r.mu.abs())
    b.coef = torch.stack([b0, b1], 1)
    return b


# ---------------------------------------------------------------------------------------------------------------------------------
# reporting

EDGE_NAMES = ["top-left", "top", "top-right", "left", "interior", "right", "bottom-left", "bottom", "bottom-right"]


def describe(idx, shape, kind):
    """Where the worst element sits, in the coordinates a kernel can go wrong in."""
    if kind == "nchw":
        f, c, y, x = idx
        h, w = shape[2:]
        return (f"frame {f} channel {c} (block {c // 32}, lane {c % 32}) pixel ({y}, {x}) edge class {EDGE_NAMES[int(edge_class(h, w)[y, x])]}"
                f" tile ({y // 16}, {x // 16}) row-in-tile {y % 16} column-in-tile {x % 16}")
    if kind == "dw":
        o, t, c = idx
        return f"cout {o} (block {o // 32}, tile {o // 128}) tap ({t // 3}, {t % 3}) cin {c} (block {c // 32}, pair {c // 64})"
    if kind == "table":
        e, o = idx
        return f"edge class {EDGE_NAMES[e]} cout {o} (block {o // 32})"
    return f"index {tuple(idx)}"


def worst(got, ref, bound, kind="frame"):
    """(max err / bound, description of that element).  A zero bound with a zero error counts as ratio 0."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.full_like(err, math.inf)))
    flat = int(ratio.reshape(-1).argmax())
    idx = [int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape)] if ratio.dim() else []
    where = describe(idx, tuple(ratio.shape), kind)
    return float(ratio.reshape(-1)[flat]) if ratio.numel() else 0.0, \
        f"{where}: got {float(got.double().reshape(-1)[flat]):.9g} want {float(ref.reshape(-1)[flat]):.9g} bound {float(bound.reshape(-1)[flat]):.3g}", int((err > bound).sum())


def check(what, got, ref, bound, kind="frame"):
    """Print `max err / bound` (the measurement) and assert it is <= 1, naming the worst element."""
    bound = bound.expand_as(ref) if torch.is_tensor(bound) else torch.full_like(ref, bound)
    ratio, where, bad = worst(got, ref, bound, kind)
    print(f"{what}: max err / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: {bad} of {ref.numel()} elements beyond the bound, worst ratio {ratio:.3f} at {where}"
    return ratio
