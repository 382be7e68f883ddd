"""Reference for vpt_layernorm_kernel and vpt_ln_bwd_kernel<4|8|12|16> + vpt_ln_bwd_finish_kernel: plain torch, importable without a GPU.  compute() runs
in one dtype: float64 = the reference with its bounds (tests/test_layernorm_ref_cpu.py pins it to autograd), float32 = the emulation the CPU tests mutate.

    xr = relu(x) if relu_in else x;  mean, var over the D columns (two passes);  rstd = 1 / sqrt(var + 1e-5f);  xh = (xr - mean) rstd;  y = xh gain + bias
    dg = dy gain;  s1 = mean(dg);  s2 = mean(dg xh);  dx = rstd (dg - s1 - xh s2) [x > 0 if relu_in] + dx_add;  dgain += sum_rows dy xh;  dbias += sum_rows dy
    (vpt_ln_bwd_finish_kernel ADDS into dgain / dbias: `dgain[col] += t[0]`, so the tests pre-fill them).

Bounds, u = 2^-24, every count read from the kernels.  A sum of positive or signed terms evaluated as a tree of depth L errs by at most L u sum|terms|.
  forward sums   L_f = ceil(D / 256) (one accumulation per float4 a lane owns) + 2 (the float4's pairwise sum) + 6 (wave_sum butterfly)
  mean           E_m = (L_f + 1) u mean|xr|                              (+ 1: the division by D)
  var            E_v = 2 E_m mean|d| + (L_f + 4) u var                   d = xr - mean carries E_m + u |d|; the square, the sum, the division
  rstd           eta_r = E_v / (2 (var + eps)) + 5 u                      the addition of eps (halved by the power -1/2) + rsqrtf.  rsqrtf: the ROCm math
                                                                        documentation is not among this installation's files, so 2 ulp = 4 u are allowed.
  xh             E_xh = rstd (E_m + u |d|) + |xh| (eta_r + u)
  y              |y - y64| <= |gain| E_xh + u |y|  (one fma)   [+ ulp16(y64) for a 16-bit output]
  backward sums  L_b = 4 ceil(D / 256) (one accumulation per ELEMENT a lane owns) + 6 + 1 (the product with 1 / D)
  s1, s2         E_s1 = (L_b + 1) u mean|dg|;   E_s2 = mean(|dg| E_xh) + (L_b + 2) u mean|dg xh|
  dx             rstd (u |dg| + E_s1 + E_xh |s2| + |xh| E_s2 + 3 u I + (eta_r + u) I) + u (|dx_add| + |dx|),  I = |dg| + |s1| + |xh s2|;
                 where the ReLU gate is closed the kernel stores 0 + dx_add: exact, bound 0
  dgain, dbias   sum_rows |dy| E_xh + n_c u sum_rows |dy xh| + u (|pre| + |dgain|),   n_c u sum_rows |dy| + u (|pre| + |dbias|);
                 n_c = 8 (a wave's rows, one fma each) + ceil(slab rows / 16) (a segment of the finish kernel) + 4 (its binary tree) + 1 (the += into the output),
                 slab rows = 4 ceil(M / 32)
Every bound is multiplied by 1 + 2^-10 for the second-order terms."""
import math
from types import SimpleNamespace

import torch

from tests import linear_ref as L

D64 = torch.float64
U = 2.0 ** -24
EPS = float(torch.tensor(1e-5, dtype=torch.float32))        # VPT_NORM_EPS, the fp32 constant
SECOND = 1.0 + 2.0 ** -10
ulp16, DT = L.ulp16, L.DT
WIDTHS = [4, 256, 1000, 1024, 1028, 2048, 2052, 3072, 3076, 4096]     # either side of the backward's template thresholds (256 float4 slots per ND4 step of 4)
ROWS = [1, 5, 33]
MUTATIONS = ["mean_over_D-1", "eps_1e-3", "no_s2", "s1_wrong_row", "colsum_drops_last_row", "gate_ignored", "dx_add_dropped"]


def case(m, d, seed=0):
    g = torch.Generator().manual_seed(31 * m + d + seed)
    return SimpleNamespace(M=m, D=d, x=torch.randn(m, d, generator=g) * 1.3 + 0.2, gain=1 + 0.2 * torch.randn(d, generator=g), bias=0.1 * torch.randn(d, generator=g),
                           dy=torch.randn(m, d, generator=g), dx_add=torch.randn(m, d, generator=g), dgain0=torch.randn(d, generator=g), dbias0=torch.randn(d, generator=g))


def compute(c, relu_in=False, use_dx_add=True, dt=D64, mut=None):
    ref = dt == D64 and mut is None
    x, g, b, dy = c.x.to(dt), c.gain.to(dt), c.bias.to(dt), c.dy.to(dt)
    m, d = c.M, c.D
    xr = torch.relu(x) if relu_in else x
    mean = xr.sum(1, keepdim=True) / ((d - 1) if mut == "mean_over_D-1" and d > 1 else d)
    dd = xr - mean
    var = (dd * dd).sum(1, keepdim=True) / d
    rstd = 1.0 / torch.sqrt(var + (1e-3 if mut == "eps_1e-3" else EPS))
    xh = dd * rstd
    o = SimpleNamespace(y=xh * g + b)
    dg = dy * g
    s1 = dg.mean(1, keepdim=True)
    if mut == "s1_wrong_row" and m > 1:
        s1 = s1.roll(1, 0)
    s2 = (dg * xh).mean(1, keepdim=True)
    inner = dg - s1 - (0 if mut == "no_s2" else xh * s2)
    gate = (x > 0) if relu_in and mut != "gate_ignored" else torch.ones_like(x, dtype=torch.bool)
    add = c.dx_add.to(dt) if use_dx_add and mut != "dx_add_dropped" else torch.zeros_like(x)
    o.dx = torch.where(gate, rstd * inner, torch.zeros_like(x)) + add
    rows = slice(0, m - 1) if mut == "colsum_drops_last_row" else slice(0, m)
    o.dgain = c.dgain0.to(dt) + (dy * xh)[rows].sum(0)
    o.dbias = c.dbias0.to(dt) + dy[rows].sum(0)
    if ref:
        it = (d // 4 + 63) // 64
        lf, lb = it + 8, 4 * it + 7
        e_m = (lf + 1) * U * xr.abs().mean(1, keepdim=True)
        e_v = 2 * e_m * dd.abs().mean(1, keepdim=True) + (lf + 4) * U * var
        eta_r = e_v / (2 * (var + EPS)) + 5 * U
        e_xh = rstd * (e_m + U * dd.abs()) + xh.abs() * (eta_r + U)
        o.b_y = SECOND * (g.abs() * e_xh + U * o.y.abs())
        e_s1 = (lb + 1) * U * dg.abs().mean(1, keepdim=True)
        e_s2 = (dg.abs() * e_xh).mean(1, keepdim=True) + (lb + 2) * U * (dg * xh).abs().mean(1, keepdim=True)
        mag_i = dg.abs() + s1.abs() + (xh * s2).abs()
        b_dx = rstd * (U * dg.abs() + e_s1 + e_xh * s2.abs() + xh.abs() * e_s2 + 3 * U * mag_i + (eta_r + U) * mag_i) + U * (add.abs() + o.dx.abs())
        o.b_dx = SECOND * torch.where(gate, b_dx, torch.zeros_like(b_dx))
        n_c = 8 + (4 * ((m + 31) // 32) + 15) // 16 + 4 + 1
        o.b_dgain = SECOND * ((dy.abs() * e_xh).sum(0) + n_c * U * (dy * xh).abs().sum(0) + U * (c.dgain0.to(dt).abs() + o.dgain.abs()))
        o.b_dbias = SECOND * (n_c * U * dy.abs().sum(0) + U * (c.dbias0.to(dt).abs() + o.dbias.abs()))
    return o


def worst(got, want, bnd):
    """-> (worst err / bound over ALL elements, its index).  err = 0 is ratio 0 also under a zero bound; a non-finite value is infinitely wrong."""
    err = (got.to(D64) - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    ratio = torch.where(torch.isfinite(got.to(D64)), ratio, torch.full_like(ratio, math.inf))
    flat = int(ratio.argmax())
    idx = (flat // ratio.shape[-1], flat % ratio.shape[-1]) if ratio.dim() == 2 else (flat,)
    return float(ratio.reshape(-1)[flat]), idx


def check(name, got, want, bnd):
    """-> (worst ratio, None or a message naming the row, the column and the column's float4 slot and lane)."""
    if tuple(got.shape) != tuple(want.shape):
        return math.inf, f"{name}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    w, idx = worst(got, want, bnd)
    if w <= 1.0:
        return w, None
    col = idx[-1]
    return w, (f"{name}: worst err / bound = {w:.3f} at {idx} (column {col}: float4 {col // 4}, lane {(col // 4) % 64}, slot {(col // 4) // 64}" +
               (f"; row {idx[0]}: workgroup {idx[0] // 32}, wave {(idx[0] % 32) // 8}" if len(idx) == 2 else "") +
               f"): got {float(got[idx])!r}, fp64 {float(want[idx])!r}, bound {float(bnd[idx]):.3e}")


def backward_ratios(o, dx, dgain, dbias):
    res, msgs = {}, []
    for nm, got, want, bnd in (("dx", dx, o.dx, o.b_dx), ("dgain", dgain, o.dgain, o.b_dgain), ("dbias", dbias, o.dbias, o.b_dbias)):
        res[nm], msg = check(nm, got, want, bnd)
        msgs += [msg] if msg else []
    return res, msgs
