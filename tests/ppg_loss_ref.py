"""fp64 reference of vpt_ppg_aux_loss_kernel (ops.ppg_aux_loss), the error bounds the kernel is held to, a float32 restatement of the kernel's
order of operations, and the seeded inputs both test files use.  A plain helper (no test, no fixture): torch / numpy on the CPU only, nothing of
vpt_amd.

With l, m the log-probs of the policy and of the snapshot (the teacher), p = exp(l), o = exp(m), per head
    D = sum o (m - l)  (o = 0 counts 0),   S = sum o,   t^ = (target - mean) / std,   vd = v - t^
    L_r  = beta (D_b + D_c) + c_v vd^2,   loss = sum w L / sum w
    dz_j = (beta (p_j - o_j)) rst,  rst = (scale w_r) / T;    dz_value = ((2 c_v) vd) (scale w_r)
The KL is KL(teacher || policy).  p - o is the gradient of D for a teacher of mass exactly 1; the exact gradient is p S - o, and
tests/test_ppg_loss_ref_cpu.py pins that difference against fp64 autograd.

Bounds, u = 2^-24, E = the relative error of the device's expf in units of u (twice the largest measured over the test's own arguments),
n = the head's width, ulp16 = one unit in the last place of the 16-bit format at the reference value:
  D        (n + E + 3) u sum o |m - l|      any-order fp32 sum of n products; each product: expf, a subtraction, a multiply
  S        (n + E) u S                      any-order fp32 sum of n exponentials
  dz_j     ulp16 / 2 + beta rst E u (|p| + |o|) + 8u |dz_j|      the two exponentials; then the subtraction, beta to fp32 and its product, rst = (scale w) x
                                                                (1 / T) (scale to fp32 and three roundings) and the last product
  dz_value ulp16 / 2 + rs 2 c_v (2u |t^| + 3u |vd|) + 2u |dz_value|                       (tests/rl_loss_ref.py's, the same arithmetic)
  records  vd^2: 2 |vd| (2u |t^| + u |vd|) + u vd^2;   w, w > 0: exact
  totals   sum_r w_r err(record_r) + (M + 1) u sum_r w_r |record_r|       one multiply by w and an any-order fp32 sum of M rows"""
import numpy as np
import torch

from tests.cnn_backward_ref import U, ulp16
from tests.rl_loss_ref import _block_sum, _wave_sum, exp_rel_error_u  # noqa: F401  (exp_rel_error_u: for the tests)

REC = 8
MUTATIONS = ("kl_swap", "no_temp", "value_left")


def make_case(m, nb, nc, seed=0, temperature=2.0, nan_rows=True, zero_prob=True):
    """Seeded inputs.  The teacher is log_softmax of the policy's tempered logits plus N(0, 1) noise, so D is of order 1.  w = 0 on the rows
    r % 7 = 4 and on row m - 1 when m > 1 (with nan_rows they hold NaN log-probs, teacher, value and target); zero_prob (m > 2, heads wider than
    8): row 2 has, in both heads, a class the teacher gives no mass (m = -inf, l finite) and one that both give none (l = m = -inf)."""
    g = torch.Generator().manual_seed(seed)
    zb, zc = torch.randn(m, nb, generator=g, dtype=torch.float64) * 2, torch.randn(m, nc, generator=g, dtype=torch.float64) * 2
    yb = zb / temperature + torch.randn(m, nb, generator=g, dtype=torch.float64)
    yc = zc / temperature + torch.randn(m, nc, generator=g, dtype=torch.float64)
    if zero_prob and m > 2 and nb > 8 and nc > 8:
        yb[2, 1] = yc[2, 3] = -float("inf")
        zb[2, 5] = yb[2, 5] = zc[2, 6] = yc[2, 6] = -float("inf")
    lb, lc = torch.log_softmax(zb / temperature, -1).float(), torch.log_softmax(zc / temperature, -1).float()
    mb, mc = torch.log_softmax(yb, -1).float(), torch.log_softmax(yc, -1).float()
    w = torch.tensor([1.0, 0.3, 2.0, 0.5, 0.0, 1.0, 0.25])[torch.arange(m) % 7].clone()
    if m > 1:
        w[m - 1] = 0.0
    value, target = torch.randn(m, generator=g), torch.randn(m, generator=g) * 3 + 1
    c = dict(m=m, nb=nb, nc=nc, temperature=temperature, zb=zb, zc=zc, yb=yb, yc=yc, lb=lb, lc=lc, mb=mb, mc=mc, value=value, target=target,
             vnorm=torch.tensor([0.7, 1.9]), w=w, scale=1.0 / float(w.double().sum()))
    if nan_rows:
        for r in (w == 0).nonzero()[:, 0].tolist():
            for k in ("lb", "lc", "mb", "mc"):
                c[k][r] = float("nan")
            c["value"][r] = c["target"][r] = float("nan")
    return c


def reference(c, *, clone_coef, value_coef, scale=None, value=True, mutate=None, e_exp=1.0):
    """fp64 closed form -> dict(dz [M, nb + nc + 1], frame_out [M, 8], totals [8], and the matching bounds b_dz_abs (without the 16-bit rounding),
    b_frame, b_totals).  Rows with w = 0: exact zeros in dz and in the totals; their frame_out is whatever the inputs give (not compared).
    mutate (a WRONG reference, for the tests' self-check): "kl_swap" = the KL taken the other way round, KL(policy || teacher) with its gradient
    p ((l - m) - K); "no_temp" = 1 / T left out of the policy columns; "value_left" = the value gradient one column to the left."""
    m, nb, nc, T = c["m"], c["nb"], c["nc"], c["temperature"]
    scale = c["scale"] if scale is None else scale
    w = c["w"].double()
    live = w != 0
    dz, bdz = torch.zeros(m, nb + nc + 1, dtype=torch.float64), torch.zeros(m, nb + nc + 1, dtype=torch.float64)
    rec, brec = torch.zeros(m, REC, dtype=torch.float64), torch.zeros(m, REC, dtype=torch.float64)
    rs = scale * w
    E = e_exp
    rst = (rs if mutate == "no_temp" else rs / T)[:, None]
    heads = []
    for l, t, n, off in ((c["lb"], c["mb"], nb, 0), (c["lc"], c["mc"], nc, nb)):
        l, t = l.double(), t.double()
        p, o = torch.exp(l), torch.exp(t)
        d = torch.where(o > 0, t - l, torch.zeros_like(l))
        D, S = (o * d).sum(-1), o.sum(-1)
        errD, errS = (n + E + 3) * U * (o * d.abs()).sum(-1), (n + E) * U * S
        if mutate == "kl_swap":
            dk = torch.where((p > 0) & (o > 0), l - t, torch.zeros_like(l))      # (a class without teacher mass counts 0: the mutant stays finite)
            D = (p * dk).sum(-1)
            gz = torch.where(p > 0, p * (dk - D[:, None]), torch.zeros_like(p))
        else:
            gz = p - o
        if clone_coef != 0:
            gz = rst * (clone_coef * gz)
            dz[:, off:off + n] = gz
            bdz[:, off:off + n] = clone_coef * rst * E * U * (p + o) + 8 * U * gz.abs()
        heads.append(dict(D=D, S=S, errD=errD, errS=errS))
    vd, that = torch.zeros(m, dtype=torch.float64), torch.zeros(m, dtype=torch.float64)
    if value:
        that = (c["target"].double() - float(c["vnorm"][0])) / float(c["vnorm"][1])
        vd = c["value"].double() - that
    err_vd = 2 * U * that.abs() + U * vd.abs()
    if value and value_coef != 0:
        gv = rs * 2 * value_coef * vd
        col = nb + nc - 1 if mutate == "value_left" else nb + nc
        dz[:, col] = dz[:, col] + gv if mutate == "value_left" else gv
        bdz[:, nb + nc] = rs * 2 * value_coef * (2 * U * that.abs() + 3 * U * vd.abs()) + 2 * U * gv.abs()
    dz[~live] = 0.0
    bdz[~live] = 0.0
    (hb, hc) = heads
    wpos = (w > 0).double()
    rec[:, :7] = torch.stack([hb["D"], hc["D"], vd * vd, hb["S"], hc["S"], w, wpos], 1)
    brec[:, :5] = torch.stack([hb["errD"], hc["errD"], 2 * vd.abs() * err_vd + U * vd * vd, hb["errS"], hc["errS"]], 1)
    zero5 = torch.zeros(m, 5, dtype=torch.float64)
    wrec = torch.where(live[:, None], w[:, None] * rec[:, :5], zero5)
    totals, btot = torch.zeros(REC, dtype=torch.float64), torch.zeros(REC, dtype=torch.float64)
    totals[:5] = wrec.sum(0)
    totals[5], totals[6] = w.sum(), wpos.sum()
    btot[:5] = torch.where(live[:, None], w[:, None] * brec[:, :5], zero5).sum(0) + (m + 1) * U * wrec.abs().sum(0)
    btot[5] = (m + 1) * U * w.sum()
    return dict(dz=dz, frame_out=rec, totals=totals, b_dz_abs=bdz, b_frame=brec, b_totals=btot, live=live)


def loss_of(totals, clone_coef, value_coef):
    return (clone_coef * (totals[0] + totals[1]) + value_coef * totals[2]) / totals[5]


def dz_bound(ref, fmt):
    """The full bound of a 16-bit dz: half an ulp16 at the reference value (taken at |value| + fp32 bound) + the fp32 part."""
    return 0.5 * ulp16(ref["dz"].abs() + ref["b_dz_abs"], fmt) + ref["b_dz_abs"]


def ratios(dz, frame_out, totals, ref, fmt):
    """max err / bound per quantity (an entry with bound 0 must be exact: its ratio is 0 or inf).  dz [M, >= nb + nc + 1]; frame_out rows with
    w = 0 are left out (unspecified).  fmt None: dz is the fp32 value before the 16-bit rounding."""
    def rat(x, r, b):
        e = (x.double() - r).abs()
        q = torch.where(b > 0, e / b.clamp(min=1e-300), torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, float("inf"))))
        return float(q.max())
    n = ref["dz"].shape[1]
    live = ref["live"]
    out = dict(dz=rat(dz[:, :n].cpu(), ref["dz"], dz_bound(ref, fmt) if fmt else ref["b_dz_abs"]))
    if dz.shape[1] > n:
        out["dz_pad"] = float(dz[:, n:].double().abs().max())
    if frame_out is not None:
        out["frame"] = rat(frame_out.cpu()[live], ref["frame_out"][live], ref["b_frame"][live])
    if totals is not None:
        out["totals"] = rat(totals.cpu(), ref["totals"], ref["b_totals"])
    return out


def exp_arguments(c):
    """Every finite argument the kernel hands expf on the live rows: the log-probs of the policy and of the teacher."""
    live = c["w"] != 0
    args = torch.cat([c[k][live].reshape(-1) for k in ("lb", "lc", "mb", "mc")])
    return args[torch.isfinite(args)].contiguous()


def torch_loss(lb, lc, ob, oc, value, that, w, *, clone_coef, value_coef):
    """The auxiliary loss written plainly on log-prob tensors: what a user of the autograd boundary would write.  ob, oc: the teacher's LOG-probs
    (every class with o > 0).  Differentiable in lb, lc, value."""
    kl = (ob.exp() * (ob - lb)).sum(-1) + (oc.exp() * (oc - lc)).sum(-1)
    return (w * (clone_coef * kl + value_coef * (value - that) ** 2)).sum() / w.sum()


# ---- a float32 restatement in the kernel's own order (numpy) --------------------------------------------------------------------------
def restate_f32(c, *, clone_coef, value_coef, scale=None, value=True):
    """float32 numpy in vpt_ppg_aux_loss_kernel's order -> (dz fp32 [M, nb + nc + 1] BEFORE the 16-bit rounding, frame_out [M, 8], totals [8] summed
    row by row; the kernel's tree differs, inside the same bound).  expf is numpy's float32 exp."""
    f = np.float32
    m, nb, nc = c["m"], c["nb"], c["nc"]
    scale = f(c["scale"] if scale is None else scale)
    inv_t = f(1.0) / f(c["temperature"])
    beta, cv = f(clone_coef), f(value_coef)
    dz, rec, slab = np.zeros((m, nb + nc + 1), f), np.zeros((m, REC), f), np.zeros((m, REC), f)
    isb = np.arange(nb + nc) < nb
    with np.errstate(all="ignore"):
        for r in range(m):
            l = np.concatenate([c["lb"][r].numpy(), c["lc"][r].numpy()]).astype(f)
            t = np.concatenate([c["mb"][r].numpy(), c["mc"][r].numpy()]).astype(f)
            p, o = np.exp(l).astype(f), np.exp(t).astype(f)
            od = np.where(o == 0, f(0), (o * (t - l).astype(f)).astype(f)).astype(f)
            s = []
            for terms, head in ((od, True), (od, False), (o, True), (o, False)):
                wv = _wave_sum(_block_sum(np.where(isb == head, terms, f(0)).astype(f)).reshape(4, 64))
                s.append(f(f(wv[0] + wv[1]) + f(wv[2] + wv[3])))
            w = f(c["w"][r])
            vd = f(0)
            if value:
                that = f(f(f(c["target"][r]) - f(c["vnorm"][0])) / f(c["vnorm"][1]))
                vd = f(f(c["value"][r]) - that)
            rs = f(scale * w)
            rst = f(rs * inv_t)
            if clone_coef != 0:
                dz[r, :nb + nc] = ((beta * (p - o).astype(f)).astype(f) * rst).astype(f)
            if value and value_coef != 0:
                dz[r, nb + nc] = f(f(f(f(2) * cv) * vd) * rs)
            if w == 0:
                dz[r] = 0
            rec[r, :7] = [s[0], s[1], f(vd * vd), s[2], s[3], w, f(w > 0)]
            if w != 0:
                slab[r, :5] = (w * rec[r, :5]).astype(f)
                slab[r, 5] = w
            slab[r, 6] = f(w > 0)
    totals = np.zeros(REC, f)
    for r in range(m):
        totals = (totals + slab[r]).astype(f)
    return torch.from_numpy(dz), torch.from_numpy(rec), torch.from_numpy(totals)
