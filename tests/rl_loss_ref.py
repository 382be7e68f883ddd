"""fp64 reference of vpt_rl_loss_kernel (ops.rl_loss) with the clip decision PINNED, the error bounds the kernel is held to, a float32 restatement
of the kernel's order of operations, and the seeded inputs both test files use.  A plain helper (no test, no fixture): torch / numpy on the CPU
only, nothing of vpt_amd.

With l, q the log-probs of policy and prior, p = exp(l), per head K = sum p (l - q), H = -sum p l (p = 0 counts 0):
    lp = l_b[a_b] + l_c[a_c],  rho = exp(lp - old_lp),  t^ = (target - mean) / std
    L_r  = -min(rho A, clamp(rho, 1 - eps, 1 + eps) A) + kappa (K_b + K_c) - beta (H_b + H_c) + c_v (v - t^)^2,   loss = sum w L / sum w
    c    = -A rho, or 0 where the row is `clipped`
    dz_j = rs [ c (onehot_j - p_j) + kappa p_j ((l_j - q_j) - K) + beta p_j (l_j + H) ] / T,   dz_value = rs 2 c_v (v - t^),   rs = scale w_r
rho at 1 +- eps is a discontinuity of c: the reference takes `clipped` as an INPUT (the kernel's own recorded flag, or the exact rule for inputs
that stay away from the boundary), so that what is left between reference and kernel is arithmetic.  tests/test_rl_loss_ref_cpu.py proves on the
CPU that this closed form is the gradient (fp64 autograd of the plainly written loss, 1e-9); tests/test_gpu_rl_loss.py holds the kernel to it.

Bounds, u = 2^-24, E = the relative error of the device's expf in units of u (twice the largest measured over the test's own arguments),
n = the head's width, ulp16 = one unit in the last place of the 16-bit format at the reference value:
  K, H     (n + 4) u sum p |l - q|,  (n + 4) u sum p |l|        any-order fp32 sum of n products; each product: expf, a subtraction, a multiply
  lp       u |lp|                                               one fp32 add of two picked values (the reductions add zeros to them: exact)
  rho      (E + 1) u rho + rho (u |lp| + u |lp - old|)          the argument's absolute error becomes a relative one of the exponential
  c        |A| err(rho) + u |c|
  dz_j     ulp16 / 2 + rst [ |c| (E u p + u |oh - p|) + err(c) |oh - p| + u |t1|
                             + kappa p ((E + 3) u |(l - q) - K| + u |l - q| + err K)
                             + beta p ((E + 3) u |l + H| + err H)
                             + 2u (|t1| + |t2| + |t3|) ] + 4u |dz_j|          t1..t3 the three terms; rst = scale w / T costs 3 roundings, the product 1
  dz_value ulp16 / 2 + rs 2 c_v (2u |t^| + 3u |v - t^|) + 2u |dz_value|
  records  surrogate: |A| err(rho) + 2u |value|;  (v - t^)^2: 2 |v - t^| (2u |t^| + u |v - t^|) + u (v - t^)^2;  old_lp - lp: u |lp| + u |old_lp - lp|;
           clipped, w, w > 0: exact
  totals   sum_r w_r err(record_r) + (M + 1) u sum_r w_r |record_r|       one multiply by w and an any-order fp32 sum of M rows"""
import numpy as np
import torch

from tests.cnn_backward_ref import U, ulp16

REC = 16


def make_case(m, nb, nc, seed=0, temperature=2.0, clip=0.2, nan_rows=True, zero_prob=True):
    """Seeded inputs with rows of every kind.  Row r's ratio is set by hand through old_log_prob: r % 4 = 0 clipped high (A > 0, rho = 1.5),
    1 clipped low (A < 0, rho = 0.6), 2 unclipped with A > 0 (rho = 0.7 or 1.1), 3 unclipped with A < 0 (rho = 1.4 or 0.95); every rho is
    further than 1e-3 from 1 +- clip (asserted by the tests).  w = 0 on the rows r % 7 = 4 and on row m - 1 (with nan_rows they hold NaN log-probs, prior,
    advantage and target); zero_prob: row 2
    has classes of probability 0 (l = -inf) in both heads, one of them with q = -inf too."""
    g = torch.Generator().manual_seed(seed)
    zb, zc = torch.randn(m, nb, generator=g, dtype=torch.float64) * 2, torch.randn(m, nc, generator=g, dtype=torch.float64) * 2
    yb, yc = zb + 0.7 * torch.randn(m, nb, generator=g, dtype=torch.float64), zc + 0.7 * torch.randn(m, nc, generator=g, dtype=torch.float64)
    ab, ac = torch.randint(0, nb, (m,), generator=g), torch.randint(0, nc, (m,), generator=g)
    avail_b, avail_c = torch.ones(m, nb, dtype=torch.bool), torch.ones(m, nc, dtype=torch.bool)
    if zero_prob:
        avail_b[2, (int(ab[2]) + 1) % nb] = avail_b[2, (int(ab[2]) + 5) % nb] = False
        avail_c[2, (int(ac[2]) + 2) % nc] = False
    zb, zc = zb.masked_fill(~avail_b, -float("inf")), zc.masked_fill(~avail_c, -float("inf"))
    if zero_prob:
        yb[2, (int(ab[2]) + 5) % nb] = -float("inf")            # p = 0 and q = -inf: l - q is NaN, the term counts 0
    lb, lc = torch.log_softmax(zb / temperature, -1).float(), torch.log_softmax(zc / temperature, -1).float()
    qb, qc = torch.log_softmax(yb / temperature, -1).float(), torch.log_softmax(yc / temperature, -1).float()
    lp = lb.double().gather(1, ab[:, None])[:, 0] + lc.double().gather(1, ac[:, None])[:, 0]
    kind = torch.arange(m) % 4
    mag = 0.5 + 1.5 * torch.rand(m, generator=g, dtype=torch.float64)
    adv = torch.where((kind == 0) | (kind == 2), mag, -mag)
    alt = (torch.arange(m) // 4) % 2 == 0
    rho = torch.where(kind == 0, torch.tensor(1.5, dtype=torch.float64), torch.where(kind == 1, torch.tensor(0.6, dtype=torch.float64), torch.where(
        kind == 2, torch.where(alt, 0.7, 1.1).double(), torch.where(alt, 1.4, 0.95).double())))
    old = (lp - torch.log(rho)).float()
    w = torch.tensor([1.0, 0.3, 2.0, 0.5, 0.0, 1.0, 0.25])[torch.arange(m) % 7].clone()
    w[m - 1] = 0.0
    if m > 4:
        w[4] = 0.0
    value, target = torch.randn(m, generator=g), torch.randn(m, generator=g) * 3 + 1
    c = dict(m=m, nb=nb, nc=nc, temperature=temperature, clip=clip, zb=zb, zc=zc, yb=yb, yc=yc, avail_b=avail_b, avail_c=avail_c, lb=lb, lc=lc,
             qb=qb, qc=qc, ab=ab, ac=ac, old=old, adv=adv.float(), value=value, target=target, vnorm=torch.tensor([0.7, 1.9]), w=w,
             scale=1.0 / float(w.double().sum()))
    if nan_rows:
        for r in (w == 0).nonzero()[:, 0].tolist():
            for k in ("lb", "lc", "qb", "qc"):
                c[k][r] = float("nan")
            c["adv"][r] = c["target"][r] = float("nan")
    return c


def exact_clip_flags(c):
    """The clip rule applied in fp64 -> (clipped bool [M], rho fp64 [M], distance of every live rho to the nearer boundary)."""
    live = c["w"] != 0
    lp = c["lb"].double().gather(1, c["ab"][:, None])[:, 0] + c["lc"].double().gather(1, c["ac"][:, None])[:, 0]
    rho = torch.exp(lp - c["old"].double())
    a = c["adv"].double()
    lo, hi = 1.0 - c["clip"], 1.0 + c["clip"]
    clipped = ((a > 0) & (rho > hi)) | ((a < 0) & (rho < lo))
    dist = torch.minimum((rho - lo).abs(), (rho - hi).abs())
    return clipped & live, rho, dist[live]


def reference(c, clipped, *, kl_coef, entropy_coef, value_coef, scale=None, prior=True, value=True, mutate=None, e_exp=1.0):
    """fp64 closed form -> dict(dz [M, nb + nc + 1], frame_out [M, 16], totals [16], and the matching bounds b_dz_abs (without the 16-bit rounding),
    b_frame, b_totals).  Rows with w = 0: exact zeros in dz and in the totals; their frame_out is whatever the inputs give (not compared).
    mutate (a WRONG reference, for the tests' self-check): "kl_swap" = KL(prior || pi), "no_K" = K left out of the gradient, "value_left" = the
    value gradient one column to the left."""
    m, nb, nc, T = c["m"], c["nb"], c["nc"], c["temperature"]
    scale = c["scale"] if scale is None else scale
    w = c["w"].double()
    live = w != 0
    A, old = c["adv"].double(), c["old"].double()
    dz, bdz = torch.zeros(m, nb + nc + 1, dtype=torch.float64), torch.zeros(m, nb + nc + 1, dtype=torch.float64)
    rec, brec = torch.zeros(m, REC, dtype=torch.float64), torch.zeros(m, REC, dtype=torch.float64)
    rs = scale * w
    E = e_exp
    heads = []
    for l, q, a, n, off in ((c["lb"], c["qb"], c["ab"], nb, 0), (c["lc"], c["qc"], c["ac"], nc, nb)):
        l, q = l.double(), q.double()
        p = torch.exp(l)
        pos = p > 0
        d = torch.where(pos, l - q, torch.zeros_like(l)) if prior else torch.zeros_like(l)
        pl = torch.where(pos, p * l, torch.zeros_like(l))
        K = (p * d).sum(-1)
        errK = (n + 4) * U * (p * d.abs()).sum(-1)
        if mutate == "kl_swap" and prior:
            pq = torch.exp(q)
            K = torch.where(pq > 0, pq * (q - l), torch.zeros_like(l)).sum(-1)
        H = -pl.sum(-1)
        errH = (n + 4) * U * pl.abs().sum(-1)
        oh = torch.zeros_like(l)
        oh[torch.arange(m), a] = 1.0
        heads.append(dict(l=l, p=p, pos=pos, d=d, K=K, H=H, errK=errK, errH=errH, oh=oh, n=n, off=off, pick=l.gather(1, a[:, None])[:, 0],
                          pq=torch.exp(q) if prior else None))
    lp = heads[0]["pick"] + heads[1]["pick"]
    rho = torch.exp(lp - old)
    err_rho = (E + 1) * U * rho + rho * U * (lp.abs() + (lp - old).abs())
    cc = torch.where(clipped, torch.zeros_like(rho), -A * rho)
    err_c = torch.where(clipped, torch.zeros_like(rho), A.abs() * err_rho + U * cc.abs())
    lo, hi = 1.0 - c["clip"], 1.0 + c["clip"]
    sur = -torch.minimum(rho * A, rho.clamp(lo, hi) * A)
    vd = torch.zeros(m, dtype=torch.float64)
    that = torch.zeros(m, dtype=torch.float64)
    if value:
        that = (c["target"].double() - float(c["vnorm"][0])) / float(c["vnorm"][1])
        vd = c["value"].double() - that
    err_vd = 2 * U * that.abs() + U * vd.abs()
    for h in heads:
        p, l, d, oh, n, off = h["p"], h["l"], h["d"], h["oh"], h["n"], h["off"]
        t1 = cc[:, None] * (oh - p)
        b1 = cc.abs()[:, None] * (E * U * p + U * (oh - p).abs()) + err_c[:, None] * (oh - p).abs() + U * t1.abs()
        t2 = b2 = t3 = b3 = torch.zeros_like(p)
        if prior and kl_coef != 0:
            if mutate == "kl_swap":
                t2 = kl_coef * (p - h["pq"])
            elif mutate == "no_K":
                t2 = kl_coef * p * d
            else:
                t2 = kl_coef * p * (d - h["K"][:, None])
            t2 = torch.where(h["pos"], t2, torch.zeros_like(t2))
            b2 = kl_coef * p * ((E + 3) * U * (d - h["K"][:, None]).abs() + U * d.abs() + h["errK"][:, None])
        if entropy_coef != 0:
            t3 = torch.where(h["pos"], entropy_coef * p * (l + h["H"][:, None]), torch.zeros_like(p))
            b3 = entropy_coef * p * ((E + 3) * U * torch.where(h["pos"], (l + h["H"][:, None]).abs(), torch.zeros_like(p)) + h["errH"][:, None])
        rst = (rs / T)[:, None]
        gz = rst * (t1 + t2 + t3)
        dz[:, off:off + n] = gz
        bdz[:, off:off + n] = rst * (b1 + b2 + b3 + 2 * U * (t1.abs() + t2.abs() + t3.abs())) + 4 * U * gz.abs()
    if value and value_coef != 0:
        gv = rs * 2 * value_coef * vd
        col = nb + nc - 1 if mutate == "value_left" else nb + nc
        dz[:, col] = dz[:, col] + gv if mutate == "value_left" else gv
        bdz[:, nb + nc] = rs * 2 * value_coef * (2 * U * that.abs() + 3 * U * vd.abs()) + 2 * U * gv.abs()
    dz[~live] = 0.0
    bdz[~live] = 0.0
    (hb, hc) = heads
    wpos = (w > 0).double()
    rec[:, :12] = torch.stack([sur, hb["K"], hc["K"], hb["H"], hc["H"], vd * vd, rho, clipped.double(), lp, old - lp, w, wpos], 1)
    brec[:, :10] = torch.stack([A.abs() * err_rho + 2 * U * sur.abs(), hb["errK"], hc["errK"], hb["errH"], hc["errH"],
                                2 * vd.abs() * err_vd + U * vd * vd, err_rho, torch.zeros(m, dtype=torch.float64), U * lp.abs(),
                                U * lp.abs() + U * (old - lp).abs()], 1)
    wrec = torch.where(live[:, None], w[:, None] * rec[:, :10], torch.zeros(m, 10, dtype=torch.float64))
    totals, btot = torch.zeros(REC, dtype=torch.float64), torch.zeros(REC, dtype=torch.float64)
    totals[:10] = wrec.sum(0)
    totals[10], totals[11] = w.sum(), wpos.sum()
    btot[:10] = torch.where(live[:, None], w[:, None] * brec[:, :10], torch.zeros(m, 10, dtype=torch.float64)).sum(0) + (m + 1) * U * wrec.abs().sum(0)
    btot[10] = (m + 1) * U * w.sum()
    return dict(dz=dz, frame_out=rec, totals=totals, b_dz_abs=bdz, b_frame=brec, b_totals=btot, live=live)


def dz_bound(ref, fmt):
    """The full bound of a 16-bit dz: half an ulp16 at the reference value (taken at |value| + fp32 bound) + the fp32 part."""
    return 0.5 * ulp16(ref["dz"].abs() + ref["b_dz_abs"], fmt) + ref["b_dz_abs"]


def ratios(dz, frame_out, totals, ref, fmt):
    """max err / bound per quantity (an entry with bound 0 must be exact: its ratio is 0 or inf).  dz [M, >= nb + nc + 1]; frame_out rows with
    w = 0 are left out (unspecified)."""
    def rat(x, r, b):
        e = (x.double() - r).abs()
        q = torch.where(b > 0, e / b.clamp(min=1e-300), torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, float("inf"))))
        return float(q.max())
    n = ref["dz"].shape[1]
    live = ref["live"]
    out = dict(dz=rat(dz[:, :n].cpu(), ref["dz"], dz_bound(ref, fmt)))
    if dz.shape[1] > n:
        out["dz_pad"] = float(dz[:, n:].double().abs().max())
    if frame_out is not None:
        out["frame"] = rat(frame_out.cpu()[live], ref["frame_out"][live], ref["b_frame"][live])
    if totals is not None:
        out["totals"] = rat(totals.cpu(), ref["totals"], ref["b_totals"])
    return out


def torch_loss(lb, lc, qb, qc, ab, ac, old, adv, value, that, w, *, clip, kl_coef, entropy_coef, value_coef):
    """The loss written plainly on log-prob tensors (torch.min, clamp, a squared error, KL and entropy from the log-probs): what a user of the
    autograd boundary would write.  Differentiable in lb, lc, value.  Every class must have p > 0."""
    lp = lb.gather(1, ab[:, None])[:, 0] + lc.gather(1, ac[:, None])[:, 0]
    rho = torch.exp(lp - old)
    pg = -torch.min(rho * adv, torch.clamp(rho, 1 - clip, 1 + clip) * adv)
    kl = (lb.exp() * (lb - qb)).sum(-1) + (lc.exp() * (lc - qc)).sum(-1) if qb is not None else 0.0
    ent = -(lb.exp() * lb).sum(-1) - (lc.exp() * lc).sum(-1)
    per = pg + kl_coef * kl - entropy_coef * ent + value_coef * (value - that) ** 2
    return (w * per).sum() / w.sum()


# ---- a float32 restatement in the kernel's own order (numpy) --------------------------------------------------------------------------
def _wave_sum(v):
    """v float32 [..., 64]: the xor-shuffle butterfly of wave_sum (every lane ends with the same value)."""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., idx ^ o]).astype(np.float32)
    return v[..., 0]


def _block_sum(terms):
    """terms float32 [n] in sweep order i = tid, tid + 256, ...: per-thread serial sums, wave butterflies, (w0 + w1) + (w2 + w3)."""
    n = terms.shape[0]
    acc = np.zeros(256, np.float32)
    for i0 in range(0, n, 256):
        chunk = terms[i0:i0 + 256]
        acc[:chunk.shape[0]] = (acc[:chunk.shape[0]] + chunk).astype(np.float32)
    return acc


def restate_f32(c, *, kl_coef, entropy_coef, value_coef, scale=None, prior=True, value=True):
    """float32 numpy in vpt_rl_loss_kernel's order -> (dz fp32 [M, nb + nc + 1] BEFORE the 16-bit rounding, frame_out [M, 16], totals [16] summed
    row by row; the kernel's tree differs, inside the same bound).  expf is numpy's float32 exp."""
    f = np.float32
    m, nb, nc = c["m"], c["nb"], c["nc"]
    scale = f(c["scale"] if scale is None else scale)
    inv_t = f(1.0) / f(c["temperature"])
    lo, hi = f(1.0) - f(c["clip"]), f(1.0) + f(c["clip"])
    kap, beta, cv = f(kl_coef), f(entropy_coef), f(value_coef)
    dz, rec, slab = np.zeros((m, nb + nc + 1), f), np.zeros((m, REC), f), np.zeros((m, REC), f)
    L = [np.concatenate([c["lb"][r].numpy(), c["lc"][r].numpy()]) for r in range(m)]
    Q = [np.concatenate([c["qb"][r].numpy(), c["qc"][r].numpy()]) for r in range(m)]
    with np.errstate(all="ignore"):
        for r in range(m):
            l, q = L[r].astype(f), Q[r].astype(f)
            p = np.exp(l).astype(f)
            isb = np.arange(nb + nc) < nb
            pl = np.where(p == 0, f(0), (p * l).astype(f)).astype(f)
            pd = np.where(p == 0, f(0), (p * (l - q).astype(f)).astype(f)).astype(f) if prior else np.zeros_like(l)
            oh = np.zeros(nb + nc, f)
            oh[int(c["ab"][r])] = 1
            oh[nb + int(c["ac"][r])] = 1
            pick = np.where(oh == 1, l, f(0)).astype(f)
            s = []
            for terms, head in ((pd, True), (pd, False), (pl, True), (pl, False), (pick, True), (pick, False)):
                acc = _block_sum(np.where(isb == head, terms, f(0)).astype(f)).reshape(4, 64)
                wv = _wave_sum(acc)
                s.append(f(f(wv[0] + wv[1]) + f(wv[2] + wv[3])))
            Kb, Kc, Hb, Hc = s[0], s[1], f(-s[2]), f(-s[3])
            lp = f(s[4] + s[5])
            old, A, w = f(c["old"][r]), f(c["adv"][r]), f(c["w"][r])
            rho = np.exp(f(lp - old)).astype(f)
            clipped = bool((A > 0 and rho > hi) or (A < 0 and rho < lo))
            cc = f(0) if clipped else f(-f(A * rho))
            vd = f(0)
            if value:
                that = f(f(f(c["target"][r]) - f(c["vnorm"][0])) / f(c["vnorm"][1]))
                vd = f(f(c["value"][r]) - that)
            rs = f(scale * w)
            rst = f(rs * inv_t)
            K = np.where(isb, Kb, Kc).astype(f)
            H = np.where(isb, Hb, Hc).astype(f)
            g = (cc * (oh - p).astype(f)).astype(f)
            if prior and kl_coef != 0:
                g = np.where(p != 0, (g + ((kap * p).astype(f) * ((l - q).astype(f) - K).astype(f)).astype(f)).astype(f), g)
            if entropy_coef != 0:
                g = np.where(p != 0, (g + ((beta * p).astype(f) * (l + H).astype(f)).astype(f)).astype(f), g)
            dz[r, :nb + nc] = (g * rst).astype(f)
            if value and value_coef != 0:
                dz[r, nb + nc] = f(f(f(f(2) * cv) * vd) * rs)
            if w == 0:
                dz[r] = 0
            sur = f(-min(f(rho * A), f(min(max(rho, lo), hi) * A)))
            rec[r, :12] = [sur, Kb, Kc, Hb, Hc, f(vd * vd), rho, f(clipped), lp, f(old - lp), w, f(w > 0)]
            if w != 0:
                slab[r, :10] = (w * rec[r, :10]).astype(f)
                slab[r, 10] = w
            slab[r, 11] = f(w > 0)
    totals = np.zeros(REC, f)
    for r in range(m):
        totals = (totals + slab[r]).astype(f)
    return torch.from_numpy(dz), torch.from_numpy(rec), torch.from_numpy(totals)


def exp_rel_error_u(args64, exp32):
    """Largest relative error, in units of u = 2^-24, of float32 exponentials `exp32` of the float32 arguments `args64` (given as fp64)."""
    ex = torch.exp(args64.double())
    ok = torch.isfinite(ex) & (ex > 2.0 ** -120)
    return float(((exp32.double() - ex).abs() / ex)[ok].max() / U)
