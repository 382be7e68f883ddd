"""Reference for the policy's action-head kernels: vpt_logsoftmax_kernel<4|16> (mask, temperature, arg-max / Gumbel-max selection, action log-prob),
vpt_nll_bwd_kernel, the dz / entropy side of vpt_bc_loss_kernel, vpt_heads_bwd_kernel and vpt_act_epilogue_kernel.  Plain torch, importable without a GPU.
compute() runs in one dtype: float64 = the reference with its bounds (tests/test_action_head_ref_cpu.py pins it to torch), float32 = an emulation of the
kernels' order of operations, which the CPU tests hold to the bounds and mutate.

    log-softmax   c = z / T (a division);  a masked element is the constant -100 AFTER the scaling;  m = max c;  tot = sum exp(c - m);  lse = m + log tot;
                  lp = c - lse;  score = lp, or lp - log(-log u) with u == 1 -> 0.999f;  action = the FIRST maximum of the scores that compare greater than
                  -3e38, index 0 when none does (a NaN row, a noise row of zeros: torch.argmax's answer);  action_logp = lp[action]
    nll backward  dz = (exp(lp) - onehot) scale per head, the value column and the padding zero
    bc_loss       the same dz at scale w[row] (w == 0: exact zeros);  nll = -lp[label] (exact);  entropy = -sum p lp with p == 0 -> 0
    heads bwd     dz = ((g - exp(lp) sum_j g_j) (1 / T)) grad_scale;  a masked element stores 0 while its g still counts in the sum;  column nb + nc is
                  g_value grad_scale;  a None gradient gives a zero block;  further columns zero
    act epilogue  log_prob = lp_b + lp_c (one fp32 addition: the fp64 sum rounded once);  vpred = fmaf(v, scale, shift): the fp64 value rounded once

Bounds, u = 2^-24, every count read from the kernels.  A sum evaluated as a tree of depth L errs by at most L u sum|terms|.  expf and logf: the ROCm math
documentation is not among this installation's files, so 2 ulp = 4 u (relative to the result) are allowed, as for rsqrtf in tests/layernorm_ref.py.
  c             E_c = u |c| (one division; a masked element is exact)
  m             exact (a maximum); the analysis below is of the kernel's own rounded c, whose maximum it is
  expf argument c - m carries u |c - m|, so  e_i = exp(c_i - m) (1 + r_i),  |r_i| <= u |c_i - m| + 4 u;  where c_i - m < -87 the result may be flushed
                (exp(-87) is the last power above the smallest normal number): the term contributes at most its own fp64 value, r_i = 1
  tot           relative error  eps = sum_i p_i r_i + L u,  p = exp(lp) in fp64 (every argument error weighted by its own probability, not by the worst
                element);  L = ceil(n / (64 NW)) (a thread's serial run) + 6 (wave_sum butterfly) + NW (thread 0 adds the waves' partials one by one)
  lse           E_lse = sum_j p_j E_c_j (d lse / d c_j = p_j) + eps + 4 u |log tot| (logf) + u |lse| (m + logf(tot))
  lp            E_lp = E_c + E_lse + u |lp| (c - lse)
  score         E_sc = E_lp + 4 u (-logf(u) relative, one log later absolute) + 4 u |log(-log u)| + u |score|;  deterministic: E_sc = E_lp
  nll / bc dz   |rs| (4 u p + u |p - onehot|) + u |dz| (+ u |dz| for bc_loss: rs = scale w is rounded);  lp < -87: p's own value in place of 4 u p
  entropy       (5 + L_e) u sum|p lp| (expf and the product per term);  L_e = ceil(n_head / 256) + 1 (the heads share one strided loop: the camera
                head starts mid-stride) + 6 + 2 (the four waves as (r0 + r1) + (r2 + r3));  lp < -87: the term's own value
  heads bwd     S = sum g errs by L_h u sum|g|,  L_h = ceil(n_head / 256) (serial run) + 6 (butterfly) + 2 (four-wave tree);  I = g - p S:
                |1 / T| grad_scale (p L_h u sum|g| + 5 u p |S| (expf, the product) + u |I|) + 3 u |dz| (fl(1 / T), the two products);  masked / None: exact 0;
                value column u |g_value grad_scale|
  16-bit output + ulp16(fp64 value) / 2 (one rounding to nearest; the fp32 error is far below half a 16-bit ulp, so a value straddling a binade is covered)
Every bound is multiplied by 1 + 2^-10 for the second-order terms."""
import math
from types import SimpleNamespace

import torch

from tests import linear_ref as L

D64, F32 = torch.float64, torch.float32
U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -10
ulp16, DT = L.ulp16, L.DT
LSM_CAP = 9                      # scaled logits a thread keeps in registers (vpt_transformer.hip)
LOG0 = -100.0
START = -3.0e38                  # the selection's start value
UNDER = -87.0
T = float(torch.tensor(1.7, dtype=F32))
U999 = float(torch.tensor(0.999, dtype=F32))

# (M, n, ld, col0): the smallest shapes that reach each path of vpt_logsoftmax_launch / vpt_logsoftmax_kernel
LSM_SHAPES = [(1, 1, 1, 0), (5, 2, 2, 0), (80, 2, 2, 0), (70, 11, 11, 0), (3, 63, 63, 0), (3, 64, 64, 0), (3, 65, 65, 0), (3, 255, 255, 0), (3, 256, 256, 0),
              (3, 257, 257, 0), (63, 1024, 1024, 0), (64, 2304, 2304, 0),                                                      # NW = 4, registers only
              (64, 2305, 2305, 0), (64, 2561, 2561, 0), (65, 8641, 8763, 0), (64, 121, 8763, 8641), (64, 1025, 1025, 0),        # NW = 4 (tail from 2305 on)
              (63, 1025, 1025, 0), (1, 8641, 8641, 0), (2, 9216, 9216, 0), (2, 9217, 9217, 0)]                                  # NW = 16 (tail from 9217 on)
# every mode runs on these: a register-only and a tail shape of each NW
MODE_SHAPES = [(3, 65, 65, 0), (70, 11, 11, 0), (64, 2304, 2304, 0), (64, 2305, 2305, 0), (65, 8641, 8763, 0), (1, 8641, 8641, 0), (2, 9216, 9216, 0),
               (2, 9217, 9217, 0)]
# (mask, action): mask none | rand (about 40 % zeros) | one (a row with every element masked but the last) | mmax (a row whose valid logits lie below
# -100 T: a masked element is the maximum);  action none | det | noise (caller uniforms holding a 1.0)
LSM_MODES = [("none", "none"), ("rand", "none"), ("one", "det"), ("mmax", "det"), ("none", "det"), ("rand", "noise"), ("none", "noise"), ("mmax", "noise")]
EVERY_SHAPE_MODES = [("none", "none"), ("rand", "noise")]
# (name, M, n, lower index, higher index): where two equal maxima fall.  NW = 4: thread = i % 256, slot = i // 256, the tail from 2304 on
TIES = [("two register slots of a thread", 3, 600, 5, 261), ("two lanes of a wave", 3, 300, 5, 9), ("two waves", 3, 300, 5, 69),
        ("register slot and tail", 64, 2900, 5, 2309), ("two tail iterations of a thread", 64, 2900, 2309, 2565),
        ("two waves of sixteen", 1, 1100, 5, 965), ("register slot and tail of sixteen waves", 1, 9300, 5, 9221)]
HEAD_SHAPES = [(300, 7, 320), (257, 64, 384), (8641, 121, 8768)]
HEAD_ROWS = [1, 5]
# (grad_scale, the gradient that is None, mask: none | b | both | row (both heads, row 0 masked but one element))
HEADS_CONFIGS = [(1.0, None, "none"), (1024.0, None, "none"), (1.0, "b", "none"), (1.0, "c", "none"), (1.0, "v", "none"), (1.0, None, "b"),
                 (1024.0, None, "both"), (1.0, None, "row"), (1024.0, "c", "b")]
MUTATIONS = ["mask_before_division", "max_skips_tail", "sum_drops_last_wave", "no_max_subtraction", "last_maximum", "no_u1_guard",
             "camera_label_not_offset", "masked_g_dropped", "value_one_column_early", "sb_for_camera"]
KINDS = {"mask_before_division": "lsm", "max_skips_tail": "lsm", "sum_drops_last_wave": "lsm", "no_max_subtraction": "lsm", "last_maximum": "lsm",
         "no_u1_guard": "lsm", "camera_label_not_offset": "nll", "masked_g_dropped": "heads", "value_one_column_early": "heads", "sb_for_camera": "heads"}


def nw_of(m, n):
    """vpt_logsoftmax_launch's rule."""
    return 16 if (m < 64 and n > 1024) else 4


# ---- cases --------------------------------------------------------------------------------------------------------------------------------------------
def lsm_case(m, n, ld=None, col0=0, mask="none", act="none", seed=0, noise=None):
    """Logits of spread 12, one row shifted by +80 and one by -80, T = 1.7.  noise: the uniforms to use as they are (the in-kernel generator's)."""
    ld = ld or col0 + n
    g = torch.Generator().manual_seed(1000003 * seed + 8641 * m + 31 * n + col0 + 7 * len(mask) + 3 * len(act))
    z = torch.randn(m, ld, generator=g) * 12.0
    hi, lo = (1 if m >= 3 else 0), (m - 1 if m >= 2 else None)
    z[hi] += 80.0
    if lo is not None:
        z[lo] -= 80.0
    mk = None
    if mask != "none":
        mk = (torch.rand(m, n, generator=g) >= 0.4).to(torch.uint8)
        if mask == "one":
            mk[hi] = 0
            mk[hi, n - 1] = 1
        if mask == "mmax":
            z[m - 1, col0:col0 + n] = -200.0 - 60.0 * torch.rand(n, generator=g)
            if n >= 2:
                mk[m - 1, 0] = 0
    u = None
    if act == "noise":
        if noise is not None:
            u = noise.clone()
        else:
            u = torch.rand(m, n, generator=g).clamp_(min=2.0 ** -24)
            u[torch.arange(m), z[:, col0:col0 + n].argmin(1)] = 1.0           # the guard's element: the row's lowest logit
    return SimpleNamespace(kind="lsm", M=m, n=n, ld=ld, col0=col0, T=T, z=z, mask=mk, noise=u, act=act, nw=nw_of(m, n))


def tie_case(m, n, i, j, higher_wins=False, seed=0):
    """Spread-3 logits under two equal maxima at columns i < j of every row (deterministic selection: i wins); higher_wins: z[j] a step above z[i]."""
    g = torch.Generator().manual_seed(77 * seed + 13 * n + i + j)
    z = torch.randn(m, n, generator=g) * 3.0
    z[:, i] = 20.0
    z[:, j] = 20.5 if higher_wins else 20.0
    return SimpleNamespace(kind="lsm", M=m, n=n, ld=n, col0=0, T=T, z=z, mask=None, noise=None, act="det", nw=nw_of(m, n))


def _mask(g, m, n, kind_on, row):
    if not kind_on:
        return None
    mk = (torch.rand(m, n, generator=g) >= 0.4).to(torch.uint8)
    if row:
        mk[0] = 0
        mk[0, n // 2] = 1
    return mk


def head_case(m, nb, nc, ldz, variant=0, mask="none", grad_scale=1.0, drop=None, scale=0.37, seed=0):
    """Inputs of the three backward kernels: the fp32 log-probs of both heads (of spread-12 logits at T = 1.7 under the masks), labels (row r: on the
    arg-max, in the head's last column, random, by (r + variant) % 3), frame weights with a zero row, incoming gradients."""
    g = torch.Generator().manual_seed(1000003 * seed + 97 * nb + 5 * nc + m + 11 * len(mask))
    mb = _mask(g, m, nb, mask in ("b", "both", "row"), mask == "row")
    mc = _mask(g, m, nc, mask in ("both", "row"), mask == "row")
    lps = []
    for n, mk in ((nb, mb), (nc, mc)):
        c = torch.randn(m, n, generator=g).double() * 12.0 / T
        if mk is not None:
            c = torch.where(mk == 0, torch.full_like(c, LOG0), c)
        lps.append(torch.log_softmax(c, 1).float())
    labs = []
    for n, lp in ((nb, lps[0]), (nc, lps[1])):
        rnd = torch.randint(0, n, (m,), generator=g)
        how = (torch.arange(m) + variant) % 3
        labs.append(torch.where(how == 0, lp.argmax(1), torch.where(how == 1, torch.full((m,), n - 1), rnd)))
    w = torch.rand(m, generator=g) * 1.5 + 0.5
    if m > 3:
        w[3] = 0.0
    return SimpleNamespace(M=m, nb=nb, nc=nc, ldz=ldz, T=T, lp_b=lps[0], lp_c=lps[1], act_b=labs[0], act_c=labs[1], weight=w,
                           scale=float(torch.tensor(scale, dtype=F32)), mask_b=mb, mask_c=mc, mask=mask, grad_scale=grad_scale, drop=drop,
                           g_b=None if drop == "b" else torch.randn(m, nb, generator=g) * 0.05, g_c=None if drop == "c" else torch.randn(m, nc, generator=g) * 0.05,
                           g_v=None if drop == "v" else torch.randn(m, generator=g))


def act_case(m, seed=0):
    g = torch.Generator().manual_seed(seed + m)
    return SimpleNamespace(kind="act", M=m, act_b=torch.randint(0, 8641, (m,), generator=g), act_c=torch.randint(0, 121, (m,), generator=g),
                           lp_b=-torch.rand(m, generator=g) * 9, lp_c=-torch.rand(m, generator=g) * 5, logits=torch.randn(m, 8763, generator=g), vcol=8762,
                           scale=float(torch.tensor(1.7320508, dtype=F32)), shift=float(torch.tensor(-0.25, dtype=F32)))


# ---- the kernels' arithmetic in one dtype -----------------------------------------------------------------------------------------------------------------
def block_sum(x, nw, pairwise=False, drop_last=False):
    """Row sums [M, 1] in the order of a 64 nw-thread workgroup: thread t adds elements t, t + 64 nw, ... to 0; wave_sum's xor butterfly; then thread 0
    adds the waves' partials one by one, or (pairwise, nw = 4) as (r0 + r1) + (r2 + r3)."""
    m, n = x.shape
    nt = 64 * nw
    k = -(-n // nt)
    xp = torch.zeros(m, k * nt, dtype=x.dtype)
    xp[:, :n] = x
    xp = xp.view(m, k, nw, 64)
    s = torch.zeros(m, nw, 64, dtype=x.dtype)
    for j in range(k):
        s = s + xp[:, j]
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lanes ^ o]
    w = s[:, :, 0]
    if pairwise:
        return ((w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3]))[:, None]
    tot = torch.zeros(m, dtype=x.dtype)
    for i in range(nw - 1 if drop_last else nw):
        tot = tot + w[:, i]
    return tot[:, None]


def select(sc, last=False):
    """The kernel's selection with the in-range rule: the first maximum among the scores that compare greater than -3e38; index 0 when none does."""
    n = sc.shape[1]
    ok = sc > START
    top = torch.where(ok, sc, torch.full_like(sc, -math.inf)).max(1, keepdim=True).values
    idx = torch.arange(n).expand_as(sc)
    hit = ok & (sc == top)
    act = torch.where(hit, idx, torch.full_like(idx, -1)).max(1).values if last else torch.where(hit, idx, torch.full_like(idx, n)).min(1).values
    return torch.where(ok.any(1), act, torch.zeros_like(act))


def _lsm(c, dt, mut):
    ref = dt == D64 and mut is None
    n, nw = c.n, c.nw
    z = c.z[:, c.col0:c.col0 + n].to(dt)
    masked = (c.mask == 0) if c.mask is not None else torch.zeros(c.M, n, dtype=torch.bool)
    tt = torch.tensor(c.T, dtype=dt)
    log0 = torch.full_like(z, LOG0)
    cc = torch.where(masked, log0, z) / tt if mut == "mask_before_division" else torch.where(masked, log0, z / tt)
    m = (cc[:, :64 * nw * LSM_CAP] if mut == "max_skips_tail" else cc).max(1, keepdim=True).values
    if mut == "no_max_subtraction":
        m = torch.zeros_like(m)
    tot = block_sum(torch.exp(cc - m), nw, drop_last=mut == "sum_drops_last_wave")
    lse = m + torch.log(tot)
    lp = cc - lse
    o = SimpleNamespace(lp=lp)
    gum = None
    if c.act != "none":
        sc = lp
        if c.noise is not None:
            u = c.noise.to(dt)
            if mut != "no_u1_guard":
                u = torch.where(u == 1.0, torch.full_like(u, U999), u)
            gum = torch.log(-torch.log(u))
            sc = lp - gum
        o.sc = sc
        o.action = select(sc, last=mut == "last_maximum")
        o.action_logp = lp.gather(1, o.action[:, None])[:, 0]
    if ref:
        p = torch.exp(lp)
        e_c = torch.where(masked, torch.zeros_like(cc), U * cc.abs())
        arg = cc - m
        r = torch.where(arg < UNDER, torch.ones_like(arg), U * arg.abs() + 4 * U)
        depth = -(-n // (64 * nw)) + 6 + nw
        eps = (p * r).sum(1, keepdim=True) + depth * U
        e_lse = (p * e_c).sum(1, keepdim=True) + eps + 4 * U * (lse - m).abs() + U * lse.abs()
        o.b_lp = SECOND * (e_c + e_lse + U * lp.abs())
        if c.act != "none":
            o.b_sc = o.b_lp if gum is None else o.b_lp + SECOND * (4 * U + 4 * U * gum.abs() + U * o.sc.abs())
            o.b_sc = torch.where(torch.isfinite(o.sc), o.b_sc, torch.zeros_like(o.b_sc))
    return o


def margin(o):
    """Per row: (winning score - the best strictly lower score) / (2 x the row's largest score bound); inf where no lower score exists.  Above 1 the
    kernel's selection cannot differ from the reference's: equal scores come from equal inputs and stay equal in the kernel."""
    top = o.sc.max(1, keepdim=True).values
    low = torch.where(o.sc < top, o.sc, torch.full_like(o.sc, -math.inf)).max(1).values
    return (top[:, 0] - low) / (2 * o.b_sc.max(1).values)


def _onehots(c, offset_camera=True):
    oh = torch.zeros(c.M, c.nb + c.nc, dtype=D64)
    r = torch.arange(c.M)
    oh[r, c.act_b] += 1.0
    oh[r, c.act_c + (c.nb if offset_camera else 0)] += 1.0
    return oh


def _nll(c, dt, mut, weighted):
    """vpt_nll_bwd_kernel (weighted False) / vpt_bc_loss_kernel's dz, nll and entropies (weighted True)."""
    ref = dt == D64 and mut is None
    nbc = c.nb + c.nc
    lp = torch.cat([c.lp_b, c.lp_c], 1).to(dt)
    p = torch.exp(lp)
    oh = _onehots(c, mut != "camera_label_not_offset").to(dt)
    rs = torch.full((c.M, 1), c.scale, dtype=dt)
    if weighted:
        rs = rs * c.weight.to(dt)[:, None]
    d = p - oh
    dz = torch.zeros(c.M, c.ldz, dtype=dt)
    dz[:, :nbc] = d * rs
    live = (c.weight != 0)[:, None] if weighted else torch.ones(c.M, 1, dtype=torch.bool)
    dz = torch.where(live, dz, torch.zeros_like(dz))
    o = SimpleNamespace(dz=dz)
    if weighted:
        r = torch.arange(c.M)
        o.nll = torch.stack([-lp[r, c.act_b], -lp[r, c.nb + c.act_c]], 1)
        term = torch.where(p == 0, torch.zeros_like(p), p * lp)
        tb, tc = term.clone(), term.clone()
        tb[:, c.nb:] = 0
        tc[:, :c.nb] = 0                                       # the camera head's elements keep their place in the strided loop
        o.ent = torch.cat([-block_sum(tb, 4, pairwise=True), -block_sum(tc, 4, pairwise=True)], 1)
    if ref:
        under = lp < UNDER
        e_p = torch.where(under, p, 4 * U * p)
        b = torch.zeros_like(dz)
        b[:, :nbc] = rs.abs() * (e_p + U * d.abs()) + (2 if weighted else 1) * U * dz[:, :nbc].abs()
        o.b_dz = SECOND * torch.where(live, b, torch.zeros_like(b))
        if weighted:
            mag = torch.where(under, torch.zeros_like(term), term.abs())
            own = torch.where(under, term.abs(), torch.zeros_like(term))
            bs = []
            for sl, n in ((slice(0, c.nb), c.nb), (slice(c.nb, nbc), c.nc)):
                depth = -(-n // 256) + 1 + 6 + 2
                bs.append((5 + depth) * U * mag[:, sl].sum(1) + own[:, sl].sum(1))
            o.b_ent = SECOND * torch.stack(bs, 1)
    return o


def _heads(c, dt, mut):
    ref = dt == D64 and mut is None
    nbc = c.nb + c.nc
    inv = torch.tensor(1.0, dtype=dt) / torch.tensor(c.T, dtype=dt)
    gs = torch.tensor(c.grad_scale, dtype=dt)
    dz = torch.zeros(c.M, c.ldz, dtype=dt)
    bnd = torch.zeros(c.M, c.ldz, dtype=D64)
    sums = {}
    for nm, lp, g, mk, sl, n in (("b", c.lp_b, c.g_b, c.mask_b, slice(0, c.nb), c.nb), ("c", c.lp_c, c.g_c, c.mask_c, slice(c.nb, nbc), c.nc)):
        if g is None:
            continue
        lp, g = lp.to(dt), g.to(dt)
        masked = (mk == 0) if mk is not None else torch.zeros_like(g, dtype=torch.bool)
        s = sums[nm] = block_sum(torch.where(masked, torch.zeros_like(g), g) if mut == "masked_g_dropped" else g, 4, pairwise=True)
        if mut == "sb_for_camera" and nm == "c" and "b" in sums:
            s = sums["b"]
        p = torch.exp(lp)
        inner = g - p * s
        dz[:, sl] = torch.where(masked, torch.zeros_like(g), (inner * inv) * gs)
        if ref:
            depth = -(-n // 256) + 6 + 2
            e_p = torch.where(lp < UNDER, p, 4 * U * p)
            b = inv * gs * (p * depth * U * g.abs().sum(1, keepdim=True) + (e_p + U * p) * s.abs() + U * inner.abs()) + 3 * U * dz[:, sl].abs()
            bnd[:, sl] = torch.where(masked, torch.zeros_like(b), b)
    if c.g_v is not None:
        dz[:, nbc - 1 if mut == "value_one_column_early" else nbc] = c.g_v.to(dt) * gs
        bnd[:, nbc] = U * dz[:, nbc].abs()
    o = SimpleNamespace(dz=dz)
    if ref:
        o.b_dz = SECOND * bnd
    return o


def _act(c):
    """Exact in either dtype: one rounding of the fp64 sum, one rounding of the fp64 v scale + shift."""
    v = c.logits[:, c.vcol]
    return SimpleNamespace(log_prob=(c.lp_b.double() + c.lp_c.double()).float(), vpred=(v.double() * c.scale + c.shift).float(), vraw=v)


def compute(c, dt=D64, mut=None, kind=None):
    """kind: lsm | nll | bc | heads | act (a head_case serves nll, bc and heads: say which)."""
    kind = kind or c.kind
    if kind == "lsm":
        return _lsm(c, dt, mut)
    if kind in ("nll", "bc"):
        return _nll(c, dt, mut, kind == "bc")
    if kind == "heads":
        return _heads(c, dt, mut)
    return _act(c)


def bound16(want, bnd, fmt):
    return bnd + ulp16(want, fmt) / 2


def worst(got, want, bnd):
    """-> (worst err / bound over ALL elements, its index).  err = 0 is ratio 0 also under a zero bound; a non-finite value is infinitely wrong."""
    err = (got.to(D64) - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    ratio = torch.where(torch.isfinite(got.to(D64)), ratio, torch.full_like(ratio, math.inf))
    flat = int(ratio.argmax())
    idx = (flat // ratio.shape[-1], flat % ratio.shape[-1]) if ratio.dim() == 2 else (flat,)
    return float(ratio.reshape(-1)[flat]), idx


def check(name, got, want, bnd):
    """-> (worst ratio, None or a message naming the element)."""
    if tuple(got.shape) != tuple(want.shape):
        return math.inf, f"{name}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    w, idx = worst(got, want, bnd)
    if w <= 1.0:
        return w, None
    return w, f"{name}: worst err / bound = {w:.3f} at {idx}: got {float(got[idx])!r}, fp64 {float(want[idx])!r}, bound {float(bnd[idx]):.3e}"


def bit_zero(t):
    """Every element +0, bit for bit."""
    return bool((t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32) == 0).all())


# ---- the in-kernel generator's draw, restated on the host (oracle/philox.py, pinned by tests/test_philox_cpu.py) --------------------------------------------
RNG_SEED, RNG_STEP, RNG_STREAM = 4242, 3, 1


def rng_noise(m, n):
    from oracle import philox
    return torch.from_numpy(philox.head_uniforms(RNG_SEED, RNG_STEP, RNG_STREAM, m, n).copy())


def lsm_cases():
    """Every log-softmax case of the GPU file as (label, case): the CPU test holds the emulation to the bounds and asserts the selection margin on these."""
    out = []
    for shape in LSM_SHAPES:
        for mask, act in (LSM_MODES if shape in MODE_SHAPES else EVERY_SHAPE_MODES):
            out.append((f"M {shape[0]} n {shape[1]} ld {shape[2]} col0 {shape[3]} mask {mask} action {act}", lsm_case(*shape, mask=mask, act=act)))
    for shape in MODE_SHAPES:
        m, n = shape[:2]
        out.append((f"M {m} n {n} ld {shape[2]} col0 {shape[3]} mask rand action rng", lsm_case(*shape, mask="rand", act="noise", noise=rng_noise(m, n))))
    for name, m, n, i, j in TIES:
        for hw in (False, True):
            out.append((f"tie: {name}, {'higher' if hw else 'lower'} index wins", tie_case(m, n, i, j, hw)))
    return out
