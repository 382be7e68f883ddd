"""Reference for the optimiser kernels of vpt_optim.hip: vpt_adam_kernel (vpt_adam_step), vpt_adam_multi_kernel<CLIP> (vpt_adam_step_multi[_clip]) and
vpt_adam_groups_kernel<CLIP, DECOUPLED> (vpt_adam_step_groups).  Plain numpy, importable without a GPU.  run() is one routine in one dtype: float64 = the
reference with its bounds (tests/test_optim_ref_cpu.py pins it to torch.optim.Adam / AdamW), float32 = an emulation of the kernels' sequence of operations,
every product and sum rounded on its own, which the CPU tests hold to the bounds and mutate.

The contract is the C ABI's, not torch's: beta1, beta2, eps, lr, weight_decay and grad_scale arrive as FLOATS.  Every hyper-parameter is therefore rounded
to fp32 first; c1 = 1 - beta1 and c2 = 1 - beta2 are formed from the fp32 betas (exact in fp32: Sterbenz); the host terms are the code's own double
expressions on those floats, rounded to float (adam_bias_terms, vpt_capi.hip; the groups kernel forms the step size per tensor from that tensor's float lr):
    step_size = fl32(lr / (1 - beta1^t))      inv_sqrt_bc2 = fl32(1 / sqrt(1 - beta2^t))      keep = fl32(1 - lr wd)  (decoupled)
and then, per element, with s = grad_scale and coef the device's clip coefficient (an INPUT here: tests/test_gpu_grad_norm.py holds its value),
    p0 = p keep (decoupled, then wd = 0) or p      gs = (g s) [coef]      g' = wd p0 + gs      m' = beta1 m + c1 g'      v' = beta2 v + c2 g'^2
    d = sqrt(v') inv_sqrt_bc2 + eps      q = m' / d      upd = step_size q      p' = p0 - upd
exact_terms=True leaves the three host terms unrounded (everything else unchanged): that is torch's own double arithmetic on the same hyper-parameters, the
form the torch pin uses, since fl32 of a host term is 2^-24 relative and the pin asks for 1e-12.  round_hyper=False takes the hyper-parameters as Python
doubles (torch.optim.Adam's view of 0.999): the distance between the two is measured in the CPU test, not hidden in a tolerance.

Bounds, u = 2^-24, per element, from the UNCONTRACTED operation count of the kernels.  hipcc contracts a * b + c where it likes (sqrtf(v) * inv + eps and
p - step * q may or may not be fused); a contraction removes a rounding and never adds one, so the count below covers both forms.  The fmaf() calls the source
spells out round once.  sqrtf and the fp32 division are given 2 ulp = 4 u each (the ROCm math documentation is not among this installation's files:
the precedent of tests/layernorm_ref.py).  A = |gs|, W = |wd p0|, all magnitudes those of the fp64 reference:
  gs     g * s: u A; with coef a second product: 2 u A                                                        (n_g = 1 or 2 roundings)
  g'     fmaf(wd, p0, gs), one rounding u |g'| <= u (W + A):      E_g = u (W + (n_g + 1) A)
  m'     fmaf(beta1, m, c1 * gk): the product u c1 |gk|, the fma u |m'|:      E_m = c1 E_g + u c1 (|g'| + E_g) + u |m'|
  v'     fmaf(beta2, v, (c2 * gk) * gk): two products, the fma:      E_v = c2 (2 |g'| E_g + E_g^2) + 2 u c2 (|g'| + E_g)^2 + u v'
  sqrt   |sqrt(v' + e) - sqrt(v')| <= E_v / (sqrt(v') + sqrt(max(v' - E_v, 0))) for |e| <= E_v (sqrt(E_v) when v' = 0), plus 4 u sqrt(v'):      E_s
  d      (sq * inv) + eps: u sqrt(v') inv and u d:      E_d = inv E_s + u sqrt(v') inv + u d
  q      m / d:      E_q = E_m / (d - E_d) + |m'| E_d / (d (d - E_d)) + 4 u |q|
  upd    step_size * q:      E_u = step_size E_q + u |upd|
  p'     p0 - upd: u |p'|; decoupled: p0 = p * keep, rounded on its own (__fmul_rn), u |p0|:      E_p = E_u + u |p'| [+ u |p0|]
b_m = E_m, b_v = E_v, b_p = E_p, each multiplied by 1 + 2^-10 for the second-order terms.  No measured constant enters.  With p = 0 the bound on p' is a few u
of the UPDATE: that is what makes a 1e-5 relative mistake in the update visible, where u |p| of a weight of order 1 hides it.
The subnormal range is left out on purpose: the inputs keep c2 g'^2 either exactly 0 or above 2^-100 (regime_ok() checks it), so no product above underflows
and the relative model u |x| holds for every rounding.

cases(): the inputs, from a fixed seed; the GPU test and the CPU test run the same bytes.  MUTATIONS: mistakes the earlier optimiser tests could not see, each
with the (case, tensor) DESIGNATED to show it."""
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -10
REGIME_FLOOR = 2.0 ** -100

Hyper = namedtuple("Hyper", "lr wd beta1 beta2 eps grad_scale")
HYPER_A = dict(lr=0.000181, wd=0.039428, beta1=0.9, beta2=0.999, eps=1e-8)          # the BC script's (behavioural_cloning.py:38-40)
HYPER_B = dict(lr=1e-2, wd=0.0, beta1=0.8, beta2=0.95, eps=1e-6)                    # nothing equals a default
PAIRS_A = ((0.000181, 0.039428), (0.0000181, 0.0))                                  # (lr, wd) of the two interleaved groups; the second without decay
PAIRS_B = ((2e-3, 0.25), (1e-2, 0.0))
SCALES = (1.0, 1.0 / 3, 2.0 ** -16)
STEPS = (1, 2, 10, 1000, 100000)
CLIP_FRAC = 0.37                                                                     # max_norm = 0.37 x the norm: a coefficient well inside (0, 1)

SINGLE_SIZES = (1, 2, 3, 4, 5, 1023, 1024, 1025)                                     # the 4-element group and its tails, the 1024-element block edge
SINGLE_LARGE = 4096 * 1024 + 1024 + 3              # vpt_adam_launch caps the grid at 4096 blocks of 256 float4: a second grid-stride sweep, then a tail of 3
TABLE_SIZES = (1, 2, 3, 4, 5, 0, 1023, 1024, 1025, 2049, 4099)                       # + 300 tensors of 1..7 elements (binary search deeper than 8) + a last 0
# the tensors the mutations are designated on (table index): p = 0 so that the bound is the update's own
ROLES = dict(eps=6,       # 1023: p = 0, |g| ~ 3e-9: eps carries the denominator
             fresh=7,     # 1024: p = 0, m = v = 0: a first step, v' = c2 g'^2 alone
             decay=8,     # 1025: |p| = 1, |g| ~ 0.05: wd p and g of one size
             zero=9,      # 2049: m = v = g = 0: the update is exactly 0, p moves by decay only
             sqrtv=10)    # 4099: p = 0, |g| ~ 1: sqrt(v) carries the denominator
MUTATIONS = ["eps_scaled", "eps_in_sqrt", "no_bc2", "bc_step_minus_1", "betas_double", "scale_after_decay", "v_without_decay", "coef_on_decay",
             "adamw_for_l2", "l2_for_adamw", "keep_after_update", "group_by_block", "tail_dropped"]
# mutation -> (case name, role).  None is provably indistinguishable in fp32 on these inputs, so none is left out.
DESIGNATED = {"eps_scaled": ("multi/A/s0/t1", "eps"), "eps_in_sqrt": ("multi/A/s0/t1", "eps"), "no_bc2": ("multi/A/s0/t1", "eps"),
              "bc_step_minus_1": ("multi/A/s1/t2", "sqrtv"), "betas_double": ("multi/A/s0/t1", "fresh"), "scale_after_decay": ("multi_clip/A/s1/t1", "decay"),
              "v_without_decay": ("multi/A/s0/t1", "decay"), "coef_on_decay": ("multi_clip/A/s1/t1", "decay"), "adamw_for_l2": ("groups/A/s0/t1", "decay"),
              "l2_for_adamw": ("groups_decoupled/A/s2/t1", "decay"), "keep_after_update": ("groups_decoupled/B/s0/t1000", "sqrtv"),
              "group_by_block": ("groups/A/s0/t1", "eps"), "tail_dropped": ("multi/A/s0/t1", "eps")}


def fl32(x):
    return float(F32(x))


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


# ---- the host side: adam_bias_terms and vpt_adam_step_groups (vpt_capi.hip) --------------------------------------------------------------------------------
def host_terms(step, hyper, lr_wd=None, *, decoupled=False, round_hyper=True, exact_terms=False, mutate=None):
    """-> the scalars one tensor's update runs on, as Python doubles.  lr_wd: that tensor's own (lr, wd) (the groups entry), else the launch-wide ones."""
    lr, wd = lr_wd if lr_wd is not None else (hyper.lr, hyper.wd)
    b1, b2, eps, s = hyper.beta1, hyper.beta2, hyper.eps, hyper.grad_scale
    rnd = fl32 if round_hyper else float
    term = float if exact_terms else fl32
    lr, wd, b1, b2, eps, s = (rnd(x) for x in (lr, wd, b1, b2, eps, s))
    hb1, hb2, hlr, hwd = b1, b2, lr, wd                       # what the host expressions see
    c1, c2 = 1.0 - b1, 1.0 - b2
    if mutate == "betas_double":                              # the hyper-parameters as Python doubles: the host terms and c1, c2 come from 0.9, not fl32(0.9)
        hb1, hb2, hlr, hwd = (float(x) for x in (hyper.beta1, hyper.beta2, lr_wd[0] if lr_wd is not None else hyper.lr, lr_wd[1] if lr_wd is not None else hyper.wd))
        c1, c2 = 1.0 - hb1, 1.0 - hb2
    t = step - 1 if mutate == "bc_step_minus_1" else step
    with np.errstate(divide="ignore", invalid="ignore"):
        step_size = term(F64(hlr) / F64(1.0 - math.pow(hb1, t)))
        inv = 1.0 if mutate == "no_bc2" else term(F64(1.0) / np.sqrt(F64(1.0 - math.pow(hb2, t))))
    keep = term(1.0 - hlr * hwd) if decoupled else 1.0
    return SimpleNamespace(b1=b1, b2=b2, c1=c1, c2=c2, eps=eps, s=s, wd=0.0 if decoupled else wd, step_size=step_size, inv=inv, keep=keep)


# ---- one tensor, one dtype ------------------------------------------------------------------------------------------------------------------------------------
def _fma(dt, a, b, c):
    """fmaf: one rounding.  float32: the product of two floats is exact in double; the sum is rounded to double, then to float (a double rounding moves
    the result by one ulp in rare cases: the emulation is held to the bounds, not to bits)."""
    if dt is F64:
        return a * b + c
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def _update(dt, p, g, m, v, T, coef, decoupled, mutate):
    """The kernels' per-element sequence in dtype dt.  T's step_size, wd and keep may be per-element arrays (mutation group_by_block)."""
    k = lambda x: np.asarray(x, dt)
    b1, b2, c1, c2, eps, s, wd, step_size, inv, keep = (k(x) for x in (T.b1, T.b2, T.c1, T.c2, T.eps, T.s, T.wd, T.step_size, T.inv, T.keep))
    p, g, m, v = k(p), k(g), k(m), k(v)
    with np.errstate(all="ignore"):
        p0 = p * keep if (decoupled and mutate != "keep_after_update") else p
        if mutate == "scale_after_decay":
            gk = _fma(dt, wd, p0, g) * s
            gs = g * s
            if coef is not None:
                gk, gs = gk * k(coef), gs * k(coef)
        else:
            gs = g * s
            if coef is not None and mutate != "coef_on_decay":
                gs = gs * k(coef)
            gk = _fma(dt, wd, p0, gs)
            if coef is not None and mutate == "coef_on_decay":
                gk, gs = gk * k(coef), gs * k(coef)
        m1 = _fma(dt, b1, m, c1 * gk)
        gv = gs if mutate == "v_without_decay" else gk
        v1 = _fma(dt, b2, v, c2 * gv * gv)
        if mutate == "eps_scaled":
            d = (np.sqrt(v1) + eps) * inv
        elif mutate == "eps_in_sqrt":
            d = np.sqrt(v1 + eps) * inv
        else:
            d = np.sqrt(v1) * inv + eps
        q = m1 / d
        upd = step_size * q
        p1 = p0 - upd
        if decoupled and mutate == "keep_after_update":
            p1 = p1 * keep
    return SimpleNamespace(p=p1, m=m1, v=v1, p0=p0, gs=gs, gk=gk, d=d, q=q, upd=upd)


def _bounds(r, T, coef, decoupled):
    """The docstring's derivation on the fp64 quantities of one tensor."""
    n_g = 2 if coef is not None else 1
    A, W, ag = np.abs(r.gs), np.abs(T.wd * r.p0), np.abs(r.gk)
    E_g = U * (W + (n_g + 1) * A)
    E_m = T.c1 * E_g + U * T.c1 * (ag + E_g) + U * np.abs(r.m)
    E_v = T.c2 * (2 * ag * E_g + E_g ** 2) + 2 * U * T.c2 * (ag + E_g) ** 2 + U * r.v
    sq = np.sqrt(r.v)
    lo = np.sqrt(np.maximum(r.v - E_v, 0.0))
    with np.errstate(all="ignore"):
        E_s = np.where(sq + lo > 0, E_v / (sq + lo), np.sqrt(E_v)) + 4 * U * sq
    E_d = T.inv * E_s + U * sq * T.inv + U * r.d
    d_lo = r.d - E_d
    assert r.d.size == 0 or float(d_lo.min()) > 0.0, "the denominator's own error reaches the denominator: outside what the derivation covers"
    E_q = E_m / d_lo + np.abs(r.m) * E_d / (r.d * d_lo) + 4 * U * np.abs(r.q)
    E_u = T.step_size * E_q + U * np.abs(r.upd)
    E_p = E_u + U * np.abs(r.p) + (U * np.abs(r.p0) if decoupled else 0.0)
    return E_p * SECOND, E_m * SECOND, E_v * SECOND


def _first_blocks(sizes):
    fb, out = 0, []
    for n in sizes:
        out.append(fb)
        fb += (n + 1023) // 1024
    return out


def run(dt, p, g, m, v, step, hyper, *, coef=None, decoupled=False, lr_wd_per_tensor=None, mutate=None, round_hyper=True, exact_terms=False):
    """p, g, m, v: lists of fp32 arrays (one per tensor, table order) -> a list of namespaces (p, m, v, upd, and for float64 b_p, b_m, b_v).
    coef: the clip coefficient as a number (None: the unclipped launch).  lr_wd_per_tensor: the groups entry's records."""
    p, g, m, v = ([_np(x) for x in part] for part in (p, g, m, v))
    if mutate == "adamw_for_l2":
        assert not decoupled
        decoupled = True
    elif mutate == "l2_for_adamw":
        assert decoupled
        decoupled = False
    sizes = [x.size for x in p]
    fbs = _first_blocks(sizes)
    out = []
    for i, n in enumerate(sizes):
        rec = None if lr_wd_per_tensor is None else lr_wd_per_tensor[i]
        T = host_terms(step, hyper, rec, decoupled=decoupled, round_hyper=round_hyper, exact_terms=exact_terms, mutate=mutate)
        if mutate == "group_by_block" and lr_wd_per_tensor is not None and n:
            # the record read at the BLOCK index: element j of tensor i lies in block first_block[i] + j // 1024
            blk = np.minimum(fbs[i] + np.arange(n) // 1024, len(sizes) - 1)
            pick = {b: host_terms(step, hyper, lr_wd_per_tensor[b], decoupled=decoupled, round_hyper=round_hyper, exact_terms=exact_terms)
                    for b in sorted(set(blk.tolist()))}
            for name in ("step_size", "wd", "keep"):
                setattr(T, name, np.array([getattr(pick[b], name) for b in blk.tolist()], F64))
        r = _update(dt, p[i], g[i], m[i], v[i], T, coef, decoupled, mutate)
        r.terms = T
        if mutate == "tail_dropped" and n & 3:                 # the last partial group of four is never written
            keep_from = n & ~3
            for name, old in (("p", p[i]), ("m", m[i]), ("v", v[i])):
                getattr(r, name)[keep_from:] = old[keep_from:]
        if dt is F64 and mutate is None:
            r.b_p, r.b_m, r.b_v = _bounds(r, T, coef, decoupled)
        out.append(r)
    return out


def reference(p, g, m, v, step, hyper, *, coef=None, decoupled=False, lr_wd_per_tensor=None, **kw):
    """fp64 on the fp32 inputs, with the bounds."""
    return run(F64, p, g, m, v, step, hyper, coef=coef, decoupled=decoupled, lr_wd_per_tensor=lr_wd_per_tensor, **kw)


def emulate_f32(p, g, m, v, step, hyper, *, coef=None, decoupled=False, lr_wd_per_tensor=None, mutate=None):
    """The same sequence op by op in numpy float32, uncontracted; mutate: one of MUTATIONS."""
    return run(F32, p, g, m, v, step, hyper, coef=None if coef is None else fl32(coef), decoupled=decoupled, lr_wd_per_tensor=lr_wd_per_tensor, mutate=mutate)


def ratios(got_p, got_m, got_v, ref):
    """max |got - reference| / bound per quantity over one tensor's elements -> (r_p, r_m, r_v); 0 / 0 counts 0, a non-finite value inf."""
    out = []
    for got, want, bound in ((got_p, ref.p, ref.b_p), (got_m, ref.m, ref.b_m), (got_v, ref.v, ref.b_v)):
        got = np.asarray(_np(got), F64)
        if got.size == 0:
            out.append(0.0)
            continue
        err = np.abs(got - want)
        with np.errstate(all="ignore"):
            r = np.where(err == 0, 0.0, err / bound)
        r = np.where(np.isfinite(got), r, np.inf)
        out.append(float(r.max()))
    return tuple(out)


def regime_ok(refs, hyper):
    """The input condition the bounds rest on: c2 g'^2 exactly 0 or above 2^-100 for every element."""
    c2 = 1.0 - fl32(hyper.beta2)
    return all(bool(np.all((r.gk == 0) | (c2 * r.gk ** 2 > REGIME_FLOOR))) for r in refs)


def clip_inputs(case):
    """-> (max_norm, torch's clip_coef_clamped in double) of a clipped case's step-0 gradients: max_norm = CLIP_FRAC x the fp64 norm of g * grad_scale."""
    s = fl32(case.hyper.grad_scale)
    norm = math.sqrt(sum(float(np.sum((x.astype(F64) * s) ** 2)) for x in case.g))
    max_norm = CLIP_FRAC * norm
    return max_norm, min(max_norm / (norm + 1e-6), 1.0)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------------------
_PMAGS = (0.0, 1e-7, 1e-3, 1.0)
_CASES = []


def _tensor(rng, n, pmag, gexp, kind=None):
    """One tensor's (p, g, m, v): |p| in pmag [0.5, 1) (0: exact zeros); |g| in 10^gexp [0.25, 1) (never near 0: the subnormal regime is left out);
    m signed, below |g|; v in 10^(2 gexp) [0.1, 1).  kind 'fresh': m = v = 0; 'zero': m = v = g = 0."""
    sign = lambda: rng.integers(0, 2, n) * 2.0 - 1.0
    gm = 10.0 ** gexp
    p = (sign() * pmag * rng.uniform(0.5, 1.0, n)).astype(F32)
    g = (sign() * gm * rng.uniform(0.25, 1.0, n)).astype(F32)
    m = (sign() * gm * 0.5 * rng.uniform(0.0, 1.0, n)).astype(F32)
    v = (gm * gm * rng.uniform(0.1, 1.0, n)).astype(F32)
    if kind in ("fresh", "zero"):
        m[:], v[:] = 0, 0
    if kind == "zero":
        g[:] = 0
    return p, g, m, v


def _table_tensors(rng):
    sizes = list(TABLE_SIZES) + [int(x) for x in rng.integers(1, 8, 300)] + [0]
    role_of = {i: r for r, i in ROLES.items()}
    spec = dict(eps=(0.0, -8.5, None), fresh=(0.0, -2.0, "fresh"), decay=(1.0, math.log10(0.05), None), zero=(1.0, 0.0, "zero"), sqrtv=(0.0, 0.0, None))
    parts = []
    for i, n in enumerate(sizes):
        pmag, gexp, kind = spec[role_of[i]] if i in role_of else (_PMAGS[i % 4], float(rng.uniform(-9, 2)), None)
        parts.append(_tensor(rng, n, pmag, gexp, kind))
    return [list(x) for x in zip(*parts)]


def _case(name, entry, data, hyper, scale_i, step, *, clip=False, decoupled=False, pairs=None, offset=None):
    p, g, m, v = data
    s = SCALES[scale_i]
    if s == 2.0 ** -16:
        g = [x * F32(65536.0) for x in g]          # a loss-scaled step: the buffers carry 2^16 x the gradient (exact), grad_scale takes it out
    lr_wd = None if pairs is None else [pairs[i % 2] for i in range(len(p))]
    return SimpleNamespace(name=name, entry=entry, p=p, g=g, m=m, v=v, hyper=Hyper(grad_scale=s, **hyper), step=step, clip=clip, decoupled=decoupled,
                           lr_wd=lr_wd, offset=offset, roles=ROLES if entry != "single" else {})


def cases():
    """Every launch the tests make: (name, entry single | multi | groups, p / g / m / v lists, hyper, first step, clip, decoupled, lr_wd).  Three consecutive
    steps start at `step`.  Built once; nobody writes into the arrays."""
    if _CASES:
        return _CASES
    rng = np.random.default_rng(20240613)
    table = _table_tensors(rng)
    A, B = HYPER_A, HYPER_B
    add = _CASES.append
    # single tensor: every size once, the hyper-parameter set, scale, first step and |p| rotating so that each value is met; n = 5 again as a view at an odd offset
    for k, n in enumerate(SINGLE_SIZES):
        data = [[x] for x in _tensor(rng, n, _PMAGS[k % 4], float(rng.uniform(-9, 2)))]
        add(_case(f"single/n{n}", "single", data, A if k % 2 == 0 else B, k % 3, STEPS[k % 5]))
    add(_case("single/n5/odd", "single", [[x] for x in _tensor(rng, 5, 0.0, -1.0)], A, 1, 1, offset=1))
    # the one large case: per-ELEMENT magnitudes (|p| one of the four, |g| = 10^U(-9, 2)), since it is a single tensor
    n = SINGLE_LARGE
    p, g, m, v = _tensor(rng, n, 1.0, 0.0)
    gm = (10.0 ** rng.uniform(-9, 2, n)).astype(F32)
    p *= np.asarray(_PMAGS, F32)[rng.integers(0, 4, n)]
    # (set B: without decay g' = g s, so no element can cancel its way under the regime's floor in any of the three steps; 4 million elements would find one)
    add(_case("single/large", "single", [[p], [g * gm], [m * gm], [v * gm * gm]], B, 1, 1))
    # the table launches: each entry point with both sets, the scales and steps spread over them
    for h, hn, si, t in ((A, "A", 0, 1), (A, "A", 1, 2), (B, "B", 1, 10), (A, "A", 2, 1000), (B, "B", 0, 100000)):
        add(_case(f"multi/{hn}/s{si}/t{t}", "multi", table, h, si, t))
    for h, hn, si, t in ((A, "A", 1, 1), (B, "B", 2, 2)):
        add(_case(f"multi_clip/{hn}/s{si}/t{t}", "multi", table, h, si, t, clip=True))
    for h, pr, hn, si, t, dec, clip in ((A, PAIRS_A, "A", 0, 1, False, False), (B, PAIRS_B, "B", 1, 10, False, False), (A, PAIRS_A, "A", 2, 1, True, False),
                                        (B, PAIRS_B, "B", 0, 1000, True, False), (A, PAIRS_A, "A", 1, 2, False, True), (B, PAIRS_B, "B", 0, 1, True, True)):
        kind = "groups" + ("_decoupled" if dec else "") + ("_clip" if clip else "")
        add(_case(f"{kind}/{hn}/s{si}/t{t}", "groups", table, h, si, t, clip=clip, decoupled=dec, pairs=pr))
    return _CASES


def case(name):
    return next(c for c in cases() if c.name == name)


def entry_point(c):
    """The C entry point a case goes through."""
    if c.entry == "single":
        return "vpt_adam_step"
    if c.entry == "multi":
        return "vpt_adam_step_multi_clip" if c.clip else "vpt_adam_step_multi"
    return "vpt_adam_step_groups[" + ("decoupled" if c.decoupled else "coupled") + (", clip" if c.clip else "") + "]"
