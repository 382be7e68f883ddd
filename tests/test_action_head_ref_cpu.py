"""tests/action_head_ref.py on the CPU: the fp64 reference is torch's log_softmax / autograd / argmax, the fp32 emulation of the kernels' order of
operations stays inside every bound on every case of tests/test_gpu_action_head_fp64.py, every mutation leaves a bound or changes a selected index, the
selection with the in-range rule answers a NaN row and an all-zero noise row as torch.argmax does, and every row of every selection case has a winning
margin of more than twice the score bound, so the GPU file compares indices exactly.  Run with -s for the ratios."""
import math

import pytest
import torch

from tests import action_head_ref as R

F = torch.float32
LSM = R.lsm_cases()


def _head_cases():
    for nb, nc, ldz in R.HEAD_SHAPES:
        for m in R.HEAD_ROWS:
            for v in ((0, 1, 2) if m == 1 else (0,)):
                yield f"nb {nb} nc {nc} ldz {ldz} M {m} labels {v}", R.head_case(m, nb, nc, ldz, variant=v)


def _heads_cases():
    for nb, nc, ldz in R.HEAD_SHAPES:
        for m in R.HEAD_ROWS:
            for gs, drop, mask in R.HEADS_CONFIGS:
                yield f"nb {nb} nc {nc} ldz {ldz} M {m} grad_scale {gs} None {drop} mask {mask}", R.head_case(m, nb, nc, ldz, mask=mask, grad_scale=gs, drop=drop)


# ---- the reference is torch's --------------------------------------------------------------------------------------------------------------------------
def test_log_softmax_reference_is_torch():
    for label, c in LSM:
        o = R.compute(c)
        z = c.z[:, c.col0:c.col0 + c.n].double() / c.T
        if c.mask is not None:
            z = torch.where(c.mask == 0, torch.full_like(z, -100.0), z)
        want = torch.log_softmax(z, 1)
        assert float((o.lp - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), label
        if c.act != "none":
            sc = want
            if c.noise is not None:
                u = torch.where(c.noise == 1.0, torch.tensor(0.999, dtype=F), c.noise).double()
                sc = want - torch.log(-torch.log(u))
            assert torch.equal(o.action, torch.argmax(o.sc, 1)), label
            assert torch.equal(o.action, torch.argmax(sc, 1)), label
            assert torch.equal(o.action_logp, o.lp.gather(1, o.action[:, None])[:, 0])


def test_backward_references_are_autograd():
    """The kernels take the fp32 log-probs as their input, so autograd runs through log_softmax of those: it renormalises by sum exp(lp) = 1 +- 1e-6, which
    is the tolerance; a misplaced one-hot, sign, sum or column is an error of order 1."""
    for label, c in _heads_cases():
        r = torch.arange(c.M)
        xs, lps = [], []
        for lp, mk in ((c.lp_b, c.mask_b), (c.lp_c, c.mask_c)):
            x = (lp.double() * c.T).requires_grad_(True)
            s = x / c.T
            lps.append(torch.log_softmax(torch.where(mk == 0, torch.full_like(s, -100.0), s) if mk is not None else s, 1))
            xs.append(x)
        # nll / bc_loss: -scale w (lp_b[label] + lp_c[label]) / with respect to the SCALED logits
        for kind, w in (("nll", torch.ones(c.M, dtype=torch.float64)), ("bc", c.weight.double())):
            ss = [(lp.double()).requires_grad_(True) for lp in (c.lp_b, c.lp_c)]
            loss = -(c.scale * w * (torch.log_softmax(ss[0], 1)[r, c.act_b] + torch.log_softmax(ss[1], 1)[r, c.act_c])).sum()
            gb, gc = torch.autograd.grad(loss, ss)
            o = R.compute(c, kind=kind)
            want = torch.zeros(c.M, c.ldz, dtype=torch.float64)
            want[:, :c.nb], want[:, c.nb:c.nb + c.nc] = gb, gc
            assert float((o.dz - want).abs().max()) <= 1e-5 * c.scale * 2, f"{kind} {label}"
            assert bool((o.dz[:, c.nb + c.nc:] == 0).all())
        o = R.compute(c, kind="bc")
        for h, lp in enumerate((c.lp_b, c.lp_c)):
            p = torch.exp(lp.double())
            assert float((o.ent[:, h] + (p * lp.double()).sum(1)).abs().max()) <= 1e-12 * 10
            assert torch.equal(o.nll[:, h], -lp.double()[r, (c.act_b, c.act_c)[h]])
        # heads backward: any incoming gradient
        gin = [g.double() if g is not None else torch.zeros_like(lp, dtype=torch.float64) for g, lp in ((c.g_b, c.lp_b), (c.g_c, c.lp_c))]
        gb, gc = torch.autograd.grad((lps[0] * gin[0]).sum() + (lps[1] * gin[1]).sum(), xs)
        want = torch.zeros(c.M, c.ldz, dtype=torch.float64)
        want[:, :c.nb], want[:, c.nb:c.nb + c.nc] = gb * c.grad_scale, gc * c.grad_scale
        if c.g_v is not None:
            want[:, c.nb + c.nc] = c.g_v.double() * c.grad_scale
        o = R.compute(c, kind="heads")
        mag = max(float(g.abs().sum(1).max()) for g in gin) * c.grad_scale
        assert float((o.dz - want).abs().max()) <= 1e-5 * max(mag, 1e-30), f"heads {label}"
        assert bool((o.dz[:, c.nb + c.nc + 1:] == 0).all())


# ---- the fp32 emulation meets every bound -------------------------------------------------------------------------------------------------------------------
def _lsm_ratios(c, o, e):
    res, msgs = {}, []
    res["lp"], m = R.check("lp", e.lp, o.lp, o.b_lp)
    msgs += [m] if m else []
    if c.act != "none":
        res["score"], m = R.check("score", e.sc, o.sc, o.b_sc)
        msgs += [m] if m else []
        if not torch.equal(e.action, o.action):
            res["action"] = math.inf
            msgs.append(f"action: rows {(e.action != o.action).nonzero()[:, 0].tolist()} differ")
        if not torch.equal(e.action_logp, e.lp.gather(1, e.action[:, None])[:, 0]):
            res["action_logp"] = math.inf
            msgs.append("action_logp is not lp[row, action]")
    return res, msgs


def _dz_ratios(name, o, e, extra=()):
    res, msgs = {}, []
    for fmt in ("bf16", "fp16"):
        res[f"{name} dz {fmt}"], m = R.check(f"{name} dz {fmt}", e.dz.to(R.DT[fmt]), o.dz, R.bound16(o.dz, o.b_dz, fmt))
        msgs += [m] if m else []
    for nm in extra:
        res[f"{name} {nm}"], m = R.check(f"{name} {nm}", getattr(e, nm), getattr(o, nm), getattr(o, "b_" + nm))
        msgs += [m] if m else []
    return res, msgs


def _gather(table, res):
    for k, v in res.items():
        table[k] = max(table.get(k, 0.0), v)


def test_fp32_emulation_stays_inside_every_bound():
    table, fails = {}, []
    for label, c in LSM:
        res, msgs = _lsm_ratios(c, R.compute(c), R.compute(c, F))
        _gather(table, {f"log_softmax NW {c.nw} {k}": v for k, v in res.items()})
        fails += [f"{label}: {x}" for x in msgs]
    for label, c in _head_cases():
        for kind in ("nll", "bc"):
            res, msgs = _dz_ratios(kind, R.compute(c, kind=kind), R.compute(c, F, kind=kind), ("ent",) if kind == "bc" else ())
            _gather(table, res)
            fails += [f"{label}: {x}" for x in msgs]
    for label, c in _heads_cases():
        res, msgs = _dz_ratios("heads", R.compute(c, kind="heads"), R.compute(c, F, kind="heads"))
        _gather(table, res)
        fails += [f"{label}: {x}" for x in msgs]
    for k in sorted(table):
        print(f"fp32 emulation, worst err / bound: {k} {table[k]:.4f}")
    assert not fails, "\n".join(fails)


# ---- every mutation is caught ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutation_leaves_a_bound_or_changes_an_index(mut):
    kind = R.KINDS[mut]
    worst_of = []
    if kind == "lsm":
        for label, c in LSM:
            o, e, w = R.compute(c), R.compute(c, F), R.compute(c, F, mut)
            if torch.equal(w.lp, e.lp) and (c.act == "none" or (torch.equal(w.sc, e.sc) and torch.equal(w.action, e.action))):
                continue                                   # the mutation does not touch this case (no mask, no tail, no tie, no u == 1 ...)
            res, _ = _lsm_ratios(c, o, w)
            worst_of.append((max(res.values()), label))
    else:
        for label, c in (_head_cases() if kind == "nll" else _heads_cases()):
            for k in (("nll", "bc") if kind == "nll" else ("heads",)):
                o, e, w = R.compute(c, kind=k), R.compute(c, F, kind=k), R.compute(c, F, mut, kind=k)
                if torch.equal(w.dz, e.dz):
                    continue
                res, _ = _dz_ratios(k, o, w)
                worst_of.append((max(res.values()), f"{k} {label}"))
    assert worst_of, "the mutation changed no case"
    caught = [x for x in worst_of if x[0] > 1.0]
    print(f"{mut}: changes {len(worst_of)} cases, caught on {len(caught)}; smallest worst ratio over the changed cases {min(worst_of)[0]:.3g} ({min(worst_of)[1]}), "
          f"largest {max(worst_of)[0]:.3g}")
    assert caught


def test_scaling_by_the_rounded_reciprocal_is_within_the_bound():
    """z * fl(1 / T) instead of z / T is a different rounding, not an error: the bound allows it."""
    for label, c in LSM[::7]:
        o = R.compute(c)
        z = c.z[:, c.col0:c.col0 + c.n]
        cc = z * (torch.tensor(1.0) / torch.tensor(c.T))
        if c.mask is not None:
            cc = torch.where(c.mask == 0, torch.full_like(cc, -100.0), cc)
        w, _ = R.worst(torch.log_softmax(cc.double(), 1).float(), o.lp, o.b_lp)
        assert w <= 1.0, (label, w)


# ---- the in-range index rule -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 65, 65, 0), (64, 2305, 2305, 0), (2, 9217, 9217, 0)])
def test_selection_of_a_nan_row_and_of_a_zero_noise_row_is_index_zero(shape):
    c = R.lsm_case(*shape, act="det")
    c.z[0, c.col0 + c.n // 2] = float("nan")
    e = R.compute(c, F)
    assert bool(torch.isnan(e.sc[0]).all()) and bool(torch.isfinite(e.sc[1:]).all())
    assert torch.equal(e.action, torch.argmax(e.sc, 1)) and int(e.action[0]) == 0
    assert bool(((e.action >= 0) & (e.action < c.n)).all()) and math.isnan(float(e.action_logp[0]))
    c = R.lsm_case(*shape, act="noise")
    c.noise[0] = 0.0
    e = R.compute(c, F)
    assert bool((e.sc[0] == -math.inf).all())
    assert torch.equal(e.action, torch.argmax(e.sc, 1)) and int(e.action[0]) == 0
    assert bool(((e.action >= 0) & (e.action < c.n)).all()) and bool(torch.isfinite(e.action_logp).all()) and bool(torch.isfinite(e.lp).all())


# ---- the selection margin: a condition on the inputs ----------------------------------------------------------------------------------------------------------
def test_every_row_wins_by_more_than_twice_the_score_bound():
    smallest = (math.inf, "")
    fails = []
    for label, c in LSM:
        if c.act == "none":
            continue
        mg = R.margin(R.compute(c))
        smallest = min(smallest, (float(mg.min()), label))
        if not bool((mg > 1.0).all()):
            fails.append(f"{label}: rows {(~(mg > 1.0)).nonzero()[:, 0].tolist()}, margin / (2 bound) = {float(mg.min()):.3g}")
    print(f"smallest (winner - runner-up) / (2 x score bound): {smallest[0]:.3g} ({smallest[1]})")
    assert not fails, "\n".join(fails)


def test_tie_cases_select_the_expected_column():
    for name, m, n, i, j in R.TIES:
        for hw in (False, True):
            for dt in (R.D64, F):
                o = R.compute(R.tie_case(m, n, i, j, hw), dt)
                assert bool((o.action == (j if hw else i)).all()), (name, hw, dt)
