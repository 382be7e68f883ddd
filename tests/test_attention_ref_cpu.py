"""tests/attention_ref.py on the CPU: (1) its closed-form backward is the fp64 gradient (autograd through an independently written forward), (2) plain
fp32 arithmetic stays inside every bound of instrument B, (3) plain fp32 arithmetic reproduces instrument A's exact values bit for bit, (4) every
mutation of the fp32 emulation -- a subtly wrong kernel -- is caught by both instruments wherever it changes the mathematical result.
The emulation is torch's float32 arithmetic in torch's own summation order: every bound of attention_ref.py counts operations and holds for ANY order of
a sum, and instrument A's inputs give the same bits in every order, so the kernels' order does not enter.  Run with -s for the tables of worst err / bound."""
import functools
from types import SimpleNamespace

import pytest
import torch

from tests import attention_ref as A

D = torch.float64
F = torch.float32


def _variants(shape):
    b, t, ml, h, where = shape
    return [(b, t, ml, h, None), (b, t, ml, h, where)]


BANDED = [v for s in A.SHAPES for v in _variants(s)]
IDS = [f"B{b}-t{t}-maxlen{ml}-heads{h}-{'qlo' if w else 'plain'}" for b, t, ml, h, w in BANDED]


@functools.lru_cache(maxsize=None)
def _real(i):
    c = A.real_case(*BANDED[i], seed=i)
    return c, A.compute(c)


@functools.lru_cache(maxsize=None)
def _real_none(t):
    c = A.real_case(2, t, 0, 2, seed=t, causal=False)
    return c, A.compute(c)


def _autograd(c):
    """out and the gradients of sum(out * dout) by autograd, the forward written with softmax over an additive mask (the form of
    tests/test_gpu_episodes.py::_attention_case), not with compute()'s pieces."""
    B, t, H, ml, hid = c.B, c.t, c.heads, c.maxlen, c.hid
    qkvr = c.qkvr.double().requires_grad_(True)
    q = qkvr[:, :hid].reshape(B, t, H, 128).permute(0, 2, 1, 3)
    if not c.causal:
        kh = qkvr[:, hid:2 * hid].reshape(B, t, H, 128).permute(0, 2, 1, 3)
        vh = qkvr[:, 2 * hid:3 * hid].reshape(B, t, H, 128).permute(0, 2, 1, 3)
        out = (torch.softmax(q @ kh.transpose(-1, -2) / 128.0, -1) @ vh).permute(0, 2, 1, 3).reshape(B * t, hid)
        (gq,) = torch.autograd.grad((out * c.dout.double()).sum(), [qkvr])
        return out.detach(), gq, None
    b_nd = c.b_nd.double().requires_grad_(True)
    i = torch.arange(t).view(1, t, 1)
    j = torch.arange(t + ml).view(1, 1, t + ml)
    rows = torch.cat([c.memvalid.bool(), torch.ones(B, t, dtype=torch.bool)], 1)
    qlo = c.qlo.long().view(B, t, 1) if c.qlo is not None else torch.zeros(B, t, 1, dtype=torch.long)
    vis = (j >= i + 1) & (j <= i + ml) & (j >= qlo) & rows.view(B, 1, -1)
    kh = torch.cat([c.kmem.double(), qkvr[:, hid:2 * hid].reshape(B, t, hid)], 1).reshape(B, -1, H, 128).permute(0, 2, 1, 3)
    vh = torch.cat([c.vmem.double(), qkvr[:, 2 * hid:3 * hid].reshape(B, t, hid)], 1).reshape(B, -1, H, 128).permute(0, 2, 1, 3)
    rel = qkvr[:, 3 * hid:3 * hid + 10 * H].reshape(B, t, H, 10).permute(0, 2, 1, 3) @ b_nd              # [B, H, t, maxlen]: by band offset
    off = (ml + i - j).clamp(0, ml - 1).expand(B, t, t + ml).unsqueeze(1).expand(B, H, t, t + ml)
    logits = q @ kh.transpose(-1, -2) / 128.0 + rel.gather(-1, off)
    logits = logits.masked_fill(~vis.unsqueeze(1), -1e30)
    out = (torch.softmax(logits, -1) @ vh).permute(0, 2, 1, 3).reshape(B * t, hid)
    gq, gb = torch.autograd.grad((out * c.dout.double()).sum(), [qkvr, b_nd])
    return out.detach(), gq, gb


def _close(a, b, what):
    scale = float(b.abs().max().clamp(min=1e-30))
    err = float((a - b).abs().max())
    assert err <= 1e-11 * scale, f"{what}: max |difference| {err:.3e} at scale {scale:.3e}"


@pytest.mark.parametrize("i", range(len(BANDED)), ids=IDS)
def test_reference_is_the_gradient(i):
    c, o = _real(i)
    out, gq, gb = _autograd(c)
    _close(o.out, out, "out")
    pad = gq.clone()
    pad[:, 3 * c.hid + 10 * c.heads:] = 0            # (autograd's gradient of the unused padding columns is zero as well)
    assert torch.equal(pad, gq)
    _close(o.dqkvr, gq, "dqkvr")
    _close(o.db, gb, "db_nd")


@pytest.mark.parametrize("t", A.NONE_TS)
def test_reference_is_the_gradient_mask_none(t):
    c, o = _real_none(t)
    out, gq, _ = _autograd(c)
    _close(o.out, out, "out")
    _close(o.dqkvr, gq, "dqkv")


def _emulate(c, o, mut=None):
    """The fp32 emulation's outputs as a kernel would hand them over (16-bit forward output in both formats)."""
    e = A.compute(c, F, mut)
    return e, {fmt: e.out.to(A.DT[fmt]) for fmt in ("bf16", "fp16")}


def _all_ratios(c, o, e, o16):
    res, msgs = A.ratios(c, o, o16["bf16"], e.dqkvr, getattr(e, "db", None), "bf16")
    r16, m16 = A.ratios(c, o, o16["fp16"], None, None, "fp16")
    res["out fp16"] = r16["out"]
    return res, msgs + m16


def test_fp32_arithmetic_stays_inside_every_bound():
    table = {}
    fails = []
    runs = [(IDS[i], _real(i)) for i in range(len(BANDED))] + [(f"none-t{t}", _real_none(t)) for t in A.NONE_TS]
    for name, (c, o) in runs:
        e, o16 = _emulate(c, o)
        res, msgs = _all_ratios(c, o, e, o16)
        fails += [f"{name}: {m}" for m in msgs]
        for k, v in res.items():
            key = ("full" if not c.causal else "banded", k)
            table[key] = max(table.get(key, 0.0), v)
        print(name, " ".join(f"{k} {v:.4f}" for k, v in res.items()))
    for ml in A.STEP_MAXLENS:                        # the t = 1 step is compute() on the step's visibility
        c = A.real_case(2, 1, ml, 2, seed=ml)
        for first in (torch.tensor([False, False]), torch.tensor([True, False])):
            o = A.step_ref(c, first)[0]
            cs = SimpleNamespace(**{**vars(c), "memvalid": (c.memvalid.bool() & ~first.view(-1, 1)).to(torch.uint8)})
            e = A.compute(cs, F, backward=False)
            for fmt in ("bf16", "fp16"):
                w, m = A.check(c, f"step out maxlen {ml}", "out", e.out.to(A.DT[fmt]), o.out, A.out_bound(o, fmt))
                table[("step", f"out {fmt}")] = max(table.get(("step", f"out {fmt}"), 0.0), w)
                fails += [m] if m else []
    for key in sorted(table):
        print("fp32 emulation, worst err / bound:", *key, f"{table[key]:.4f}")
    assert not fails, "\n".join(fails)


def _exact_run(shape_i, fam, rule):
    c = A.exact_case(*BANDED[shape_i], family=fam, rule=rule, seed=shape_i)
    return c, A.compute(c, flush=True)


@pytest.mark.parametrize("i", range(len(BANDED)), ids=IDS)
def test_fp32_arithmetic_gives_the_exact_values(i):
    """... and the construction is what the module docstring says: every weight is 0, 1/2 or 1, every visible query has weight 1 in total."""
    seen = set()
    for fam, rule in A.EXACT_RUNS:
        c, o = _exact_run(i, fam, rule)
        vals = set(o.p.unique().tolist())
        assert vals <= {0.0, 0.5, 1.0}, f"{fam} {rule}: weights {sorted(vals)}"
        assert bool((o.p.sum(-1) == 1.0).all())
        e = A.compute(c, F)
        for fmt in ("bf16", "fp16"):
            msgs = A.exact_failures(c, o, e.out.to(A.DT[fmt]), e.dqkvr, e.db)
            assert not msgs, f"{fam} {rule} {fmt}:\n" + "\n".join(msgs)
        if fam != "bias":
            assert not bool(o.db.any())
            for b in range(c.B):
                for h in range(c.heads):
                    for q, tg in enumerate(c.targets[b][h]):
                        seen |= {("off", c.maxlen + q - j) for j in tg} | {("slot", j - (q & ~31) - 1) for j in tg} | {("row", j) for j in tg}
        if fam == "tie":
            assert bool(o.dqkvr[:, :3 * c.hid].any()) or c.maxlen == 1, "the tie family must give nonzero dQ / dK"
        if fam == "bias":
            assert bool(o.db.any()) or c.maxlen == 1
    b, t, ml, h, w = BANDED[i]
    want = {("off", 0), ("off", ml - 1), ("row", ml)} | ({("row", ml - 1)} if ml > 1 else set())
    if t >= 32 and ml >= 128:
        want |= {("slot", 127), ("slot", 128), ("slot", ml + 30)}          # ml + 30: the last query of a tile itself -- slot 159 of 160 at maxlen = 129
    assert want <= seen, f"targets never placed at {sorted(want - seen)}"


def test_fp32_arithmetic_gives_the_exact_values_mask_none():
    for t in A.NONE_TS:
        for fam, rule in A.EXACT_RUNS[:-1]:
            c = A.exact_case(2, t, 0, 2, family=fam, rule=rule, seed=t, causal=False)
            o = A.compute(c, flush=True)
            assert set(o.p.unique().tolist()) <= {0.0, 0.5, 1.0}
            e = A.compute(c, F)
            msgs = A.exact_failures(c, o, e.out.to(torch.bfloat16), e.dqkvr, None)
            assert not msgs, f"t = {t} {fam} {rule}:\n" + "\n".join(msgs)


# Mutations instrument B cannot see at a shape, with the reason; they must still fail instrument A there.
B_BLIND = {}


def _differs(c, o, m):
    """The mutation changes the mathematical result of this case (fp64, any output, any element)."""
    return any(not torch.equal(getattr(m, f), getattr(o, f)) for f in ("out", "dqkvr", "db") if hasattr(o, f))


MUT_SHAPES = [i for i, v in enumerate(BANDED) if v[1] != 200]          # (the t = 200 case adds tiles, no new mutation site)


@pytest.mark.parametrize("mut", A.MUTATIONS)
def test_every_mutation_fails_both_instruments(mut):
    lines, fails, applied = [], [], 0
    for i in MUT_SHAPES:
        c, o = _real(i)
        applies_b = _differs(c, o, A.compute(c, D, mut))
        if applies_b:
            e, o16 = _emulate(c, o, mut)
            res, _ = _all_ratios(c, o, e, o16)
            worst = max(res.values())
            lines.append(f"{mut} {IDS[i]}: instrument B worst ratio {worst:.3g} ({max(res, key=res.get)})")
            if (IDS[i], mut) in B_BLIND:
                assert worst <= 1.0, f"{IDS[i]} {mut} is listed as invisible to instrument B but has ratio {worst}"
            elif not worst > 1.0:
                fails.append(f"instrument B does not see {mut} at {IDS[i]}: worst ratio {worst:.3g}")
        caught_a = applies_a = False
        for fam, rule in A.EXACT_RUNS:
            ce, oe = _exact_run(i, fam, rule)
            if not _differs(ce, oe, A.compute(ce, D, mut, flush=True)):
                continue
            applies_a = True
            e = A.compute(ce, F, mut)
            if A.exact_failures(ce, oe, e.out.to(torch.bfloat16), e.dqkvr, e.db):
                caught_a = True
                break
        if applies_a and not caught_a:
            fails.append(f"instrument A does not see {mut} at {IDS[i]}")
        if applies_b and not applies_a:
            fails.append(f"{mut} changes the real-valued result at {IDS[i]} but none of instrument A's runs")
        applied += applies_b or applies_a
    print("\n".join(lines))
    assert applied, f"{mut} applies to no shape"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mut", A.NONE_MUTATIONS)
def test_every_mutation_fails_both_instruments_mask_none(mut):
    for t in (33, 160):
        c, o = _real_none(t)
        e = A.compute(c, F, mut)
        res, _ = A.ratios(c, o, e.out.to(torch.float16), e.dqkvr, None, "fp16")
        print(f"{mut} none-t{t}: instrument B worst ratio {max(res.values()):.3g}")
        assert max(res.values()) > 1.0
        caught = False
        for fam, rule in A.EXACT_RUNS[:-1]:
            ce = A.exact_case(2, t, 0, 2, family=fam, rule=rule, seed=t, causal=False)
            e = A.compute(ce, F, mut)
            caught = caught or bool(A.exact_failures(ce, A.compute(ce, flush=True), e.out.to(torch.bfloat16), e.dqkvr, None))
        assert caught, f"instrument A does not see {mut} at t = {t}"
