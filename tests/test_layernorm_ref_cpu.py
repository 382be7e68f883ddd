"""tests/layernorm_ref.py on the CPU: its backward is the fp64 gradient, plain fp32 arithmetic stays inside every bound, and every mutation of the
fp32 emulation leaves a bound wherever it changes the result.  Run with -s for the ratios."""
import pytest
import torch

from tests import layernorm_ref as R

F = torch.float32
CONFIGS = [(relu_in, use_add) for relu_in in (False, True) for use_add in (False, True)]


@pytest.mark.parametrize("d", [4, 1000, 1028])
def test_reference_is_the_gradient(d):
    c = R.case(5, d)
    for relu_in, use_add in CONFIGS:
        o = R.compute(c, relu_in, use_add)
        x, g, b = c.x.double().requires_grad_(True), c.gain.double().requires_grad_(True), c.bias.double().requires_grad_(True)
        xr = torch.relu(x) if relu_in else x
        y = torch.nn.functional.layer_norm(xr, (d,), g, b, eps=R.EPS)
        gx, gg, gb = torch.autograd.grad((y * c.dy.double()).sum(), [x, g, b])
        for got, want, nm in ((o.y, y.detach(), "y"), (o.dx, gx + (c.dx_add.double() if use_add else 0), "dx"), (o.dgain, gg + c.dgain0.double(), "dgain"),
                              (o.dbias, gb + c.dbias0.double(), "dbias")):
            err = float((got - want).abs().max())
            assert err <= 1e-11 * float(want.abs().max()), f"{nm} relu_in={relu_in} dx_add={use_add}: {err:.3e}"


def _ratios(c, o, e):
    res, msgs = R.backward_ratios(o, e.dx, e.dgain, e.dbias)
    res["y"], m = R.check("y", e.y, o.y, o.b_y)
    msgs += [m] if m else []
    for fmt in ("bf16", "fp16"):
        res[f"y {fmt}"], m = R.check(f"y {fmt}", e.y.to(R.DT[fmt]), o.y, o.b_y + R.ulp16(o.y, fmt))
        msgs += [m] if m else []
    return res, msgs


def test_fp32_arithmetic_stays_inside_every_bound():
    table, fails = {}, []
    for d in R.WIDTHS:
        for m in R.ROWS:
            c = R.case(m, d)
            for relu_in, use_add in CONFIGS:
                o = R.compute(c, relu_in, use_add)
                res, msgs = _ratios(c, o, R.compute(c, relu_in, use_add, F))
                fails += [f"M {m} D {d} relu_in {relu_in} dx_add {use_add}: {x}" for x in msgs]
                for k, v in res.items():
                    table[k] = max(table.get(k, 0.0), v)
    for k in sorted(table):
        print(f"fp32 emulation, worst err / bound: layernorm {k} {table[k]:.4f}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutation_leaves_a_bound(mut):
    applied = 0
    for m, d in [(5, 256), (33, 1028), (5, 4096)]:
        c = R.case(m, d)
        for relu_in, use_add in CONFIGS:
            o = R.compute(c, relu_in, use_add)
            w = R.compute(c, relu_in, use_add, mut=mut)
            if all(torch.equal(getattr(w, f), getattr(o, f)) for f in ("y", "dx", "dgain", "dbias")):
                continue                                  # (gate_ignored without relu_in, dx_add_dropped without dx_add)
            applied += 1
            res, _ = _ratios(c, o, R.compute(c, relu_in, use_add, F, mut))
            print(f"{mut} M {m} D {d} relu_in {relu_in} dx_add {use_add}: worst ratio {max(res.values()):.3g} ({max(res, key=res.get)})")
            assert max(res.values()) > 1.0
    assert applied
