"""vpt_layernorm_kernel and vpt_ln_bwd_kernel<4|8|12|16> + vpt_ln_bwd_finish_kernel against the fp64 reference of tests/layernorm_ref.py under its derived
per-element bounds.  Needs an MI355X.  Widths on either side of the backward's template thresholds (1024 | 1028, 2048 | 2052, 3072 | 3076), D = 4 (one
lane of a wave holds the row) and 4096 (the widest the backward takes); M = 1, 5 and 33 (a second workgroup holding one row); the ReLU on the input and the
residual gradient both ways; dgain / dbias pre-filled, because the finish kernel adds into them.  Every check prints `max err / bound`."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from tests import layernorm_ref as R  # noqa: E402

DEV = "cuda"
RATIOS = {}


def _note(res):
    for k, v in res.items():
        RATIOS[k] = max(RATIOS.get(k, 0.0), v)


@pytest.mark.parametrize("m", R.ROWS)
@pytest.mark.parametrize("d", R.WIDTHS)
def test_layernorm_forward(d, m):
    c = R.case(m, d)
    x, gain, bias = c.x.to(DEV), c.gain.to(DEV), c.bias.to(DEV)
    fails = []
    for relu_in in (False, True):
        o = R.compute(c, relu_in, False)
        for fmt in ("bf16", "fp16"):
            y32, y16 = ops.layernorm(x, gain, bias, relu_in=relu_in, out_f32=True, out_bf16=True, dtype=R.DT[fmt])
            only32, none16 = ops.layernorm(x, gain, bias, relu_in=relu_in, out_f32=True, out_bf16=False)
            torch.cuda.synchronize()
            assert none16 is None and torch.equal(only32, y32) and y16.dtype == R.DT[fmt]
            res = {}
            res["y"], m32 = R.check("y", y32.cpu(), o.y, o.b_y)
            res[f"y {fmt}"], m16 = R.check(f"y {fmt}", y16.cpu(), o.y, o.b_y + R.ulp16(o.y, fmt))
            print(f"layernorm M {m} D {d} relu_in {relu_in} {fmt}: max err / bound: " + "  ".join(f"{k} {v:.4f}" for k, v in res.items()))
            _note(res)
            fails += [f"relu_in {relu_in} {fmt}: {x_}" for x_ in (m32, m16) if x_]
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("m", R.ROWS)
@pytest.mark.parametrize("d", R.WIDTHS)
def test_layernorm_backward(d, m):
    c = R.case(m, d)
    x, gain, dy, add = c.x.to(DEV), c.gain.to(DEV), c.dy.to(DEV), c.dx_add.to(DEV)
    fails = []
    for relu_in in (False, True):
        for use_add in (False, True):
            o = R.compute(c, relu_in, use_add)
            dgain, dbias = c.dgain0.to(DEV), c.dbias0.to(DEV)
            dx = ops.layernorm_backward(x, gain, dy, dgain, dbias, relu_in=relu_in, dx_add=add if use_add else None)
            torch.cuda.synchronize()
            res, msgs = R.backward_ratios(o, dx.cpu(), dgain.cpu(), dbias.cpu())
            print(f"layernorm_backward M {m} D {d} relu_in {relu_in} dx_add {use_add}: max err / bound: " + "  ".join(f"{k} {v:.4f}" for k, v in res.items()))
            _note(res)
            fails += [f"relu_in {relu_in} dx_add {use_add}: {x_}" for x_ in msgs]
    assert not fails, "\n".join(fails)


def test_print_worst_ratios():
    """Not a check: the table profiles/attention_fp64_ratios.md quotes (run the module with -s)."""
    for key in sorted(RATIOS):
        print("worst err / bound: layernorm", key, f"{RATIOS[key]:.4f}")
