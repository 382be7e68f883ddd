"""vpt_grouped_lp_bwd_kernel (ops.grouped_logprob_backward: the backward of the IDM's grouped log-softmax heads for an arbitrary incoming gradient)
on the GPU against the fp64 reference tests/grouped_logprob_ref.py with its derived bound, bit for bit against the verified loss kernel
(ops.idm_loss) where the two must coincide, exact zeros where the definition has zeros, reproducibility, exact power-of-two scaling, the argument
checks.  Needs an MI355X.  Shapes (M, gb, nb, gc, nc): (1, 1, 1, 1, 1) one-class groups; (3, 20, 2, 2, 11) the released heads, 62 columns + 2 of
padding; (5, 3, 7, 2, 5) odd widths and a partly filled workgroup; (2, 6, 11, 1, 3) 69 columns, ldz = 128, a lane owns two columns."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from tests import grouped_logprob_ref as R  # noqa: E402

DEV = "cuda"
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
MIN_NORMAL = {"bf16": 2.0 ** -126, "fp16": 2.0 ** -14}
_CASES = {}


def _case(shape, temperature=2.0, masks=True):
    key = (shape, temperature, masks)
    if key not in _CASES:
        c = R.make_case(*R.SHAPES[shape], temperature=temperature, masks=masks)
        g = {k: c[k].to(DEV) for k in ("lb", "lc", "gb_in", "gc_in")}
        g["mask_b"] = c["mask_b"].to(torch.uint8).to(DEV) if masks else None
        g["mask_c"] = c["mask_c"].to(torch.uint8).to(DEV) if masks else None
        _CASES[key] = (c, g)
    return _CASES[key]


def _run(c, g, fmt, buttons=True, camera=True, grad_scale=1.0):
    return ops.grouped_logprob_backward(g["lb"], g["lc"], g["gb_in"] if buttons else None, g["gc_in"] if camera else None, c["temperature"],
                                        mask_buttons=g["mask_b"], mask_camera=g["mask_c"], dtype=DT[fmt], grad_scale=grad_scale)


@pytest.mark.parametrize("temperature", [1.0, 2.0])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_against_the_fp64_reference(shape, fmt, temperature):
    """max err / bound <= 1 (printed) with the bound of tests/grouped_logprob_ref.py; padding columns and masked elements are exact zeros (their
    bound is 0: the ratio is inf otherwise, and they are asserted on their own as well); a one-class shape is all zeros.  Every mutated reference
    -- 1 / T left out, the sum over the whole head, the camera block one column to the right -- fails the same assertion wherever it is another
    reference at all, and is asserted to BE the reference elsewhere."""
    c, g = _case(shape, temperature)
    dz = _run(c, g, fmt)
    torch.cuda.synchronize()
    ref = R.reference(c)
    m, cols, ldz = c["m"], ref["cols"], ref["ldz"]
    assert dz.dtype == DT[fmt] and tuple(dz.shape) == (m, ldz)
    r = R.ratio(dz, ref, fmt)
    print(f"grouped_logprob_backward[{shape}, {fmt}, T={temperature}] max err / bound: {r:.3f}")
    assert r <= 1.0
    assert float(dz[:, cols:].float().abs().max()) == 0.0
    masked = ~torch.cat([c["mask_b"].reshape(m, -1), c["mask_c"].reshape(m, -1)], 1)
    if shape == "one":
        assert float(dz.float().abs().max()) == 0.0
    else:
        assert int(masked.sum()) > 0 and float(dz[:, :cols][masked.to(DEV)].float().abs().max()) == 0.0
        assert float(dz.float().abs().max()) > 0.1
    for mut in R.MUTATIONS:
        bad = R.reference(c, mutate=mut)
        if not R.mutant_differs(mut, c):
            assert torch.equal(bad["dz"], ref["dz"]), mut
            continue
        rb = R.ratio(dz, bad, fmt)
        print(f"    mutated reference {mut}: err / bound {rb:.1f}")
        assert not rb <= 1.0, (mut, rb)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_a_head_without_gradient_is_a_zero_block(shape, fmt):
    c, g = _case(shape)
    nbt, cols = c["gb"] * c["nb"], c["gb"] * c["nb"] + c["gc"] * c["nc"]
    full = _run(c, g, fmt)
    no_b, no_c, none = _run(c, g, fmt, buttons=False), _run(c, g, fmt, camera=False), _run(c, g, fmt, buttons=False, camera=False)
    torch.cuda.synchronize()
    assert float(no_b[:, :nbt].float().abs().max()) == 0.0 and torch.equal(no_b[:, nbt:], full[:, nbt:])
    assert float(no_c[:, nbt:].float().abs().max()) == 0.0 and torch.equal(no_c[:, :nbt], full[:, :nbt])
    assert float(none.float().abs().max()) == 0.0
    for fl, kw in ((no_b, dict(use_buttons=False)), (no_c, dict(use_camera=False))):
        assert R.ratio(fl, R.reference(c, **kw), fmt) <= 1.0


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_ten_identical_calls_give_the_same_bits(shape, fmt):
    c, g = _case(shape)
    outs = [_run(c, g, fmt) for _ in range(10)]
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs[1:])


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s != "one"])
def test_grad_scale_is_an_exact_power_of_two_factor(shape, fmt):
    """grad_scale 256 against 4096: both scalings are exact in fp32 and the one rounding commutes with a factor 16, so the outputs differ by exactly
    16 on every element that is a normal number of the format at the smaller scale -- at least 99 % of them (100 % on these inputs,
    tests/test_grouped_logprob_ref_cpu.py), the rest may have lost bits to a subnormal."""
    c, g = _case(shape, masks=False)
    lo, hi = _run(c, g, fmt, grad_scale=256.0).double(), _run(c, g, fmt, grad_scale=4096.0).double()
    torch.cuda.synchronize()
    cols = c["gb"] * c["nb"] + c["gc"] * c["nc"]
    normal = lo[:, :cols].abs() >= MIN_NORMAL[fmt]
    assert float(normal.double().mean()) >= 0.99 and bool(torch.isfinite(hi).all())
    assert torch.equal(hi[:, :cols][normal], 16.0 * lo[:, :cols][normal])
    assert float(hi[:, cols:].abs().max()) == 0.0


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_mean_nll_gradient_equals_the_loss_kernel_bit_for_bit(fmt):
    """The anchor to the verified loss kernel: M = 16, T = 2, g = -onehot / 16 (what autograd of the mean NLL delivers), grad_scale = 1 -> dz is
    torch.equal to ops.idm_loss(..., scale = 1 / (16 * 2)).  With M and T powers of two every scaling is exact: s = -1 / 16, p s = -p / 16 and
    g - p s = (p - onehot) / 16 rounds exactly where the loss kernel's fl(p - onehot) rounds, so both kernels round fl(p - onehot) once and then
    scale it exactly; a difference would mean a contraction or another order of operations than the contract's."""
    m, (_, gb, nb, gc, nc) = 16, R.SHAPES["released"]
    c = R.make_case(m, gb, nb, gc, nc, temperature=2.0, masks=False)
    gen = torch.Generator().manual_seed(3)
    ab, ac = torch.randint(0, nb, (m, gb), generator=gen), torch.randint(0, nc, (m, gc), generator=gen)
    g_b = -torch.nn.functional.one_hot(ab, nb).float() / m
    g_c = -torch.nn.functional.one_hot(ac, nc).float() / m
    lb, lc = c["lb"].to(DEV), c["lc"].to(DEV)
    dz = ops.grouped_logprob_backward(lb, lc, g_b.to(DEV), g_c.to(DEV), 2.0, dtype=DT[fmt], grad_scale=1.0)
    want, _, _ = ops.idm_loss(lb, lc, ab.to(DEV), ac.to(DEV), 1.0 / (m * 2.0), dtype=DT[fmt], want_frames=False, want_totals=False)
    torch.cuda.synchronize()
    assert dz.shape == want.shape and float(want.float().abs().max()) > 0
    assert torch.equal(dz, want)


def test_argument_checks():
    c, g = _case("released")
    lb, lc = g["lb"], g["lc"]
    with pytest.raises(RuntimeError, match="temperature"):
        ops.grouped_logprob_backward(lb, lc, g["gb_in"], g["gc_in"], 0.0)
    with pytest.raises(ValueError):
        ops.grouped_logprob_backward(lb.reshape(3, 40), lc, None, None, 1.0)
    with pytest.raises(ValueError):
        ops.grouped_logprob_backward(lb, lc, g["gb_in"][:, :10].contiguous(), None, 1.0)
    with pytest.raises(TypeError):
        ops.grouped_logprob_backward(lb, lc, g["gb_in"].double(), None, 1.0)
    with pytest.raises(TypeError):
        ops.grouped_logprob_backward(lb, lc, None, None, 1.0, mask_buttons=g["mask_b"].bool())
    # the C entry's own checks (the Python front end never produces these)
    import ctypes
    from vpt_amd import _native
    lib = _native.load("bf16")
    dz = torch.zeros(3, 64, dtype=torch.bfloat16, device=DEV)
    p = _native.ptr
    f = ctypes.c_float
    for args, word in (((0, 20, 2, 2, 11, 64, f(1.0)), "M must be positive"), ((3, 20, 2, 2, 11, 64, f(-1.0)), "temperature"),
                       ((3, 20, 0, 2, 11, 64, f(1.0)), "at least 1"), ((3, 20, 2, 2, 11, 61, f(1.0)), "ldz")):
        rc = lib.vpt_grouped_logprob_backward(p(lb), p(lc), None, None, None, None, p(dz), *args, f(1.0), None)
        assert rc == -1 and word in lib.vpt_last_error().decode(), (args, lib.vpt_last_error())
    torch.cuda.synchronize()
    assert float(dz.float().abs().max()) == 0.0
