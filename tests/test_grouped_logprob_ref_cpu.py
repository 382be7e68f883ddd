"""tests/grouped_logprob_ref.py on the CPU: the fp64 closed form IS torch's fp64 gradient through log_softmax(where(mask, z, LOG0) / T) (1e-12, masks
included); on the GPU tests' own inputs the reference rounded to bf16 / fp16 and a float32 restatement in the kernel's order pass the bound (the
bound is satisfiable), every mutated reference fails it wherever it is another reference at all, and the scale-256 outputs are normal numbers of
the format on at least 99 % of the elements (what the GPU test's exact-factor-16 check needs).  The native library declares and exports the entry."""
import ctypes
import os

import pytest
import torch

from tests import grouped_logprob_ref as R

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
MIN_NORMAL = {"bf16": 2.0 ** -126, "fp16": 2.0 ** -14}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("temperature", [1.0, 2.0])
@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_closed_form_is_the_fp64_gradient(shape, temperature):
    c = R.make_case(*R.SHAPES[shape], temperature=temperature)
    leaves, c64 = {}, dict(c)
    loss = 0.0
    for h in ("b", "c"):
        z = c["z" + h].clone().requires_grad_(True)
        lp = torch.log_softmax(torch.where(c["mask_" + h], z, torch.full_like(z, R.LOG0)) / temperature, -1)
        leaves[h], c64["l" + h] = z, lp.detach()
        loss = loss + (lp * c["g" + h + "_in"].double()).sum()          # d loss / d lp = g
    gb, gc = torch.autograd.grad(loss, [leaves["b"], leaves["c"]])
    m = c["m"]
    auto = torch.cat([gb.reshape(m, -1), gc.reshape(m, -1)], 1)
    ref = R.reference(c64)
    big = float(auto.abs().max())
    err = float((ref["dz"][:, :ref["cols"]] - auto).abs().max())
    print(f"closed form vs fp64 autograd [{shape}, T={temperature}]: max err {err:.3e} at largest magnitude {big:.3e}")
    assert err <= 1e-12 * max(big, 1.0)
    assert float(ref["dz"][:, ref["cols"]:].abs().max()) == 0.0
    if shape == "one":
        assert big == 0.0
    else:
        assert big > 0.1
        masked = ~torch.cat([c["mask_b"].reshape(m, -1), c["mask_c"].reshape(m, -1)], 1)
        assert int(masked.sum()) > 0 and float(auto[masked].abs().max()) == 0.0


@pytest.mark.parametrize("temperature", [1.0, 2.0])
@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_bound_is_met_by_the_reference_and_the_restatement_and_by_no_mutant(shape, temperature):
    c = R.make_case(*R.SHAPES[shape], temperature=temperature)
    ref = R.reference(c)
    r32 = R.ratio(R.restate_f32(c), ref, None)
    print(f"fp32 restatement [{shape}, T={temperature}] before rounding: max err / bound {r32:.3f}")
    assert r32 <= 1.0
    for fmt, dt in DT.items():
        r_ref, r_re = R.ratio(ref["dz"].to(dt), ref, fmt), R.ratio(R.restate_f32(c).to(dt), ref, fmt)
        print(f"    {fmt}: the reference rounded {r_ref:.3f}, the restatement rounded {r_re:.3f}")
        assert r_ref <= 1.0 and r_re <= 1.0
        for mut in R.MUTATIONS:
            bad = R.reference(c, mutate=mut)
            if not R.mutant_differs(mut, c):
                assert torch.equal(bad["dz"], ref["dz"]), mut
                continue
            assert not torch.equal(bad["dz"], ref["dz"]), mut
            rb = R.ratio(ref["dz"].to(dt), bad, fmt)
            print(f"    {fmt}: mutated reference {mut}: err / bound {rb:.1f}")
            assert not rb <= 1.0, (mut, rb)


@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s != "one"])
def test_scale_256_outputs_are_normal_numbers(shape):
    """grad_scale 256 against 4096: rounding commutes with the factor 16 on every element that is a normal number at 256 and finite at 4096."""
    c = R.make_case(*R.SHAPES[shape], temperature=2.0, masks=False)
    lo, hi = R.reference(c, grad_scale=256.0), R.reference(c, grad_scale=4096.0)
    x = lo["dz"][:, :lo["cols"]].abs()
    assert float(hi["dz"].abs().max()) < 0.5 * 65504.0
    for fmt in DT:
        share = float((x >= MIN_NORMAL[fmt]).double().mean())
        print(f"[{shape}] {fmt}: {100 * share:.2f} % of the elements are normal at scale 256")
        assert share >= 0.99


def test_signature_table_and_library_have_the_entry():
    import __graft_entry__ as ge
    ge.build()
    import vpt_amd  # noqa: F401
    from vpt_amd import _native
    assert list(_native.load("bf16").vpt_grouped_logprob_backward.argtypes) == [ctypes.c_void_p] * 7 + [ctypes.c_int] * 6 + [ctypes.c_float] * 2 + [ctypes.c_void_p]
    hdr = open(os.path.join(ROOT, "include", "vpt_hip.h")).read()
    assert "int vpt_grouped_logprob_backward(" in hdr
    for fmt in ("bf16", "fp16"):
        assert hasattr(_native.load(fmt), "vpt_grouped_logprob_backward")
