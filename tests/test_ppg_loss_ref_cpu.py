"""tests/ppg_loss_ref.py on the CPU: the fp64 closed form IS the gradient of the plainly written auxiliary loss for a teacher of mass 1 (fp64 torch
autograd through log_softmax(z / T), 1e-12), it differs from autograd by exactly (S - 1) p for a teacher of another mass (the documented p - o
convention), and a float32 restatement in vpt_ppg_aux_loss_kernel's order of operations stays inside the bounds the GPU test holds the kernel to."""
import numpy as np
import pytest
import torch

from tests import ppg_loss_ref as R

COEF = dict(clone_coef=0.7, value_coef=0.5)
SHAPES = [(10, 70, 11), (5, 8641, 121), (1, 1, 1)]


def _case64(mass=1.0):
    """The (10, 70 + 11) case with fp64 log-probs: the policy's are log_softmax(z / T) exactly as autograd will compute them, the teacher's are
    normalised in fp64 (S = 1 to rounding) and then shifted by log(mass)."""
    c = R.make_case(10, 70, 11, nan_rows=False, zero_prob=False)
    T = c["temperature"]
    c64 = dict(c)
    c64["lb"], c64["lc"] = torch.log_softmax(c["zb"] / T, -1), torch.log_softmax(c["zc"] / T, -1)
    c64["mb"], c64["mc"] = torch.log_softmax(c["yb"], -1) + np.log(mass), torch.log_softmax(c["yc"], -1) + np.log(mass)
    return c64


def _autograd(c64, coef):
    T, nb, nc = c64["temperature"], c64["nb"], c64["nc"]
    zb, zc = c64["zb"].clone().requires_grad_(True), c64["zc"].clone().requires_grad_(True)
    v = c64["value"].double().clone().requires_grad_(True)
    that = (c64["target"].double() - float(c64["vnorm"][0])) / float(c64["vnorm"][1])
    loss = R.torch_loss(torch.log_softmax(zb / T, -1), torch.log_softmax(zc / T, -1), c64["mb"], c64["mc"], v, that, c64["w"].double(), **coef)
    gb, gc, gv = torch.autograd.grad(loss, [zb, zc, v])
    return loss.detach(), torch.cat([gb, gc, gv[:, None]], 1)


@pytest.mark.parametrize("coef", [COEF, dict(clone_coef=1.0, value_coef=0.0), dict(clone_coef=0.0, value_coef=0.5)])
def test_closed_form_is_the_gradient_for_a_teacher_of_mass_one(coef):
    c64 = _case64()
    ref = R.reference(c64, **coef)
    loss, auto = _autograd(c64, coef)
    live = c64["w"] != 0
    big, err = float(auto.abs().max()), float((ref["dz"] - auto).abs().max())
    print(f"closed form vs fp64 autograd: max err {err:.3e} at largest magnitude {big:.3e}; teacher mass - 1: {float((ref['frame_out'][:, 3:5] - 1).abs().max()):.2e}")
    assert big > 0 and err <= 1e-12 * big
    assert float(ref["dz"][~live].abs().max()) == 0.0 and int((~live).sum()) == 2
    loss_ref = R.loss_of(ref["totals"], **coef)
    assert abs(float(loss_ref) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss)))
    assert float(ref["totals"][6]) == float(live.sum())
    nb, nc = c64["nb"], c64["nc"]
    if coef["value_coef"] == 0:
        assert float(ref["dz"][:, nb + nc].abs().max()) == 0.0
    if coef["clone_coef"] == 0:
        assert float(ref["dz"][:, :nb + nc].abs().max()) == 0.0
    else:
        assert float(ref["frame_out"][live][:, :2].min()) > 0.05           # D is of order 1, not of order rounding


def test_a_teacher_of_mass_0_9_differs_from_autograd_by_exactly_the_documented_term():
    """dz holds p - o; the exact gradient is p S - o.  With S = 0.9 the closed form and autograd differ by (S - 1) p (times clone_coef and the row's
    scale / T), and by nothing else."""
    c64 = _case64(mass=0.9)
    ref = R.reference(c64, **COEF)
    _, auto = _autograd(c64, COEF)
    nb, nc, T = c64["nb"], c64["nc"], c64["temperature"]
    rst = (c64["scale"] * c64["w"].double() / T)[:, None]
    S = ref["frame_out"][:, 3:5]
    assert float((S - 0.9).abs().max()) < 1e-14
    term = torch.cat([rst * COEF["clone_coef"] * (S[:, 0:1] - 1) * c64["lb"].exp(), rst * COEF["clone_coef"] * (S[:, 1:2] - 1) * c64["lc"].exp()], 1)
    diff = auto[:, :nb + nc] - ref["dz"][:, :nb + nc]
    big = float(auto.abs().max())
    assert float(term.abs().max()) > 1e-4 * big                             # the term is there ...
    assert float((diff - term).abs().max()) <= 1e-12 * big                  # ... and it is the whole difference
    assert float((auto[:, nb + nc] - ref["dz"][:, nb + nc]).abs().max()) <= 1e-12 * big


def test_inputs_hold_rows_of_every_kind():
    c = R.make_case(10, 70, 11)
    dead = c["w"] == 0
    assert int(dead.sum()) == 2 and bool(torch.isnan(c["lb"][dead]).all()) and bool(torch.isnan(c["mb"][dead]).all()) and bool(torch.isnan(c["value"][dead]).all())
    assert float(c["w"][2]) != 0
    for l, t in ((c["lb"][2], c["mb"][2]), (c["lc"][2], c["mc"][2])):
        assert bool((torch.isinf(t) & torch.isfinite(l)).any()) and bool((torch.isinf(t) & torch.isinf(l)).any())
        assert not bool((torch.isfinite(t) & torch.isinf(l)).any())          # never o > 0 where l = -inf: that is D = +inf (documented, not tested)
    one = R.make_case(1, 1, 1)
    assert float(one["w"][0]) == 1.0 and float(one["lb"][0, 0]) == 0.0 and float(one["mc"][0, 0]) == 0.0


@pytest.mark.parametrize("temperature", [1.0, 2.0])
@pytest.mark.parametrize("m,nb,nc", SHAPES)
def test_float32_restatement_in_the_kernels_order_meets_the_bounds(m, nb, nc, temperature):
    """numpy float32, the kernel's sweep / shuffle / LDS order, numpy's own float32 exp (its error measured over these inputs, doubled, as the GPU
    test does for the device's expf): every quantity inside its bound, before and after the 16-bit rounding.  A mutated reference either is the
    same reference (a one-class head has p = o = 1: no policy gradient either way; at T = 1 there is no 1 / T to leave out) or is outside."""
    c = R.make_case(m, nb, nc, temperature=temperature)
    args = R.exp_arguments(c)
    e_exp = 2 * R.exp_rel_error_u(args.double(), torch.from_numpy(np.exp(args.numpy())))
    ref = R.reference(c, e_exp=e_exp, **COEF)
    dz, frame_out, totals = R.restate_f32(c, **COEF)
    rt32 = R.ratios(dz, frame_out, totals, ref, None)
    print(f"fp32 restatement [{m}x{nb}+{nc}, T={temperature}] (exp error bound {e_exp:.2f} u): before rounding {rt32}")
    assert all(v <= 1.0 for v in rt32.values()), rt32
    for fmt, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        rt = R.ratios(dz.to(dt), frame_out, totals, ref, fmt)
        print(f"fp32 restatement [{m}x{nb}+{nc}, T={temperature}] {fmt}: max err / bound {rt}")
        assert all(v <= 1.0 for v in rt.values()), rt
        live_muts = []
        for mut in R.MUTATIONS:
            bad_ref = R.reference(c, e_exp=e_exp, mutate=mut, **COEF)
            if torch.equal(bad_ref["dz"], ref["dz"]):
                continue
            live_muts.append(mut)
            bad = R.ratios(dz.to(dt), frame_out, totals, bad_ref, fmt)
            print(f"    mutated reference {mut}: {bad}")
            assert not bad["dz"] <= 1.0, (mut, bad)
        want = ["value_left"] if nb == 1 else [mu for mu in R.MUTATIONS if mu != "no_temp" or temperature != 1.0]
        assert live_muts == want, live_muts
