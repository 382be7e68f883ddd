"""tests/rl_loss_ref.py on the CPU: the fp64 closed form IS the gradient of the plainly written fine-tuning loss (fp64 torch autograd, 1e-9 of the
largest magnitude), and a float32 restatement in vpt_rl_loss_kernel's order of operations stays inside the bounds the GPU test holds the kernel to."""
import pytest
import torch

from tests import rl_loss_ref as R

COEF = dict(kl_coef=0.3, entropy_coef=0.02, value_coef=0.5)


def _kinds(c, clipped):
    live, a = c["w"] != 0, c["adv"]
    return [bool((live & clipped & (a > 0)).any()), bool((live & clipped & (a < 0)).any()), bool((live & ~clipped & (a > 0)).any()),
            bool((live & ~clipped & (a < 0)).any())]


def test_inputs_hold_rows_of_every_kind_away_from_the_clip_boundary():
    c = R.make_case(10, 70, 11)
    clipped, rho, dist = R.exact_clip_flags(c)
    assert float(dist.min()) > 1e-3, dist
    assert all(_kinds(c, clipped)), _kinds(c, clipped)
    assert int((c["w"] == 0).sum()) == 2 and bool(torch.isnan(c["lb"][c["w"] == 0]).all())           # w = 0 rows of NaN log-probs
    assert bool(torch.isinf(c["lb"][2]).any()) and bool(torch.isinf(c["lc"][2]).any())                # a head with p_j = 0
    assert float(c["w"][2]) != 0


@pytest.mark.parametrize("coef", [COEF, dict(kl_coef=0.0, entropy_coef=0.0, value_coef=0.0), dict(kl_coef=1.0, entropy_coef=0.0, value_coef=0.0)])
def test_closed_form_is_the_gradient_of_the_plain_loss(coef):
    """fp64 autograd through log_softmax(z / T) of the loss written with torch.min / clamp / a squared error, row by row over the classes of
    non-zero probability (a class with logit -inf is not part of the graph: its gradient is 0, as the closed form says)."""
    c = R.make_case(10, 70, 11)
    T, m, nb, nc = c["temperature"], c["m"], c["nb"], c["nc"]
    c64 = dict(c)
    c64["lb"], c64["lc"] = torch.log_softmax(c["zb"] / T, -1), torch.log_softmax(c["zc"] / T, -1)
    c64["qb"], c64["qc"] = torch.log_softmax(c["yb"] / T, -1), torch.log_softmax(c["yc"] / T, -1)
    lp = c64["lb"].gather(1, c["ab"][:, None])[:, 0] + c64["lc"].gather(1, c["ac"][:, None])[:, 0]
    rho_t = torch.exp(c["lb"].double().gather(1, c["ab"][:, None])[:, 0] + c["lc"].double().gather(1, c["ac"][:, None])[:, 0] - c["old"].double())
    c64["old"] = lp - torch.log(rho_t)                         # the same ratios as the fp32 case, now exactly consistent with the fp64 log-probs
    live = c["w"] != 0
    for k in ("lb", "lc", "qb", "qc"):
        c64[k][~live] = float("nan")
    clipped, rho, dist = R.exact_clip_flags(c64)
    assert float(dist.min()) > 1e-3 and all(_kinds(c64, clipped))
    ref = R.reference(c64, clipped, **coef)
    that = (c["target"].double() - float(c["vnorm"][0])) / float(c["vnorm"][1])
    w = c["w"].double()
    zb, zc = c["zb"].clone().requires_grad_(True), c["zc"].clone().requires_grad_(True)
    v = c["value"].double().clone().requires_grad_(True)
    total = 0.0
    for r in range(m):
        if not live[r]:
            continue
        ib, ic = c["avail_b"][r].nonzero()[:, 0], c["avail_c"][r].nonzero()[:, 0]
        lb, lc = torch.log_softmax(zb[r, ib] / T, -1)[None], torch.log_softmax(zc[r, ic] / T, -1)[None]
        ab, ac = (ib == c["ab"][r]).nonzero()[0], (ic == c["ac"][r]).nonzero()[0]
        total = total + w[r] * R.torch_loss(lb, lc, c64["qb"][r, ib][None], c64["qc"][r, ic][None], ab, ac, c64["old"][r:r + 1],
                                            c["adv"].double()[r:r + 1], v[r:r + 1], that[r:r + 1], torch.ones(1, dtype=torch.float64), clip=c["clip"], **coef)
    loss = total / w.sum()
    gb, gc, gv = torch.autograd.grad(loss, [zb, zc, v])
    auto = torch.cat([gb, gc, gv[:, None]], 1)
    big = float(auto.abs().max())
    err = float((ref["dz"] - auto).abs().max())
    print(f"closed form vs fp64 autograd: max err {err:.3e} at largest magnitude {big:.3e}")
    assert err <= 1e-9 * big
    assert float(ref["dz"][~live].abs().max()) == 0.0
    t = ref["totals"]
    loss_ref = (t[0] + coef["kl_coef"] * (t[1] + t[2]) - coef["entropy_coef"] * (t[3] + t[4]) + coef["value_coef"] * t[5]) / t[10]
    assert abs(float(loss_ref) - float(loss.detach())) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    if coef["value_coef"] == 0:
        assert float(ref["dz"][:, nb + nc].abs().max()) == 0.0
    assert float(t[11]) == float(live.sum())


@pytest.mark.parametrize("m,nb,nc", [(10, 70, 11), (5, 8641, 121)])
def test_float32_restatement_in_the_kernels_order_meets_the_bounds(m, nb, nc):
    """numpy float32, the kernel's sweep / shuffle / LDS order, numpy's own float32 exp (its error measured over these inputs, doubled, as the GPU
    test does for the device's expf): every quantity inside its bound, before and after the 16-bit rounding; wrong references are far outside."""
    c = R.make_case(m, nb, nc)
    clipped, rho, dist = R.exact_clip_flags(c)
    assert float(dist.min()) > 1e-3
    live = c["w"] != 0
    args = torch.cat([c["lb"][live].reshape(-1), c["lc"][live].reshape(-1)])
    lp32 = (c["lb"].gather(1, c["ab"][:, None])[:, 0] + c["lc"].gather(1, c["ac"][:, None])[:, 0])
    args = torch.cat([args, (lp32 - c["old"])[live]])
    args = args[torch.isfinite(args)]
    e_exp = 2 * R.exp_rel_error_u(args.double(), torch.from_numpy(__import__("numpy").exp(args.numpy())))
    ref = R.reference(c, clipped, e_exp=e_exp, **COEF)
    dz, frame_out, totals = R.restate_f32(c, **COEF)
    assert torch.equal(frame_out[:, 7].bool() & live, clipped)                     # away from the boundary the fp32 flags are the exact ones
    e = (dz.double() - ref["dz"]).abs()
    fp32_ratio = float((e / ref["b_dz_abs"].clamp(min=1e-300))[ref["b_dz_abs"] > 0].max())
    assert float(e[ref["b_dz_abs"] == 0].max()) == 0.0
    print(f"fp32 restatement [{m}x{nb}+{nc}] (exp error bound {e_exp:.2f} u): dz before rounding err/bound {fp32_ratio:.3f}")
    assert fp32_ratio <= 1.0
    for fmt, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        rt = R.ratios(dz.to(dt), frame_out, totals, ref, fmt)
        print(f"fp32 restatement [{m}x{nb}+{nc}] {fmt}: max err / bound {rt}")
        assert all(v <= 1.0 for v in rt.values()), rt
        for mut in ("kl_swap", "no_K", "value_left"):
            bad = R.ratios(dz.to(dt), frame_out, totals, R.reference(c, clipped, e_exp=e_exp, mutate=mut, **COEF), fmt)
            print(f"    mutated reference {mut}: {bad}")
            assert bad["dz"] > 50.0, (mut, bad)
