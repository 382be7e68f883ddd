"""The host twin of the gradient-norm kernels (tests/grad_norm_ref.py) against its fp64 reference, and its clip coefficient against torch's, on the CPU."""
import numpy as np
import pytest
import torch

from tests import grad_norm_ref as R

SIZES = [1, 3, 4, 1023, 1024, 1025, 4097, 262149]
SCALES = [1.0, 1.0 / 2560, 1.0 / 3, 7e-5]


def make_grads(seed):
    """The fixed sizes + one random size < 50 000, each tensor with its own magnitude in 1e-6 .. 1e3."""
    rng = np.random.default_rng(seed)
    sizes = SIZES + [int(rng.integers(1, 50000))]
    return [(rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3)).astype(np.float32) for n in sizes]


@pytest.mark.parametrize("scale", SCALES)
def test_twin_within_the_derived_bound_of_fp64(scale):
    worst = 0.0
    for seed in range(3):
        grads = make_grads(seed)
        ref = R.norm_f64(grads, scale)
        got = R.restate_f32(grads, scale)
        err = abs(float(got["norm"]) - ref) / ref
        worst = max(worst, err)
        for g, pt in zip(grads, got["per_tensor"]):
            r1 = R.norm_f64([g], scale)
            assert abs(float(pt) - r1) <= R.BOUND * r1
    print(f"scale {scale:g}: max err / bound = {worst / R.BOUND:.3f} ({worst / R.U:.2f} u of {R.BOUND_ULPS:g} u)")
    assert worst <= R.BOUND


def test_mutated_twins_land_far_outside_the_bound():
    """What the bound can see: each of the three mutations must miss by far more than the bound."""
    rng = np.random.default_rng(5)
    grads = [rng.standard_normal(n).astype(np.float32) for n in (3, 7, 1023, 1025, 4097)] + [rng.standard_normal(2).astype(np.float32) * 30]
    scale = 1.0 / 3
    ref = R.norm_f64(grads, scale)
    assert abs(float(R.restate_f32(grads, scale)["norm"]) - ref) <= R.BOUND * ref
    for mut in (dict(drop_tail=True), dict(use_scale=False), dict(cross_wave=False)):
        err = abs(float(R.restate_f32(grads, scale, **mut)["norm"]) - ref) / ref
        assert err > 1000 * R.BOUND, (mut, err)


def test_tail_padding_and_exact_values():
    g = [np.zeros(1023, np.float32), np.zeros(1025, np.float32)]
    g[1][-1] = 1e4
    out = R.restate_f32(g, 1.0, 5.0)
    assert float(out["norm"]) == 1e4 and len(out["partials"][1]) == 2 and out["partials"][1][1] == np.float32(1e8)
    assert float(out["per_tensor"][0]) == 0.0 and float(out["per_tensor"][1]) == 1e4
    many = [np.full(1, 2.0, np.float32)] * 300        # more than 256 tensors: stage two's strided pass
    assert float(R.restate_f32(many)["norm"]) == np.float32(np.sqrt(1200.0))


def test_coefficient_equals_torch_bit_for_bit():
    rng = np.random.default_rng(1)
    norms = np.concatenate([10.0 ** rng.uniform(-8, 8, 4000), rng.uniform(0, 20, 4000), [0.0, 5.0, 4.9999995, 5.0000005]]).astype(np.float32)
    for max_norm in (5.0, 1.0, 0.1, 1e-3, 37.5):
        ours = np.array([R.coef_f32(n, max_norm) for n in norms], dtype=np.float32)
        t = torch.from_numpy(norms)
        elementwise = torch.clamp(max_norm / (t + 1e-6), max=1.0).numpy()
        assert np.array_equal(ours, elementwise), max_norm
        for n in norms[:200]:                          # and on a 0-dim tensor, the shape clip_grad_norm_ works with
            assert torch.clamp(max_norm / (torch.tensor(n) + 1e-6), max=1.0).item() == float(R.coef_f32(n, max_norm))


def test_coefficient_against_clip_grad_norm_itself():
    rng = np.random.default_rng(2)
    grads = [rng.standard_normal(n).astype(np.float32) for n in (5, 1025, 300)]
    out = R.restate_f32(grads, 1.0, 2.0)
    ps = [torch.nn.Parameter(torch.zeros(g.shape)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = torch.from_numpy(g.copy())
    tn = torch.nn.utils.clip_grad_norm_(ps, 2.0)
    assert abs(float(tn) - float(out["norm"])) <= 2 * R.BOUND * float(out["norm"])
    assert float(out["coef"]) == float(R.coef_f32(out["norm"], 2.0)) < 1.0
    for p, g in zip(ps, grads):                         # torch scaled its gradients by its coefficient: ours agrees to the norms' distance
        np.testing.assert_allclose(p.grad.numpy(), g * out["coef"], rtol=4 * R.BOUND, atol=0)


def test_infinite_threshold_and_nonfinite_sum():
    rng = np.random.default_rng(3)
    grads = [rng.standard_normal(100).astype(np.float32)]
    assert float(R.restate_f32(grads, 1.0, float("inf"))["coef"]) == 1.0
    assert float(R.restate_f32(grads, 1.0, None)["coef"]) == 1.0
    for bad in (np.inf, np.nan):
        g = [grads[0].copy()]
        g[0][-1] = bad
        out = R.restate_f32(g, 1.0, 5.0)
        assert out["nonfinite"] and float(out["coef"]) == 0.0 and out["out"][2] == 1.0
    big = [np.full(8, 3e38, np.float32)]               # finite gradients whose squares overflow fp32
    out = R.restate_f32(big, 1.0, 5.0)
    assert out["nonfinite"] and float(out["coef"]) == 0.0
