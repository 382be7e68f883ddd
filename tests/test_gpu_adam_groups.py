"""ops.adam_step_groups_ (vpt_adam_step_groups: one Adam launch with an (lr, weight_decay) per tensor, optionally AdamW's decoupled decay) on the GPU.
Tensor sizes 1, 3, 1023, 1024, 1025, 4099: the 1024-element block edge and tails of 1..3 elements; two groups interleaved in table order; three
steps.  The references are ops.adam_step_multi_, which tests/test_gpu_optim_fp64.py holds to an fp64 reference with derived bounds (as it does this
entry point itself; tests/test_gpu_kernels.py runs the single-tensor ops.adam_step_ only), and torch.optim.AdamW.  Needs an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402

DEV = "cuda"
SIZES = (1, 3, 1023, 1024, 1025, 4099)
GROUP = (0, 1, 0, 1, 0, 1)                          # interleaved in table order
HYPER = ((0.000181, 0.039428), (0.0000181, 0.0))    # (lr, weight_decay) of group 0 (the BC script's, behavioural_cloning.py:38-40) and group 1
STEPS = 3
KW = dict(beta1=0.9, beta2=0.999, eps=1e-8)


def _state(seed=3):
    g = torch.Generator().manual_seed(seed)
    p = [torch.randn(n, generator=g).to(DEV) for n in SIZES]
    grads = [[(torch.randn(n, generator=g) * 0.1).to(DEV) for n in SIZES] for _ in range(STEPS)]
    return p, [torch.zeros(n, device=DEV) for n in SIZES], [torch.zeros(n, device=DEV) for n in SIZES], grads


def _equal(a, b):
    return [i for part_a, part_b in zip(a, b) for i, (x, y) in enumerate(zip(part_a, part_b)) if not torch.equal(x, y)]


@pytest.mark.parametrize("max_grad_norm", [None, 0.5], ids=["plain", "clip"])
def test_one_group_with_the_launch_wide_values_is_adam_step_multi(max_grad_norm):
    """(a) every tensor carrying adam_step_multi_'s launch-wide (lr, wd): p, m, v torch.equal after each of three steps; with max_grad_norm the
    reference is the _clip launch (0.1-scale gradients of 7175 elements times grad_scale 0.5 have a norm near 4: the coefficient is well below 1)."""
    lr, wd = HYPER[0]
    pa, ma, va, grads = _state()
    pb, mb, vb, _ = _state()
    for step in range(1, STEPS + 1):
        g = grads[step - 1]
        na, nb_ = torch.empty(4, device=DEV), torch.empty(4, device=DEV)
        ops.adam_step_multi_(pa, g, ma, va, step, lr=lr, weight_decay=wd, grad_scale=0.5, max_grad_norm=max_grad_norm, norm_out=na, **KW)
        ops.adam_step_groups_(pb, g, mb, vb, step, [lr] * len(SIZES), [wd] * len(SIZES), grad_scale=0.5, max_grad_norm=max_grad_norm, norm_out=nb_, **KW)
        torch.cuda.synchronize()
        assert not _equal((pa, ma, va), (pb, mb, vb)), (step, _equal((pa, ma, va), (pb, mb, vb)))
        if max_grad_norm is not None:
            assert torch.equal(na, nb_) and 0 < float(nb_[1]) < 1
    assert all(float(x.abs().max()) > 0 for x in mb)


def test_two_interleaved_groups_are_two_launches_one_per_group():
    """(b) the per-TENSOR read of the hyper-parameter array: two groups with different lr and wd, interleaved in table order, against two
    adam_step_multi_ launches, one over each group's tensors with that group's values.  The table's first blocks are 0, 1, 2, 3, 4, 6: tensor 4
    (1025 elements, group 0) owns blocks 4 and 5, so a kernel that indexed the array by BLOCK would update its second block -- one element -- with
    record 5, group 1's values, and fail here; tensors 0..3 own one block each and would pass by coincidence."""
    pa, ma, va, grads = _state()
    pb, mb, vb, _ = _state()
    lrs, wds = [HYPER[k][0] for k in GROUP], [HYPER[k][1] for k in GROUP]
    for step in range(1, STEPS + 1):
        g = grads[step - 1]
        for k in (0, 1):
            idx = [i for i, gk in enumerate(GROUP) if gk == k]
            pick = lambda xs: [xs[i] for i in idx]
            ops.adam_step_multi_(pick(pa), pick(g), pick(ma), pick(va), step, lr=HYPER[k][0], weight_decay=HYPER[k][1], **KW)
        ops.adam_step_groups_(pb, g, mb, vb, step, lrs, wds, **KW)
        torch.cuda.synchronize()
        assert not _equal((pa, ma, va), (pb, mb, vb)), (step, _equal((pa, ma, va), (pb, mb, vb)))
    # the two groups really were updated differently: the same launch with group 0's values everywhere moves group 1's tensors elsewhere
    pc, mc, vc, _ = _state()
    ops.adam_step_groups_(pc, grads[0], mc, vc, 1, [HYPER[0][0]] * len(SIZES), [HYPER[0][1]] * len(SIZES), **KW)
    pd, md, vd, _ = _state()
    ops.adam_step_groups_(pd, grads[0], md, vd, 1, lrs, wds, **KW)
    torch.cuda.synchronize()
    assert [i for i in range(len(SIZES)) if not torch.equal(pc[i], pd[i])] == [1, 3, 5]


def test_decoupled_decay_matches_torch_adamw():
    """(c) decoupled=True against torch.optim.AdamW on the inputs of tests/test_gpu_kernels.py::test_adam_step_matches_torch (n = 100003, three
    steps, the script's lr and decay), to that test's own bound of 2e-6 max-abs (a float32 numpy restatement of the decoupled update sits 1.2e-7
    from torch on the CPU for these inputs); the coupled result lies further from AdamW than the bound, so the flag is not a no-op."""
    g = torch.Generator().manual_seed(10)
    n = 100003
    p0 = torch.randn(n, generator=g)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=0.000181, weight_decay=0.039428)
    p, m, v = p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pc, mc, vc = p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step in range(1, 4):
        grad = torch.randn(n, generator=g) * 0.1
        ref.grad = grad.clone()
        opt.step()
        gd = grad.to(DEV)
        ops.adam_step_groups_([p], [gd], [m], [v], step, [0.000181], [0.039428], decoupled=True)
        ops.adam_step_groups_([pc], [gd], [mc], [vc], step, [0.000181], [0.039428], decoupled=False)
    torch.cuda.synchronize()
    err, coupled = float((p.cpu() - ref.detach()).abs().max()), float((pc.cpu() - ref.detach()).abs().max())
    print(f"decoupled vs torch.optim.AdamW: max abs {err:.3e} (bound 2e-6); coupled vs AdamW: {coupled:.3e}")
    assert err < 2e-6
    assert coupled > 2e-6


@pytest.mark.parametrize("decoupled", [False, True])
def test_a_raised_found_inf_leaves_every_tensor_untouched(decoupled):
    """(d) an inf planted in the last tensor's tail element: the overflow launch in front raises the flag, the Adam launch is a no-op on the device."""
    p, m, v, grads = _state()
    before = [[x.clone() for x in part] for part in (p, m, v)]
    g = [x.clone() for x in grads[0]]
    g[-1][-1] = float("inf")
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.adam_step_groups_(p, g, m, v, 1, [HYPER[k][0] for k in GROUP], [HYPER[k][1] for k in GROUP], decoupled=decoupled, found_inf=flag, **KW)
    torch.cuda.synchronize()
    assert int(flag) == 1 and not _equal((p, m, v), before)
    flag.fill_(7)            # (zeroed by the call, as adam_step_multi_'s) -- finite gradients: the step is taken
    ops.adam_step_groups_(p, grads[0], m, v, 1, [HYPER[k][0] for k in GROUP], [HYPER[k][1] for k in GROUP], decoupled=decoupled, found_inf=flag, **KW)
    torch.cuda.synchronize()
    assert int(flag) == 0 and len(_equal((p, m, v), before)) == 3 * len(SIZES)


def test_mismatched_lengths_and_other_dtypes_are_refused():
    """(e) ValueError before anything is launched."""
    p, m, v, grads = _state()
    before = [x.clone() for x in p]
    lrs, wds = [1e-3] * len(SIZES), [0.0] * len(SIZES)
    with pytest.raises(ValueError, match="one entry per tensor"):
        ops.adam_step_groups_(p, grads[0], m, v, 1, lrs[:-1], wds)
    with pytest.raises(ValueError, match="one entry per tensor"):
        ops.adam_step_groups_(p, grads[0][:-1], m, v, 1, lrs, wds)
    with pytest.raises(ValueError, match="one entry per tensor"):
        ops.adam_step_groups_(p, grads[0], m, v, 1, lrs, wds + [0.0])
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.adam_step_groups_(p, [x.to(torch.bfloat16) for x in grads[0]], m, v, 1, lrs, wds)
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.adam_step_groups_([x.double() for x in p], grads[0], m, v, 1, lrs, wds)
    with pytest.raises(ValueError, match="elements"):
        ops.adam_step_groups_(p, grads[0], m[:-1] + [torch.zeros(5, device=DEV)], v, 1, lrs, wds)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(p, before))
