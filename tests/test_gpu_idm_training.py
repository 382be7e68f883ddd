"""IDMTrainer (fine-tuning of the inverse-dynamics model behind its frozen CNN) on the GPU, in both operand formats: the saving forward equals the
inference forward bit for bit, every trainable tensor's gradient is held to the fp64 reference (tests/idm_trainer_ref.py) run from the GPU's own
CNN output with the assertions and constants of tests/test_gpu_training.py::test_bc_gradients_vs_oracle, and the step / loss-scaling / checkpoint /
repacking behaviour is BCTrainer's.  Tiny IDM, temperature 2, B = 2, T = 12.  Needs an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from vpt_amd.idm_training import IDMTrainer  # noqa: E402
from vpt_amd.lib.policy import InverseActionPolicy  # noqa: E402
from vpt_amd.lib.types import idm_action_space  # noqa: E402
from tests import idm_trainer_ref as IR  # noqa: E402
from tests import labeler_ref as R  # noqa: E402
from tests import parity as P  # noqa: E402

DEV = "cuda"
B, T = 2, 12
FROZEN = ("net.conv3d_layer.", "net.img_process.cnn.")


def _l2(a, ref):
    return float((a - ref).norm() / ref.norm().clamp(min=1e-30))


def _policy(precision):
    kw, cfg, sd = R.tiny_idm()
    pol = InverseActionPolicy(idm_action_space(), pi_head_kwargs=dict(temperature=R.TEMPERATURE), idm_net_kwargs=kw, precision=precision)
    missing, unexpected = pol.load_state_dict(sd, strict=False)
    assert not missing and not unexpected
    return pol.to(DEV), cfg, sd


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def idm(request):
    return _policy(request.param)


@pytest.fixture(scope="module")
def batch():
    g = torch.Generator().manual_seed(21)
    img = P.structured_frames(B, T, g)
    buttons = torch.randint(0, 2, (B, T, 20), generator=g)
    camera = torch.randint(0, 11, (B, T, 2), generator=g)
    return img, buttons, camera


def _gpu(batch):
    return tuple(x.to(DEV) for x in batch)


def _params(pol):
    return {n: p.detach().clone() for n, p in pol.named_parameters()}


def test_forward_saving_equals_the_inference_forward(idm, batch):
    pol, _, sd = idm
    pol.load_state_dict(sd, strict=False)
    img = batch[0].to(DEV)
    with torch.no_grad():
        (pd, _, _), _ = pol({"img": img}, None, None)
    S = IDMTrainer(pol, optimizer_state=False).forward_saving(img)
    torch.cuda.synchronize()
    assert torch.equal(S["lp_b"].view(B, T, 20, 2), pd["buttons"]) and torch.equal(S["lp_c"].view(B, T, 2, 11), pd["camera"])


def test_gradients_vs_the_fp64_reference(idm, batch):
    """test_bc_gradients_vs_oracle's assertions, constants included: per tensor d_gpu < 1.5 d_em + 0.1, cosine > min(0.93, cos_em - 0.15), norm ratio
    in (0.75, 1.3); mean_gpu < 1.15 mean_em + 0.02; the means within parity.GRAD_BOUNDS[mode].  d_* = rel-L2 to the unrounded fp64 reference,
    `em` = the same reference rounding at the kernels' points; both run from the GPU's own dense-layer output."""
    pol, cfg, sd = idm
    pol.load_state_dict(sd, strict=False)
    mode = pol.precision
    tr = IDMTrainer(pol, optimizer_state=False)
    img, buttons, camera = _gpu(batch)
    d = tr.forward_saving(img)["d"].cpu()
    loss, grads = tr.loss_and_grads(img, buttons, camera)
    torch.cuda.synchronize()
    torch.set_num_threads(max(1, min(32, len(__import__("os").sched_getaffinity(0)))))
    loss_ref, grads_ref = IR.loss_and_grads(sd, cfg, d, B, T, batch[1], batch[2])
    loss_em, grads_em = IR.loss_and_grads(sd, cfg, d, B, T, batch[1], batch[2], rnd=mode)
    print(f"PARITY[{mode}] IDM loss: GPU {float(loss):.5f}, fp64 reference {loss_ref:.5f}, {mode}-rounding reference {loss_em:.5f}")
    assert abs(float(loss) - loss_ref) < 2e-2 and abs(float(loss) - loss_em) < 1e-2, (float(loss), loss_ref, loss_em)
    assert set(grads) == set(tr.trainable) == set(grads_ref)
    worst, cos_ref, l2_em = {}, {}, {}
    for name in tr.trainable:
        ref, em = grads_ref[name], grads_em[name]
        mine = grads[name].cpu().double().reshape(ref.shape)
        if float(ref.norm()) == 0.0:          # r_layer: unreached under mask "none"
            assert float(mine.abs().max()) == 0.0, name
            continue
        d_gpu, d_em = _l2(mine, ref), _l2(em, ref)
        worst[name] = (d_gpu, d_em)
        l2_em[name] = _l2(mine, em)
        cos_ref[name] = float((mine * ref).sum() / (mine.norm() * ref.norm()))
        assert d_gpu < 1.5 * d_em + 0.1, (name, d_gpu, d_em)
        cos_em = float((em * ref).sum() / (em.norm() * ref.norm()))
        assert cos_ref[name] > min(0.93, cos_em - 0.15), (name, cos_ref[name], cos_em)
        ratio = float(mine.norm() / ref.norm())
        assert 0.75 < ratio < 1.3, (name, ratio)
    assert len(worst) >= 35
    print(f"PARITY[{mode}] IDM grads vs the {mode}-rounding reference: worst rel-L2", sorted(l2_em.items(), key=lambda kv: -kv[1])[:4])
    print(f"PARITY[{mode}] IDM grads: largest (GPU-vs-fp64, rounding-reference-vs-fp64) rel-L2", sorted(worst.items(), key=lambda kv: -kv[1][0])[:3])
    mean_gpu = sum(v[0] for v in worst.values()) / len(worst)
    mean_em = sum(v[1] for v in worst.values()) / len(worst)
    mean_cos = sum(cos_ref.values()) / len(cos_ref)
    print(f"PARITY[{mode}] IDM grads: mean rel-L2 to the fp64 reference over {len(worst)} tensors: GPU {mean_gpu:.4f}, {mode} rounding reference {mean_em:.4f}; "
          f"cosine to the fp64 reference: mean {mean_cos:.5f}, worst {min(cos_ref.values()):.4f}")
    assert mean_gpu < 1.15 * mean_em + 0.02, (mean_gpu, mean_em)
    GB = P.GRAD_BOUNDS[mode]
    assert mean_gpu < GB["l2_mean"] and mean_cos > GB["cos_mean"] and min(cos_ref.values()) > GB["cos_min_small"], (mean_gpu, mean_cos, min(cos_ref.values()))


def test_gradients_are_reproducible_and_frozen_tensors_stay_out(idm, batch):
    pol, _, sd = idm
    pol.load_state_dict(sd, strict=False)
    tr = IDMTrainer(pol, lr=1e-4, weight_decay=0.01)
    img, buttons, camera = _gpu(batch)
    w = torch.ones(B, T)
    w[1, 8:] = 0.0                              # a padded tail
    l1, g1 = tr.loss_and_grads(img, buttons, camera, frame_weight=w)
    l2, g2 = tr.loss_and_grads(img, buttons, camera, frame_weight=w)
    torch.cuda.synchronize()
    assert torch.equal(l1, l2) and set(g1) == set(g2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    assert not any(n.startswith(FROZEN) or n.startswith("net.lastlayer.") for n in g1)
    assert any(n.startswith(FROZEN) for n, _ in pol.named_parameters())
    before = _params(pol)
    try:
        tr.step(img, buttons, camera, frame_weight=w)
        torch.cuda.synchronize()
        after = _params(pol)
        for n in before:
            if n.startswith(FROZEN) or n.startswith("net.lastlayer.") or n.endswith("b_nd"):
                assert torch.equal(before[n], after[n]), n
        assert not torch.equal(before["net.final_ln.weight"], after["net.final_ln.weight"])
        assert not torch.equal(before["net.img_process.linear.layer.weight"], after["net.img_process.linear.layer.weight"])
    finally:
        pol.load_state_dict(sd, strict=False)


def test_weighted_loss_metrics_and_evaluate(idm, batch):
    """A zero-weight frame adds nothing whatever its labels hold (in range); evaluate() reports the loss the training forward reports."""
    pol, _, sd = idm
    pol.load_state_dict(sd, strict=False)
    tr = IDMTrainer(pol, optimizer_state=False)
    img, buttons, camera = _gpu(batch)
    w = torch.ones(B, T)
    w[0, :3] = 0.0
    metrics = {}
    loss, g = tr.loss_and_grads(img, buttons, camera, frame_weight=w, metrics=metrics)
    b2, c2 = buttons.clone(), camera.clone()
    b2[0, :3] = 1 - b2[0, :3]
    c2[0, :3] = 10 - c2[0, :3]
    loss2, g2 = tr.loss_and_grads(img, b2, c2, frame_weight=w)
    ev = tr.evaluate(img, buttons, camera, frame_weight=w)
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2) and all(torch.equal(g[n], g2[n]) for n in g)
    assert float(metrics["weight_sum"]) == float(w.sum()) and float(metrics["frames"]) == float((w > 0).sum())
    # (the returned loss is formed from the per-frame records, evaluate()'s from the fixed-order totals: the same terms in another association)
    assert abs(float(metrics["loss"]) - float(ev["loss"])) < 1e-4 and abs(float(loss) - float(ev["loss"])) < 1e-4
    assert 0.0 <= float(ev["acc_buttons"]) <= 1.0 and metrics["frame_nll"].shape == (B, T)


def test_steps_reduce_the_loss(idm, batch):
    """The criterion of test_bc_step_reduces_loss: eight steps on one fixed batch, monotonic within +0.05, at least 0.2 lower overall."""
    pol, _, sd = idm
    pol.load_state_dict(sd, strict=False)
    tr = IDMTrainer(pol, lr=2e-4, weight_decay=0.0)
    img, buttons, camera = _gpu(batch)
    losses = []
    try:
        for _ in range(8):
            losses.append(tr.step(img, buttons, camera))
        torch.cuda.synchronize()
    finally:
        pol.load_state_dict(sd, strict=False)
    print(f"IDM losses on a fixed batch [{pol.precision}]:", [round(l, 3) for l in losses])
    assert tr.step_count == 8 and tr.skipped_steps == 0
    assert losses[-1] < losses[0] - 0.2 and all(b_ < a_ + 0.05 for a_, b_ in zip(losses, losses[1:]))


def test_overflowing_fp16_step_is_skipped_on_the_device(batch):
    pol, _, _ = _policy("fp16")
    tr = IDMTrainer(pol, lr=1e-4, loss_scale=2.0 ** 24)
    img, buttons, camera = _gpu(batch)
    before = _params(pol)
    tr.step(img, buttons, camera)
    torch.cuda.synchronize()
    after = _params(pol)
    assert all(torch.equal(before[n], after[n]) for n in before)
    assert tr.skipped_steps == 1 and tr.step_count == 0 and tr.loss_scale == 2.0 ** 23
    assert all(float(m.abs().max()) == 0.0 for m in tr.m.values())


def test_checkpoint_resume(idm, batch):
    pol, _, sd = idm
    img, buttons, camera = _gpu(batch)
    try:
        pol.load_state_dict(sd, strict=False)
        tr = IDMTrainer(pol, lr=1e-4, weight_decay=0.01)
        tr.step(img, buttons, camera)
        tr.step(img, buttons, camera)
        straight = _params(pol)
        pol.load_state_dict(sd, strict=False)
        tr1 = IDMTrainer(pol, lr=1e-4, weight_decay=0.01)
        tr1.step(img, buttons, camera)
        ck = tr1.state_dict()
        assert {"step", "lr", "weight_decay", "betas", "eps", "loss_scale", "train_cnn", "exp_avg", "exp_avg_sq"} <= set(ck)
        tr2 = IDMTrainer(pol, lr=9.0, weight_decay=9.0)          # hyper-parameters come from the checkpoint
        tr2.load_state_dict(ck)
        tr2.step(img, buttons, camera)
        torch.cuda.synchronize()
        resumed = _params(pol)
        assert tr2.step_count == 2
        for n in straight:
            assert torch.equal(straight[n], resumed[n]), n
    finally:
        pol.load_state_dict(sd, strict=False)


def test_policy_sees_the_new_weights(idm, batch):
    pol, _, sd = idm
    pol.load_state_dict(sd, strict=False)
    img, buttons, camera = _gpu(batch)
    try:
        _, _, before = pol.predict({"img": img})
        IDMTrainer(pol, lr=1e-3, weight_decay=0.0).step(img, buttons, camera)
        _, _, after = pol.predict({"img": img})
        assert not torch.equal(before["pd"]["buttons"], after["pd"]["buttons"])
        kw, _, _ = R.tiny_idm()
        fresh = InverseActionPolicy(idm_action_space(), pi_head_kwargs=dict(temperature=R.TEMPERATURE), idm_net_kwargs=kw, precision=pol.precision)
        fresh.load_state_dict(pol.state_dict(), strict=False)
        ac_f, _, out_f = fresh.to(DEV).predict({"img": img})
        ac, _, _ = pol.predict({"img": img})
        torch.cuda.synchronize()
        for h in ("buttons", "camera"):
            assert torch.equal(after["pd"][h], out_f["pd"][h]) and torch.equal(ac[h], ac_f[h]), h
        assert torch.equal(after["log_prob"], out_f["log_prob"])
    finally:
        pol.load_state_dict(sd, strict=False)


def test_argument_checks(idm, batch):
    pol, _, sd = idm
    pol.load_state_dict(sd, strict=False)
    tr = IDMTrainer(pol, optimizer_state=False)
    img, buttons, camera = _gpu(batch)
    bad_b = buttons.clone()
    bad_b[1, 3, 7] = 2
    bad_c = camera.clone()
    bad_c[0, 0, 1] = 11
    neg = torch.ones(B, T)
    neg[0, 0] = -1.0
    for kwargs in (dict(buttons=bad_b, camera=camera), dict(buttons=buttons, camera=bad_c),
                   dict(buttons=buttons, camera=camera, frame_weight=neg), dict(buttons=buttons, camera=camera, frame_weight=torch.zeros(B, T))):
        with pytest.raises(ValueError):
            tr.loss_and_grads(img, **kwargs)
    with pytest.raises(RuntimeError):
        tr.step(img, buttons, camera)           # optimizer_state=False: gradients only
    with pytest.raises(NotImplementedError):
        tr.forward_saving(torch.zeros(1, 161, 128, 128, 3, dtype=torch.uint8, device=DEV))


def test_factored_labels_of_a_joint_chunk():
    g = torch.Generator().manual_seed(8)
    chunk = dict(act_buttons=torch.randint(0, 8641, (B, T), generator=g).to(DEV), act_camera=torch.randint(0, 121, (B, T), generator=g).to(DEV))
    b, c = IDMTrainer.factored_labels(chunk)
    torch.cuda.synchronize()
    assert b.shape == (B, T, 20) and c.shape == (B, T, 2) and b.dtype == torch.int64
    assert int(b.min()) >= 0 and int(b.max()) <= 1 and int(c.min()) >= 0 and int(c.max()) <= 10
    b_ref, c_ref = ops.action_to_factored(chunk["act_buttons"].reshape(-1), chunk["act_camera"].reshape(-1))
    assert torch.equal(b.view(-1, 20), b_ref) and torch.equal(c.view(-1, 2), c_ref)
