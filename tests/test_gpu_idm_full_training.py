"""IDMTrainer(train_cnn=True): the inverse dynamics model trained through the whole network -- temporal conv, IMPALA CNN, trunk, heads -- on the GPU,
in both operand formats.  Needs an MI355X.

Gradients: every trainable tensor against fp64 autograd FROM THE PIXELS (tests/idm_full_ref.py: the oracle's conv3d_temporal and impala_cnn composed
with tests/idm_trainer_ref.forward) with the assertions and constants of tests/test_gpu_training.py::test_bc_gradients_vs_oracle.  The yardstick is the
rounding reference's own distance to fp64 (the same reference rounding where the kernels round), never the GPU's own output:
    per tensor  d_gpu < 1.5 d_em + 0.1,  norm ratio in (0.75, 1.3),  cosine > min(0.93, cos_em - 0.15);   over all tensors  mean_gpu < 1.15 mean_em + 0.02
and, because tests/test_idm_full_ref_cpu.py shows that the rounding reference alone meets it on this batch, parity.GRAD_BOUNDS[mode].
Tiny IDM, temperature 2, B = 2, T = 6, parity.structured_frames (idm_full_ref.batch).

Measured on an MI355X (this test's printout; rounding reference in brackets; 91 reached tensors):
    bf16: loss GPU 18.86283, fp64 18.87043 [18.86654]; mean rel-L2 0.3120 [0.3450], mean cosine 0.9411, worst cosine 0.7720;
          worst tensor net.conv3d_layer.layer.bias 0.711 [0.890]
    fp16: loss GPU 18.87151, fp64 18.87043 [18.87113]; mean rel-L2 0.0981 [0.0992], mean cosine 0.9937, worst cosine 0.9711;
          worst tensor net.conv3d_layer.layer.bias 0.244 [0.285]
    GRAD_BOUNDS: bf16 l2_mean 0.40, cos_mean 0.90, cos_min 0.40; fp16 0.15, 0.985, 0.90

The trainable set grows by the 56 tensors of `net.conv3d_layer.*` and `net.img_process.cnn.*` (2 + 3 stacks x 17 + 3 of the dense layer; stack 0's
firstconv carries norm.* and no bias).  Behaviour: reproducible bits, chunking, the step against train_cnn=False, the fp16 overflow skip, resume,
re-packing, and the default trainer unchanged."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd.idm_training import IDMTrainer  # noqa: E402
from vpt_amd.lib.policy import InverseActionPolicy  # noqa: E402
from vpt_amd.lib.types import idm_action_space  # noqa: E402
from tests import idm_full_ref as F  # noqa: E402
from tests import labeler_ref as R  # noqa: E402
from tests import parity as P  # noqa: E402

DEV = "cuda"
B, T = F.B, F.T
NEW = F.CNN_PREFIXES


def _l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm().clamp(min=1e-30))


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
    return tuple(x.to(DEV) for x in F.batch())


def _params(pol):
    return {n: p.detach().clone() for n, p in pol.named_parameters()}


def test_gradients_vs_fp64_autograd_from_the_pixels(idm, batch):
    pol, cfg, sd = idm
    pol.load_state_dict(sd, strict=False)
    mode = pol.precision
    tr = IDMTrainer(pol, optimizer_state=False, train_cnn=True)
    new = [n for n in tr.trainable if n.startswith(NEW)]
    assert new == [n for n, _ in pol.named_parameters() if n.startswith(NEW)]             # the policy's state-dict order
    assert set(new) == {k for k in sd if k.startswith(NEW)} and len(new) == 56, len(new)
    loss, grads = tr.loss_and_grads(*batch)
    torch.cuda.synchronize()
    torch.set_num_threads(max(1, min(32, len(__import__("os").sched_getaffinity(0)))))
    loss_ref, g_ref = F.reference(None)
    loss_em, g_em = F.reference(mode)
    print(f"PARITY[{mode}] IDM full loss: GPU {float(loss):.5f}, fp64 reference {loss_ref:.5f}, {mode}-rounding reference {loss_em:.5f}")
    assert abs(float(loss) - loss_ref) < 2e-2 and abs(float(loss) - loss_em) < 1e-2, (float(loss), loss_ref, loss_em)
    assert set(grads) == set(tr.trainable) == set(g_ref)
    for n in tr.trainable:
        if ".r_layer." in n:              # unreached under mask "none"
            assert float(g_ref[n].norm()) == 0.0 and float(grads[n].abs().max()) == 0.0, n
        else:
            assert float(grads[n].abs().max()) > 0.0 and bool(torch.isfinite(grads[n]).all()), n
    st, st_em = F.grad_stats(grads, g_ref), F.grad_stats(g_em, g_ref)
    for n in st["l2"]:
        d_gpu, d_em = st["l2"][n], st_em["l2"][n]
        assert d_gpu < 1.5 * d_em + 0.1, (n, d_gpu, d_em)
        assert st["cos"][n] > min(0.93, st_em["cos"][n] - 0.15), (n, st["cos"][n], st_em["cos"][n])
        assert 0.75 < st["ratio"][n] < 1.3, (n, st["ratio"][n])
    assert len(st["l2"]) == len(tr.trainable) - 4
    gb = P.GRAD_BOUNDS[mode]
    print(f"PARITY[{mode}] IDM full grads over {len(st['l2'])} tensors: mean rel-L2 to fp64 GPU {st['l2_mean']:.4f}, rounding reference {st_em['l2_mean']:.4f}; "
          f"mean cosine {st['cos_mean']:.5f}, worst cosine {st['cos_min']:.4f}; worst tensor GPU {st['worst']}, rounding reference {st_em['worst']}; GRAD_BOUNDS {gb}")
    print(f"PARITY[{mode}] IDM full grads vs the rounding reference: worst rel-L2", sorted(F.grad_stats(grads, g_em)["l2"].items(), key=lambda kv: -kv[1])[:4])
    assert st["l2_mean"] < 1.15 * st_em["l2_mean"] + 0.02, (st["l2_mean"], st_em["l2_mean"])
    if F.meets_table(st_em, gb):          # (tests/test_idm_full_ref_cpu.py: it does, in both formats)
        assert F.meets_table(st, gb), (st["l2_mean"], st["cos_mean"], st["cos_min"])


def test_gradients_are_reproducible_and_independent_of_the_chunking(idm, batch):
    """Two calls give the same bits; cnn_chunk = one window and = two windows agree to 1e-5 rel-L2 (the BC chunking test's bound: only the
    association of the fp32 sums over the chunks differs)."""
    pol, _, sd = idm
    pol.load_state_dict(sd, strict=False)
    tr = IDMTrainer(pol, optimizer_state=False, train_cnn=True)
    eng = pol._engine
    old = eng.cnn_chunk
    try:
        eng.cnn_chunk = 2 * T
        l1, g1 = tr.loss_and_grads(*batch)
        l2, g2 = tr.loss_and_grads(*batch)
        eng.cnn_chunk = T
        l3, g3 = tr.loss_and_grads(*batch)
        torch.cuda.synchronize()
    finally:
        eng.cnn_chunk = old
    assert torch.equal(l1, l2) and set(g1) == set(g2) == set(g3)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
        if float(g1[n].norm()) > 0:
            assert _l2(g3[n], g1[n]) < 1e-5, (n, _l2(g3[n], g1[n]))
    assert abs(float(l3) - float(l1)) < 1e-5


def test_default_trainer_is_unchanged_and_the_argument_is_checked(idm, batch, monkeypatch):
    pol, _, sd = idm
    pol.load_state_dict(sd, strict=False)
    l0, g0 = IDMTrainer(pol, optimizer_state=False).loss_and_grads(*batch)
    l1, g1 = IDMTrainer(pol, optimizer_state=False, train_cnn=False).loss_and_grads(*batch)
    torch.cuda.synchronize()
    assert torch.equal(l0, l1) and set(g0) == set(g1) and not any(n.startswith(NEW) for n in g0)
    assert all(torch.equal(g0[n], g1[n]) for n in g0)
    small, full = IDMTrainer(pol), IDMTrainer(pol, train_cnn=True)
    assert small.state_dict()["train_cnn"] is False and full.state_dict()["train_cnn"] is True
    with pytest.raises(KeyError):
        full.load_state_dict(small.state_dict())
    monkeypatch.setenv("VPT_BC_FUSED_POOL", "0")
    with pytest.raises(RuntimeError, match="pool-fused"):
        IDMTrainer(pol, optimizer_state=False, train_cnn=True)
    IDMTrainer(pol, optimizer_state=False)          # the default never needed it


def test_steps_reduce_the_loss_further_than_with_a_frozen_cnn(idm, batch):
    pol, _, sd = idm
    losses = {}
    try:
        for train_cnn in (False, True):
            pol.load_state_dict(sd, strict=False)
            pol._packed_key = None
            tr = IDMTrainer(pol, lr=2e-4, weight_decay=0.0, train_cnn=train_cnn)
            losses[train_cnn] = [tr.step(*batch) for _ in range(8)]
            assert tr.step_count == 8 and tr.skipped_steps == 0
        torch.cuda.synchronize()
    finally:
        pol.load_state_dict(sd, strict=False)
        pol._packed_key = None
    print(f"IDM losses on a fixed batch [{pol.precision}]: train_cnn=True", [round(l, 3) for l in losses[True]], "train_cnn=False", [round(l, 3) for l in losses[False]])
    assert all(b_ < a_ for a_, b_ in zip(losses[True], losses[True][1:])), losses[True]
    assert losses[True][0] - losses[True][-1] > losses[False][0] - losses[False][-1], (losses[True], losses[False])


def test_overflowing_fp16_step_is_skipped_on_the_device(batch):
    pol, _, _ = _policy("fp16")
    tr = IDMTrainer(pol, lr=1e-4, loss_scale=2.0 ** 24, train_cnn=True)
    before = _params(pol)
    tr.step(*batch)
    torch.cuda.synchronize()
    after = _params(pol)
    assert all(torch.equal(before[n], after[n]) for n in before)
    assert tr.skipped_steps == 1 and tr.step_count == 0 and tr.loss_scale == 2.0 ** 23
    assert all(float(m.abs().max()) == 0.0 for m in tr.m.values())


def test_checkpoint_resume(idm, batch):
    pol, _, sd = idm
    try:
        pol.load_state_dict(sd, strict=False)
        pol._packed_key = None
        tr = IDMTrainer(pol, lr=1e-4, weight_decay=0.01, train_cnn=True)
        tr.step(*batch)
        tr.step(*batch)
        straight = _params(pol)
        pol.load_state_dict(sd, strict=False)
        pol._packed_key = None
        tr1 = IDMTrainer(pol, lr=1e-4, weight_decay=0.01, train_cnn=True)
        tr1.step(*batch)
        ck = tr1.state_dict()
        assert ck["train_cnn"] is True and "net.conv3d_layer.layer.weight" in ck["exp_avg"]
        tr2 = IDMTrainer(pol, lr=9.0, weight_decay=9.0, train_cnn=True)          # hyper-parameters come from the checkpoint
        tr2.load_state_dict(ck)
        tr2.step(*batch)
        torch.cuda.synchronize()
        resumed = _params(pol)
        assert tr2.step_count == 2
        for n in straight:
            assert torch.equal(straight[n], resumed[n]), n
        assert not torch.equal(straight["net.conv3d_layer.layer.weight"].cpu(), sd["net.conv3d_layer.layer.weight"])
    finally:
        pol.load_state_dict(sd, strict=False)
        pol._packed_key = None


def test_policy_sees_the_new_weights(idm, batch):
    pol, _, sd = idm
    pol.load_state_dict(sd, strict=False)
    pol._packed_key = None
    img = batch[0]
    try:
        _, _, before = pol.predict({"img": img})
        IDMTrainer(pol, lr=1e-3, weight_decay=0.0, train_cnn=True).step(*batch)
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
        pol._packed_key = None
