"""micro_batches=K of BCTrainer / PPOTrainer / IDMTrainer on the GPU, both operand formats: the default keyword changes nothing, a K = 2 step is
the hand-run sequence (loss_and_grads per row group under the window's frame count -> their sum in torch, in order -> the unchanged Adam launch) bit
for bit, the accumulated gradients agree with the whole batch's to the bound tests/test_gpu_distributed.py holds the two-shard sum to, a non-finite
window is ONE skipped step, the records and the state are the row-wise concatenations, and the data-parallel path reports the local path's bits.
1x policy (temperature 2) and the tiny IDM of tests/test_gpu_idm_training.py, T = 4, B = 3 or 4.  Needs an MI355X."""
import copy
import os
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from vpt_amd.idm_training import IDMTrainer  # noqa: E402
from vpt_amd.rl_training import PPOTrainer  # noqa: E402
from vpt_amd.training import BCTrainer  # noqa: E402
from vpt_amd.lib.policy import InverseActionPolicy, MinecraftAgentPolicy  # noqa: E402
from vpt_amd.lib.types import idm_action_space, minecraft_action_space  # noqa: E402
from oracle import vpt_oracle as O  # noqa: E402
from tests import labeler_ref as LR  # noqa: E402
from tests import parity as P  # noqa: E402

DEV = "cuda"
NB, NC = 8641, 121
T = 4
INF = float("inf")
ROWS = {(4, 2): [(0, 2), (2, 4)], (3, 2): [(0, 2), (2, 3)]}          # distributed.shard_range's cut, written out


def _policy(precision):
    pk = O.policy_kwargs_for("1x")
    cfg = O.config_from_policy_kwargs(pk, dict(temperature=2.0))
    sd = O.synthetic_state_dict(cfg, seed=0)
    pol = MinecraftAgentPolicy(minecraft_action_space(), pk, dict(temperature=2.0), precision=precision)
    pol.load_state_dict(sd, strict=False)
    return pol.to(DEV)


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def trainer_1x(request):
    pol = _policy(request.param)
    return pol, copy.deepcopy(pol.state_dict())


_BATCH = {}


def _batch(pol, b):
    """-> (img, first, state_in, act_buttons, act_camera) for b sequences; state_in is the state a previous chunk left (memories and masks that are
    not zero), one sequence starts an episode.  Made once per (format, b) and never written."""
    key = (pol.precision, b)
    if key not in _BATCH:
        g = torch.Generator().manual_seed(29 + b)
        img = torch.randint(0, 256, (b, T, 128, 128, 3), generator=g, dtype=torch.uint8).to(DEV)
        prev = torch.randint(0, 256, (b, T, 128, 128, 3), generator=g, dtype=torch.uint8).to(DEV)
        first = torch.zeros(b, T, dtype=torch.bool, device=DEV)
        ab, ac = torch.randint(0, NB, (b, T), generator=g).to(DEV), torch.randint(0, NC, (b, T), generator=g).to(DEV)
        _, state = BCTrainer(pol, optimizer_state=False).evaluate(prev, first, pol.initial_state(b), ab, ac)
        first = first.clone()
        first[1, 0] = True
        _BATCH[key] = (img, first, state, ab, ac)
    return _BATCH[key]


def _weights(b, kind):
    if kind is None:
        return None
    g = torch.Generator().manual_seed(7 + b)
    w = torch.rand(b, T, generator=g) + 0.25
    w[0, 1] = 0.0
    if kind == "zero_group":          # the last row group carries no weight at all
        w[ROWS[(b, 2)][1][0]:] = 0.0
    return w.to(DEV)


def _count(b, fw):
    return b * T if fw is None else float(fw.to(torch.float32).to(torch.float64).sum())


def _rows(tree, lo, hi):
    if tree is None:
        return None
    if isinstance(tree, torch.Tensor):
        return tree[lo:hi]
    return type(tree)(_rows(x, lo, hi) for x in tree)


def _leaves(tree):
    if tree is None:
        return []
    if isinstance(tree, torch.Tensor):
        return [tree]
    return [leaf for x in tree for leaf in _leaves(x)]


def _snapshot(pol, tr):
    return ({k: v.detach().clone() for k, v in pol.named_parameters()}, {k: v.clone() for k, v in tr.m.items()}, {k: v.clone() for k, v in tr.v.items()},
            {k: v.detach().clone() for k, v in pol.named_buffers()})


def _same(a, b):
    return [k for part_a, part_b in zip(a, b) for k in part_a if not torch.equal(part_a[k], part_b[k])]


def _sum64(totals):
    acc = totals[0].double()
    for t_ in totals[1:]:
        acc = acc + t_.double()
    return acc.float()


def _hand_adam(tr, grads, grad_scale, max_norm=None):
    """The unchanged ops.adam_step_multi_ on the summed gradients; with max_norm the hand-run clip of tests/test_gpu_grad_clip_training.py: ops.grad_norm ->
    (g * grad_scale) * coef in torch -> the unclipped launch with grad_scale = 1.  -> norm_out | None."""
    names = [n for n in tr.trainable if n in grads]
    flat = [grads[n].contiguous().view(-1) for n in names]
    norm_out = None
    if max_norm is not None:
        norm_out = ops.grad_norm(flat, scale=grad_scale, max_norm=max_norm)
        gs = torch.tensor(grad_scale, dtype=torch.float32, device=DEV)
        flat, grad_scale = [(g * gs) * norm_out[1] for g in flat], 1.0
    ops.adam_step_multi_([tr.params[n].data.view(-1) for n in names], flat, [tr.m[n].view(-1) for n in names], [tr.v[n].view(-1) for n in names],
                         tr.step_count + 1, lr=tr.lr, beta1=tr.betas[0], beta2=tr.betas[1], eps=tr.eps, weight_decay=tr.wd, grad_scale=grad_scale)
    return norm_out


def _torch_sum(parts):
    """The gradient dicts summed in torch, in order."""
    acc = {n: g.clone() for n, g in parts[0].items()}
    for p_ in parts[1:]:
        acc = {n: acc[n] + p_[n] for n in acc}
    return acc


# ---- (f) ------------------------------------------------------------------------------------------------------------------------------------
def test_default_keyword_changes_nothing(trainer_1x):
    """(f) two steps with micro_batches=1 == two steps without the keyword: parameters, both moments, the loss -- with and without metrics."""
    pol, sd = trainer_1x
    batch = _batch(pol, 4)
    runs = []
    try:
        for kw in ({}, dict(micro_batches=1)):
            pol.load_state_dict(sd)
            tr = BCTrainer(pol)
            losses = [tr.step(*batch, **kw)[0], tr.step(*batch, metrics={}, **kw)[0]]
            runs.append((losses, _snapshot(pol, tr)))
    finally:
        pol.load_state_dict(sd)
    assert runs[0][0] == runs[1][0] and not _same(runs[0][1], runs[1][1])


# ---- (g), (k) -------------------------------------------------------------------------------------------------------------------------------
def _bc_hand_window(pol, tr, batch, fw, rows, count):
    img, first, state, ab, ac = batch
    grads, totals, states, mets = [], [], [], []
    for lo, hi in rows:
        met = {}
        _, g, s_out = tr.loss_and_grads(img[lo:hi], first[lo:hi], _rows(state, lo, hi), ab[lo:hi], ac[lo:hi], global_frames=count, unscaled=False,
                                        frame_weight=None if fw is None else fw[lo:hi], metrics=met)
        grads.append({n: g[n].clone() for n in tr.trainable if n in g})
        totals.append(tr._bc_totals.clone())
        states.append(s_out)
        mets.append(met)
    return _torch_sum(grads), _sum64(totals), states, mets, grads


@pytest.mark.parametrize("b,weights", [(4, None), (4, "some"), (4, "zero_group"), (3, None), (3, "some")])
def test_bc_step_is_the_hand_run_sequence(trainer_1x, b, weights):
    """(g) one step(micro_batches=2) == loss_and_grads per row group (global_frames = the window's count, unscaled=False, metrics={}) -> the sum in
    torch, in order -> the unchanged Adam launch with grad_scale = grad_unscale(count): parameters, moments, state_out, the loss and the totals'
    metrics bit for bit; again with max_grad_norm at half the measured norm (grad_norm and clip_coef included).  (k) frame_nll / frame_out are
    [B, T, .] and row for row the micro-batches' own records."""
    pol, sd = trainer_1x
    batch, fw, rows = _batch(pol, b), _weights(b, weights), ROWS[(b, 2)]
    count = _count(b, fw)
    try:
        tr_h = BCTrainer(pol)
        g_sum, t_sum, states, mets, parts = _bc_hand_window(pol, tr_h, batch, fw, rows, count)
        _hand_adam(tr_h, g_sum, tr_h.grad_unscale(count))
        hand = _snapshot(pol, tr_h)

        pol.load_state_dict(sd)
        tr = BCTrainer(pol, max_grad_norm=INF)
        met = {}
        loss, state_out = tr.step(*batch, frame_weight=fw, metrics=met, micro_batches=2)
        stepped = _snapshot(pol, tr)
        half = float(met["grad_norm"]) / 2

        pol.load_state_dict(sd)
        tr_hc = BCTrainer(pol)
        g_sum_c, _, _, _, _ = _bc_hand_window(pol, tr_hc, batch, fw, rows, count)
        norm_h = _hand_adam(tr_hc, g_sum_c, tr_hc.grad_unscale(count), half)
        hand_c = _snapshot(pol, tr_hc)

        pol.load_state_dict(sd)
        tr_c = BCTrainer(pol, max_grad_norm=half)
        met_c = {}
        loss_c, _ = tr_c.step(*batch, frame_weight=fw, metrics=met_c, micro_batches=2)
        stepped_c = _snapshot(pol, tr_c)
        torch.cuda.synchronize()
    finally:
        pol.load_state_dict(sd)
    assert not _same(stepped, hand), _same(stepped, hand)[:4]
    assert tr.step_count == 1 and tr.skipped_steps == 0
    want_loss = (t_sum[0] + t_sum[1]) / t_sum[6]
    assert loss == float(want_loss) == loss_c and torch.equal(met["loss"], want_loss)
    for i, key in enumerate(("nll_buttons", "nll_camera", "entropy_buttons", "entropy_camera", "acc_buttons", "acc_camera")):
        assert torch.equal(met[key], t_sum[i] / t_sum[6]), key
    assert torch.equal(met["weight_sum"], t_sum[6]) and torch.equal(met["frames"], t_sum[7])
    assert float(met["weight_sum"]) == pytest.approx(count, rel=1e-6)
    want_state = [torch.cat(parts, 0) for parts in zip(*[_leaves(s) for s in states])]
    got_state = _leaves(state_out)
    assert len(got_state) == len(want_state) >= 8 and all(torch.equal(a, c) for a, c in zip(got_state, want_state))
    assert got_state[0].shape[0] == b
    # (k)
    assert met["frame_nll"].shape == (b, T) and met["frame_out"].shape == (b, T, 8)
    for (lo, hi), mk in zip(rows, mets):
        assert torch.equal(met["frame_out"][lo:hi], mk["frame_out"]) and torch.equal(met["frame_nll"][lo:hi], mk["frame_nll"])
    # the clipped window
    assert not _same(stepped_c, hand_c), _same(stepped_c, hand_c)[:4]
    assert _same(stepped_c, stepped)
    assert torch.equal(met_c["grad_norm"], norm_h[0]) and torch.equal(met_c["clip_coef"], norm_h[1]) and torch.equal(met_c["grad_norm"], met["grad_norm"])
    assert abs(float(met_c["clip_coef"]) - 0.5) < 1e-6
    if weights == "zero_group":       # the weightless micro-batch added exact zeros: the window is its first row group's under the same count
        assert all(float(g.abs().max()) == 0.0 for g in parts[1].values()) and any(float(g.abs().max()) > 0.0 for g in parts[0].values())
        assert float(met["frames"]) == float(mets[0]["frames"]) and float(mets[1]["frames"]) == 0.0


# ---- (h) ------------------------------------------------------------------------------------------------------------------------------------
def _tiny_idm(precision):
    kw, cfg, sd = LR.tiny_idm()
    pol = InverseActionPolicy(idm_action_space(), pi_head_kwargs=dict(temperature=LR.TEMPERATURE), idm_net_kwargs=kw, precision=precision)
    pol.load_state_dict(sd, strict=False)
    return pol.to(DEV), sd


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("weights", [None, "some"])
def test_idm_step_is_the_hand_run_sequence(precision, weights):
    """(h) IDMTrainer, B = 3, K = 2 (groups of 2 and 1): the same equality, loss_and_grads(global_weight=count) per row group.  (m) for this trainer."""
    b = 3
    pol, sd = _tiny_idm(precision)
    g = torch.Generator().manual_seed(21)
    img = P.structured_frames(b, T, g).to(DEV)
    buttons, camera = torch.randint(0, 2, (b, T, 20), generator=g).to(DEV), torch.randint(0, 11, (b, T, 2), generator=g).to(DEV)
    fw, rows = _weights(b, weights), ROWS[(b, 2)]
    count = float(_count(b, fw))
    tr_h = IDMTrainer(pol)
    grads, totals, mets = [], [], []
    for lo, hi in rows:
        met = {}
        _, gk = tr_h.loss_and_grads(img[lo:hi], buttons[lo:hi], camera[lo:hi], frame_weight=None if fw is None else fw[lo:hi], metrics=met, unscaled=False,
                                    global_weight=count)
        grads.append({n: gk[n].clone() for n in tr_h.trainable if n in gk})
        totals.append(tr_h._idm_totals.clone())
        mets.append(met)
    t_sum = _sum64(totals)
    _hand_adam(tr_h, _torch_sum(grads), tr_h.grad_unscale(count))
    hand = _snapshot(pol, tr_h)
    pol.load_state_dict(sd, strict=False)
    tr = IDMTrainer(pol)
    with pytest.raises(ValueError, match="micro_batches"):
        tr.step(img, buttons, camera, micro_batches=b + 1)
    with pytest.raises(ValueError, match="micro_batches"):
        tr.step(img, buttons, camera, micro_batches=0)
    assert tr.step_count == 0
    met = {}
    loss = tr.step(img, buttons, camera, frame_weight=fw, metrics=met, micro_batches=2)
    torch.cuda.synchronize()
    assert not _same(_snapshot(pol, tr), hand), _same(_snapshot(pol, tr), hand)[:4]
    assert loss == float((t_sum[0] + t_sum[1]) / t_sum[6]) and tr.step_count == 1
    assert met["frame_out"].shape == (b, T, 8) and met["frame_nll"].shape == (b, T)
    for (lo, hi), mk in zip(rows, mets):
        assert torch.equal(met["frame_out"][lo:hi], mk["frame_out"])
    # the default keyword is the code as it was
    pol.load_state_dict(sd, strict=False)
    tr_a = IDMTrainer(pol)
    la = tr_a.step(img, buttons, camera, frame_weight=fw)
    snap_a = _snapshot(pol, tr_a)
    pol.load_state_dict(sd, strict=False)
    tr_b = IDMTrainer(pol)
    lb = tr_b.step(img, buttons, camera, frame_weight=fw, micro_batches=1)
    assert la == lb and not _same(_snapshot(pol, tr_b), snap_a)
    assert abs(la - loss) < 1e-4


def _ppo_inputs(pol, batch, b):
    """-> dict of [b, T] rollout quantities and perturbed prior log-probs; the old log-probs sit 0.1 below the policy's own (ratio inside the clip range)."""
    g = torch.Generator().manual_seed(31)
    img, first, state, ab, ac = batch
    adv = (torch.rand(b, T, generator=g) - 0.3).to(DEV)
    target = torch.randn(b, T, generator=g).to(DEV)
    tr = PPOTrainer(pol, optimizer_state=False, train_cnn=False, normalize_advantages=False, update_value_normalizer=False)
    met, _ = tr.evaluate(img, first, state, ab, ac, torch.zeros(b, T, device=DEV), adv, target)
    old = met["frame_out"][..., 8].clone() - 0.1
    lb, lc, _ = tr.prior_logprobs(pol, img, first, state)
    qb = torch.log_softmax(lb + 0.3 * torch.randn(lb.shape, generator=g).to(DEV), -1).view(b, T, -1)
    qc = torch.log_softmax(lc + 0.3 * torch.randn(lc.shape, generator=g).to(DEV), -1).view(b, T, -1)
    return dict(old=old, adv=adv, target=target, qb=qb, qc=qc)


PPO_KW = dict(kl_coef=0.1, entropy_coef=0.01, normalize_advantages=True, update_value_normalizer=True)


def test_ppo_step_is_the_hand_run_sequence(trainer_1x):
    """(h) PPOTrainer, B = 4, K = 2, kl_coef > 0 with prior log-probs, advantage normalisation and the normaliser update on.  The hand-run sequence
    normalises the advantages, updates the value normaliser and takes _loss_gradient_scale ONCE over the whole batch, then calls
    loss_and_grads(global_weight=...) per row group with both switches off.  The normaliser's buffers are compared too."""
    pol, sd = trainer_1x
    b = 4
    batch, rows = _batch(pol, b), ROWS[(b, 2)]
    img, first, state, ab, ac = batch
    x = _ppo_inputs(pol, batch, b)
    m = b * T
    try:
        pol.load_state_dict(sd)
        tr_h = PPOTrainer(pol, **PPO_KW)
        adv_n = tr_h._normalized(x["adv"].reshape(m).float().contiguous(), None, float(m)).view(b, T)
        tr_h._value_norm(x["target"].reshape(m).float().contiguous(), None)             # the update, once
        tr_h.normalize_advantages = tr_h.update_value_normalizer = False
        grads, totals, states = [], [], []
        for lo, hi in rows:
            _, gk, s_out = tr_h.loss_and_grads(img[lo:hi], first[lo:hi], _rows(state, lo, hi), ab[lo:hi], ac[lo:hi], x["old"][lo:hi], adv_n[lo:hi],
                                               x["target"][lo:hi], prior_lp=(x["qb"][lo:hi], x["qc"][lo:hi]), unscaled=False, global_weight=float(m))
            grads.append({n: gk[n].clone() for n in tr_h.trainable if n in gk})
            totals.append(tr_h._rl_totals.clone())
            states.append(s_out)
        t_sum = _sum64(totals)
        _hand_adam(tr_h, _torch_sum(grads), tr_h.grad_unscale(tr_h._global_frames))
        hand = _snapshot(pol, tr_h)

        pol.load_state_dict(sd)
        tr = PPOTrainer(pol, **PPO_KW)
        fresh = _snapshot(pol, tr)
        with pytest.raises(ValueError, match="micro_batches"):
            tr.step(img, first, state, ab, ac, x["old"], x["adv"], x["target"], prior_lp=(x["qb"], x["qc"]), micro_batches=b + 1)
        with pytest.raises(ValueError, match="micro_batches"):
            tr.step(img, first, state, ab, ac, x["old"], x["adv"], x["target"], prior_lp=(x["qb"], x["qc"]), micro_batches=-1)
        assert not _same(_snapshot(pol, tr), fresh), "a refused call moved a parameter or the normaliser"
        met = {}
        loss, state_out = tr.step(img, first, state, ab, ac, x["old"], x["adv"], x["target"], prior_lp=(x["qb"], x["qc"]), metrics=met, micro_batches=2)
        stepped = _snapshot(pol, tr)
        torch.cuda.synchronize()
    finally:
        pol.load_state_dict(sd)
    assert "value_head.linear.weight" in grads[0]
    assert not _same(stepped, hand), _same(stepped, hand)[:4]
    assert loss == float(tr_h._loss_of(t_sum)) and tr.step_count == 1
    assert float(met["kl_buttons"]) > 0 and met["frame_out"].shape == (b, T, 16)
    want_state = [torch.cat(parts, 0) for parts in zip(*[_leaves(s) for s in states])]
    assert all(torch.equal(a, c) for a, c in zip(_leaves(state_out), want_state))


# ---- (i) ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [6, 7])
def test_accumulated_gradients_agree_with_the_whole_batch(trainer_1x, b):
    """(i) per-tensor rel-L2 distance between the gradients behind step(micro_batches=2) and the one-piece batch's below 1e-3 (the bound
    tests/test_gpu_distributed.py holds the two-shard sum to: the same quantity), tensors of norm zero left out; the losses within 1e-4.
    B = 6 (groups of 3 + 3 sequences) and B = 7 (4 + 3): every micro-batch holds MORE than 8 frames, as every shard of that test does (T = 5 there).
    BCTrainer's linear layers run with tiling "auto" -- ops.linear picks the weight-streaming kernel of the acting step for M <= 8 rows and the MFMA
    GEMM above, "part of this trainer's bits" (training.py) -- so a micro-batch of at most 8 frames is computed by other kernels than the whole batch,
    with other operand roundings: a property of that threshold, not of the accumulation (measured at B = 4, T = 4, bf16: worst tensor 9.4e-2, median
    6.0e-2, losses 5e-4 apart).  The bit-for-bit tests above cover those small groups against their own kernels."""
    pol, sd = trainer_1x
    batch = _batch(pol, b)
    tr = BCTrainer(pol, optimizer_state=False)
    loss1, g1, _ = tr.reduced_loss_and_grads(*batch)
    g1 = {n: g1[n].clone() for n in tr.trainable}
    loss2, g2, _ = tr.reduced_loss_and_grads(*batch, micro_batches=2)
    torch.cuda.synchronize()
    errs = []
    for n, a in g1.items():
        if float(a.norm()) == 0:
            continue
        errs.append((float((g2[n].reshape(a.shape) - a).norm() / a.norm()), n))
    errs.sort(reverse=True)
    print(f"[{pol.precision}, B={b}] accumulated (K=2) vs whole-batch BC gradients: worst rel-L2 {errs[0][0]:.3e} ({errs[0][1]}), median {errs[len(errs) // 2][0]:.3e} "
          f"over {len(errs)} tensors; losses {float(loss2)!r} / {float(loss1)!r}")
    assert len(errs) >= 100
    assert errs[0][0] < 1e-3, errs[0]
    assert abs(float(loss2) - float(loss1)) < 1e-4


# ---- (j) ------------------------------------------------------------------------------------------------------------------------------------
def test_nonfinite_window_is_one_skipped_step():
    """(j) fp16 at loss scale 2^30: the window is skipped on the device -- skipped_steps == 1, the scale halved ONCE, no parameter bit changes.  bf16
    with an advantage of 1e30 in the second micro-batch and clipping on: the norm is not finite, the window is skipped likewise."""
    pol = _policy("fp16")
    batch = _batch(pol, 4)
    tr = BCTrainer(pol, lr=1e-4, weight_decay=0.0, loss_scale=2.0 ** 30)
    before = _snapshot(pol, tr)
    tr.step(*batch, micro_batches=2)
    torch.cuda.synchronize()
    assert tr.skipped_steps == 1 and tr.step_count == 0 and tr.loss_scale == 2.0 ** 29
    assert not _same(_snapshot(pol, tr), before)
    del pol, tr
    pol = _policy("bf16")
    batch = _batch(pol, 4)
    img, first, state, ab, ac = batch
    x = _ppo_inputs(pol, batch, 4)
    adv = x["adv"].clone()
    adv[3, 2] = 1e30
    tr = PPOTrainer(pol, max_grad_norm=5.0, normalize_advantages=False, update_value_normalizer=False)
    before = _snapshot(pol, tr)
    met = {}
    tr.step(img, first, state, ab, ac, x["old"], adv, x["target"], metrics=met, micro_batches=2)
    torch.cuda.synchronize()
    assert tr.skipped_steps == 1 and tr.step_count == 0 and tr.loss_scale == 1.0
    assert float(met["clip_coef"]) == 0.0 and not bool(torch.isfinite(met["grad_norm"]))
    assert not _same(_snapshot(pol, tr), before)
    # the same window without the planted value steps
    tr.step(img, first, state, ab, ac, x["old"], x["adv"], x["target"], metrics=met, micro_batches=2)
    assert tr.skipped_steps == 1 and tr.step_count == 1 and bool(torch.isfinite(met["grad_norm"]))


# ---- (m) ------------------------------------------------------------------------------------------------------------------------------------
def test_micro_batch_count_is_checked_before_anything_runs(trainer_1x):
    """(m) ValueError for K > B and K < 1, from step and from reduced_loss_and_grads; nothing moved."""
    pol, sd = trainer_1x
    batch = _batch(pol, 3)
    tr = BCTrainer(pol)
    before = _snapshot(pol, tr)
    for k in (4, 0, -2):
        with pytest.raises(ValueError, match="micro_batches"):
            tr.step(*batch, micro_batches=k)
        with pytest.raises(ValueError, match="micro_batches"):
            tr.reduced_loss_and_grads(*batch, micro_batches=k)
    assert tr.step_count == 0 and not _same(_snapshot(pol, tr), before)
    loss, _ = tr.step(*batch, micro_batches=3)          # K == B: three groups of one sequence
    assert tr.step_count == 1 and loss == loss
    pol.load_state_dict(sd)


# ---- (l) ------------------------------------------------------------------------------------------------------------------------------------
def _rccl_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", VPT_DP_FORCE_EXCHANGE="1")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        pol = _policy("bf16")
        sd = copy.deepcopy(pol.state_dict())
        batch = _batch(pol, 4)
        fw = _weights(4, "some")
        res = []
        for force in (False, True):
            pol.load_state_dict(sd)
            tr = BCTrainer(pol, max_grad_norm=1.0)
            assert tr.force_exchange              # (the environment variable, read by the constructor)
            tr.force_exchange = force
            met = {}
            loss, state_out = tr.step(*batch, frame_weight=fw, metrics=met, micro_batches=2)
            torch.cuda.synchronize()
            assert (tr._arenas is not None) == force
            res.append((loss, met["grad_norm"].clone(), met["clip_coef"].clone(), {k: v.detach().clone() for k, v in pol.named_parameters()},
                        met["frame_out"].clone(), [x.clone() for x in _leaves(state_out)], met["loss"].clone()))
        assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2]) and 0 < float(res[0][2]) < 1
        assert all(torch.equal(res[0][3][k], res[1][3][k]) for k in res[0][3])
        assert torch.equal(res[0][4], res[1][4]) and all(torch.equal(a, c) for a, c in zip(res[0][5], res[1][5])) and torch.equal(res[0][6], res[1][6])
        with open(os.path.join(out_dir, "ok"), "w") as f:
            f.write(f"{float(res[0][1])!r}")
    finally:
        dist.destroy_process_group()


def test_data_parallel_window_reports_the_local_bits():
    """(l) a one-rank RCCL group with VPT_DP_FORCE_EXCHANGE=1: step(micro_batches=2) through both arenas, the early exchange under the last
    micro-batch's CNN backward and the late one gives the local path's parameters, loss and norm bit for bit."""
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_rccl_worker, args=(1, 29583, d), nprocs=1, join=True)
        assert float(open(os.path.join(d, "ok")).read()) > 0
