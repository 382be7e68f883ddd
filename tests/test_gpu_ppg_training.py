"""The auxiliary phase of PPOTrainer (vpt_amd.rl_training: policy_snapshot, aux_loss_and_grads, aux_step, aux_evaluate) on the GPU, both operand
formats: its wiring against the hand-run pieces (bit for bit), its gradients against the same loss written in torch on the autograd boundary of
lib/policy.py, micro-batches, its behaviour over a few steps, padding by frame weights, checkpointing, the shared optimiser, and a guard that the
policy phase's step is what it was.  Needs an MI355X.  Policy: the 1x model of tests/test_gpu_rl_training.py (temperature 2.0), B = 2, T = 4..6."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from vpt_amd.rl_training import AUX_METRICS, PPOTrainer  # noqa: E402
from vpt_amd.lib.policy import MinecraftAgentPolicy  # noqa: E402
from vpt_amd.lib.types import minecraft_action_space  # noqa: E402
from oracle import vpt_oracle as O  # noqa: E402
from tests import ppg_loss_ref as R  # noqa: E402

DEV = "cuda"
NB, NC = 8641, 121
AUX = dict(clone_coef=0.7, aux_value_coef=0.4)


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


def _batch(pol, b=2, t=5):
    """A fixed batch: images, value targets, the policy's own snapshot at the initial weights (snap_*) and a perturbed teacher (old_*: the
    snapshot's log-probs + 0.3 N(0, 1), re-normalised), so that the clone term has a gradient at the initial weights."""
    key = (b, t, pol.precision)
    if key not in _BATCH:
        g = torch.Generator().manual_seed(29)
        d = dict(b=b, t=t, img=torch.randint(0, 256, (b, t, 128, 128, 3), generator=g, dtype=torch.uint8).to(DEV),
                 first=torch.zeros(b, t, dtype=torch.bool, device=DEV), target=(torch.randn(b, t, generator=g) * 2 + 0.5).to(DEV))
        tr = PPOTrainer(pol, optimizer_state=False, train_cnn=False)
        sb, sc, _ = tr.policy_snapshot(d["img"], d["first"], pol.initial_state(b))
        d["snap"] = (sb.clone(), sc.clone())
        d["old"] = (torch.log_softmax(sb + 0.3 * torch.randn(sb.shape, generator=g).to(DEV), -1),
                    torch.log_softmax(sc + 0.3 * torch.randn(sc.shape, generator=g).to(DEV), -1))
        _BATCH[key] = d
    return _BATCH[key]


def _l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm().clamp(min=1e-300))


def _vnorm(pol):
    mean, var = pol.value_head.normalizer.running_mean_var()
    return torch.stack([mean.reshape(-1)[0], torch.sqrt(var).reshape(-1)[0]]).float().contiguous()


def _leaves(tree):
    if isinstance(tree, torch.Tensor):
        return [tree]
    return [x for part in tree for x in _leaves(part)]


def _same_state(a, b):
    return all(torch.equal(x, y) for x, y in zip(_leaves(a), _leaves(b)))


def _far_targets(pol, target):
    """Targets 30 normalised units above the prediction's neighbourhood (tests/test_gpu_rl_training.py (h) explains why nearer ones overshoot)."""
    mean, var = pol.value_head.normalizer.running_mean_var()
    return (mean.reshape(-1)[0] + torch.sqrt(var).reshape(-1)[0] * (30.0 + target)).float()


def test_aux_loss_and_grads_is_the_hand_run_sequence(trainer_1x):
    """(g)  forward_saving -> ops.ppg_aux_loss -> backward_from(value_grads=True) by hand: torch.equal on the loss, all 131 gradient tensors and the
    state; the metrics are the totals'; the value normaliser does not move unless asked to."""
    pol, sd = trainer_1x
    d = _batch(pol)
    b, t = d["b"], d["t"]
    m = b * t
    tr = PPOTrainer(pol, optimizer_state=False, **AUX)
    nrm = copy.deepcopy(pol.value_head.normalizer.state_dict())
    metrics = {}
    loss, grads, state = tr.aux_loss_and_grads(d["img"], d["first"], pol.initial_state(b), d["old"], d["target"], metrics=metrics)
    assert all(torch.equal(v, nrm[k]) for k, v in pol.value_head.normalizer.state_dict().items())
    S = tr.forward_saving(d["img"], d["first"], pol.initial_state(b))
    pow2 = 16.0                                            # fp16: the power-of-two part of the mean's 1 / 10 is taken out again (_loss_gradient_scale)
    scale = tr.loss_scale * (pow2 / m) if tr.scaled else 1.0 / m
    dz, frame_out, totals = ops.ppg_aux_loss(S["lp_b"], S["lp_c"], d["old"][0], d["old"][1], S["ldz"], scale, value=S["logits"][:, NB + NC],
                                             value_target=d["target"].reshape(m).float().contiguous(), vnorm=_vnorm(pol), clone_coef=AUX["clone_coef"],
                                             value_coef=AUX["aux_value_coef"], temperature=2.0, dtype=tr.dtype)
    state_h = S["state_out"]
    hand = tr.backward_from(S, dz, value_grads=True)
    if tr.scaled:
        for v in hand.values():
            v.mul_(1.0 / (tr.loss_scale * pow2))
    torch.cuda.synchronize()
    loss_h = (AUX["clone_coef"] * (totals[0] + totals[1]) + AUX["aux_value_coef"] * totals[2]) / totals[5]
    assert torch.equal(loss, loss_h) and bool(torch.isfinite(loss)) and float(loss) > 0
    assert set(grads) == set(hand) and set(tr.trainable) <= set(grads) and len([n for n in tr.trainable if n in grads]) == 131
    assert all(torch.equal(grads[k], hand[k]) for k in hand), [k for k in hand if not torch.equal(grads[k], hand[k])][:4]
    assert _same_state(state, state_h)
    assert float(grads["value_head.linear.weight"].abs().max()) > 0 and sum(float(grads[n].abs().max()) > 0 for n in tr.trainable) >= 120
    assert set(AUX_METRICS) | {"frame_out"} == set(metrics) and tuple(metrics["frame_out"].shape) == (b, t, 8)
    assert torch.equal(metrics["frame_out"].reshape(m, 8), frame_out) and torch.equal(metrics["loss"], loss)
    assert float(metrics["frames"]) == m and float(metrics["weight_sum"]) == m
    assert float(metrics["clone_kl_buttons"]) > 0 and float(metrics["clone_kl_camera"]) > 0 and float(metrics["value_loss"]) > 0
    assert abs(float(metrics["teacher_mass_buttons"]) - 1) < 1e-4 and abs(float(metrics["teacher_mass_camera"]) - 1) < 1e-4
    tr_v = PPOTrainer(pol, optimizer_state=False, value_coef=0.4, clone_coef=0.7)              # aux_value_coef = None means value_coef
    loss_v, g_v, _ = tr_v.aux_loss_and_grads(d["img"], d["first"], pol.initial_state(b), d["old"], d["target"])
    assert torch.equal(loss_v, loss) and all(torch.equal(g_v[k], grads[k]) for k in grads)
    with pytest.raises(ValueError, match="old_lp"):
        tr.aux_loss_and_grads(d["img"], d["first"], pol.initial_state(b), None, d["target"])
    try:
        tr.aux_loss_and_grads(d["img"], d["first"], pol.initial_state(b), d["old"], d["target"], update_value_normalizer=True)
        assert not all(torch.equal(v, nrm[k]) for k, v in pol.value_head.normalizer.state_dict().items())
    finally:
        pol.load_state_dict(sd)


def test_gradients_against_the_same_loss_on_the_autograd_boundary(trainer_1x):
    """(h)  The loss written in torch (tests/ppg_loss_ref.torch_loss) on get_output_for_observation's outputs, then .backward(): both routes share
    the forward and every ReLU gate and differ only in how dz is rounded to 16 bits.  The boundary is run twice, the torch loss in fp32 and in
    fp64; their per-tensor rel-L2 distance d_ref is the boundary's own sensitivity to last-bit changes of dz, and the trainer must be within
    max(4 d_ref, one 16-bit ulp) of the fp64 run, per tensor (tests/test_gpu_rl_training.py (g)'s rule).
    fp16: the rule's premise is that the two routes round to 16 bits at the same points, which a power-of-two difference between their gradient
    lifts keeps only while the CNN backward's 16-bit buffers stay in IEEE half's normal range.  With this loss (a few large value gradients, 8762
    small policy ones per frame) the boundary's default lift is 512 against the trainer's 4096, its buffers underflow, and the boundary becomes
    insensitive to its own loss's precision (d_ref = 0 exactly) while sitting 1.7e-3 from every route that does not underflow -- the trainer against
    ITSELF at loss scales 64 .. 8 moves by 1.5e-3 .. 2.1e-3 on the same stack-0 / stack-1 CNN tensors, at 128 .. 1024 by 4e-5 (measured).  The boundary
    is therefore run at the trainer's lift (autograd_lift, its own knob): the same reference, rounding where the trainer rounds.
    The batch is 2 x 4 frames: on 2 x 5 each route rounds its own 1 / 10 into dz (the trainer inside its row scale, autograd inside the incoming
    gradient) and, at equal lifts, one fp16 tensor of the 131 was outside the rule -- recurrent_layer.blocks.1 ... k_layer.weight, 5.9e-4 with d_ref
    1.1e-4 against the 4.9e-4 floor (bf16: inside, 4.9e-5); with 8 frames 1 / M is exact in both routes.  Measured on 2 x 4: bf16 largest distance
    7.8e-5 (d_ref 7.5e-5), fp16 1.71e-3 on cnn.stacks.0.blocks.1.conv0.norm.bias (d_ref 6.5e-4: 0.66 of 4 d_ref).  The bound is the issue's, unchanged."""
    pol, sd = trainer_1x
    d = _batch(pol, 2, 4)           # 8 frames: the mean's 1 / M is a power of two, exact in both routes (with 10 frames each route rounds its own 1 / 10)
    b, t = d["b"], d["t"]
    m = b * t
    tr = PPOTrainer(pol, optimizer_state=False, **AUX)
    _, grads, _ = tr.aux_loss_and_grads(d["img"], d["first"], pol.initial_state(b), d["old"], d["target"])
    that = pol.value_head.normalizer.normalize(d["target"].reshape(m, 1)).reshape(m)
    runs, overflows0 = {}, pol.grad_overflows
    for dt in (torch.float32, torch.float64):
        pol.zero_grad(set_to_none=True)
        (pd, vpred, _), _ = pol({"img": d["img"]}, d["first"], pol.initial_state(b))
        assert pd["buttons"].requires_grad and vpred.requires_grad
        if tr.scaled:
            # the largest gradient element the loss below hands the boundary, and the lift that places it where the trainer's scale does
            gmax = max(float(2 * AUX["aux_value_coef"] * (vpred.detach().reshape(m) - that).abs().max()) / m,
                       AUX["clone_coef"] * float(max(d["old"][0].max(), d["old"][1].max()).exp()) / m)
            for eng in pol._grad_engines.values():
                eng.autograd_lift = 1.25 * gmax * tr.loss_scale * tr._global_frames         # (_global_frames: 2^ceil(log2 M), _loss_gradient_scale)
        loss = R.torch_loss(pd["buttons"].reshape(m, NB).to(dt), pd["camera"].reshape(m, NC).to(dt), d["old"][0].to(dt), d["old"][1].to(dt),
                            vpred.reshape(m).to(dt), that.to(dt), torch.ones(m, dtype=dt, device=DEV), clone_coef=AUX["clone_coef"],
                            value_coef=AUX["aux_value_coef"])
        loss.backward()
        runs[dt] = {n: p.grad.detach().clone() for n, p in pol.named_parameters() if p.grad is not None}
    pol.zero_grad(set_to_none=True)
    for eng in pol._grad_engines.values():
        eng.autograd_lift = 256.0
    torch.cuda.synchronize()
    assert pol.grad_overflows == overflows0                     # (the raised lift overflowed nothing: the runs above returned gradients)
    r32, r64 = runs[torch.float32], runs[torch.float64]
    assert set(r64) >= set(grads) and "value_head.linear.weight" in r64
    floor = 2.0 ** -8 if pol.precision == "bf16" else 2.0 ** -11
    rows = []
    for n in grads:
        ref = r64[n].reshape(grads[n].shape)
        if float(ref.norm()) == 0.0:
            assert float(grads[n].abs().max()) == 0.0, n
            continue
        rows.append((n, _l2(r32[n].reshape(ref.shape), ref), _l2(grads[n], ref)))
    rows.sort(key=lambda r: -r[2])
    for n, d_ref, d_tr in rows[:4]:
        print(f"PPG aux grads [{pol.precision}] {n}: trainer vs fp64-loss boundary rel-L2 {d_tr:.3e}, d_ref (fp32 vs fp64 loss) {d_ref:.3e}")
    print(f"PPG aux grads [{pol.precision}] largest d_ref {max(r[1] for r in rows):.3e}, largest trainer distance {rows[0][2]:.3e}, floor {floor:.3e}, {len(rows)} tensors")
    assert len(rows) >= 120
    bad = [(n, d_ref, d_tr) for n, d_ref, d_tr in rows if not d_tr <= max(4 * d_ref, floor)]
    assert not bad, bad[:4]


def test_two_micro_batches_are_the_two_rows_summed(trainer_1x):
    """(i)  micro_batches = 2 on B = 2: each row run by hand under the whole batch's scale (global_weight), the gradients summed with
    ops.grad_accumulate_: torch.equal on every gradient, the loss (the rows' totals summed in fp64), the records and the state."""
    pol, sd = trainer_1x
    d = _batch(pol)
    b, t = d["b"], d["t"]
    m = b * t
    tr = PPOTrainer(pol, optimizer_state=False, **AUX)
    ob, oc = d["old"]
    parts, totals, states, recs = [], [], [], []
    for r in range(b):
        met = {}
        _, gk, s_out = tr.aux_loss_and_grads(d["img"][r:r + 1], d["first"][r:r + 1], pol.initial_state(1), (ob[r * t:(r + 1) * t], oc[r * t:(r + 1) * t]),
                                             d["target"][r:r + 1], unscaled=False, global_weight=float(m), metrics=met)
        parts.append({n: gk[n].clone() for n in tr.trainable if n in gk})
        totals.append(tr._aux_totals.clone()); states.append(s_out); recs.append(met["frame_out"].clone())
    names = list(parts[0])
    ops.grad_accumulate_([parts[0][n].view(-1) for n in names], [parts[1][n].contiguous().view(-1) for n in names])
    met = {}
    loss, grads, state = tr.aux_loss_and_grads(d["img"], d["first"], pol.initial_state(b), d["old"], d["target"], unscaled=False, micro_batches=2, metrics=met)
    torch.cuda.synchronize()
    assert len(names) == 131 and not [n for n in names if not torch.equal(grads[n], parts[0][n])]
    t_sum = (totals[0].double() + totals[1].double()).float()
    assert torch.equal(loss, tr._aux_loss_of(t_sum)) and bool(torch.isfinite(loss))
    assert torch.equal(met["frame_out"], torch.cat(recs, 0))
    assert all(torch.equal(x, torch.cat([y, z], 0)) for x, y, z in zip(_leaves(state), _leaves(states[0]), _leaves(states[1])))
    with pytest.raises(ValueError, match="micro_batches"):
        tr.aux_loss_and_grads(d["img"], d["first"], pol.initial_state(b), d["old"], d["target"], micro_batches=3)


def test_aux_steps_fit_the_value_and_the_clone_term_holds_the_policy(trainer_1x):
    """(j)  Six aux_steps, lr 1e-4, no weight decay, targets 30 normalised units away, the snapshot taken before the first step: the value loss
    falls under clone_coef = 1 and under clone_coef = 0, and the clone KL to the snapshot after the six steps (aux_evaluate) is smaller with
    clone_coef = 1 than with 0.  Only the directions are asserted."""
    pol, sd = trainer_1x
    d = dict(_batch(pol, 2, 4))
    b = d["b"]
    d["target"] = _far_targets(pol, d["target"])
    final_kl, traces = {}, {}
    try:
        for beta in (0.0, 1.0):
            pol.load_state_dict(sd)
            tr = PPOTrainer(pol, lr=1e-4, weight_decay=0.0, clone_coef=beta, value_coef=0.5)
            sb, sc, _ = tr.policy_snapshot(d["img"], d["first"], pol.initial_state(b))
            snap = (sb.clone(), sc.clone())
            vls = []
            for _ in range(6):
                met = {}
                tr.aux_step(d["img"], d["first"], pol.initial_state(b), snap, d["target"], metrics=met)
                vls.append(float(met["value_loss"]))
            assert tr.step_count == 6 and tr.skipped_steps == 0
            met, _ = tr.aux_evaluate(d["img"], d["first"], pol.initial_state(b), snap, d["target"])
            final_kl[beta] = float(met["clone_kl_buttons"] + met["clone_kl_camera"])
            traces[beta] = vls
        torch.cuda.synchronize()
    finally:
        pol.load_state_dict(sd)
    print(f"PPG aux steps [{pol.precision}] value loss clone_coef 0: {[round(x, 3) for x in traces[0.0]]}, clone_coef 1: {[round(x, 3) for x in traces[1.0]]}; "
          f"final clone KL to the snapshot: clone_coef 0 -> {final_kl[0.0]:.4e}, clone_coef 1 -> {final_kl[1.0]:.4e}")
    assert traces[0.0][-1] < traces[0.0][0] and traces[1.0][-1] < traces[1.0][0]
    assert final_kl[1.0] < final_kl[0.0]


def test_zero_weight_padding_checkpoint_and_the_shared_optimiser(trainer_1x):
    """(k)  frame_weight with a zero-padded tail: replacing the padded frames' images, teacher rows and targets (NaN included) changes no bit of the
    gradients or of the loss.  state_dict round-trips; a policy-phase step after an aux_step continues the same step count and moments."""
    pol, sd = trainer_1x
    d = dict(_batch(pol, 2, 6))
    b, t = d["b"], d["t"]
    w = torch.ones(b, t, device=DEV)
    w[1, 4:] = 0.0
    w[0, 2] = 0.5
    tr = PPOTrainer(pol, lr=1e-4, weight_decay=0.0, normalize_advantages=False, update_value_normalizer=False, **AUX)
    loss_a, ga, _ = tr.aux_loss_and_grads(d["img"], d["first"], pol.initial_state(b), d["old"], d["target"], frame_weight=w)
    g = torch.Generator().manual_seed(99)
    img, target = d["img"].clone(), d["target"].clone()
    img[1, 4:] = torch.randint(0, 256, (2, 128, 128, 3), generator=g, dtype=torch.uint8).to(DEV)
    target[1, 4:] = float("nan")
    ob, oc = d["old"][0].clone(), d["old"][1].clone()
    ob[t + 4:], oc[t + 4:] = float("nan"), float("nan")
    loss_b, gb, _ = tr.aux_loss_and_grads(img, d["first"], pol.initial_state(b), (ob, oc), target, frame_weight=w)
    torch.cuda.synchronize()
    assert torch.equal(loss_a, loss_b) and bool(torch.isfinite(loss_a))
    assert all(bool(torch.isfinite(v).all()) for v in ga.values())
    assert not [k for k in ga if not torch.equal(ga[k], gb[k])]
    with pytest.raises(ValueError, match="frame_weight"):
        tr.aux_loss_and_grads(d["img"], d["first"], pol.initial_state(b), d["old"], d["target"], frame_weight=-w)
    zeros = torch.zeros(b, t, device=DEV)
    ab, ac = torch.zeros(b, t, dtype=torch.int64, device=DEV), torch.zeros(b, t, dtype=torch.int64, device=DEV)
    try:
        for _ in range(2):
            tr.aux_step(d["img"], d["first"], pol.initial_state(b), d["old"], d["target"], frame_weight=w)
        state = tr.state_dict()
        assert state["step"] == 2 and float(state["exp_avg"]["value_head.linear.weight"].abs().max()) > 0
        tr2 = PPOTrainer(pol, lr=1.0, **AUX)
        tr2.load_state_dict(state)
        assert tr2.step_count == 2 and tr2.lr == 1e-4
        assert all(torch.equal(tr2.m[k], tr.m[k]) and torch.equal(tr2.v[k], tr.v[k]) for k in tr.m)
        m_before = {k: v.clone() for k, v in tr.m.items()}
        met, _ = tr.evaluate(d["img"], d["first"], pol.initial_state(b), ab, ac, zeros, zeros + 1, d["target"])
        old = met["frame_out"][..., 8].clone()
        _, gp, _ = tr.loss_and_grads(d["img"], d["first"], pol.initial_state(b), ab, ac, old, zeros + 1, d["target"])
        gp = {k: v.clone() for k, v in gp.items()}
        tr.step(d["img"], d["first"], pol.initial_state(b), ab, ac, old, zeros + 1, d["target"])
        torch.cuda.synchronize()
        assert tr.step_count == 3 and tr.skipped_steps == 0
        # the policy phase's step moved the auxiliary steps' first moments on: m <- 0.9 m + 0.1 g (the default betas), to the 16-bit route's rounding
        for k in ("value_head.linear.weight", "value_head.linear.bias"):
            want = 0.9 * m_before[k] + 0.1 * gp[k].reshape(m_before[k].shape)
            assert float((tr.m[k] - want).abs().max()) <= 1e-3 * float(want.abs().max()) and float(m_before[k].abs().max()) > 0, k
    finally:
        pol.load_state_dict(sd)


def test_fp16_huge_target_skips_the_aux_step_on_the_device():
    """(k, fp16)  A value target of 1e30 overflows the value column of dz: the overflow check flags it, the Adam launch leaves every tensor
    untouched, the step count stays, the loss scale halves; the same trainer then trains on the sane batch."""
    pol = _policy("fp16")
    d = dict(_batch(pol, 2, 4))
    b = d["b"]
    tr = PPOTrainer(pol, lr=1e-4, weight_decay=0.0, **AUX)
    scale0 = tr.loss_scale
    before = {k: v.detach().clone() for k, v in pol.named_parameters()}
    huge = d["target"].clone()
    huge[0, 1] = 1e30
    tr.aux_step(d["img"], d["first"], pol.initial_state(b), d["old"], huge)
    torch.cuda.synchronize()
    assert tr.skipped_steps == 1 and tr.step_count == 0 and tr.loss_scale == scale0 / 2
    assert all(torch.equal(v.detach(), before[k]) for k, v in pol.named_parameters())
    assert all(float(x.abs().max()) == 0.0 for x in tr.m.values()) and all(float(x.abs().max()) == 0.0 for x in tr.v.values())
    loss, _ = tr.aux_step(d["img"], d["first"], pol.initial_state(b), d["old"], d["target"])
    torch.cuda.synchronize()
    assert tr.skipped_steps == 1 and tr.step_count == 1 and loss == loss
    moved = sum(int(not torch.equal(v.detach(), before[k])) for k, v in pol.named_parameters() if k in tr.m)
    assert moved == len(tr.m)


def test_policy_phase_step_is_what_it_was(trainer_1x):
    """(l)  Regression guard.  A PPOTrainer built without the new arguments steps exactly as the existing call pattern does -- forward_saving,
    ops.rl_loss, backward_from, the Adam launch, written out by hand here -- and a trainer built WITH unusual auxiliary coefficients takes the
    same policy-phase step: torch.equal on every parameter, both moments and the loss."""
    pol, sd = trainer_1x
    d = _batch(pol, 2, 4)
    b, t = d["b"], d["t"]
    m = b * t
    g = torch.Generator().manual_seed(3)
    ab, ac = torch.randint(0, NB, (b, t), generator=g).to(DEV), torch.randint(0, NC, (b, t), generator=g).to(DEV)
    adv = (torch.rand(b, t, generator=g) - 0.4).to(DEV)
    coef = dict(kl_coef=0.3, entropy_coef=0.01, value_coef=0.5)
    kw = dict(lr=1e-4, weight_decay=0.01, normalize_advantages=False, update_value_normalizer=False, **coef)
    flat = lambda x, dt=torch.float32: x.reshape(m).to(dt).contiguous()
    results = {}
    try:
        for name, extra in (("default", {}), ("aux", dict(clone_coef=3.0, aux_value_coef=0.125)), ("hand", {})):
            pol.load_state_dict(sd)
            tr = PPOTrainer(pol, **kw, **extra)
            old = (d["snap"][0].gather(1, flat(ab, torch.int64)[:, None]) + d["snap"][1].gather(1, flat(ac, torch.int64)[:, None])).reshape(b, t) - 0.05
            if name != "hand":
                loss, _ = tr.step(d["img"], d["first"], pol.initial_state(b), ab, ac, old, adv, d["target"], prior_lp=d["old"])
            else:
                S = tr.forward_saving(d["img"], d["first"], pol.initial_state(b))
                pow2 = 8.0
                scale = tr.loss_scale * (pow2 / m) if tr.scaled else 1.0 / m
                dz, _, totals = ops.rl_loss(S["lp_b"], S["lp_c"], flat(ab, torch.int64), flat(ac, torch.int64), flat(old), flat(adv), S["ldz"], scale,
                                            prior_buttons=d["old"][0], prior_camera=d["old"][1], value=S["logits"][:, NB + NC],
                                            value_target=flat(d["target"]), vnorm=_vnorm(pol), clip=0.2, temperature=2.0, dtype=tr.dtype, **coef)
                grads = tr.backward_from(S, dz, value_grads=True)
                loss, _ = tr._optimizer_tail(tr._loss_of(totals), grads, tr.grad_unscale(pow2 if tr.scaled else float(m)), DEV)
            torch.cuda.synchronize()
            assert tr.step_count == 1
            results[name] = (loss, {k: v.detach().clone() for k, v in pol.named_parameters()}, {k: v.clone() for k, v in tr.m.items()},
                             {k: v.clone() for k, v in tr.v.items()})
    finally:
        pol.load_state_dict(sd)
    base = results["default"]
    assert any(not torch.equal(v, sd[k].to(DEV)) for k, v in base[1].items() if k in sd)
    for other in ("aux", "hand"):
        r = results[other]
        assert r[0] == base[0], other
        for i in (1, 2, 3):
            assert not [k for k in base[i] if not torch.equal(base[i][k], r[i][k])], other
