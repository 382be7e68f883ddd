"""PPOTrainer (vpt_amd.rl_training) on the GPU, both operand formats: its wiring against the hand-run pieces (bit for bit), its gradients against the
same loss written in torch on the autograd boundary of lib/policy.py, its behaviour over a few steps, padding by frame weights, checkpointing.
Needs an MI355X.  Policy: the 1x model of tests/test_gpu_training.py (temperature 2.0), B = 2, T = 4..6."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from vpt_amd.rl_training import METRICS, PPOTrainer  # noqa: E402
from vpt_amd.training import BCTrainer  # noqa: E402
from vpt_amd.lib.policy import MinecraftAgentPolicy  # noqa: E402
from vpt_amd.lib.types import minecraft_action_space  # noqa: E402
from oracle import vpt_oracle as O  # noqa: E402
from tests import rl_loss_ref as R  # noqa: E402

DEV = "cuda"
NB, NC = 8641, 121
COEF = dict(kl_coef=0.3, entropy_coef=0.01, value_coef=0.5)


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
    """A fixed rollout-like batch: images, actions, the behaviour log-prob set so that the ratios are 1.5, 0.6, 0.9, 1.1, ... (clipped both ways and
    not), advantages of both signs, value targets, and a random prior."""
    key = (b, t, pol.precision)
    if key not in _BATCH:
        g = torch.Generator().manual_seed(23)
        m = b * t
        d = dict(b=b, t=t, img=torch.randint(0, 256, (b, t, 128, 128, 3), generator=g, dtype=torch.uint8).to(DEV),
                 first=torch.zeros(b, t, dtype=torch.bool, device=DEV),
                 ab=torch.randint(0, NB, (b, t), generator=g).to(DEV), ac=torch.randint(0, NC, (b, t), generator=g).to(DEV),
                 adv=((0.5 + torch.rand(b, t, generator=g)) * torch.tensor([1.0, -1.0, 1.0, -1.0, -1.0, 1.0] * 4)[:m].view(b, t)).to(DEV),
                 target=(torch.randn(b, t, generator=g) * 2 + 0.5).to(DEV),
                 qb=torch.log_softmax(torch.randn(m, NB, generator=g), -1).to(DEV), qc=torch.log_softmax(torch.randn(m, NC, generator=g), -1).to(DEV))
        tr = PPOTrainer(pol, optimizer_state=False, train_cnn=False, normalize_advantages=False, update_value_normalizer=False, **COEF)
        zeros = torch.zeros(b, t, device=DEV)
        met, _ = tr.evaluate(d["img"], d["first"], pol.initial_state(b), d["ab"], d["ac"], zeros, d["adv"], d["target"], prior_lp=(d["qb"], d["qc"]))
        d["lp0"] = met["frame_out"][..., 8].clone()
        rho = torch.tensor([1.5, 0.6, 0.9, 1.1, 1.5, 0.6] * 4)[:m].view(b, t).to(DEV)
        d["old"] = d["lp0"] - torch.log(rho)
        _BATCH[key] = d
    return _BATCH[key]


def _args(d):
    return d["img"], d["first"], None, d["ab"], d["ac"], d["old"], d["adv"], d["target"]


def _call(fn, pol, d, **kw):
    a = list(_args(d))
    a[2] = pol.initial_state(d["b"])
    return fn(*a, **kw)


def _l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm().clamp(min=1e-300))


def _vnorm(pol):
    mean, var = pol.value_head.normalizer.running_mean_var()
    return torch.stack([mean.reshape(-1)[0], torch.sqrt(var).reshape(-1)[0]]).float().contiguous()


def test_loss_and_grads_is_the_hand_run_sequence(trainer_1x):
    """(f)  forward_saving -> ops.rl_loss -> backward_from(value_grads=True) by hand: torch.equal on the loss, every gradient tensor and the state;
    the value head's gradients are non-zero with value_coef > 0 and exactly zero with value_coef = 0; the metrics are the totals'."""
    pol, sd = trainer_1x
    d = _batch(pol)
    m, prior = d["b"] * d["t"], (d["qb"], d["qc"])
    tr = PPOTrainer(pol, optimizer_state=False, normalize_advantages=False, update_value_normalizer=False, **COEF)
    assert "value_head.linear.weight" in tr.trainable and "value_head.linear.bias" in tr.trainable
    assert "value_head.linear.weight" not in BCTrainer(pol, optimizer_state=False).trainable
    assert not any("normalizer" in n for n in tr.trainable)
    metrics = {}
    loss, grads, state = _call(tr.loss_and_grads, pol, d, prior_lp=prior, metrics=metrics)
    S = tr.forward_saving(d["img"], d["first"], pol.initial_state(d["b"]))
    pow2 = 16.0                                            # fp16: the power-of-two part of the mean's 1 / 10 is taken out again (PPOTrainer._loss_gradient_scale)
    scale = tr.loss_scale * (pow2 / m) if tr.scaled else 1.0 / m
    flat = lambda x, dt=torch.float32: x.reshape(m).to(dt).contiguous()
    dz, frame_out, totals = ops.rl_loss(S["lp_b"], S["lp_c"], flat(d["ab"], torch.int64), flat(d["ac"], torch.int64), flat(d["old"]), flat(d["adv"]),
                                        S["ldz"], scale, prior_buttons=d["qb"], prior_camera=d["qc"], value=S["logits"][:, NB + NC],
                                        value_target=flat(d["target"]), vnorm=_vnorm(pol), clip=0.2, temperature=2.0, dtype=tr.dtype, **COEF)
    state_h = S["state_out"]
    hand = tr.backward_from(S, dz, value_grads=True)
    if tr.scaled:
        for v in hand.values():
            v.mul_(1.0 / (tr.loss_scale * pow2))
    torch.cuda.synchronize()
    loss_h = (totals[0] + COEF["kl_coef"] * (totals[1] + totals[2]) - COEF["entropy_coef"] * (totals[3] + totals[4]) + COEF["value_coef"] * totals[5]) / totals[10]
    assert torch.equal(loss, loss_h) and bool(torch.isfinite(loss))
    assert set(grads) == set(hand) and set(tr.trainable) <= set(grads) and len(grads) >= 122
    assert all(torch.equal(grads[k], hand[k]) for k in hand), [k for k in hand if not torch.equal(grads[k], hand[k])][:4]
    for (m0, (k0, v0)), (m1, (k1, v1)) in zip(state, state_h):
        assert torch.equal(m0, m1) and torch.equal(k0, k1) and torch.equal(v0, v1)
    assert float(grads["value_head.linear.weight"].abs().max()) > 0 and float(grads["value_head.linear.bias"].abs().max()) > 0
    assert set(METRICS) | {"frame_out"} == set(metrics) and tuple(metrics["frame_out"].shape) == (d["b"], d["t"], 16)
    assert torch.equal(metrics["frame_out"].reshape(m, 16), frame_out) and torch.equal(metrics["loss"], loss)
    assert float(metrics["frames"]) == m and float(metrics["weight_sum"]) == m
    assert 0.0 < float(metrics["clip_frac"]) < 1.0 and float(metrics["kl_buttons"]) > 0 and float(metrics["entropy_camera"]) > 0
    tr0 = PPOTrainer(pol, optimizer_state=False, train_cnn=False, normalize_advantages=False, update_value_normalizer=False, **dict(COEF, value_coef=0.0))
    _, g0, _ = _call(tr0.loss_and_grads, pol, d, prior_lp=prior)
    assert float(g0["value_head.linear.weight"].abs().max()) == 0.0 and float(g0["value_head.linear.bias"].abs().max()) == 0.0
    with pytest.raises(ValueError, match="prior_lp"):
        _call(tr.loss_and_grads, pol, d)


def test_gradients_against_the_same_loss_on_the_autograd_boundary(trainer_1x):
    """(g)  The loss written in torch (tests/rl_loss_ref.torch_loss: torch.min, clamp, squared error, KL and entropy from the log-probs) on
    get_output_for_observation's outputs, then .backward(): both routes share the forward and every ReLU gate and differ only in how dz is rounded
    to 16 bits.  The boundary is run twice, the torch loss in fp32 and in fp64; their per-tensor rel-L2 distance d_ref is the boundary's own
    sensitivity to last-bit changes of dz, and the trainer must be within max(4 d_ref, one 16-bit ulp) of the fp64 run, per tensor."""
    pol, sd = trainer_1x
    d = _batch(pol)
    b, t = d["b"], d["t"]
    m = b * t
    tr = PPOTrainer(pol, optimizer_state=False, normalize_advantages=False, update_value_normalizer=False, **COEF)
    _, grads, _ = _call(tr.loss_and_grads, pol, d, prior_lp=(d["qb"], d["qc"]))
    that = pol.value_head.normalizer.normalize(d["target"].reshape(m, 1)).reshape(m)
    runs = {}
    for dt in (torch.float32, torch.float64):
        pol.zero_grad(set_to_none=True)
        (pd, vpred, _), _ = pol({"img": d["img"]}, d["first"], pol.initial_state(b))
        assert pd["buttons"].requires_grad and vpred.requires_grad
        loss = R.torch_loss(pd["buttons"].reshape(m, NB).to(dt), pd["camera"].reshape(m, NC).to(dt), d["qb"].to(dt), d["qc"].to(dt),
                            d["ab"].reshape(m), d["ac"].reshape(m), d["old"].reshape(m).to(dt), d["adv"].reshape(m).to(dt), vpred.reshape(m).to(dt),
                            that.to(dt), torch.ones(m, dtype=dt, device=DEV), clip=0.2, **COEF)
        loss.backward()
        runs[dt] = {n: p.grad.detach().clone() for n, p in pol.named_parameters() if p.grad is not None}
    pol.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
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
        print(f"PPO grads [{pol.precision}] {n}: trainer vs fp64-loss boundary rel-L2 {d_tr:.3e}, d_ref (fp32 vs fp64 loss) {d_ref:.3e}")
    print(f"PPO grads [{pol.precision}] largest d_ref {max(r[1] for r in rows):.3e}, largest trainer distance {rows[0][2]:.3e}, floor {floor:.3e}, {len(rows)} tensors")
    assert len(rows) >= 120
    bad = [(n, d_ref, d_tr) for n, d_ref, d_tr in rows if not d_tr <= max(4 * d_ref, floor)]
    assert not bad, bad[:4]


def test_steps_on_a_fixed_batch_behave(trainer_1x):
    """(h)  Six steps, lr 1e-4, no weight decay: with positive advantages and value_coef = 0.5 the mean log-prob of the taken actions rises and the
    value loss falls; with the prior's log-probs taken from the initial weights, kl_coef = 1 ends nearer the prior than kl_coef = 0."""
    pol, sd = trainer_1x
    d = dict(_batch(pol, 2, 4))
    b = d["b"]
    d["adv"] = d["adv"].abs()
    d["old"] = d["lp0"].clone()
    # Where the value targets sit.  Adam's first steps move EVERY weight by about lr whatever its gradient's size, all in the direction that lowers the
    # loss.  Through one 1024-wide layer in front of the heads that shifts each of the 1024 latent inputs by about lr x sum|x| ~ 1e-4 x 1024 x 0.8 = 0.08,
    # and the raw value by sum|w_v| x 0.08 ~ 32 x 0.08 = 2.6 normalised units per step and layer (|w_v| = 1: an orthogonal row).  Measured with targets
    # one unit away: |v - t^| went 1.4 -> 4.3 -> 8.6 and back, the value loss 2.1 -> 18.7 -> 73.8 -> 3.7 -> 14.1 -> 3.0.  A target within a few units
    # of the prediction is overshot at this lr (the step size this test is specified at) by ANY correct gradient; "falls" says something about the descent direction
    # only for targets that six such steps cannot cross: they sit 30 normalised units away.
    mean, var = pol.value_head.normalizer.running_mean_var()
    d["target"] = (mean.reshape(-1)[0] + torch.sqrt(var).reshape(-1)[0] * (30.0 + d["target"])).float()
    final_kl, traces = {}, {}
    try:
        for kl in (0.0, 1.0):
            pol.load_state_dict(sd)
            tr = PPOTrainer(pol, lr=1e-4, weight_decay=0.0, kl_coef=kl, value_coef=0.5, normalize_advantages=False)
            qb, qc, _ = tr.prior_logprobs(pol, d["img"], d["first"], pol.initial_state(b))
            prior = (qb.clone(), qc.clone())
            lps, vls = [], []
            for _ in range(6):
                met = {}
                loss, _ = _call(tr.step, pol, d, prior_lp=prior, metrics=met)
                lps.append(float(met["frame_out"][..., 8].mean()))
                vls.append(float(met["value_loss"]))
            assert tr.step_count == 6 and tr.skipped_steps == 0
            met, _ = _call(tr.evaluate, pol, d, prior_lp=prior)
            final_kl[kl] = float(met["kl_buttons"] + met["kl_camera"])
            traces[kl] = (lps, vls)
        torch.cuda.synchronize()
    finally:
        pol.load_state_dict(sd)
    lps, vls = traces[0.0]
    print(f"PPO steps [{pol.precision}] mean lp of the taken actions {[round(x, 3) for x in lps]}, value loss {[round(x, 4) for x in vls]}, "
          f"final KL to the prior: kl_coef 0 -> {final_kl[0.0]:.4e}, kl_coef 1 -> {final_kl[1.0]:.4e}")
    assert lps[-1] > lps[0] and vls[-1] < vls[0]
    assert final_kl[1.0] < final_kl[0.0]


def test_fp16_huge_advantage_skips_the_step_on_the_device():
    """(h, fp16)  An advantage far beyond IEEE half's range overflows dz: vpt_grads_nonfinite_multi flags it, the Adam launch leaves every tensor
    untouched, the step count stays, the loss scale halves; the same trainer then trains on the sane batch."""
    pol = _policy("fp16")
    d = dict(_batch(pol, 2, 4))
    tr = PPOTrainer(pol, lr=1e-4, weight_decay=0.0, normalize_advantages=False, **COEF)
    before = {k: v.detach().clone() for k, v in pol.named_parameters()}
    huge = d["adv"].clone()
    huge[0, 1] = 1e30
    prior = (d["qb"], d["qc"])
    bad = dict(d, adv=huge)
    _call(tr.step, pol, bad, prior_lp=prior)
    torch.cuda.synchronize()
    assert tr.skipped_steps == 1 and tr.step_count == 0 and tr.loss_scale == 128.0
    assert all(torch.equal(v.detach(), before[k]) for k, v in pol.named_parameters() if "normalizer" not in k)
    assert all(float(x.abs().max()) == 0.0 for x in tr.m.values()) and all(float(x.abs().max()) == 0.0 for x in tr.v.values())
    loss, _ = _call(tr.step, pol, d, prior_lp=prior)
    torch.cuda.synchronize()
    assert tr.skipped_steps == 1 and tr.step_count == 1 and loss == loss
    moved = sum(int(not torch.equal(v.detach(), before[k])) for k, v in pol.named_parameters() if k in tr.m)
    assert moved == len(tr.m)


def test_zero_weight_padding_and_checkpoint(trainer_1x):
    """(i)  frame_weight with a zero-padded tail: replacing the padded frames' images, actions, log-probs, advantages and targets (NaN included)
    changes no bit of the gradients or of the loss.  state_dict round-trips step_count and the moments, the value head's among them."""
    pol, sd = trainer_1x
    d = dict(_batch(pol, 2, 6))
    b, t = d["b"], d["t"]
    w = torch.ones(b, t, device=DEV)
    w[1, 4:] = 0.0
    w[0, 2] = 0.5
    tr = PPOTrainer(pol, lr=1e-4, weight_decay=0.0, update_value_normalizer=False, **COEF)
    prior = (d["qb"], d["qc"])
    loss_a, ga, _ = _call(tr.loss_and_grads, pol, d, prior_lp=prior, frame_weight=w)
    e = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}
    g = torch.Generator().manual_seed(99)
    e["img"][1, 4:] = torch.randint(0, 256, (2, 128, 128, 3), generator=g, dtype=torch.uint8).to(DEV)
    e["ab"][1, 4:], e["ac"][1, 4:] = 0, NC - 1
    for k in ("old", "adv", "target"):
        e[k][1, 4:] = float("nan")
    qb, qc = d["qb"].clone(), d["qc"].clone()
    qb[t + 4:], qc[t + 4:] = float("nan"), float("nan")
    loss_b, gb, _ = _call(tr.loss_and_grads, pol, e, prior_lp=(qb, qc), frame_weight=w)
    torch.cuda.synchronize()
    assert torch.equal(loss_a, loss_b) and bool(torch.isfinite(loss_a))
    assert all(bool(torch.isfinite(v).all()) for v in ga.values())
    assert not [k for k in ga if not torch.equal(ga[k], gb[k])]
    with pytest.raises(ValueError, match="frame_weight"):
        _call(tr.loss_and_grads, pol, d, prior_lp=prior, frame_weight=-w)
    try:
        for _ in range(2):
            _call(tr.step, pol, d, prior_lp=prior, frame_weight=w)
        state = tr.state_dict()
        assert state["step"] == 2 and "value_head.linear.weight" in state["exp_avg"] and float(state["exp_avg"]["value_head.linear.weight"].abs().max()) > 0
        tr2 = PPOTrainer(pol, lr=1.0, **COEF)
        tr2.load_state_dict(state)
        assert tr2.step_count == 2 and tr2.lr == 1e-4
        assert all(torch.equal(tr2.m[k], tr.m[k]) and torch.equal(tr2.v[k], tr.v[k]) for k in tr.m)
    finally:
        pol.load_state_dict(sd)
