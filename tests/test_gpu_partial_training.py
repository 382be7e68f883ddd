"""Partial fine-tuning on the GPU: trainable= / param_groups= / decoupled_weight_decay= of BCTrainer, PPOTrainer and IDMTrainer.
A subset's gradients are the full run's tensors bit for bit, the backward launches nothing below its cut and no wgrad / bias sum for a frozen
tensor, the saving forward keeps nothing the shortened backward does not read, step() moves the trainable tensors only, and parameter groups are
the hand-run sequence of two ops.adam_step_multi_ launches.  1x policy (temperature 2) and the tiny IDM of tests/labeler_ref.py, B = 2, T = 4,
both operand formats.  Needs an MI355X."""
import collections
import copy

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
B, T = 2, 4
INF = float("inf")
HEADS = ("pi_head.buttons.linear_layer.weight", "pi_head.buttons.linear_layer.bias", "pi_head.camera.linear_layer.weight", "pi_head.camera.linear_layer.bias")


def _policy(precision):
    pk = O.policy_kwargs_for("1x")
    cfg = O.config_from_policy_kwargs(pk, dict(temperature=2.0))
    sd = O.synthetic_state_dict(cfg, seed=0)
    pol = MinecraftAgentPolicy(minecraft_action_space(), pk, dict(temperature=2.0), precision=precision)
    pol.load_state_dict(sd, strict=False)
    return pol.to(DEV)


def _batch():
    g = torch.Generator().manual_seed(29)
    img = torch.randint(0, 256, (B, T, 128, 128, 3), generator=g, dtype=torch.uint8).to(DEV)
    first = torch.zeros(B, T, dtype=torch.bool, device=DEV)
    return img, first, torch.randint(0, NB, (B, T), generator=g).to(DEV), torch.randint(0, NC, (B, T), generator=g).to(DEV)


def _args(pol, batch):
    img, first, ab, ac = batch
    return img, first, pol.initial_state(B), ab, ac


def _subsets(pol):
    n = pol._cfg["n_layers"]
    s2 = ["net.lastlayer", "net.final_ln", "pi_head"]
    behind_cnn = BCTrainer.rule_trainable(dict(pol.named_parameters()), False)
    return dict(S1=["pi_head"], S2=s2, S3=s2 + [f"net.recurrent_layer.blocks.{n - 1}"], S4=[x for x in behind_cnn if x.endswith(".bias")])


def _flat_state(state):
    return [t for m, (k, v) in state for t in (m, k, v) if t is not None]


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def ctx(request):
    """The policy, its start weights, the batch and -- computed once, never modified -- the full trainer's loss, gradients and state_out on it
    (train_cnn=False: the subsets below live behind the CNN)."""
    pol = _policy(request.param)
    sd = copy.deepcopy(pol.state_dict())
    batch = _batch()
    full = BCTrainer(pol, train_cnn=False, optimizer_state=False)
    loss, g, state_out = full.loss_and_grads(*_args(pol, batch))
    torch.cuda.synchronize()
    return dict(pol=pol, sd=sd, batch=batch, full=full, loss=loss.clone(), g={k: v.clone() for k, v in g.items()}, state_out=state_out,
                subsets=_subsets(pol))


def _backward_counts(tr, pol, batch, **kw):
    """Records of ops.TIMER by entry-point name around backward_from ONLY (the forward and the loss gradient run before it is switched on)."""
    img, first, ab, ac = batch
    S = tr.forward_saving(img, first, pol.initial_state(B))
    m = S["m"]
    scale = (tr.loss_scale if tr.scaled else 1.0 / m) / pol._cfg["temperature"]
    dz = ops.nll_backward(S["lp_b"], S["lp_c"], ab.reshape(m).contiguous(), ac.reshape(m).contiguous(), S["ldz"], scale, dtype=tr.dtype)
    ops.TIMER.reset()
    ops.TIMER.enabled = True
    try:
        g = tr.backward_from(S, dz, **kw)
        torch.cuda.synchronize()
    finally:
        ops.TIMER.enabled = False
    counts = collections.Counter(rec[0] for rec in ops.TIMER.records)
    ops.TIMER.reset()
    return g, counts


def _attention_backwards(counts):
    return sum(v for k, v in counts.items() if k.startswith("vpt_masked_attention_backward"))


@pytest.mark.parametrize("which", ["S1", "S2", "S3", "S4"])
def test_subset_gradients_are_the_full_runs_tensors(ctx, which):
    """(f) set(g) is the effective set; every g[name] is torch.equal to the full trainer's gradient on the same batch; loss and state_out too."""
    pol, sel = ctx["pol"], ctx["subsets"][which]
    tr = BCTrainer(pol, train_cnn=False, optimizer_state=False, trainable=sel)
    expect = [n for n in ctx["full"].trainable if any(n == s or n.startswith(s + ".") for s in sel)]
    assert tr.trainable == expect and len(expect) >= (4 if which == "S1" else 9)
    assert not tr.m and not tr.v
    loss, g, state_out = tr.loss_and_grads(*_args(pol, ctx["batch"]))
    torch.cuda.synchronize()
    assert set(g) == set(expect)
    bad = [n for n in expect if not torch.equal(g[n], ctx["g"][n])]
    assert not bad, bad[:4]
    assert torch.equal(loss, ctx["loss"])
    assert all(torch.equal(a, b) for a, b in zip(_flat_state(state_out), _flat_state(ctx["state_out"])))
    assert all(float(g[n].abs().max()) > 0 for n in expect if n.startswith(("pi_head.", "net.final_ln.")) or n.endswith("mlp1.layer.bias"))


def test_backward_launches_stop_at_the_cut(ctx):
    """(g) launch counts around backward_from: S1 one linear wgrad and no LayerNorm backward, attention backward or dgrad GEMM; S3 exactly one
    masked-attention backward; S4 (biases only) no linear wgrad; the full set spelled out as a selection launches what a default trainer does."""
    pol, batch, sub = ctx["pol"], ctx["batch"], ctx["subsets"]
    g1, c1 = _backward_counts(BCTrainer(pol, train_cnn=False, optimizer_state=False, trainable=sub["S1"]), pol, batch)
    assert c1["vpt_linear_wgrad"] == 1 and c1["vpt_layernorm_backward"] == 0 and _attention_backwards(c1) == 0 and c1["vpt_linear_forward"] == 0, c1
    assert c1["vpt_column_sum"] == 1 and set(g1) == set(HEADS)
    _, c3 = _backward_counts(BCTrainer(pol, train_cnn=False, optimizer_state=False, trainable=sub["S3"]), pol, batch)
    assert _attention_backwards(c3) == 1, c3
    _, c4 = _backward_counts(BCTrainer(pol, train_cnn=False, optimizer_state=False, trainable=sub["S4"]), pol, batch)
    assert c4["vpt_linear_wgrad"] == 0 and c4["vpt_column_sum"] > 0 and c4["vpt_layernorm_backward"] > 0, c4
    default = BCTrainer(pol, train_cnn=False, optimizer_state=False)
    gd, cd = _backward_counts(default, pol, batch)
    ga, ca = _backward_counts(BCTrainer(pol, train_cnn=False, optimizer_state=False, trainable=list(default.trainable)), pol, batch)
    assert ca == cd and cd["vpt_linear_wgrad"] > c3["vpt_linear_wgrad"] > 1
    assert _attention_backwards(cd) == pol._cfg["n_layers"]
    assert set(ga) == set(default.trainable) and all(torch.equal(ga[n], gd[n]) for n in default.trainable)
    # the cut shows in the counts: S3 walks one block, the default walks them all
    assert c3["vpt_layernorm_backward"] < cd["vpt_layernorm_backward"] and c3["vpt_linear_forward"] < cd["vpt_linear_forward"]


def test_heads_only_keeps_no_block_and_moves_only_the_heads(ctx):
    """(h) under S1 the saving forward keeps no block (nor the inputs of the units below the cut); step() leaves every frozen parameter as it was,
    changes every trainable one, and those equal a full trainer's after the same step.  With train_cnn=True and no CNN tensor selected the CNN's
    saving forward still runs (the loss is the train_cnn=True trainer's, bit for bit) and none of its activations are kept."""
    pol, sd, batch = ctx["pol"], ctx["sd"], ctx["batch"]
    try:
        tr = BCTrainer(pol, train_cnn=False, trainable=["pi_head"])
        assert set(tr.m) == set(tr.v) == set(HEADS) == set(tr.trainable)
        img, first = batch[:2]
        S = tr.forward_saving(img, first, pol.initial_state(B))
        assert len(S["saved"]) == pol._cfg["n_layers"] and all(s is None for s in S["saved"])
        assert all(S[k] is None for k in ("dn", "x_lin16", "x_pre", "d", "xb", "y", "y16")) and S["lb"] is not None
        del S
        before = {k: v.detach().clone() for k, v in pol.named_parameters()}
        loss, _ = tr.step(*_args(pol, batch))
        after = {k: v.detach().clone() for k, v in pol.named_parameters()}
        pol.load_state_dict(sd)
        full = BCTrainer(pol, train_cnn=False)
        loss_full, _ = full.step(*_args(pol, batch))
        torch.cuda.synchronize()
        assert loss == loss_full == float(ctx["loss"])
        for k in before:
            if k in HEADS:
                assert not torch.equal(after[k], before[k]), k
                assert torch.equal(after[k], pol.get_parameter(k).detach()), k
                assert torch.equal(tr.m[k], full.m[k]) and torch.equal(tr.v[k], full.v[k]), k
            else:
                assert torch.equal(after[k], before[k]), k
        assert tr.step_count == 1 and tr.skipped_steps == 0
        pol.load_state_dict(sd)
        whole = BCTrainer(pol, train_cnn=True, optimizer_state=False)
        loss_w, g_w, _ = whole.loss_and_grads(*_args(pol, batch))
        heads = BCTrainer(pol, train_cnn=True, optimizer_state=False, trainable=["pi_head"])
        S = heads.forward_saving(img, first, pol.initial_state(B))
        assert S["cnn_saved"] == []
        loss_h, g_h, _ = heads.loss_and_grads(*_args(pol, batch))
        torch.cuda.synchronize()
        assert torch.equal(loss_h, loss_w) and set(g_h) == set(HEADS) and all(torch.equal(g_h[n], g_w[n]) for n in HEADS)
    finally:
        pol.load_state_dict(sd)


def test_a_callable_that_accepts_everything_is_the_default_set(ctx):
    """(i) trainable=lambda n: True and trainable=None: the same names, torch.equal gradients for the trunk and the heads."""
    pol = ctx["pol"]
    tr = BCTrainer(pol, train_cnn=False, optimizer_state=False, trainable=lambda n: True)
    assert tr.trainable == ctx["full"].trainable
    _, g, _ = tr.loss_and_grads(*_args(pol, ctx["batch"]))
    torch.cuda.synchronize()
    assert set(g) == set(ctx["g"]) and all(torch.equal(g[n], ctx["g"][n]) for n in g)
    picky = BCTrainer(pol, train_cnn=False, optimizer_state=False, trainable=lambda n: n.endswith("mlp1.layer.weight"))
    assert picky.trainable == [f"net.recurrent_layer.blocks.{l}.mlp1.layer.weight" for l in range(pol._cfg["n_layers"])]


def _snapshot(pol, tr):
    return ({k: v.detach().clone() for k, v in pol.named_parameters()}, {k: v.clone() for k, v in tr.m.items()}, {k: v.clone() for k, v in tr.v.items()})


def _same(a, b):
    return [k for part_a, part_b in zip(a, b) for k in part_a if not torch.equal(part_a[k], part_b[k])]


@pytest.mark.parametrize("decoupled", [False, True])
def test_param_groups_step_is_two_adam_launches(ctx, decoupled):
    """(j) the heads at lr_scale=0.1, weight_decay=0 and the rest at the trainer's values: one step() is loss_and_grads followed by two
    ops.adam_step_multi_ launches, bit for bit -- parameters and both moments.  decoupled_weight_decay=True changes the decayed group only (the heads
    carry no decay), and a host schedule that assigns trainer.lr reaches both groups."""
    pol, sd, batch = ctx["pol"], ctx["sd"], ctx["batch"]
    m = B * T
    try:
        tr_h = BCTrainer(pol, train_cnn=False)
        _, grads, _ = tr_h.loss_and_grads(*_args(pol, batch), unscaled=False)
        names = [n for n in tr_h.trainable if n in grads]
        for pick, lr, wd in ((lambda n: n in HEADS, tr_h.lr * 0.1, 0.0), (lambda n: n not in HEADS, tr_h.lr, tr_h.wd)):
            ns = [n for n in names if pick(n)]
            ops.adam_step_multi_([tr_h.params[n].data.view(-1) for n in ns], [grads[n].contiguous().view(-1) for n in ns], [tr_h.m[n].view(-1) for n in ns],
                                 [tr_h.v[n].view(-1) for n in ns], 1, lr=lr, beta1=tr_h.betas[0], beta2=tr_h.betas[1], eps=tr_h.eps, weight_decay=wd,
                                 grad_scale=tr_h.grad_unscale(m))
        hand = _snapshot(pol, tr_h)
        pol.load_state_dict(sd)
        tr = BCTrainer(pol, train_cnn=False, param_groups=[dict(params=["pi_head"], lr_scale=0.1, weight_decay=0.0)], decoupled_weight_decay=decoupled)
        tr.step(*_args(pol, batch))
        got = _snapshot(pol, tr)
        torch.cuda.synchronize()
        diff = _same(got, hand)
        if not decoupled:
            assert not diff, diff[:4]
        else:       # the heads (wd = 0: the factor is exactly 1) still match; every decayed tensor's parameter differs, AdamW's moments do not see the decay
            assert not [k for k in diff if k in HEADS]
            assert all(not torch.equal(got[0][k], hand[0][k]) for k in names if k not in HEADS and float(sd[k].abs().max()) > 0)
        tr.lr = tr.lr * 0.5      # a host schedule: lr_scale multiplies the lr of the step
        before = {k: v.clone() for k, v in got[0].items()}
        tr.step(*_args(pol, batch))
        torch.cuda.synchronize()
        assert tr.step_count == 2 and all(not torch.equal(pol.get_parameter(k).detach(), before[k]) for k in HEADS)
    finally:
        pol.load_state_dict(sd)


def test_norm_and_accumulation_run_over_the_subset(ctx):
    """(k) max_grad_norm=inf under S2: last_grad_norm is ops.grad_norm over S2's gradients (clip_grad_norm_(trainable_parameters)).
    micro_batches=2 under S3 equals the full trainer's micro_batches=2 step on S3's parameters."""
    pol, sd, batch, sub = ctx["pol"], ctx["sd"], ctx["batch"], ctx["subsets"]
    try:
        tr = BCTrainer(pol, train_cnn=False, trainable=sub["S2"], max_grad_norm=INF)
        met = {}
        tr.step(*_args(pol, batch), metrics=met)
        pol.load_state_dict(sd)
        probe = BCTrainer(pol, train_cnn=False, optimizer_state=False, trainable=sub["S2"])
        _, g, _ = probe.loss_and_grads(*_args(pol, batch), unscaled=True, metrics={})
        norm = ops.grad_norm([g[n].contiguous().view(-1) for n in probe.trainable])
        torch.cuda.synchronize()
        assert torch.equal(tr.last_grad_norm, norm[0]) and list(met["grad_norm_per_tensor"]) == probe.trainable and float(norm[0]) > 0
        full_norm = ops.grad_norm([ctx["g"][n].contiguous().view(-1) for n in ctx["full"].trainable])
        assert float(norm[0]) < float(full_norm[0])
        pol.load_state_dict(sd)
        part = BCTrainer(pol, train_cnn=False, trainable=sub["S3"])
        loss_p, _ = part.step(*_args(pol, batch), micro_batches=2)
        after = {n: pol.get_parameter(n).detach().clone() for n in part.trainable}
        pol.load_state_dict(sd)
        full = BCTrainer(pol, train_cnn=False)
        loss_f, _ = full.step(*_args(pol, batch), micro_batches=2)
        torch.cuda.synchronize()
        assert loss_p == loss_f
        bad = [n for n in part.trainable if not torch.equal(after[n], pol.get_parameter(n).detach())]
        assert not bad, bad[:4]
    finally:
        pol.load_state_dict(sd)


def test_ppo_subset(ctx):
    """(l) PPOTrainer(trainable=["pi_head", "value_head"]): the gradient set, bit-equality to the full run, one step that moves those tensors only."""
    pol, sd, batch = ctx["pol"], ctx["sd"], ctx["batch"]
    img, first, ab, ac = batch
    gen = torch.Generator().manual_seed(31)
    adv = (torch.rand(B, T, generator=gen) - 0.3).to(DEV)
    target = torch.randn(B, T, generator=gen).to(DEV)
    kw = dict(train_cnn=False, normalize_advantages=False, update_value_normalizer=False, entropy_coef=0.01)
    met, _ = PPOTrainer(pol, optimizer_state=False, **kw).evaluate(img, first, pol.initial_state(B), ab, ac, torch.zeros(B, T, device=DEV), adv, target)
    old = met["frame_out"][..., 8].clone() - 0.1
    args = lambda: (img, first, pol.initial_state(B), ab, ac, old, adv, target)
    names = list(HEADS) + ["value_head.linear.weight", "value_head.linear.bias"]
    try:
        loss_f, g_f, _ = PPOTrainer(pol, optimizer_state=False, **kw).loss_and_grads(*args())
        tr = PPOTrainer(pol, trainable=["pi_head", "value_head"], **kw)
        assert set(tr.trainable) == set(names) == set(tr.m)
        loss, g, _ = tr.loss_and_grads(*args())
        torch.cuda.synchronize()
        assert set(g) == set(names) and all(torch.equal(g[n], g_f[n]) for n in names) and torch.equal(torch.as_tensor(loss), torch.as_tensor(loss_f))
        assert float(g["value_head.linear.weight"].abs().max()) > 0
        only_pi = PPOTrainer(pol, optimizer_state=False, trainable=["pi_head"], **kw)
        _, g_pi, _ = only_pi.loss_and_grads(*args())
        assert set(g_pi) == set(HEADS) and all(torch.equal(g_pi[n], g_f[n]) for n in HEADS)
        before = {k: v.detach().clone() for k, v in pol.named_parameters()}
        tr.step(*args())
        torch.cuda.synchronize()
        moved = {k for k, v in pol.named_parameters() if not torch.equal(v.detach(), before[k])}
        assert moved == set(names)
    finally:
        pol.load_state_dict(sd)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_idm_subset(precision):
    """(l) IDMTrainer(trainable=["pi_head"]) on the tiny IDM: the gradient set, bit-equality to the full run, no block kept, one step."""
    kw, cfg, sd = LR.tiny_idm()
    pol = InverseActionPolicy(idm_action_space(), pi_head_kwargs=dict(temperature=LR.TEMPERATURE), idm_net_kwargs=kw, precision=precision)
    pol.load_state_dict(sd, strict=False)
    pol = pol.to(DEV)
    g = torch.Generator().manual_seed(21)
    img = P.structured_frames(B, T, g).to(DEV)
    buttons, camera = torch.randint(0, 2, (B, T, 20), generator=g).to(DEV), torch.randint(0, 11, (B, T, 2), generator=g).to(DEV)
    full = IDMTrainer(pol, optimizer_state=False)
    loss_f, g_f = full.loss_and_grads(img, buttons, camera)
    tr = IDMTrainer(pol, trainable=["pi_head"])
    assert set(tr.trainable) == set(HEADS) == set(tr.m)
    S = tr.forward_saving(img)
    assert all(s is None for s in S["saved"]) and S["d"] is None
    del S
    loss, g_s = tr.loss_and_grads(img, buttons, camera)
    torch.cuda.synchronize()
    assert set(g_s) == set(HEADS) and all(torch.equal(g_s[n], g_f[n]) for n in HEADS) and torch.equal(loss, loss_f)
    last = f"net.recurrent_layer.blocks.{cfg['n_layers'] - 1}"
    blk = IDMTrainer(pol, optimizer_state=False, trainable=[last, "net.final_ln"])
    _, g_b = blk.loss_and_grads(img, buttons, camera)
    assert set(g_b) == set(blk.trainable) and all(torch.equal(g_b[n], g_f[n]) for n in g_b) and len(g_b) > 10
    before = {k: v.detach().clone() for k, v in pol.named_parameters()}
    tr.step(img, buttons, camera)
    torch.cuda.synchronize()
    assert {k for k, v in pol.named_parameters() if not torch.equal(v.detach(), before[k])} == set(HEADS)
    with pytest.raises(ValueError, match="does not train"):
        IDMTrainer(pol, trainable=["net.lastlayer"])
    with pytest.raises(ValueError, match="does not train"):
        IDMTrainer(pol, trainable=["net.img_process.cnn"])


def test_state_dict_round_trip_with_groups(ctx):
    """(m) state_dict carries the names, the groups and the flag; a dict without them leaves the constructor's in place; another subset: KeyError."""
    pol, sub = ctx["pol"], ctx["subsets"]
    groups = [dict(params=["pi_head"], lr_scale=0.1, weight_decay=0.0)]
    tr = BCTrainer(pol, train_cnn=False, trainable=sub["S2"], param_groups=groups, decoupled_weight_decay=True)
    state = tr.state_dict()
    assert state["trainable"] == tr.trainable and state["param_groups"] == groups and state["decoupled_weight_decay"] is True
    assert set(state["exp_avg"]) == set(tr.trainable)
    tr2 = BCTrainer(pol, train_cnn=False, trainable=sub["S2"])
    assert tr2.param_groups == [] and not tr2.decoupled_weight_decay
    tr2.load_state_dict(state)
    assert tr2.param_groups == groups and tr2.decoupled_weight_decay and tr2._group_of == tr._group_of
    plain = BCTrainer(pol, train_cnn=False, trainable=sub["S2"]).state_dict()
    assert "param_groups" not in plain and "trainable" in plain
    tr3 = BCTrainer(pol, train_cnn=False, trainable=sub["S2"], param_groups=groups)
    tr3.load_state_dict(plain)
    assert tr3.param_groups == groups
    assert "trainable" not in BCTrainer(pol, train_cnn=False).state_dict()
    with pytest.raises(KeyError, match="optimizer state does not match the trainable parameters"):
        BCTrainer(pol, train_cnn=False, trainable=sub["S1"]).load_state_dict(state)
    with pytest.raises(KeyError, match="optimizer state does not match the trainable parameters"):
        BCTrainer(pol, train_cnn=False).load_state_dict(state)


def test_every_refusal(ctx):
    """(n) the ValueErrors of trainable= and param_groups=, each naming its offenders."""
    pol = ctx["pol"]
    kw = dict(train_cnn=False, optimizer_state=False)
    with pytest.raises(ValueError, match=r"\['pi_heads'\] match no parameter"):
        BCTrainer(pol, trainable=["pi_heads"], **kw)
    with pytest.raises(ValueError, match="match no parameter"):
        BCTrainer(pol, trainable=["net.recurrent_layer.blocks.9"], **kw)
    with pytest.raises(ValueError, match="leaves no trainable parameter"):
        BCTrainer(pol, trainable=lambda n: False, **kw)
    with pytest.raises(ValueError, match="leaves no trainable parameter"):
        BCTrainer(pol, trainable=[], **kw)
    with pytest.raises(ValueError, match=r"does not train \['value_head\.linear\.weight'"):
        BCTrainer(pol, trainable=["pi_head", "value_head"], **kw)
    with pytest.raises(ValueError, match=r"does not train \['net\.img_process\.cnn\."):
        BCTrainer(pol, trainable=["net.img_process.cnn"], **kw)
    assert BCTrainer(pol, trainable=["net.img_process.cnn.dense"], optimizer_state=False).trainable[0].startswith("net.img_process.cnn.dense.")
    with pytest.raises(ValueError, match="are in group 0 and in group 1"):
        BCTrainer(pol, param_groups=[dict(params=["pi_head"]), dict(params=["pi_head.camera"], lr_scale=2.0)], **kw)
    with pytest.raises(ValueError, match="not trainable"):
        BCTrainer(pol, trainable=["pi_head"], param_groups=[dict(params=["net.final_ln"])], **kw)
    with pytest.raises(ValueError, match="not trainable"):
        BCTrainer(pol, param_groups=[dict(params=["value_head"])], **kw)
    with pytest.raises(ValueError, match="match no parameter"):
        BCTrainer(pol, param_groups=[dict(params=["nothing.here"])], **kw)
    with pytest.raises(ValueError, match="must be dict"):
        BCTrainer(pol, param_groups=[dict(params=["pi_head"], lr=1e-3)], **kw)
    with pytest.raises(ValueError, match="finite and non-negative"):
        BCTrainer(pol, param_groups=[dict(params=["pi_head"], lr_scale=-1.0)], **kw)
