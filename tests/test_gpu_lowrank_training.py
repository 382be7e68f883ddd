"""Low-rank adapters in the trainers on an MI355X: BCTrainer / PPOTrainer / IDMTrainer with adapters=, both operand formats.
1x policy (temperature 2) and the tiny IDM of tests/labeler_ref.py, B = 2, T = 4.

(a) fresh adapters (B = 0) are the adapter-less trainer bit for bit, every dA is exact zeros, every dB lies within tests/lowrank_ref.py's bound of
s dW A16^T (dW: the parent path's dense gradient of that weight);  (b) A = 0, random B: the same forward, dB exact zeros, dA within the bound of
s B^T dW;  (c) both nonzero: log-probs against the fp32 oracle on the merged weights, gradients against the dense projection on the merged policy;
(d) six steps: the loss falls, nothing outside the selection moves, the launches, micro-batches, the state-dict round trip;  (e) merge_ / unmerge_
and the acting path;  (f) PPOTrainer with the policy itself as the prior, IDMTrainer;  (g) the refusals."""
import collections
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from vpt_amd.adapters import LowRankAdapters  # noqa: E402
from vpt_amd.idm_training import IDMTrainer  # noqa: E402
from vpt_amd.rl_training import PPOTrainer  # noqa: E402
from vpt_amd.training import BCTrainer  # noqa: E402
from vpt_amd.lib.policy import InverseActionPolicy, MinecraftAgentPolicy  # noqa: E402
from vpt_amd.lib.types import idm_action_space, minecraft_action_space  # noqa: E402
from oracle import vpt_oracle as O  # noqa: E402
from tests import labeler_ref as LR  # noqa: E402
from tests import lowrank_ref as R  # noqa: E402
from tests import parity as P  # noqa: E402

DEV = "cuda"
D = torch.float64
NB, NC = 8641, 121
B, T = 2, 4
BLK = "net.recurrent_layer.blocks."
TARGETS = (BLK + "1", BLK + "2", BLK + "3")          # block 0 stays plain: a capture trainer can then cut below every adapted block
RANK, ALPHA = 8, 16.0
HEADS = ("pi_head.buttons.linear_layer.weight", "pi_head.buttons.linear_layer.bias", "pi_head.camera.linear_layer.weight", "pi_head.camera.linear_layer.bias")


def _policy(precision, sd=None):
    pk = O.policy_kwargs_for("1x")
    cfg = O.config_from_policy_kwargs(pk, dict(temperature=2.0))
    pol = MinecraftAgentPolicy(minecraft_action_space(), pk, dict(temperature=2.0), precision=precision)
    pol.load_state_dict(O.synthetic_state_dict(cfg, seed=0) if sd is None else sd, strict=sd is not None)
    return pol.to(DEV), cfg


def _batch():
    g = torch.Generator().manual_seed(29)
    img = P.structured_frames(B, T, g)
    first = torch.zeros(B, T, dtype=torch.bool)
    return img.to(DEV), first.to(DEV), torch.randint(0, NB, (B, T), generator=g).to(DEV), torch.randint(0, NC, (B, T), generator=g).to(DEV)


def _flat_state(state):
    return [t for m, (k, v) in state for t in (m, k, v) if t is not None]


def _run(tr, pol, batch, debug=None):
    """forward_saving + the BC loss gradient + backward_from -> (S, g): the raw (in fp16 loss-scaled) gradients, the same scale in every trainer."""
    img, first, ab, ac = batch
    S = tr.forward_saving(img, first, pol.initial_state(B))
    m = S["m"]
    scale = (tr.loss_scale if tr.scaled else 1.0 / m) / pol._cfg["temperature"]
    dz = ops.nll_backward(S["lp_b"], S["lp_c"], ab.reshape(m).contiguous(), ac.reshape(m).contiguous(), S["ldz"], scale, dtype=tr.dtype)
    g = tr.backward_from(S, dz, debug=debug)
    torch.cuda.synchronize()
    return S, g


def _randomise(ad, which, std, seed):
    g = torch.Generator().manual_seed(seed)
    for n, t in ad.params.items():
        if n.endswith(which):
            t.copy_((torch.randn(t.shape, generator=g) * std).to(DEV))


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def ctx(request):
    """The policy, its start weights, the batch and -- computed once, never modified -- the adapter-less trainer's forward and head gradients and the
    parent path's dense gradient of every weight the adapters sit on."""
    mode = request.param
    pol, cfg = _policy(mode)
    sd = copy.deepcopy(pol.state_dict())
    batch = _batch()
    plain = BCTrainer(pol, train_cnn=False, optimizer_state=False, trainable=("pi_head",))
    S, g = _run(plain, pol, batch)
    ad = LowRankAdapters(pol, targets=TARGETS, rank=RANK, alpha=ALPHA, seed=0)
    dense = BCTrainer(pol, train_cnn=False, optimizer_state=False, trainable=ad.adapted_weights)
    _, dw = _run(dense, pol, batch)
    return dict(mode=mode, pol=pol, cfg=cfg, sd=sd, batch=batch, lp_b=S["lp_b"].clone(), lp_c=S["lp_c"].clone(), state_out=S["state_out"],
                g={k: v.clone() for k, v in g.items()}, dw={k: v.clone() for k, v in dw.items()})


def _operands_of(S, dbg, module, hid):
    """(dy16, x16) of one adapted module from a capture run: the 16-bit gradient entering its GEMM and the 16-bit activation it read."""
    l = int(module[len(BLK):].split(".")[0])
    s = S["saved"][l]
    leaf = module.split(".", 4)[4]
    if leaf == "mlp1.layer":
        return dbg[f"dout16_{l}"], s["h2"]
    if leaf == "mlp0.layer":
        return dbg[f"dh16_{l}"], s["hb"]
    if leaf == "r.orc_block.proj_layer":
        return dbg[f"dx2_16_{l}"], s["att"]
    i = "qkvr".index(leaf[len("r.orc_block.")])
    return dbg[f"dq16_{l}"][:, i * hid:(i + 1) * hid], s["x1b"]


def _forward_is_plain(ctx, S):
    assert torch.equal(S["lp_b"], ctx["lp_b"]) and torch.equal(S["lp_c"], ctx["lp_c"])
    loss = -(S["lp_b"].gather(1, ctx["batch"][2].reshape(-1, 1)) + S["lp_c"].gather(1, ctx["batch"][3].reshape(-1, 1))).mean()
    ref = -(ctx["lp_b"].gather(1, ctx["batch"][2].reshape(-1, 1)) + ctx["lp_c"].gather(1, ctx["batch"][3].reshape(-1, 1))).mean()
    assert torch.equal(loss, ref)
    assert all(torch.equal(a, b) for a, b in zip(_flat_state(S["state_out"]), _flat_state(ctx["state_out"])))


def _capture(ctx, ad):
    """A trainer whose cut lies below every adapted block (block 0's mlp1 bias trains too), so the walk stores every adapted GEMM's operands."""
    pol = ctx["pol"]
    cap = BCTrainer(pol, train_cnn=False, optimizer_state=False, adapters=ad, trainable=("pi_head", BLK + "0.mlp1.layer.bias"))
    dbg: dict = {}
    S, g = _run(cap, pol, ctx["batch"], debug=dbg)
    return S, g, dbg


def test_fresh_adapters_are_the_plain_trainer_and_db_is_the_projected_dense_gradient(ctx):
    """(a)"""
    pol, mode, hid = ctx["pol"], ctx["mode"], ctx["cfg"]["hidsize"]
    ad = LowRankAdapters(pol, targets=TARGETS, rank=RANK, alpha=ALPHA, seed=0)
    tr = BCTrainer(pol, train_cnn=False, optimizer_state=False, adapters=ad, trainable=("pi_head",))
    assert set(tr.trainable[:4]) == set(HEADS) and tr.trainable[4:] == list(ad.params) and tr._cut == 3
    S, g = _run(tr, pol, ctx["batch"])
    _forward_is_plain(ctx, S)
    assert set(g) == set(tr.trainable)
    assert all(torch.equal(g[n], ctx["g"][n]) for n in HEADS)
    assert all(not bool(g[m + ".lora_A"].any()) for m in ad.modules), "B = 0: every dA is exact zeros"
    Sc, gc, dbg = _capture(ctx, ad)
    assert all(torch.equal(gc[n], g[n]) for n in g)
    fails, worst = [], 0.0
    for m in ad.modules:
        dy16, x16 = _operands_of(Sc, dbg, m, hid)
        n = ad.shapes[m][0]
        a16 = R.rnd16(ad.pair(m)[0].cpu(), mode)
        u64, du = R.stage_one(x16.cpu().to(D), a16, 1, mode)
        db64, bnd = R.db_ref(dy16.cpu(), u64, du, n, s=ad.scale)
        # the reference the issue names: s dW A16^T with the parent path's fp32 dW, itself within linear_ref.bound(|dy|^T |x|, M) of dy^T x
        dw = ctx["dw"][m + ".weight"].cpu().to(D)
        ref = ad.scale * dw @ a16.t()
        bnd = bnd + ad.scale * R.bound(dy16.cpu().to(D)[:, :n].abs().t() @ x16.cpu().to(D).abs(), x16.shape[0]) @ a16.abs().t()
        w_, msg = R.bound_ratio(g[m + ".lora_B"].cpu(), ref, bnd)
        worst = max(worst, w_)
        if msg:
            fails.append(f"{m}.lora_B: {msg}")
        assert float(g[m + ".lora_B"].abs().max()) > 0
    print(f"(a) {mode}: worst |dB - s dW A^T| / bound = {worst:.3f}")
    assert not fails, "\n".join(fails[:6])


def test_zero_a_keeps_the_forward_and_da_is_the_projected_dense_gradient(ctx):
    """(b)"""
    pol, mode, hid = ctx["pol"], ctx["mode"], ctx["cfg"]["hidsize"]
    ad = LowRankAdapters(pol, targets=TARGETS, rank=RANK, alpha=ALPHA, seed=0)
    for n, t in ad.params.items():
        if n.endswith(".lora_A"):
            t.zero_()
    _randomise(ad, ".lora_B", 0.05, 7)
    tr = BCTrainer(pol, train_cnn=False, optimizer_state=False, adapters=ad, trainable=("pi_head",))
    S, g = _run(tr, pol, ctx["batch"])
    _forward_is_plain(ctx, S)
    assert all(torch.equal(g[n], ctx["g"][n]) for n in HEADS)
    assert all(not bool(g[m + ".lora_B"].any()) for m in ad.modules), "A = 0: u16 = 0 and every dB is exact zeros"
    Sc, gc, dbg = _capture(ctx, ad)
    fails, worst = [], 0.0
    for m in ad.modules:
        dy16, x16 = _operands_of(Sc, dbg, m, hid)
        n = ad.shapes[m][0]
        sb16 = R.rnd16(ad.pair(m)[1].cpu() * ad.scale, mode)                        # [n, r]: the packed operand s B
        dy, x = dy16.cpu().to(D)[:, :n], x16.cpu().to(D)
        du64, ddu = R.stage_one(dy, sb16.t(), 1, mode)                              # du = dy (sB)
        da64, bnd = R.da_ref(du64, ddu, x)
        dw = ctx["dw"][m + ".weight"].cpu().to(D)
        ref = sb16.t() @ dw                                                        # s B^T dW
        bnd = bnd + sb16.abs().t() @ R.bound(dy.abs().t() @ x.abs(), x.shape[0])
        w_, msg = R.bound_ratio(g[m + ".lora_A"].cpu(), ref, bnd)
        worst = max(worst, w_)
        if msg:
            fails.append(f"{m}.lora_A: {msg}")
        assert float(g[m + ".lora_A"].abs().max()) > 0
    print(f"(b) {mode}: worst |dA - s B^T dW| / bound = {worst:.3f}")
    assert not fails, "\n".join(fails[:6])


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm()).clamp(min=1e-300))


def test_both_nonzero_against_the_oracle_on_the_merged_weights(ctx):
    """(c)"""
    pol, mode, cfg = ctx["pol"], ctx["mode"], ctx["cfg"]
    img, first, ab, ac = ctx["batch"]
    ad = LowRankAdapters(pol, targets=TARGETS, rank=RANK, alpha=ALPHA, seed=0)
    _randomise(ad, ".lora_B", 0.05, 11)
    tr = BCTrainer(pol, train_cnn=False, optimizer_state=False, adapters=ad)
    S, g = _run(tr, pol, ctx["batch"])
    assert not torch.equal(S["lp_b"], ctx["lp_b"])
    msd = ad.merged_state_dict(pol)
    ref = O.policy_forward({k: v.detach().cpu() for k, v in msd.items()}, cfg, img.cpu(), first.cpu(), O.initial_state(cfg, B))
    shape = lambda x, n: x.reshape(B, T, 1, n)          # (the oracle's heads keep the reference's singleton axis)
    P.check(P.policy_metrics(dict(buttons=shape(S["lp_b"], NB), camera=shape(S["lp_c"], NC)), ref), mode, "adapter trainer vs oracle(merged)", model="1x")
    pol2, _ = _policy(mode, sd=msd)          # strict=True
    full2 = BCTrainer(pol2, train_cnn=False, optimizer_state=False, trainable=ad.adapted_weights)
    S2, dw = _run(full2, pol2, ctx["batch"])
    P.check(P.policy_metrics(dict(buttons=shape(S2["lp_b"], NB), camera=shape(S2["lp_c"], NC)), ref), mode, "merged policy vs oracle(merged)", model="1x")
    cos = {}
    for m in ad.modules:
        a, b = ad.pair(m)
        d = dw[m + ".weight"]
        cos[m + ".lora_A"] = _cos(g[m + ".lora_A"], ad.scale * b.t() @ d)
        cos[m + ".lora_B"] = _cos(g[m + ".lora_B"], ad.scale * d @ a.t())
    GB = P.GRAD_BOUNDS[mode]
    mean = sum(cos.values()) / len(cos)
    print(f"(c) {mode}: adapter gradients vs the dense projection on the merged policy: min cosine {min(cos.values()):.4f}, mean {mean:.4f}")
    assert min(cos.values()) > GB["cos_min_small"] and mean > GB["cos_mean"], (min(cos, key=cos.get), min(cos.values()), mean)


def _backward_counts(tr, pol, batch):
    img, first, ab, ac = batch
    S = tr.forward_saving(img, first, pol.initial_state(B))
    m = S["m"]
    scale = (tr.loss_scale if tr.scaled else 1.0 / m) / pol._cfg["temperature"]
    dz = ops.nll_backward(S["lp_b"], S["lp_c"], ab.reshape(m).contiguous(), ac.reshape(m).contiguous(), S["ldz"], scale, dtype=tr.dtype)
    ops.TIMER.reset()
    ops.TIMER.enabled = True
    try:
        tr.backward_from(S, dz)
        torch.cuda.synchronize()
    finally:
        ops.TIMER.enabled = False
    counts = collections.Counter(rec[0] for rec in ops.TIMER.records)
    ops.TIMER.reset()
    return counts


def test_six_steps_move_only_adapters_and_selection(ctx):
    """(d)"""
    pol, sd, batch = ctx["pol"], ctx["sd"], ctx["batch"]
    img, first, ab, ac = batch
    args = lambda: (img, first, pol.initial_state(B), ab, ac)
    try:
        ad = LowRankAdapters(pol, targets=TARGETS, rank=RANK, alpha=ALPHA, seed=0)
        tr = BCTrainer(pol, lr=1e-3, weight_decay=0.0, train_cnn=False, adapters=ad, trainable=("pi_head",))
        assert set(tr.m) == set(tr.v) == set(HEADS) | set(ad.params)
        # launches: one wgrad for the heads, two skinny ones (dB, dA) per adapted GEMM (4 per block: the fused projection, proj, mlp0, mlp1), no
        # [n, K] wgrad for a frozen adapted weight; nothing below the cut (block 1): three attention backwards, seven LayerNorm backwards
        c = _backward_counts(tr, pol, batch)
        assert c["vpt_linear_wgrad"] == 1 + 2 * 4 * 3, c
        assert sum(v for k, v in c.items() if k.startswith("vpt_masked_attention_backward")) == 3 and c["vpt_layernorm_backward"] == 7, c
        # micro_batches=2 is the hand-run accumulation, bit for bit
        _, g2, _ = tr.reduced_loss_and_grads(*args(), micro_batches=2)
        parts = []
        for lo in range(B):
            _, gp, _ = tr.loss_and_grads(img[lo:lo + 1], first[lo:lo + 1], pol.initial_state(1), ab[lo:lo + 1], ac[lo:lo + 1], global_frames=B * T,
                                         unscaled=False, metrics={})
            parts.append({k: v.clone() for k, v in gp.items()})
        torch.cuda.synchronize()
        assert set(g2) == set(tr.trainable) and all(torch.equal(g2[n], parts[0][n] + parts[1][n]) for n in tr.trainable)
        losses, snap = [], None
        for i in range(6):
            if i == 3:
                snap = (copy.deepcopy(tr.state_dict()), ad.state_dict(), copy.deepcopy(pol.state_dict()))
            loss, _ = tr.step(*args())
            losses.append(loss)
        torch.cuda.synchronize()
        print(f"(d) {ctx['mode']}: losses {[round(x, 4) for x in losses]}")
        assert losses[-1] < losses[0] and tr.skipped_steps == 0
        moved = {k for k, v in pol.named_parameters() if not torch.equal(v.detach(), sd[k])}
        assert moved == set(HEADS), moved ^ set(HEADS)
        assert all(float(t.abs().max()) > 0 for t in ad.params.values())
        end = {n: t.clone() for n, t in ad.params.items()}
        end_heads = {n: dict(pol.named_parameters())[n].detach().clone() for n in HEADS}
        # the round trip: steps 4-6 again from the snapshot, on fresh objects
        pol.load_state_dict(snap[2])
        ad2 = LowRankAdapters(pol, targets=TARGETS, rank=RANK, alpha=1.0, seed=5)
        ad2.load_state_dict(snap[1])
        tr2 = BCTrainer(pol, lr=7.0, train_cnn=False, adapters=ad2, trainable=("pi_head",))
        tr2.load_state_dict(snap[0])
        for _ in range(3):
            tr2.step(*args())
        torch.cuda.synchronize()
        assert all(torch.equal(ad2.params[n], end[n]) for n in end)
        assert all(torch.equal(dict(pol.named_parameters())[n].detach(), end_heads[n]) for n in HEADS)
        # evaluate() sees base + adapters and leaves the masters as they were
        before = {k: v.detach().clone() for k, v in pol.named_parameters()}
        met, _ = tr2.evaluate(*args())
        assert all(torch.equal(v.detach(), before[k]) for k, v in pol.named_parameters()) and not ad2.merged
        assert abs(float(met["loss"]) - losses[-1]) < abs(float(met["loss"]) - losses[0])
    finally:
        pol.load_state_dict(sd)


def test_merge_reaches_the_acting_path_and_unmerge_restores_the_masters(ctx):
    """(e)"""
    pol, mode, sd = ctx["pol"], ctx["mode"], ctx["sd"]
    g = torch.Generator().manual_seed(3)
    frames = P.structured_frames(2, 4, g).to(DEV)          # 2 environments, 4 acting steps
    first = torch.zeros(2, dtype=torch.bool, device=DEV)

    def act_all(p, graph):
        p.disable_step_graph()
        if graph:
            p.enable_step_graph(2, alias_state=False)
        state, out = p.initial_state(2), []
        for t in range(4):
            ac, state, res = p.act({"img": frames[:, t]}, first, state, stochastic=False)
            out.append((ac["buttons"].clone(), ac["camera"].clone(), res["log_prob"].clone()))
        p.disable_step_graph()
        p.auto_step_graph(True)
        return out

    same = lambda x, y: all(torch.equal(a, b) for sx, sy in zip(x, y) for a, b in zip(sx, sy))
    try:
        ad = LowRankAdapters(pol, targets=TARGETS, rank=RANK, alpha=ALPHA, seed=0)
        _randomise(ad, ".lora_B", 0.3, 13)
        base = {graph: act_all(pol, graph) for graph in (False, True)}
        pol2, _ = _policy(mode, sd=ad.merged_state_dict(pol))
        want = {graph: act_all(pol2, graph) for graph in (False, True)}
        pol.enable_step_graph(2, alias_state=False)
        warm = pol.act({"img": frames[:, 0]}, first, pol.initial_state(2), stochastic=False)          # a graph captured on the BASE weights
        del warm
        ad.merge_(pol)
        assert ad.merged
        state, got = pol.initial_state(2), []
        for t in range(4):                                  # the captured graph must have refreshed with the packed weights
            ac, state, res = pol.act({"img": frames[:, t]}, first, state, stochastic=False)
            got.append((ac["buttons"].clone(), ac["camera"].clone(), res["log_prob"].clone()))
        assert same(got, want[True])
        assert same(act_all(pol, False), want[False])
        assert not same(want[False], base[False]), "the update must show in the actions' log-probs"
        assert all(torch.equal(dict(pol.named_parameters())[n].detach(), dict(pol2.named_parameters())[n].detach()) for n in ad.adapted_weights)
        with pytest.raises(RuntimeError, match="merged"):
            BCTrainer(pol, train_cnn=False, adapters=ad).step(*(ctx["batch"][:2] + (pol.initial_state(B),) + ctx["batch"][2:]))
        with pytest.raises(RuntimeError, match="already merged"):
            ad.merge_(pol)
        ad.unmerge_(pol)
        assert all(torch.equal(v.detach(), sd[k]) for k, v in pol.named_parameters()), "unmerge_ restores every master bit for bit"
        assert same(act_all(pol, False), base[False]) and same(act_all(pol, True), base[True])
    finally:
        pol.load_state_dict(sd)
        pol.disable_step_graph()
        pol.auto_step_graph(True)


def test_ppo_with_the_policy_itself_as_the_prior(ctx):
    """(f) the frozen base is the prior: prior_logprobs(policy) on the SAME object; the KL slots are 0 at B = 0 and positive after three steps.
    Exactly 0.0 against the saving forward's own log-probs (the anchor).  prior_logprobs runs the engine's INFERENCE forward, whose kernels at 8 rows
    round differently from the saving forward's -- so has it been before adapters --: against it the slots measure 2.1e-6 / 2.0e-6 (bf16) and
    -3.1e-7 / -2.6e-8 (fp16) at B = 0, held below lp_max^2 (derived below), and 7.4e-5 / 7.7e-5 (bf16), 6.3e-5 / 6.7e-5 (fp16) after three steps."""
    pol, sd, batch = ctx["pol"], ctx["sd"], ctx["batch"]
    img, first, ab, ac = batch
    gen = torch.Generator().manual_seed(31)
    adv = (torch.rand(B, T, generator=gen) - 0.3).to(DEV)
    target = torch.randn(B, T, generator=gen).to(DEV)
    try:
        ad = LowRankAdapters(pol, targets=TARGETS, rank=RANK, alpha=ALPHA, seed=0)
        tr = PPOTrainer(pol, lr=1e-3, weight_decay=0.0, train_cnn=False, normalize_advantages=False, update_value_normalizer=False, kl_coef=0.1, adapters=ad)
        assert tr.trainable == list(ad.params)
        pb, pc, _ = tr.prior_logprobs(pol, img, first, pol.initial_state(B))
        old = (pb.gather(1, ab.reshape(-1, 1)) + pc.gather(1, ac.reshape(-1, 1))).reshape(B, T).clone()
        args = lambda: (img, first, pol.initial_state(B), ab, ac, old, adv, target)
        # against the log-probs of the saving forward itself (at B = 0 the adapter-less trainer's, bit for bit) the KL slots are exactly 0
        S0 = tr.forward_saving(img, first, pol.initial_state(B))
        own = (S0["lp_b"].clone(), S0["lp_c"].clone())
        assert torch.equal(own[0], ctx["lp_b"]) and torch.equal(own[1], ctx["lp_c"])
        del S0
        met: dict = {}
        tr.loss_and_grads(*args(), prior_lp=own, metrics=met)
        assert float(met["kl_buttons"]) == 0.0 and float(met["kl_camera"]) == 0.0, (met["kl_buttons"], met["kl_camera"])
        met = {}
        tr.loss_and_grads(*args(), prior_lp=(pb, pc), metrics=met)
        # pi comes from the saving forward, the prior from the inference forward: the same function through other kernels at 8 rows, log-probs apart
        # by at most parity.BOUNDS' lp_max = d.  Both are normalised, so the KL is second order in that difference: <= d^2 / 2 (1 + O(d)) < d^2.
        kl0 = (float(met["kl_buttons"]), float(met["kl_camera"]))
        d = P.BOUNDS[ctx["mode"]]["lp_max"]
        assert abs(kl0[0]) < d * d and abs(kl0[1]) < d * d, kl0
        before = {k: v.detach().clone() for k, v in pol.named_parameters()}
        for _ in range(3):
            tr.step(*args(), prior_lp=(pb, pc))
        met = {}
        tr.loss_and_grads(*args(), prior_lp=(pb, pc), metrics=met)
        torch.cuda.synchronize()
        print(f"(f) {ctx['mode']}: KL to the base, buttons / camera: {kl0} at B = 0, {(float(met['kl_buttons']), float(met['kl_camera']))} after three steps")
        assert float(met["kl_buttons"]) > 10 * abs(kl0[0]) and float(met["kl_camera"]) > 10 * abs(kl0[1]) and min(float(met["kl_buttons"]), float(met["kl_camera"])) > 0
        assert all(torch.equal(v.detach(), before[k]) for k, v in pol.named_parameters()), "the base is the prior: no base tensor moves"
        pb2, pc2, _ = tr.prior_logprobs(pol, img, first, pol.initial_state(B))
        assert torch.equal(pb2, pb) and torch.equal(pc2, pc)
    finally:
        pol.load_state_dict(sd)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_idm_one_step_moves_only_the_adapters(precision):
    """(f) IDMTrainer on the tiny IDM: r_layer is outside its fused projection and not adaptable; one step moves the adapters and nothing else."""
    kw, cfg, sd = LR.tiny_idm()
    pol = InverseActionPolicy(idm_action_space(), pi_head_kwargs=dict(temperature=LR.TEMPERATURE), idm_net_kwargs=kw, precision=precision)
    pol.load_state_dict(sd, strict=False)
    pol = pol.to(DEV)
    g = torch.Generator().manual_seed(21)
    img = P.structured_frames(B, T, g).to(DEV)
    buttons, camera = torch.randint(0, 2, (B, T, 20), generator=g).to(DEV), torch.randint(0, 11, (B, T, 2), generator=g).to(DEV)
    ad = LowRankAdapters(pol, targets=("net.recurrent_layer.blocks",), rank=4, alpha=4.0)
    assert len(ad.modules) == 6 * cfg["n_layers"] and not any(m.endswith("r_layer") for m in ad.modules)
    with pytest.raises(ValueError, match="is not adaptable"):
        LowRankAdapters(pol, targets=(BLK + "0.r.orc_block.r_layer",))
    plain_loss, _ = IDMTrainer(pol, optimizer_state=False, trainable=["pi_head"]).loss_and_grads(img, buttons, camera)
    tr = IDMTrainer(pol, lr=1e-3, weight_decay=0.0, adapters=ad)
    loss, grads = tr.loss_and_grads(img, buttons, camera)
    assert torch.equal(loss, plain_loss) and set(grads) == set(ad.params)
    assert all(not bool(grads[m + ".lora_A"].any()) and float(grads[m + ".lora_B"].abs().max()) > 0 for m in ad.modules)
    before = {k: v.detach().clone() for k, v in pol.named_parameters()}
    start = {n: t.clone() for n, t in ad.params.items()}
    tr.step(img, buttons, camera)
    torch.cuda.synchronize()
    assert all(torch.equal(v.detach(), before[k]) for k, v in pol.named_parameters())
    assert all(not torch.equal(ad.params[m + ".lora_B"], start[m + ".lora_B"]) for m in ad.modules)
    met = tr.evaluate(img, buttons, camera)
    assert all(torch.equal(v.detach(), before[k]) for k, v in pol.named_parameters()) and float(met["loss"]) == float(met["loss"])


def test_refusals(ctx, monkeypatch):
    """(g)"""
    pol = ctx["pol"]
    with pytest.raises(ValueError, match="is not adaptable"):
        LowRankAdapters(pol, targets=("net.lastlayer",))
    with pytest.raises(ValueError, match="is not adaptable"):
        LowRankAdapters(pol, targets=(BLK + "0", "pi_head"))
    with pytest.raises(ValueError, match="is not adaptable"):
        LowRankAdapters(pol, targets=("net.img_process.linear",))
    with pytest.raises(ValueError, match="rank must be"):
        LowRankAdapters(pol, rank=65)
    ad = LowRankAdapters(pol, targets=(BLK + "3.mlp0",), rank=2)
    with pytest.raises(ValueError, match="frozen under an adapter"):
        BCTrainer(pol, train_cnn=False, adapters=ad, trainable=(BLK + "3.mlp0.layer.weight",))
    with pytest.raises(ValueError, match="does not train"):
        BCTrainer(pol, train_cnn=False, adapters=ad, trainable=("value_head",))
    pol2, _ = _policy(ctx["mode"])
    with pytest.raises(ValueError, match="another policy object"):
        BCTrainer(pol2, train_cnn=False, adapters=ad)
    with pytest.raises(ValueError, match="another policy object"):
        ad.merge_(pol2)
    sd = ad.state_dict()
    with pytest.raises(ValueError, match="another target set"):
        LowRankAdapters(pol, targets=(BLK + "3.mlp1",), rank=2).load_state_dict(sd)
    tr = BCTrainer(pol, train_cnn=False, adapters=ad, param_groups=[dict(params=[BLK + "3.mlp0.layer.lora_B"], lr_scale=0.5)])
    assert tr._group_of == {BLK + "3.mlp0.layer.lora_B": 0} and tr._cut == 5
    import torch.distributed as dist
    assert tr._check_adapters_ready() is None
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="data-parallel steps with adapters"):
        tr._check_adapters_ready()
