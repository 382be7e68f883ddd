"""RolloutBuffer (vpt_amd.rollout) end to end on the GPU, both operand formats: against INTEGRATION.md's hand loop around policy.act() bit for bit, the
per-chunk state snapshots under an aliased step graph, the stored log-probs against the training forward, chunks() against hand slices through
PPOTrainer, a second rollout, the PPG snapshot, misuse.  Needs an MI355X.  Policy: the 1x model (temperature 2.0); B = 2, T = 6, L = 3; a scripted
on-device environment: a frame table, rewards a fixed function of the action, environment 0 resets at frame 3 (a chunk start), environment 1 at frame 4
(mid-chunk); in the second rollout environment 1 resets at frame 8 and environment 0 at frame 10, so both finished episodes span the rollout boundary."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd.rl_training import PPOTrainer  # noqa: E402
from vpt_amd.rollout import CHUNK_KEYS, RolloutBuffer  # noqa: E402
from vpt_amd.lib.policy import MinecraftAgentPolicy  # noqa: E402
from vpt_amd.lib.types import minecraft_action_space  # noqa: E402
from oracle import vpt_oracle as O  # noqa: E402
from tests import parity as P  # noqa: E402
from tests import rollout_ref as R  # noqa: E402

DEV = "cuda"
B, T, L = 2, 6, 3
SEED = 1234
FIRST_AT = {0: (True, True), 3: (True, False), 4: (False, True), 8: (False, True), 10: (True, False)}      # frame index -> which environments start an episode
GRADS = ("value_head.linear.weight", "pi_head.camera.linear_layer.bias", "net.recurrent_layer.blocks.0.r.orc_block.q_layer.weight")      # trunk and heads: summed in a fixed order


class ScriptedEnv:
    """Frames from a fixed table, `first` from FIRST_AT, reward a fixed function of the action; everything on the device."""

    def __init__(self, n_frames=16):
        self.table = P.structured_frames(B, n_frames, torch.Generator().manual_seed(5)).to(DEV)
        self.s = 0

    def _now(self):
        first = torch.tensor(FIRST_AT.get(self.s, (False, False)), device=DEV)
        return self.table[:, self.s % self.table.shape[1]].contiguous(), first

    def reset(self):
        self.s = 0
        return self._now()

    def step(self, action):
        reward = (action["buttons"][:, 0] % 7).float() * 0.25 - action["camera"][:, 0].float() * 0.01
        self.s += 1
        obs, first = self._now()
        return obs, reward, first


def _policy(precision):
    pk = O.policy_kwargs_for("1x")
    cfg = O.config_from_policy_kwargs(pk, dict(temperature=2.0))
    sd = O.synthetic_state_dict(cfg, seed=0)
    pol = MinecraftAgentPolicy(minecraft_action_space(), pk, dict(temperature=2.0), precision=precision)
    pol.load_state_dict(sd, strict=False)
    return pol.to(DEV)


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def policy_1x(request):
    pol = _policy(request.param)
    return pol, copy.deepcopy(pol.state_dict())


def _set_graph(pol, graph):
    if graph:
        pol.enable_step_graph(B, alias_state=True)
    else:
        pol.disable_step_graph()


def _clone_state(state):
    return [(None if m is None else m.clone(), (k.clone(), v.clone())) for m, (k, v) in state]


def _state_equal(a, b):
    """Two recurrent states; a None mask (initial_state) is a mask with nothing valid."""
    for (m0, (k0, v0)), (m1, (k1, v1)) in zip(a, b):
        z0 = m0 if m0 is not None else torch.zeros_like(m1 if m1 is not None else k0[..., 0].bool())
        z1 = m1 if m1 is not None else torch.zeros_like(z0)
        if not (torch.equal(k0, k1) and torch.equal(v0, v1) and torch.equal(z0.reshape(-1), z1.reshape(-1))):
            return False
    return len(a) == len(b)


def _same(a, b):
    """Bit-for-bit equality of two losses (step() hands out a host float, loss_and_grads a device scalar) or tensors."""
    if isinstance(a, torch.Tensor):
        return bool(torch.isfinite(a).all()) and torch.equal(a, b)
    return np.isfinite(a) and a == b


def _trainer(pol, **kw):
    return PPOTrainer(pol, episode_starts="frame", **kw)


def _hand_rollout(pol, trainer, env, obs, first, state, horizon=T):
    """INTEGRATION.md's hand loop on the pre-existing API, with the per-chunk state clones a careful user takes."""
    z = lambda dtype, *shape: torch.zeros(B, horizon, *shape, dtype=dtype, device=DEV)
    d = dict(img=z(torch.uint8, 128, 128, 3), first=z(torch.bool), act_buttons=z(torch.int64), act_camera=z(torch.int64), old_log_prob=z(torch.float32),
             vpred=z(torch.float32), reward=z(torch.float32), states=[])
    for t in range(horizon):
        if t % L == 0:
            d["states"].append(_clone_state(state))
        action, state, info = pol.act({"img": obs}, first, state, stochastic=True)
        d["img"][:, t], d["first"][:, t] = obs, first
        d["act_buttons"][:, t], d["act_camera"][:, t] = action["buttons"][:, 0], action["camera"][:, 0]
        d["old_log_prob"][:, t], d["vpred"][:, t] = info["log_prob"], info["vpred"].reshape(B)
        obs, d["reward"][:, t], first = env.step(action)
    last_value = pol.v({"img": obs}, first, state)
    d["advantage"], d["value_target"] = trainer.advantages(d["reward"], d["vpred"], d["first"], last_value, next_first=first)
    return d


def _collect(buf, env, obs, first, state, trainer):
    buf.begin(state)
    for t in range(buf.horizon):
        action, state = buf.act(obs, first, state, stochastic=True)
        assert tuple(action["buttons"].shape) == (B, 1) and tuple(action["camera"].shape) == (B, 1)
        obs, reward, first = env.step(action)
        buf.add_reward(reward, first)
    buf.finish(trainer, obs, first, state)
    return obs, first, state


_PAIRS = {}


def _pair(pol, sd, graph):
    """One rollout by the hand loop and one by the collector: same weights, same sampler seed, same step-graph setting.  Computed once per
    (precision, setting) and left unchanged."""
    key = (pol.precision, graph)
    if key not in _PAIRS:
        pol.load_state_dict(sd)
        _set_graph(pol, graph)
        trainer = _trainer(pol, optimizer_state=False)
        env = ScriptedEnv()
        pol.seed_sampler(SEED)
        hand = _hand_rollout(pol, trainer, env, *env.reset(), pol.initial_state(B))
        pol.seed_sampler(SEED)
        buf = RolloutBuffer(pol, num_envs=B, horizon=T, chunk_len=L)
        obs, first = env.reset()
        state0 = pol.initial_state(B)
        _, _, final_state = _collect(buf, env, obs, first, state0, trainer)
        torch.cuda.synchronize()
        assert (pol._step_graph is not None) == graph and (not graph or pol._step_graph["alias"])      # the collector left the setting as it found it
        _PAIRS[key] = dict(hand=hand, buf=buf, state0=state0, final_state=_clone_state(final_state))
    return _PAIRS[key]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "aliased_graph"])
def test_collector_equals_the_hand_loop_bit_for_bit(policy_1x, graph):
    """(a)"""
    pol, sd = policy_1x
    p = _pair(pol, sd, graph)
    hand, buf = p["hand"], p["buf"]
    for name, mine in (("img", buf.img), ("first", buf.first), ("act_buttons", buf.act_buttons), ("act_camera", buf.act_camera),
                       ("old_log_prob", buf.old_log_prob), ("vpred", buf.vpred), ("reward", buf.reward), ("advantage", buf.advantage),
                       ("value_target", buf.value_target)):
        assert mine.dtype == hand[name].dtype and torch.equal(mine, hand[name]), name
    assert hand["first"].cpu().tolist() == [[True, False, False, True, False, False], [True, False, False, False, True, False]]
    assert len(set(hand["act_buttons"].reshape(-1).tolist())) > 1 and bool(torch.isfinite(hand["advantage"]).all())
    chunks = buf.chunks()
    assert len(chunks) == T // L and all(tuple(c) == CHUNK_KEYS for c in chunks)
    for k, c in enumerate(chunks):                                      # views, no copies
        assert c["img_u8"].data_ptr() == buf.img[:, k * L].data_ptr() and c["advantage"].data_ptr() == buf.advantage[:, k * L].data_ptr()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "aliased_graph"])
def test_chunk_states_are_snapshots_not_aliases(policy_1x, graph):
    """(b)  The state before step 3 equals the clone the hand loop took there, and chunk 0's is still the initial state after the rollout: a snapshot
    that aliased the step graph's static buffers would hold the state after the rollout in both."""
    pol, sd = policy_1x
    p = _pair(pol, sd, graph)
    chunks, hand = p["buf"].chunks(), p["hand"]
    assert _state_equal(chunks[1]["state_in"], hand["states"][1])
    assert _state_equal(chunks[0]["state_in"], p["state0"]) and _state_equal(chunks[0]["state_in"], hand["states"][0])
    assert not bool(chunks[0]["state_in"][0][0].any()) and float(chunks[0]["state_in"][0][1][0].abs().max()) == 0.0
    assert not _state_equal(chunks[1]["state_in"], p["final_state"]) and not _state_equal(chunks[1]["state_in"], chunks[0]["state_in"])
    if graph:
        static = pol._step_graph["state"]
        for c in chunks:
            for (m, (k, v)), (m_s, (k_s, v_s)) in zip(c["state_in"], static):
                assert k.data_ptr() != k_s.data_ptr() and v.data_ptr() != v_s.data_ptr() and m.data_ptr() != m_s.data_ptr()


def test_stored_logprob_is_consistent_with_the_training_forward(policy_1x):
    """(c)  old_log_prob comes from the T = 1 latency kernels, the training forward recomputes it with the throughput kernels over [B, L] under
    episode_starts="frame".  Each path is held to parity.BOUNDS[mode]["lp_max"] (max |d| / max |lp| per head) of the same reference, so
    |old_lp - lp| <= 2 lp_max (max |lp_buttons| + max |lp_camera|).  Measured on MI355X, 1x model, this rollout (max over both chunks, aliased graph /
    eager): see DESIGN.md section 18."""
    pol, sd = policy_1x
    for graph in (True, False):
        p = _pair(pol, sd, graph)
        pol.load_state_dict(sd)
        tr = _trainer(pol, optimizer_state=False)
        for c in p["buf"].chunks():
            met, _ = tr.evaluate(**c)
            lp_b, lp_c, _ = tr.prior_logprobs(pol, c["img_u8"], c["first"], c["state_in"])
            bound = 2.0 * P.BOUNDS[pol.precision]["lp_max"] * (float(lp_b.abs().max()) + float(lp_c.abs().max()))
            diff = float(met["frame_out"][..., 9].abs().max())                      # slot 9: old_lp - lp
            print(f"rollout[{pol.precision}, {'aliased graph' if graph else 'eager'}] max |old_lp - lp| = {diff:.3e}  (bound {bound:.3e})")
            assert diff <= bound, (diff, bound)


def test_chunks_equal_hand_slices_through_the_trainer(policy_1x):
    """(d)  loss_and_grads over chunks() against the hand loop's tensors sliced by hand with the hand-cloned states: the loss and three named gradients;
    then step() over both, from the same weights: the losses."""
    pol, sd = policy_1x
    p = _pair(pol, sd, True)
    hand, chunks = p["hand"], p["buf"].chunks()

    def hand_chunk(k):
        s = slice(k * L, (k + 1) * L)
        return (hand["img"][:, s], hand["first"][:, s], hand["states"][k], hand["act_buttons"][:, s], hand["act_camera"][:, s], hand["old_log_prob"][:, s],
                hand["advantage"][:, s], hand["value_target"][:, s])

    pol.load_state_dict(sd)
    tr = _trainer(pol, optimizer_state=False, update_value_normalizer=False, train_cnn=False)
    for k, c in enumerate(chunks):
        loss, grads, state = tr.loss_and_grads(**c)
        loss_h, grads_h, state_h = tr.loss_and_grads(*hand_chunk(k))
        assert bool(torch.isfinite(loss)) and torch.equal(loss, loss_h), k
        for name in GRADS:
            assert float(grads[name].abs().max()) > 0 and torch.equal(grads[name], grads_h[name]), (k, name)
        assert _state_equal(state, state_h)
    losses = {}
    for who in ("chunks", "hand"):
        pol.load_state_dict(sd)
        tr = _trainer(pol, lr=1e-4, train_cnn=False)
        losses[who] = [tr.step(**c)[0] if who == "chunks" else tr.step(*hand_chunk(k))[0] for k, c in enumerate(chunks)]
        losses[who].append(pol.value_head.linear.weight.detach().clone())
    assert all(_same(a, b) for a, b in zip(losses["chunks"], losses["hand"])), losses
    assert not torch.equal(losses["chunks"][-1], sd["value_head.linear.weight"].to(DEV))      # the steps did move the weights
    pol.load_state_dict(sd)


def test_second_rollout_snapshot_and_episode_stats(policy_1x):
    """(e)  Two rollouts of 6 steps against ONE rollout of 12 by the same collector: the second continues from the first's final state (finish() leaves
    the aliased state as it found it), episodes that span the boundary report their whole return, the first rollout's snapshot() is unchanged by
    the second, and aux_step over the snapshot's chunks equals aux_step over the hand loop's tensors."""
    pol, sd = policy_1x
    hand = _pair(pol, sd, True)["hand"]
    pol.load_state_dict(sd)
    _set_graph(pol, True)
    trainer = _trainer(pol, optimizer_state=False)
    env = ScriptedEnv()
    pol.seed_sampler(SEED)
    long = RolloutBuffer(pol, num_envs=B, horizon=2 * T, chunk_len=L)
    _collect(long, env, *env.reset(), pol.initial_state(B), trainer)
    stats_long = long.episode_stats()

    pol.seed_sampler(SEED)
    buf = RolloutBuffer(pol, num_envs=B, horizon=T, chunk_len=L)
    obs, first = env.reset()
    obs, first, state = _collect(buf, env, obs, first, pol.initial_state(B), trainer)
    snap, stats1 = buf.snapshot(), buf.episode_stats()
    after_first = _clone_state(state)
    first_cols = {k: getattr(buf, k).clone() for k in ("img", "first", "act_buttons", "act_camera", "old_log_prob", "vpred", "reward")}
    _collect(buf, env, obs, first, state, trainer)
    stats2 = buf.episode_stats()
    torch.cuda.synchronize()

    chunks2 = buf.chunks()
    assert _state_equal(chunks2[0]["state_in"], after_first) and _state_equal(chunks2[0]["state_in"], long.chunks()[T // L]["state_in"])
    for k, v in first_cols.items():                                      # the two rollouts are the long one's halves
        assert torch.equal(v, getattr(long, k)[:, :T]) and torch.equal(getattr(buf, k), getattr(long, k)[:, T:]), k
    assert torch.equal(buf.done_return, long.done_return[:, T:]) and torch.equal(buf.done_length, long.done_length[:, T:])
    # episodes: rollout 1 ends (frames 0..2) of environment 0 and (0..3) of environment 1; rollout 2 ends (4..7) of environment 1 and (3..9) of environment 0
    ref = R.new_reward_bufs(B, 2 * T)
    reward, firsts = long.reward.cpu().numpy(), long.first.cpu().numpy()
    done = np.concatenate([firsts[:, 1:], np.array([FIRST_AT.get(2 * T, (False, False))]).T], axis=1)
    for t in range(2 * T):
        R.reward_step(ref, t, reward[:, t], done[:, t])
    assert np.array_equal(long.done_return.cpu().numpy().view(np.uint32), ref["done_return"].view(np.uint32))
    assert np.array_equal(long.done_length.cpu().numpy(), ref["done_length"])
    assert stats1["episodes"] == 2 and stats1["length_mean"] == 3.5
    assert stats2["episodes"] == 2 and stats2["length_mean"] == (4 + 7) / 2
    spanning = [float(reward[1, 4:8].astype(np.float64).sum()), float(reward[0, 3:10].astype(np.float64).sum())]
    assert stats2["return_mean"] == pytest.approx(sum(spanning) / 2, rel=1e-5, abs=1e-5)
    assert float(buf.done_return[1, 7 - T]) == pytest.approx(spanning[0], rel=1e-5, abs=1e-5) and int(buf.done_length[0, 9 - T]) == 7
    assert stats_long["episodes"] == 4 and stats_long["length_mean"] == (3 + 4 + 4 + 7) / 4

    # the snapshot of rollout 1 after rollout 2: still rollout 1 (= the hand loop's, test (a)), states included
    sc = snap.chunks()
    assert len(sc) == T // L and all(tuple(c) == CHUNK_KEYS for c in sc) and torch.equal(snap.value_target, hand["value_target"])
    for k, c in enumerate(sc):
        s = slice(k * L, (k + 1) * L)
        for name, key in (("img_u8", "img"), ("first", "first"), ("act_buttons", "act_buttons"), ("act_camera", "act_camera"), ("old_log_prob", "old_log_prob"),
                          ("advantage", "advantage"), ("value_target", "value_target")):
            assert torch.equal(c[name], hand[key][:, s]), (k, name)
        assert _state_equal(c["state_in"], hand["states"][k]) and c["state_in"] is snap.state_in[k]
        assert c["img_u8"].data_ptr() != buf.img[:, s].data_ptr()
    assert not torch.equal(sc[0]["img_u8"], buf.chunks()[0]["img_u8"])

    losses = {}
    for who in ("snapshot", "hand"):
        pol.load_state_dict(sd)
        tr = _trainer(pol, lr=1e-4, train_cnn=False)
        losses[who] = []
        for k, c in enumerate(sc):
            s = slice(k * L, (k + 1) * L)
            img, fr, st, vt = (c["img_u8"], c["first"], c["state_in"], c["value_target"]) if who == "snapshot" else \
                (hand["img"][:, s], hand["first"][:, s], hand["states"][k], hand["value_target"][:, s])
            old = tr.policy_snapshot(img, fr, st)[:2]
            losses[who].append(tr.aux_step(img, fr, st, old, vt)[0])
    assert all(_same(a, b) for a, b in zip(losses["snapshot"], losses["hand"])), losses
    pol.load_state_dict(sd)


def test_misuse_raises(policy_1x):
    """(f)"""
    pol, sd = policy_1x
    pol.load_state_dict(sd)
    with pytest.raises(ValueError):
        RolloutBuffer(pol, num_envs=B, horizon=7, chunk_len=3)
    pol.disable_step_graph()
    buf = RolloutBuffer(pol, num_envs=B, horizon=2, chunk_len=1)
    env = ScriptedEnv()
    obs, first = env.reset()
    state = pol.initial_state(B)
    with pytest.raises(RuntimeError, match="begin"):
        buf.act(obs, first, state)
    buf.begin(state)
    assert pol._step_graph is None                                      # a switched-off graph stays off ...
    pol.auto_step_graph(True)
    buf.begin(state)
    assert pol._step_graph == dict(batch=B, alias=True)                 # ... an unconfigured one becomes the aliased graph
    pol.enable_step_graph(B, alias_state=False)
    buf.begin(state)
    assert pol._step_graph == dict(batch=B, alias=False)                # ... and a configured one is left alone
    pol.disable_step_graph()
    buf.begin(state)
    with pytest.raises(RuntimeError, match="add_reward"):
        buf.add_reward(torch.zeros(B), first)                           # before any act
    with pytest.raises(RuntimeError, match="finish"):
        buf.chunks()
    action, state = buf.act(obs, first, state)
    with pytest.raises(RuntimeError, match="twice"):
        buf.act(obs, first, state)                                      # a second act without add_reward
    buf.add_reward([0.5, -0.5], [False, True])                          # array-likes are fine
    with pytest.raises(RuntimeError, match="finish"):
        buf.finish(_trainer(pol, optimizer_state=False), obs, first, state)      # one of two steps
    action, state = buf.act(obs, first, state)
    buf.add_reward(torch.zeros(B), first.cpu())
    with pytest.raises(RuntimeError, match="horizon"):
        buf.act(obs, first, state)                                      # past the horizon
    with pytest.raises(ValueError, match="frame"):
        buf.finish(PPOTrainer(pol, optimizer_state=False), obs, first, state)    # episode_starts="chunk"
    buf.nan_flag.fill_(1)
    with pytest.raises(AssertionError, match="NaN"):
        buf.finish(_trainer(pol, optimizer_state=False), obs, first, state)
    buf.nan_flag.zero_()
    adv, ret = buf.finish(_trainer(pol, optimizer_state=False), obs, first, state)
    assert tuple(adv.shape) == (B, 2) and len(buf.chunks()) == 2
    assert buf.reward[:, 0].cpu().tolist() == [0.5, -0.5]
    assert buf.episode_stats() == dict(episodes=3, return_mean=0.0, length_mean=4 / 3)      # environment 1 after step 0 (-0.5, 1 step), both after step 1 (0.5 over 2 steps, 0.0 over 1)


def test_act_and_add_reward_do_not_synchronise(policy_1x):
    """A whole rollout of act() / add_reward() under torch's synchronisation debug mode "error", inputs resident on the device: no call makes the host wait
    (the NaN check is the sticky flag finish() reads).  policy.act() on the same step does: its NaN assert reads the device."""
    pol, sd = policy_1x
    pol.load_state_dict(sd)
    _set_graph(pol, True)
    trainer = _trainer(pol, optimizer_state=False)
    table = P.structured_frames(B, 2 * T + 1, torch.Generator().manual_seed(6)).to(DEV)
    firsts = torch.tensor([FIRST_AT.get(s, (False, False)) for s in range(2 * T + 1)], device=DEV)
    buf = RolloutBuffer(pol, num_envs=B, horizon=T, chunk_len=L)
    state, s = pol.initial_state(B), 0
    for rollout in range(2):                                            # the first one warms up: graph capture, lazy kernel loading
        buf.begin(state)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error" if rollout else "default")
        try:
            for t in range(T):
                action, state = buf.act(table[:, s].contiguous(), firsts[s], state)
                s += 1
                buf.add_reward(action["camera"][:, 0].float() * 0.01, firsts[s])
            if rollout:
                with pytest.raises(RuntimeError, match="synchroniz"):
                    pol.act({"img": table[:, s].contiguous()}, firsts[s], state)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        if rollout == 0:
            buf.finish(trainer, table[:, s].contiguous(), firsts[s], state)
    assert buf._t == T and int(buf.nan_flag) == 0
