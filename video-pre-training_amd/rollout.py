"""On-device rollout collection for RL fine-tuning: the link from MinecraftAgentPolicy.act() to PPOTrainer (what labeler.labelled_chunks is for stage 2).

A rollout of T environment steps of B environments is trained on in T / L chunks of L frames.  RolloutBuffer owns every [B, T] tensor PPOTrainer.step reads,
fills column t with ONE launch per acting step (ops.rollout_record) and one after the environment has stepped (ops.rollout_reward), and hands the chunks out
as views under PPOTrainer.step's own argument names:

    buf = RolloutBuffer(policy, num_envs=B, horizon=T, chunk_len=L)
    state = policy.initial_state(B)
    for it in range(ITERS):
        buf.begin(state)
        for t in range(T):
            action, state = buf.act(obs, first, state, stochastic=True)
            obs, reward, first = env_step(action)
            buf.add_reward(reward, first)
        buf.finish(trainer, obs, first, state)
        for epoch in range(EPOCHS):
            for chunk in buf.chunks():
                loss, _ = trainer.step(**chunk)

Three things a hand-written loop around policy.act() gets wrong are handled here:
  * the recurrent state at chunk boundaries.  Chunk k needs the state from just before frame k L.  Under an aliased step graph
    (enable_step_graph(B, alias_state=True), the fast acting mode) the state act() returns IS the graph's static buffers and the next step overwrites it:
    a reference kept for chunk k silently becomes the state after the rollout.  The buffer copies the incoming state into storage of its own before step
    k L -- T / L copies per rollout, not the T copies of the automatic (alias_state=False) graph -- and chunks()[k]["state_in"] is that copy;
  * the host synchronisation of every step.  act() asserts the NaN flag before returning; here the record launch keeps a sticky flag on the device and
    finish() reads it once;
  * policy.v() after the last step advances an aliased state IN PLACE by the frame it evaluates, which the next rollout's first step would then see twice;
    finish() puts the state back.
"""
from typing import List, Optional, Tuple

import torch

from . import ops
from .lib.tree_util import tree_map

CHUNK_KEYS = ("img_u8", "first", "state_in", "act_buttons", "act_camera", "old_log_prob", "advantage", "value_target")


def chunk_bounds(horizon: int, chunk_len: int) -> List[Tuple[int, int]]:
    """[(k L, (k + 1) L)] for the T / L chunks of a rollout; T % L != 0 is a ValueError (a ragged tail chunk would need frame weights)."""
    horizon, chunk_len = int(horizon), int(chunk_len)
    if horizon < 1 or chunk_len < 1 or chunk_len > horizon or horizon % chunk_len:
        raise ValueError(f"the horizon ({horizon}) must be a positive multiple of the chunk length ({chunk_len})")
    return [(lo, lo + chunk_len) for lo in range(0, horizon, chunk_len)]


def _chunks(tensors: dict, states: list, bounds):
    for k, (lo, hi) in enumerate(bounds):
        yield dict(img_u8=tensors["img"][:, lo:hi], first=tensors["first"][:, lo:hi], state_in=states[k], act_buttons=tensors["act_buttons"][:, lo:hi],
                   act_camera=tensors["act_camera"][:, lo:hi], old_log_prob=tensors["old_log_prob"][:, lo:hi], advantage=tensors["advantage"][:, lo:hi],
                   value_target=tensors["value_target"][:, lo:hi])


class RolloutSnapshot:
    """A detached copy of a finished rollout (RolloutBuffer.snapshot): what the PPG auxiliary phase keeps of it.  chunks() yields the same dicts as the
    buffer's; `value_target` [B, T] and `state_in` (one recurrent state per chunk) are policy_snapshot / aux_step's inputs.  Later rollouts do not change it."""

    def __init__(self, tensors: dict, states: list, bounds):
        self._tensors, self.state_in, self._bounds = tensors, states, bounds
        self.value_target = tensors["value_target"]

    def chunks(self):
        return list(_chunks(self._tensors, self.state_in, self._bounds))


class RolloutBuffer:
    def __init__(self, policy, num_envs: int, horizon: int, chunk_len: int):
        """Every buffer is allocated here, once, on the policy's device: the [B, T] rollout tensors, the per-environment episode accumulators (they persist
        across rollouts: an episode that spans two reports its whole return) and T / L + 1 recurrent states (one per chunk, one scratch for finish())."""
        self.policy = policy
        self.num_envs, self.horizon, self.chunk_len = int(num_envs), int(horizon), int(chunk_len)
        if self.num_envs < 1:
            raise ValueError("num_envs must be positive")
        self._bounds = chunk_bounds(self.horizon, self.chunk_len)
        b, t, dev, cfg = self.num_envs, self.horizon, policy._device(), policy._cfg
        if dev.type != "cuda":
            raise RuntimeError("RolloutBuffer needs the policy on the GPU (the HIP path has no CPU fallback)")
        z = lambda dtype, *shape: torch.zeros(*shape, dtype=dtype, device=dev)
        self.img = z(torch.uint8, b, t, *cfg["img_shape"])
        self.first = z(torch.bool, b, t)
        self.act_buttons, self.act_camera = z(torch.int64, b, t), z(torch.int64, b, t)
        self.old_log_prob, self.vpred, self.reward = z(torch.float32, b, t), z(torch.float32, b, t), z(torch.float32, b, t)
        self.done_return, self.done_length = z(torch.float32, b, t), z(torch.int32, b, t)
        self.ep_return, self.ep_length = z(torch.float32, b), z(torch.int32, b)
        self.nan_flag = z(torch.uint8, 1)
        self.advantage = self.value_target = None
        nbytes = cfg["n_layers"] * (2 * b * cfg["maxlen"] * cfg["hidsize"] * 4 + b * cfg["maxlen"])
        self._flat = [z(torch.uint8, (nbytes + 15) // 16 * 16) for _ in range(len(self._bounds) + 1)]      # the policy's own flat layout (_state_views)
        self._states = [policy._state_views(f, b) for f in self._flat]
        self._t, self._begun, self._awaiting_reward, self._finished = 0, False, False, False

    # ---- state snapshots ----------------------------------------------------------------------
    def _flat_source(self, state, slot: int) -> Optional[torch.Tensor]:
        """The ONE flat byte buffer `state` is a view of, when it has this buffer's layout (the step graph's static state and the copies a non-aliased
        graph hands out do) -> a snapshot is a single copy; None otherwise (initial_state(), an eager step's outputs)."""
        base = getattr(state[0][1][0], "_base", None)
        own = self._flat[slot]
        if base is None or base.dtype != torch.uint8 or base.dim() != 1 or base.numel() != own.numel() or not base.is_contiguous():
            return None
        p0, q0 = base.data_ptr(), own.data_ptr()
        for (m, (k, v)), (m_o, (k_o, v_o)) in zip(state, self._states[slot]):
            for x, x_o in ((m, m_o), (k, k_o), (v, v_o)):
                if x is None or x.shape != x_o.shape or x.dtype != x_o.dtype or not x.is_contiguous() or x.data_ptr() - p0 != x_o.data_ptr() - q0:
                    return None
        return base

    def _save_state(self, slot: int, state):
        if len(state) != len(self._states[slot]):
            raise ValueError(f"the recurrent state has {len(state)} layers, the policy {len(self._states[slot])}")
        if state[0][1][0].shape[0] != self.num_envs:
            raise ValueError(f"the recurrent state holds {state[0][1][0].shape[0]} environments, the buffer {self.num_envs}")
        base = self._flat_source(state, slot)
        if base is not None:
            self._flat[slot].copy_(base)
            return
        for (m, (k, v)), (m_o, (k_o, v_o)) in zip(state, self._states[slot]):
            k_o.copy_(k); v_o.copy_(v)
            if m is None:          # initial_state(): nothing of the memory is valid yet
                m_o.zero_()
            else:
                m_o.copy_(m)

    def _aliases_step_graph(self, state) -> bool:
        sg = self.policy._step_graph
        return bool(sg is not None and sg.get("alias") and "state" in sg and state[0][1][0].data_ptr() == sg["state"][0][1][0].data_ptr())

    # ---- the rollout --------------------------------------------------------------------------
    def begin(self, state=None):
        """Start a rollout: column 0 is next, the NaN flag is cleared, the previous rollout's chunks() are gone (its snapshot()s are not).  The episode
        accumulators carry on.  `state`, when given, is only checked against the buffer's shape; the state chunk 0 starts from is the one act() receives.
        THE STEP GRAPH: if the policy has no step graph enabled, its automatic capture has not been switched off (disable_step_graph(), VPT_STEP_GRAPH=0)
        and num_envs is graph-eligible, this call enables the ALIASED graph, policy.enable_step_graph(num_envs, alias_state=True): the automatic one
        would copy the whole state on every step, and the buffer keeps the only copies a rollout needs.  A graph the caller has configured, or switched
        off, is left as it is."""
        pol = self.policy
        if state is not None and (len(state) != pol._cfg["n_layers"] or state[0][1][0].shape[0] != self.num_envs):
            raise ValueError(f"begin(): the recurrent state does not match {self.num_envs} environments x {pol._cfg['n_layers']} layers")
        if pol._step_graph is None and pol._auto_graph["enabled"] and self.num_envs <= ops.LN_LINEAR_MAX_ROWS:
            pol.enable_step_graph(self.num_envs, alias_state=True)
        self.nan_flag.zero_()
        self.advantage = self.value_target = None
        self._t, self._begun, self._awaiting_reward, self._finished = 0, True, False, False

    def _device_flags(self, first):
        first = torch.as_tensor(first)
        if first.dtype not in (torch.bool, torch.uint8):
            first = first != 0
        return first.to(self.img.device).reshape(self.num_envs).contiguous()

    @torch.no_grad()
    def act(self, obs, first, state_in, stochastic: bool = True):
        """The step policy.act() runs (MinecraftAgentPolicy._run with the fused sampling; act()'s own fall-backs where a path lacks the fused outputs),
        then ONE launch that stores it in column t.  -> (action {"buttons": [B, 1], "camera": [B, 1]} as act() returns it, state_out).  Nothing here reads
        the device: the NaN check of the log-prob is a sticky flag that finish() reads.  obs: uint8 [B, 128, 128, 3] (or {"img": that}); first: bool [B].
        taken_action / return_pd are act()'s own business: not offered."""
        if not self._begun:
            raise RuntimeError("RolloutBuffer.act() before begin()")
        if self._awaiting_reward:
            raise RuntimeError("RolloutBuffer.act() twice without add_reward() in between")
        if self._t >= self.horizon:
            raise RuntimeError(f"RolloutBuffer.act() past the horizon ({self.horizon} steps): finish() and begin() the next rollout")
        pol, t = self.policy, self._t
        img = obs["img"] if isinstance(obs, dict) else obs
        first = self._device_flags(first)
        if t % self.chunk_len == 0:
            self._save_state(t // self.chunk_len, state_in)
        mode = "stochastic" if stochastic else "deterministic"
        (pd, vpred, _), state_out, extra = pol._run({"img": img.unsqueeze(1)}, first.unsqueeze(1), state_in, sample=mode, auto_graph=True, keep_pd=False)
        if "action" in extra:
            ac, log_prob = {k: extra["action"][k] for k in pd}, extra["action_log_prob"]
        else:
            ac = pol.pi_head.sample(pd, deterministic=not stochastic)
            log_prob = pol.pi_head.logprob(ac, pd)
        if "vpred_denorm" in extra and "action" in extra:
            vp = extra["vpred_denorm"]                        # computed inside the step graph
        else:
            vp = pol.value_head.denormalize(vpred)[:, 0]
        ops.rollout_record(img, first, ac["buttons"], ac["camera"], log_prob, vp, t, self.img, self.first, self.act_buttons, self.act_camera,
                           self.old_log_prob, self.vpred, self.nan_flag)
        self._awaiting_reward = True
        return tree_map(lambda x: x[:, 0], ac), state_out

    @torch.no_grad()
    def add_reward(self, reward, first):
        """The environment's answer to the step act() just recorded: reward [B] and `first` [B] of the NEXT frame (tensors on any device, or array-likes).
        One launch: the reward into column t, the episode accumulators advanced, finished episodes' return and length into column t."""
        if not self._awaiting_reward:
            raise RuntimeError("RolloutBuffer.add_reward() without an act() to answer")
        dev = self.img.device
        r = torch.as_tensor(reward).to(device=dev, dtype=torch.float32).reshape(self.num_envs).contiguous()
        ops.rollout_reward(r, self._device_flags(first), self._t, self.reward, self.done_return, self.done_length, self.ep_return, self.ep_length)
        self._t += 1
        self._awaiting_reward = False

    @torch.no_grad()
    def finish(self, trainer, obs, first, state):
        """After the last add_reward(): the rollout's ONE read of the NaN flag (AssertionError, as act() asserts it per step), the value of the frame after
        the rollout (policy.v) and trainer.advantages() -> (advantage, value_target) fp32 [B, T], which chunks() then hands out.  obs, first, state: what the
        next act() would receive; `state` is left exactly as it is (an aliased step-graph state, which policy.v() advances in place, is put back).
        The trainer must honour `first` at every frame (episode_starts="frame"): environments reset at any step, and "chunk" mode reads first[:, 0] only."""
        if self._t != self.horizon or self._awaiting_reward:
            raise RuntimeError(f"RolloutBuffer.finish() after {self._t} of {self.horizon} complete steps")
        if trainer.episode_starts != "frame":
            raise ValueError('RolloutBuffer needs a trainer with episode_starts="frame": "chunk" mode would silently ignore the resets inside a chunk')
        if bool(self.nan_flag.item()):
            raise AssertionError("a sampled action's log-prob was NaN during this rollout")
        pol = self.policy
        img = obs["img"] if isinstance(obs, dict) else obs
        first = self._device_flags(first)
        aliased = self._aliases_step_graph(state)
        if aliased:
            self._save_state(len(self._bounds), state)
        last_value = pol.v({"img": img}, first, state)
        if aliased:
            for (m, (k, v)), (m_s, (k_s, v_s)) in zip(state, self._states[-1]):
                k.copy_(k_s); v.copy_(v_s); m.copy_(m_s)
        self.advantage, self.value_target = trainer.advantages(self.reward, self.vpred, self.first, last_value, first)
        self._finished = True
        return self.advantage, self.value_target

    # ---- what the trainer reads -----------------------------------------------------------------
    def _tensors(self):
        return dict(img=self.img, first=self.first, act_buttons=self.act_buttons, act_camera=self.act_camera, old_log_prob=self.old_log_prob,
                    advantage=self.advantage, value_target=self.value_target)

    def chunks(self):
        """The T / L chunks as dicts with exactly PPOTrainer.step's argument names (CHUNK_KEYS): views of [B, k L:(k + 1) L], no copies; state_in is the
        buffer's own copy of the state before frame k L.  Valid until the next begin()."""
        if not self._finished:
            raise RuntimeError("RolloutBuffer.chunks() before finish(): the advantages are not there yet")
        return list(_chunks(self._tensors(), self._states[:len(self._bounds)], self._bounds))

    @torch.no_grad()
    def prior_logprobs(self, trainer, prior, prior_state=None):
        """The frozen prior's log-probs of every chunk -> ([(lp_buttons, lp_camera)] one entry per chunk, the prior's state after the rollout).  The prior
        carries ITS OWN recurrent state from chunk to chunk (prior_state: where it stood before this rollout; None: prior.initial_state)."""
        if not self._finished:
            raise RuntimeError("RolloutBuffer.prior_logprobs() before finish()")
        state = prior.initial_state(self.num_envs) if prior_state is None else prior_state
        lps = []
        for lo, hi in self._bounds:
            qb, qc, state = trainer.prior_logprobs(prior, self.img[:, lo:hi], self.first[:, lo:hi], state)
            lps.append((qb, qc))
        return lps, state

    @torch.no_grad()
    def snapshot(self) -> RolloutSnapshot:
        """A detached copy of the finished rollout for the PPG auxiliary phase (clones of every tensor chunks() hands out, the states included)."""
        if not self._finished:
            raise RuntimeError("RolloutBuffer.snapshot() before finish()")
        n = len(self._bounds)
        states = [self.policy._state_views(f.clone(), self.num_envs) for f in self._flat[:n]]
        return RolloutSnapshot({k: v.clone() for k, v in self._tensors().items()}, states, list(self._bounds))

    def episode_stats(self) -> dict:
        """dict(episodes, return_mean, length_mean) over the episodes that finished in the current rollout so far: torch sums over done_return /
        done_length, read back in one transfer -- the one method besides finish() that synchronises.  No finished episode: the means are 0."""
        t = self._t
        n = (self.done_length[:, :t] > 0).sum().double()
        tot = torch.stack([n, self.done_return[:, :t].sum().double(), self.done_length[:, :t].sum().double()]).tolist()
        episodes = int(tot[0])
        return dict(episodes=episodes, return_mean=tot[1] / episodes if episodes else 0.0, length_mean=tot[2] / episodes if episodes else 0.0)
