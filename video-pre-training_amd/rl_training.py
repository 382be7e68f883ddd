"""Reinforcement-learning fine-tuning of the cloned policy on MI355X: the third stage of the VPT method (clone -> label -> FINE-TUNE).

The reference ships no RL training script; it ships what such a step is made of -- the heads' logprob / entropy / kl_divergence
(lib/action_head.py:176-203,252-275), the value head whose loss lives in normalised space (lib/scaled_mse_head.py:37-43) and its EWMA normaliser
(lib/normalize_ewma.py:33-55) -- and MinecraftAgentPolicy.act returns the `log_prob` and `vpred` a rollout stores.  The step here is PPO with an
auxiliary KL to the frozen pre-trained policy, per frame r of a [B, T] chunk:

    rho  = exp(log pi(a_r) - old_log_prob_r)
    L_r  = -min(rho A, clamp(rho, 1 - clip, 1 + clip) A) + kl_coef KL(pi || prior) - entropy_coef H(pi) + value_coef (v - normalise(target))^2
    loss = sum w_r L_r / sum w_r

KL and H are summed over the two heads.  One launch (ops.rl_loss) turns the head log-probs into dz, the per-frame records and their totals; everything
below the head logits is BCTrainer's: forward_saving, backward_from(value_grads=True), the fused Adam launch and the fp16 loss scaling.  Advantages come
from ops.gae (one launch per rollout).  Data-parallel steps and logit masks are not built.

VPT's fine-tuning is PHASIC policy gradient: after every few policy-phase iterations an auxiliary ("sleep") phase keeps fitting the value head on the
stored returns through the whole shared trunk, the policy held at a snapshot taken just before the phase (policy_snapshot):

    L_r  = clone_coef KL(pi_old || pi) + aux_value_coef (v - normalise(target))^2

One network, one value head (PPG's single-network variant, what the released models are).  aux_step is that phase's step: one launch
(ops.ppg_aux_loss, one sweep over the two rows of log-probs) between the same forward and backward, the same Adam moments and step count."""
import math
from typing import Optional

import torch
import torch.distributed as dist

from . import ops
from .training import BCTrainer

METRICS = ("loss", "pg_loss", "kl_buttons", "kl_camera", "entropy_buttons", "entropy_camera", "value_loss", "clip_frac", "approx_kl", "ratio_mean",
           "weight_sum", "frames")
AUX_METRICS = ("loss", "clone_kl_buttons", "clone_kl_camera", "value_loss", "teacher_mass_buttons", "teacher_mass_camera", "weight_sum", "frames")


class PPOTrainer(BCTrainer):
    def __init__(self, policy, clip: float = 0.2, kl_coef: float = 0.0, entropy_coef: float = 0.0, value_coef: float = 0.5, gamma: float = 0.999,
                 lam: float = 0.95, normalize_advantages: bool = True, update_value_normalizer: bool = True, clone_coef: float = 1.0,
                 aux_value_coef: Optional[float] = None, **bc_kwargs):
        """clip: the ratio's clipping range; kl_coef: weight of KL(pi || prior) (needs prior_lp in every call when > 0); entropy_coef: entropy bonus;
        value_coef: weight of the squared value error in normalised space; gamma, lam: advantages()'s discount and GAE lambda.
        normalize_advantages: (A - mean) / (std + 1e-8) over the weighted frames of the call (the population std).
        update_value_normalizer: every loss_and_grads / step first feeds its value targets to the value head's EWMA normaliser, as the reference's
        ScaledMSEHead.loss does in training mode (lib/scaled_mse_head.py:43 -> lib/normalize_ewma.py:37-52), then normalises with the new statistics.
        clone_coef, aux_value_coef: the auxiliary phase's weights of KL(pi_old || pi) and of the squared value error (aux_step; None: value_coef);
        nothing outside the aux_* methods reads them.
        bc_kwargs: BCTrainer's arguments (lr, weight_decay, betas, eps, train_cnn, optimizer_state, loss_scale, scale_growth_interval, episode_starts,
        max_grad_norm -- global-norm gradient clipping, off by default; trainable, param_groups, decoupled_weight_decay -- partial fine-tuning, e.g.
        trainable=["pi_head", "value_head"]; see there).
        The value head's Linear trains here (BCTrainer excludes it: it has no gradient under the BC loss)."""
        super().__init__(policy, **bc_kwargs)
        self.clip, self.kl_coef, self.entropy_coef, self.value_coef = float(clip), float(kl_coef), float(entropy_coef), float(value_coef)
        self.gamma, self.lam = float(gamma), float(lam)
        self.normalize_advantages, self.update_value_normalizer = bool(normalize_advantages), bool(update_value_normalizer)
        self.clone_coef = float(clone_coef)
        self.aux_value_coef = self.value_coef if aux_value_coef is None else float(aux_value_coef)

    def _is_trainable(self, name: str) -> bool:
        if name.startswith("value_head.linear."):
            return True
        return super()._is_trainable(name)      # (the normaliser's buffers stay out: they move by update(), not by gradients)

    @staticmethod
    def _single_rank():
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("PPOTrainer: data-parallel steps are not built (torch.distributed is initialised with more than one rank)")

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def advantages(self, reward, value, first, last_value, next_first):
        """GAE over a [B, T] rollout -> (advantage, value_target) fp32 [B, T].  value, last_value: denormalised predictions (act()'s `vpred`);
        first[b, t]: frame t starts an episode; next_first [B]: so does the frame after the rollout (its value is last_value)."""
        dev = reward.device
        f32 = lambda x: torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()
        reward = f32(reward)
        b = reward.shape[0]
        return ops.gae(reward, f32(value), torch.as_tensor(first).to(dev), f32(last_value).reshape(b), torch.as_tensor(next_first).to(dev).reshape(b),
                       gamma=self.gamma, lam=self.lam)

    @torch.no_grad()
    def prior_logprobs(self, prior_policy, img_u8, first, state_in):
        """The frozen prior's log-probs of a chunk -> (lp_buttons [M, nb], lp_camera [M, nc], state_out): its inference forward, as evaluate runs
        the policy's; nothing is saved.  state_in / state_out are the PRIOR's recurrent state."""
        prior_policy._ensure_packed()
        eng = prior_policy._engine
        m = img_u8.shape[0] * img_u8.shape[1]
        out = eng.forward(img_u8, first, state_in, episode_starts=self.episode_starts)
        return out["buttons"].reshape(m, eng.n_buttons), out["camera"].reshape(m, eng.n_camera), out["state_out"]

    # ------------------------------------------------------------------------------------------
    def _frame_inputs(self, img_u8, act_buttons, act_camera, old_log_prob, advantage, value_target, prior_lp, frame_weight, global_weight=None):
        """Validation + flattening shared by loss_and_grads and evaluate -> dict of [M] device tensors, w / wsum, the priors.
        global_weight: the weight sum of a larger batch these frames are a part of; it becomes `wsum` (the advantages' normalisation, when on, still
        runs over THIS call's frames under this call's own sum), and all-zero weights of this call are then legal."""
        self._single_rank()
        if self.kl_coef > 0 and prior_lp is None:
            raise ValueError("PPOTrainer: kl_coef > 0 needs prior_lp = (lp_buttons, lp_camera) of the frozen prior (prior_logprobs)")
        m = img_u8.shape[0] * img_u8.shape[1]
        dev = img_u8.device
        w, wsum = None, float(m)
        if frame_weight is not None:
            w, wsum = self._checked_weights(frame_weight, img_u8)
            if wsum == 0 and global_weight is None:
                raise ValueError("frame_weight: every weight is zero (the loss sum w L / sum w is undefined)")
        f32 = lambda x, nme: self._per_frame(x, m, dev, nme)
        adv = f32(advantage, "advantage")
        if self.normalize_advantages:
            adv = self._normalized(adv, w, wsum)
        if global_weight is not None:
            wsum = float(global_weight)
        qb = qc = None
        if prior_lp is not None:
            qb, qc = (q.reshape(m, -1).to(torch.float32).contiguous() for q in prior_lp)
        return dict(m=m, w=w, wsum=wsum, qb=qb, qc=qc, adv=adv, old=f32(old_log_prob, "old_log_prob"), target=f32(value_target, "value_target"),
                    ab=act_buttons.reshape(m).to(torch.int64).contiguous(), ac=act_camera.reshape(m).to(torch.int64).contiguous())

    @staticmethod
    def _per_frame(x, m, dev, name):
        x = torch.as_tensor(x)
        if x.numel() != m:
            raise ValueError(f"{name} must hold one value per frame ({m}), got {tuple(x.shape)}")
        return x.reshape(m).to(device=dev, dtype=torch.float32).contiguous()

    @staticmethod
    def _normalized(adv, w, wsum):
        """(A - mean) / (std + 1e-8) over the weighted frames (population moments; a zero-weight frame counts nothing and keeps a finite value)."""
        if w is None:
            mean = adv.mean()
            std = ((adv - mean) ** 2).mean().sqrt()
            return (adv - mean) / (std + 1e-8)
        live = w != 0
        a = torch.where(live, adv, torch.zeros_like(adv))
        mean = (w * a).sum() / wsum
        std = ((w * (a - mean) ** 2).sum() / wsum).sqrt()
        return torch.where(live, (a - mean) / (std + 1e-8), torch.zeros_like(a))

    def _value_norm(self, target, w, update: bool = True):
        """The optional normaliser update, then (mean, std) as a device pair: torch ops on the buffers, no host transfer."""
        nrm = self.policy.value_head.normalizer
        if update and self.update_value_normalizer:
            nrm.update(target.reshape(-1, *nrm.running_mean.shape), weight=w)
        mean, var = nrm.running_mean_var()
        return torch.stack([mean.reshape(-1)[0], torch.sqrt(var).reshape(-1)[0]]).to(torch.float32).contiguous()

    def _loss_gradient_scale(self, wsum: float):
        """-> (ops.rl_loss's `scale`, the frame count grad_unscale() / the Adam launch divide by).  bf16: 1 / sum w, the gradient of the mean.
        fp16: loss_scale x 2^ceil(log2 sum w) / sum w, in [loss_scale, 2 loss_scale): the mean's 1 / sum w is folded in and its power-of-two part
        taken out again.  The 16-bit gradient buffers then hold magnitudes that do not depend on the batch size (why BCTrainer leaves 1 / frames
        out altogether), and dz carries the significands that autograd of the MEAN loss produces at the boundary of lib/policy.py, whose lift is
        a power of two as well: the two routes round to 16 bits at the same points (tests/test_gpu_rl_training.py (g))."""
        if not self.scaled:
            return 1.0 / wsum, wsum
        pow2 = 2.0 ** math.ceil(math.log2(wsum))
        return self.loss_scale * (pow2 / wsum), pow2

    def _loss_of(self, totals):
        return (totals[0] + self.kl_coef * (totals[1] + totals[2]) - self.entropy_coef * (totals[3] + totals[4]) + self.value_coef * totals[5]) / totals[10]

    def _fill_rl_metrics(self, metrics: dict, totals, frame_out, bsz: int, t: int):
        """totals [16] + the per-frame records -> the metrics dict; device arithmetic only."""
        ws = totals[10]
        metrics.update(loss=self._loss_of(totals), pg_loss=totals[0] / ws, kl_buttons=totals[1] / ws, kl_camera=totals[2] / ws,
                       entropy_buttons=totals[3] / ws, entropy_camera=totals[4] / ws, value_loss=totals[5] / ws, ratio_mean=totals[6] / ws,
                       clip_frac=totals[7] / ws, approx_kl=totals[9] / ws, weight_sum=ws, frames=totals[11], frame_out=frame_out.view(bsz, t, 16))

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def loss_and_grads(self, img_u8, first, state_in, act_buttons, act_camera, old_log_prob, advantage, value_target, *, prior_lp=None,
                       frame_weight=None, metrics: Optional[dict] = None, unscaled: bool = True, global_weight: Optional[float] = None,
                       micro_batches: int = 1):
        """Forward (saving activations) + the fused loss + backward.  Returns (loss, grads dict incl. value_head.linear.*, state_out).
        act_*, old_log_prob, advantage, value_target: [B, T] -- the taken actions, act()'s `log_prob` at rollout time, advantages()'s two outputs.
        prior_lp: (lp_buttons, lp_camera) of the frozen prior on the same frames (prior_logprobs); required when kl_coef > 0, and with kl_coef = 0 it
        still fills the KL metrics.  frame_weight: [B, T] finite non-negative weights (0: padding, whatever the frame's inputs hold).
        metrics: a dict this call fills -- loss, pg_loss, kl_buttons, kl_camera, entropy_buttons, entropy_camera, value_loss (normalised space),
        clip_frac, approx_kl (mean of old_lp - lp), ratio_mean, weight_sum, frames, frame_out fp32 [B, T, 16] -- device tensors, nothing synchronises.
        unscaled: as BCTrainer.loss_and_grads (False leaves the fp16 gradients multiplied by 1 / grad_unscale(self._global_frames), _loss_gradient_scale).
        global_weight (default: this call's own frame count / weight sum): the count of a larger batch these frames are a part of; _loss_gradient_scale
        takes it, so the gradients are this part's share of the gradient of THAT batch's mean loss (all-zero weights are then legal).  Whoever cuts
        a batch by hand normalises the advantages and updates the value normaliser over the whole batch first, with both switches of this trainer off.
        micro_batches=K > 1 (gradient accumulation): the advantages' normalisation, the value normaliser's update and
        _loss_gradient_scale run ONCE on the whole batch; then the B sequences run as K row groups (micro_batch_rows) one after the other under that
        one (mean, std) pair and scale, their gradients summed in order (ops.grad_accumulate_).  The loss is _loss_of the groups' totals summed in
        fp64; frame_out and state_out are the row-wise concatenations."""
        rows = self.micro_batch_rows(img_u8.shape[0], micro_batches) if micro_batches != 1 else None
        f = self._frame_inputs(img_u8, act_buttons, act_camera, old_log_prob, advantage, value_target, prior_lp, frame_weight, global_weight)
        bsz, t = img_u8.shape[:2]
        if rows is None:
            S = self.forward_saving(img_u8, first, state_in)
            vnorm = self._value_norm(f["target"], f["w"])
            scale, self._global_frames = self._loss_gradient_scale(f["wsum"])
            g, totals, frame_out, state_out = self._loss_and_backward(S, f, vnorm, scale)
        else:
            vnorm = self._value_norm(f["target"], f["w"])
            scale, self._global_frames = self._loss_gradient_scale(f["wsum"])
            first = torch.as_tensor(first)

            def run(k, lo, hi):
                fk = {q: (x[lo * t:hi * t] if isinstance(x, torch.Tensor) else x) for q, x in f.items()}
                S = self.forward_saving(img_u8[lo:hi], first[lo:hi], self._tree_rows(state_in, lo, hi))
                return self._loss_and_backward(S, fk, vnorm, scale)

            g, totals, frame_out, states = self._accumulated_window(rows, run)
            state_out = self._tree_cat_rows(states)
        self._rl_totals = totals
        loss = self._loss_of(totals)
        if metrics is not None:
            self._fill_rl_metrics(metrics, totals, frame_out, bsz, t)
        if unscaled and self.scaled:
            self._unscale_(g, self._global_frames)
        return loss, g, state_out

    def _loss_and_backward(self, S, f, vnorm, scale):
        """ops.rl_loss on a saving forward's log-probs and the backward behind it -> (grads, totals [16], records [M, 16], state_out).
        f: _frame_inputs's dict (or its rows); vnorm, scale: _value_norm's pair and _loss_gradient_scale's factor."""
        nb, nc = self.engine.n_buttons, self.engine.n_camera
        dz, frame_out, totals = ops.rl_loss(S["lp_b"], S["lp_c"], f["ab"], f["ac"], f["old"], f["adv"], S["ldz"], scale, prior_buttons=f["qb"],
                                            prior_camera=f["qc"], value=S["logits"][:, nb + nc], value_target=f["target"], vnorm=vnorm, weight=f["w"],
                                            clip=self.clip, kl_coef=self.kl_coef, entropy_coef=self.entropy_coef, value_coef=self.value_coef,
                                            temperature=self.engine.cfg["temperature"], dtype=self.dtype)
        return self.backward_from(S, dz, value_grads=True), totals, frame_out, S["state_out"]

    @torch.no_grad()
    def evaluate(self, img_u8, first, state_in, act_buttons, act_camera, old_log_prob, advantage, value_target, *, prior_lp=None, frame_weight=None):
        """Forward-only loss and metrics of a [B, T] chunk -> (metrics dict as loss_and_grads fills it, state_out): the inference forward + ops.rl_loss
        without dz.  The value normaliser is NOT updated."""
        f = self._frame_inputs(img_u8, act_buttons, act_camera, old_log_prob, advantage, value_target, prior_lp, frame_weight)
        eng = self.engine
        bsz, t = img_u8.shape[:2]
        m = bsz * t
        with self._adapters_applied():
            self.policy._ensure_packed()
            out = eng.forward(img_u8, first, state_in, episode_starts=self.episode_starts)
        lp_b, lp_c = out["buttons"].reshape(m, eng.n_buttons), out["camera"].reshape(m, eng.n_camera)
        vnorm = self._value_norm(f["target"], f["w"], update=False)
        _, frame_out, totals = ops.rl_loss(lp_b, lp_c, f["ab"], f["ac"], f["old"], f["adv"], 0, 0.0, prior_buttons=f["qb"], prior_camera=f["qc"],
                                           value=out["vpred"].reshape(m), value_target=f["target"], vnorm=vnorm, weight=f["w"], clip=self.clip,
                                           kl_coef=self.kl_coef, entropy_coef=self.entropy_coef, value_coef=self.value_coef,
                                           temperature=eng.cfg["temperature"], dtype=self.dtype, want_dz=False)
        metrics: dict = {}
        self._fill_rl_metrics(metrics, totals, frame_out, bsz, t)
        return metrics, out["state_out"]

    @torch.no_grad()
    def step(self, img_u8, first, state_in, act_buttons, act_camera, old_log_prob, advantage, value_target, *, prior_lp=None, frame_weight=None,
             metrics: Optional[dict] = None, micro_batches: int = 1):
        """One optimiser step on a [B, T] chunk.  Returns (loss, state_out).  micro_batches=K: loss_and_grads's gradient accumulation over K row
        groups; one Adam launch, clip and loss-scale decision for the window.  The Adam launch, the optional gradient-norm clip and the loss-scale
        bookkeeping are BCTrainer.step's (TrainerBase._optimizer_tail; metrics gains grad_norm / clip_coef / grad_norm_per_tensor when max_grad_norm is set)."""
        self._need_optimizer_state()
        loss, grads, state_out = self.loss_and_grads(img_u8, first, state_in, act_buttons, act_camera, old_log_prob, advantage, value_target,
                                                     prior_lp=prior_lp, frame_weight=frame_weight, metrics=metrics, unscaled=False,
                                                     micro_batches=micro_batches)
        loss, _ = self._optimizer_tail(loss, grads, self.grad_unscale(self._global_frames), img_u8.device, metrics)
        return loss, state_out

    # ---- the auxiliary ("sleep") phase of phasic policy gradient ("The auxiliary phase") ---------------------------------------
    @torch.no_grad()
    def policy_snapshot(self, img_u8, first, state_in):
        """pi_old of an auxiliary phase: the trainer's OWN policy through its inference forward (prior_logprobs applied to self.policy)
        -> (lp_buttons [M, nb], lp_camera [M, nc], state_out), fp32 (64 x 128 frames: 287 MB).  Taken once per phase, before the first aux_step; the
        tensors do not follow the weights afterwards.  Take it under the same logit masks as the steps that use it."""
        with self._adapters_applied():      # (with adapters pi_old is base + adapters; prior_logprobs(self.policy, ...) alone is the frozen base)
            return self.prior_logprobs(self.policy, img_u8, first, state_in)

    def _aux_inputs(self, img_u8, old_lp, value_target, frame_weight, global_weight=None):
        """Validation + flattening shared by aux_loss_and_grads and aux_evaluate -> dict of [M] / [M, n] device tensors, w / wsum."""
        self._single_rank()
        if old_lp is None or len(old_lp) != 2 or old_lp[0] is None or old_lp[1] is None:
            raise ValueError("PPOTrainer: the auxiliary phase needs old_lp = (lp_buttons, lp_camera) of the snapshot (policy_snapshot)")
        m = img_u8.shape[0] * img_u8.shape[1]
        w, wsum = None, float(m)
        if frame_weight is not None:
            w, wsum = self._checked_weights(frame_weight, img_u8)
            if wsum == 0 and global_weight is None:
                raise ValueError("frame_weight: every weight is zero (the loss sum w L / sum w is undefined)")
        if global_weight is not None:
            wsum = float(global_weight)
        ob, oc = (q.reshape(m, -1).to(torch.float32).contiguous() for q in old_lp)
        if ob.shape[1] != self.engine.n_buttons or oc.shape[1] != self.engine.n_camera:
            raise ValueError(f"old_lp must hold [{m}, {self.engine.n_buttons}] and [{m}, {self.engine.n_camera}] log-probs, got {tuple(ob.shape)} and {tuple(oc.shape)}")
        return dict(m=m, w=w, wsum=wsum, ob=ob, oc=oc, target=self._per_frame(value_target, m, img_u8.device, "value_target"))

    def _aux_value_norm(self, target, w, update: bool):
        """(mean, std) as a device pair; update=True first feeds the targets to the normaliser (whatever the policy phase's switch says)."""
        if update:
            nrm = self.policy.value_head.normalizer
            nrm.update(target.reshape(-1, *nrm.running_mean.shape), weight=w)
        return self._value_norm(target, w, update=False)

    def _aux_loss_of(self, totals):
        """The weighted mean loss from ops.ppg_aux_loss's totals; a term whose coefficient is 0 is left out (not multiplied by 0), as in the kernel."""
        loss = torch.zeros((), dtype=torch.float32, device=totals.device)
        if self.clone_coef != 0:
            loss = loss + self.clone_coef * (totals[0] + totals[1])
        if self.aux_value_coef != 0:
            loss = loss + self.aux_value_coef * totals[2]
        return loss / totals[5]

    def _fill_aux_metrics(self, metrics: dict, totals, frame_out, bsz: int, t: int):
        """totals [8] + the per-frame records -> the AUX_METRICS dict; device arithmetic only."""
        ws = totals[5]
        metrics.update(loss=self._aux_loss_of(totals), clone_kl_buttons=totals[0] / ws, clone_kl_camera=totals[1] / ws, value_loss=totals[2] / ws,
                       teacher_mass_buttons=totals[3] / ws, teacher_mass_camera=totals[4] / ws, weight_sum=ws, frames=totals[6],
                       frame_out=frame_out.view(bsz, t, 8))

    def _aux_loss_and_backward(self, S, f, vnorm, scale):
        """ops.ppg_aux_loss on a saving forward's log-probs and the backward behind it -> (grads, totals [8], records [M, 8], state_out)."""
        nb, nc = self.engine.n_buttons, self.engine.n_camera
        dz, frame_out, totals = ops.ppg_aux_loss(S["lp_b"], S["lp_c"], f["ob"], f["oc"], S["ldz"], scale, value=S["logits"][:, nb + nc],
                                                 value_target=f["target"], vnorm=vnorm, weight=f["w"], clone_coef=self.clone_coef,
                                                 value_coef=self.aux_value_coef, temperature=self.engine.cfg["temperature"], dtype=self.dtype)
        return self.backward_from(S, dz, value_grads=True), totals, frame_out, S["state_out"]

    @torch.no_grad()
    def aux_loss_and_grads(self, img_u8, first, state_in, old_lp, value_target, *, frame_weight=None, metrics: Optional[dict] = None,
                           unscaled: bool = True, global_weight: Optional[float] = None, micro_batches: int = 1,
                           update_value_normalizer: bool = False):
        """Forward (saving activations) + the fused auxiliary loss + backward.  Returns (loss, grads dict incl. value_head.linear.*, state_out).
            L_r = clone_coef (KL_buttons + KL_camera)(pi_old || pi) + aux_value_coef (v - normalise(target))^2,   loss = sum w_r L_r / sum w_r
        old_lp: (lp_buttons, lp_camera) of the snapshot on the same frames (policy_snapshot), [M, n] or [B, T, n]; value_target: [B, T], the stored
        returns.  frame_weight, unscaled, global_weight, micro_batches: as loss_and_grads takes them (the scale and the (mean, std) pair are computed
        once for the whole batch, old_lp is cut by rows).  update_value_normalizer: feed the targets to the value normaliser first -- off by
        default, the policy phase has already seen these targets.  metrics: a dict this call fills with AUX_METRICS + frame_out fp32 [B, T, 8]
        (D_b, D_c, (v - t^)^2, S_b, S_c, w, w > 0, 0): device tensors, nothing synchronises.
        The gradient of the clone term is p - pi_old, exact for a snapshot whose mass is 1 (teacher_mass_* report it)."""
        rows = self.micro_batch_rows(img_u8.shape[0], micro_batches) if micro_batches != 1 else None
        f = self._aux_inputs(img_u8, old_lp, value_target, frame_weight, global_weight)
        bsz, t = img_u8.shape[:2]
        if rows is None:
            S = self.forward_saving(img_u8, first, state_in)
            vnorm = self._aux_value_norm(f["target"], f["w"], update_value_normalizer)
            scale, self._global_frames = self._loss_gradient_scale(f["wsum"])
            g, totals, frame_out, state_out = self._aux_loss_and_backward(S, f, vnorm, scale)
        else:
            vnorm = self._aux_value_norm(f["target"], f["w"], update_value_normalizer)
            scale, self._global_frames = self._loss_gradient_scale(f["wsum"])
            first = torch.as_tensor(first)

            def run(k, lo, hi):
                fk = {q: (x[lo * t:hi * t] if isinstance(x, torch.Tensor) else x) for q, x in f.items()}
                S = self.forward_saving(img_u8[lo:hi], first[lo:hi], self._tree_rows(state_in, lo, hi))
                return self._aux_loss_and_backward(S, fk, vnorm, scale)

            g, totals, frame_out, states = self._accumulated_window(rows, run)
            state_out = self._tree_cat_rows(states)
        self._aux_totals = totals
        loss = self._aux_loss_of(totals)
        if metrics is not None:
            self._fill_aux_metrics(metrics, totals, frame_out, bsz, t)
        if unscaled and self.scaled:
            self._unscale_(g, self._global_frames)
        return loss, g, state_out

    @torch.no_grad()
    def aux_evaluate(self, img_u8, first, state_in, old_lp, value_target, *, frame_weight=None):
        """Forward-only auxiliary loss and metrics of a [B, T] chunk -> (metrics dict as aux_loss_and_grads fills it, state_out): the inference
        forward + ops.ppg_aux_loss without dz.  The value normaliser is NOT updated."""
        f = self._aux_inputs(img_u8, old_lp, value_target, frame_weight)
        eng = self.engine
        bsz, t = img_u8.shape[:2]
        m = bsz * t
        with self._adapters_applied():
            self.policy._ensure_packed()
            out = eng.forward(img_u8, first, state_in, episode_starts=self.episode_starts)
        lp_b, lp_c = out["buttons"].reshape(m, eng.n_buttons), out["camera"].reshape(m, eng.n_camera)
        vnorm = self._value_norm(f["target"], f["w"], update=False)
        _, frame_out, totals = ops.ppg_aux_loss(lp_b, lp_c, f["ob"], f["oc"], 0, 0.0, value=out["vpred"].reshape(m), value_target=f["target"], vnorm=vnorm,
                                                weight=f["w"], clone_coef=self.clone_coef, value_coef=self.aux_value_coef,
                                                temperature=eng.cfg["temperature"], dtype=self.dtype, want_dz=False)
        metrics: dict = {}
        self._fill_aux_metrics(metrics, totals, frame_out, bsz, t)
        return metrics, out["state_out"]

    @torch.no_grad()
    def aux_step(self, img_u8, first, state_in, old_lp, value_target, *, frame_weight=None, metrics: Optional[dict] = None, micro_batches: int = 1,
                 update_value_normalizer: bool = False):
        """One optimiser step of the auxiliary phase on a [B, T] chunk.  Returns (loss, state_out).  The Adam moments, the step count, the
        max_grad_norm clip and the loss-scale bookkeeping are step()'s own (TrainerBase._optimizer_tail): one optimiser, as in single-network PPG."""
        self._need_optimizer_state()
        loss, grads, state_out = self.aux_loss_and_grads(img_u8, first, state_in, old_lp, value_target, frame_weight=frame_weight, metrics=metrics,
                                                         unscaled=False, micro_batches=micro_batches, update_value_normalizer=update_value_normalizer)
        loss, _ = self._optimizer_tail(loss, grads, self.grad_unscale(self._global_frames), img_u8.device, metrics)
        return loss, state_out
