"""Behavioural-cloning step on MI355X (behavioural_cloning.py:86-123 generalised to [B, T] chunks).

    loss = -mean_{b,t}[ log pi(buttons_bt) + log pi(camera_bt) ]      (lib/action_head.py:176-184,252-253)
    th.optim.Adam(lr=1.81e-4, weight_decay=0.039428)                   (behavioural_cloning.py:38-40,63-67)
    gradient clipping: none by default -- the reference's clip_grad_norm_ receives an exhausted generator and is a no-op
                       (behavioural_cloning.py:60,63,121; SURVEY.md §2 'latent bugs'); BCTrainer(max_grad_norm=5.0) applies what the
                       script meant, on the device (ops.grad_norm's launches + the coefficient inside the Adam launch)
    state: the KV memory is carried between chunks detached (behavioural_cloning.py:111)

Every layer's backward runs on the HIP kernels: both action heads, final_ln, lastlayer, the four transformer blocks
(attention incl. the relative-position bias and b_nd, MLPs, LayerNorms), ImgObsProcess.linear + its LayerNorm
(vpt_gemm_kernel as dgrad / wgrad, vpt_attn_bwd_kernel, vpt_ln_bwd_kernel, vpt_nll_bwd_kernel), and -- with
train_cnn=True, the reference's behaviour (behavioural_cloning.py:57-63 trains every parameter) -- the IMPALA CNN:
dense layer GEMMs, per-element / per-channel affine backward, max-pool routing, the folded GroupNorm convolutions
(vpt_conv_bwd_prep_kernel -> vpt_conv3x3_kernel in dgrad mode + vpt_conv_wgrad_kernel -> conv_param_grads) and the
fused first conv (vpt_conv_first_bwd_kernel).  train_cnn=False freezes `net.img_process.cnn.*` and fine-tunes the
trunk and heads only (71 % of the 2x model's parameters).  Data parallelism: one process per GPU, sequences sharded by rank, the
gradients summed over RCCL in buckets -- trunk + heads while the CNN backward runs, the CNN's at the end
(BCTrainer.reduced_loss_and_grads); the 1 / global_frames factor is already in the loss gradient."""
import contextlib
import os
from typing import Dict, List, Optional

import torch
import torch.distributed as dist

from . import distributed as D
from . import ops, packing
from .cnn_training import CnnTrainingMixin, _tap_sum, conv_param_grads  # noqa: F401  (conv_param_grads: this module's long-standing name for it)
from .engine import DENSE_SPLITK, EpisodeMasks, check_episode_starts


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def linear_backward(dy16: torch.Tensor, n: int, x16: Optional[torch.Tensor], weight: torch.Tensor, need_dx: bool = True,
                    res: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                    dx_f32: bool = True, dx_bf16_ld: Optional[int] = None, need_dw: bool = True):
    """Backward of y = x W^T on the MFMA GEMM kernel.
    dy16: bf16 [M, Np] (Np >= n, Np % 64 == 0, padding zero); x16: bf16 [M, K]; weight fp32 [n, K].
    Returns (dx fp32 or None, dx bf16 or None, dW fp32 [n, K] or None).
    dgrad:  dx = dy W      -> GEMM(A = dy, weights = W^T packed), optional ReLU gate `mask` and skip-sum `res`;
    wgrad:  dW = dy^T x    -> the TN GEMM (ops.linear_wgrad): both operands row-major over the M frames, no transposes."""
    m, np_ = dy16.shape
    k = weight.shape[1]
    dev = dy16.device
    dx32 = dx16 = dw = None
    if need_dx:   # W^T packed straight from the fp32 master by one kernel (was: zero, transpose, cast, permute -- four tensor ops)
        wt = ops.pack_linear(weight.contiguous(), transposed=True, k_pad=np_, dtype=dy16.dtype)
        dx32, dx16 = ops.linear(dy16, wt, k, res=res, mask=mask, out_f32=dx_f32,
                                out_bf16=dx_bf16_ld is not None, out_bf16_ld=dx_bf16_ld)
        del wt
    if need_dw:       # dW = dy^T x straight from the row-major activations (vpt_gemm_tn_kernel: LDS transpose reads, no copies)
        dw = ops.linear_wgrad(dy16, x16, np_)[:n]
    return dx32, dx16, dw


class BCTrainer(CnnTrainingMixin):
    def __init__(self, policy, lr: float = 0.000181, weight_decay: float = 0.039428, betas=(0.9, 0.999), eps: float = 1e-8,
                 train_cnn: bool = True, optimizer_state: bool = True, loss_scale: Optional[float] = None,
                 scale_growth_interval: int = 200, episode_starts: str = "chunk", max_grad_norm: Optional[float] = None):
        """max_grad_norm: None (default: no clipping -- the reference's actual behaviour, its clip_grad_norm_ call receives an exhausted generator),
        5.0 (MAX_GRAD_NORM, what behavioural_cloning.py:38-40,121 meant) or float("inf") (measure the norm, never clip).  When set, step() takes the
        global l2 norm of the gradients of the mean loss on the device -- after the all-reduce, un-scaled: neither fp16's loss scale nor 1 / frames
        reaches the threshold -- and the Adam launch multiplies by torch's clip coefficient; `metrics` gains grad_norm, clip_coef and
        grad_norm_per_tensor, `last_grad_norm` keeps the norm.  A non-finite norm SKIPS the step on the device in both operand formats
        (skipped_steps; fp16 also halves its loss scale) where torch would write NaN into every parameter (CnnTrainingMixin._optimizer_tail).
        episode_starts: "chunk" (default: first[:, 0] only) or "frame": `first` honoured at every frame of the chunk, forward and backward,
        so that chunks cut from a stream of recordings of arbitrary length (sequence_batcher.SequenceBatcher) train as the reference's
        frame-by-frame loop does (behavioural_cloning.py:95-112).
        train_cnn=True (default, as the reference: behavioural_cloning.py:57-63 optimises policy.parameters(), i.e. every
        parameter) or False to freeze `net.img_process.cnn.*` and fine-tune trunk + heads only (no CNN activations kept).
        optimizer_state=False: gradients only (the autograd boundary of lib/policy.py), no Adam moments allocated.

        Both operand formats train.  precision="fp16" (the parity mode) keeps every 16-bit gradient buffer -- dz, the GEMM /
        conv operands dacc, the inter-layer dx -- inside IEEE half's range by LOSS SCALING: the loss gradient is written as
        (loss_scale / temperature) x (softmax - one-hot) per frame, i.e. the 1 / global_frames of the mean is left out as well, so
        the magnitudes in the 16-bit buffers do not depend on the batch size; vpt_adam_step_multi multiplies the fp32 gradients by
        1 / (loss_scale x global_frames).  `loss_scale` (default 256 for fp16, 1 = off for bf16) is dynamic as in
        torch.cuda.amp.GradScaler: vpt_grads_nonfinite_multi checks the (all-reduced) gradients; an overflowed step is skipped on
        the device (the Adam launch reads the flag) and the scale halves, it doubles after `scale_growth_interval` clean steps."""
        self.train_cnn = bool(train_cnn)
        self.max_grad_norm = self._checked_max_grad_norm(max_grad_norm)
        self.episode_starts = check_episode_starts(episode_starts)
        self.policy = policy
        self.engine = policy._engine
        self.dtype = self.engine.dtype
        self.scaled = self.engine.precision == "fp16"
        self.loss_scale = float(loss_scale) if loss_scale is not None else (256.0 if self.scaled else 1.0)
        self.scale_growth_interval, self._clean_steps, self.skipped_steps = int(scale_growth_interval), 0, 0
        # the autograd boundary's counterpart of loss_scale (lib/policy.py:_PolicyForwardFn.backward): where the largest incoming
        # gradient element is lifted to before it enters the 16-bit buffers; halved on every overflow it detects
        self.autograd_lift, self.autograd_overflows = 256.0, 0
        self.lr, self.wd, self.betas, self.eps = lr, weight_decay, betas, eps
        self.step_count = 0
        # Frame chunks of the CNN (forward-saving AND backward) alternate over this many HIP streams, chunk ci always on stream
        # ci % n: one chunk's HBM-bound passes (conv_backward_prepare, the affine backward, pool) and launch tails overlap the
        # other chunks' MFMA-bound convolutions, as in the inference engine.  Each stream accumulates its weight-gradient pieces in
        # its own buffers, merged in stream order at the end (the merge order is fixed; WITHIN a buffer the wgrad / first-conv kernels
        # add their per-workgroup pieces with fp32 atomics in arrival order, so the last bits of the stack-0 gradients vary from run to
        # run -- 1e-7 relative in bf16, up to 1e-4 on heavily cancelling fp16 sums, tests/test_gpu_training.py); a chunk's saved
        # activations are allocated, used and released on ONE stream, so the caching allocator's per-stream pools need no cross-stream
        # bookkeeping.  The streams are created ONCE per trainer and only ever appended to (never replaced): the activations a
        # forward_saving() left for a later backward stay tied to the stream object that produced them.
        self.cnn_streams = int(os.environ.get("VPT_BC_STREAMS", self.engine.cnn_streams))
        self._cnn_flags_from_env()       # gated_dgrad, fused_pool, fold_n_backward, fold_n_backward0 (cnn_training.py)
        self.force_exchange = os.environ.get("VPT_DP_FORCE_EXCHANGE", "0") == "1"      # see reduced_loss_and_grads
        self._arenas = None      # (key, (GradArena trunk + heads, GradArena CNN)) of the data-parallel step, built on first use
        self._streams: List[torch.cuda.Stream] = []
        self.params: Dict[str, torch.nn.Parameter] = dict(policy.named_parameters())
        self.trainable = [n for n in self.params if self._is_trainable(n)]
        self.m = {n: torch.zeros_like(self.params[n], dtype=torch.float32) for n in self.trainable} if optimizer_state else {}
        self.v = {n: torch.zeros_like(self.params[n], dtype=torch.float32) for n in self.trainable} if optimizer_state else {}

    # ---- checkpoint / resume ---------------------------------------------------
    def state_dict(self) -> dict:
        """Optimizer state next to the policy's own `.weights` state_dict (behavioural_cloning.py:131-132 saves only the
        latter): Adam moments keyed by the reference's parameter names, the step count and the hyper-parameters."""
        self._need_optimizer_state()
        return dict(step=self.step_count, lr=self.lr, weight_decay=self.wd, betas=tuple(self.betas), eps=self.eps,
                    loss_scale=self.loss_scale, train_cnn=self.train_cnn, max_grad_norm=self.max_grad_norm,
                    exp_avg={n: t.detach().clone() for n, t in self.m.items()},
                    exp_avg_sq={n: t.detach().clone() for n, t in self.v.items()})

    def _need_optimizer_state(self):
        if not self.m and self.trainable:
            raise RuntimeError("this BCTrainer was built with optimizer_state=False (gradients only): step / state_dict / load_state_dict need the Adam moments")

    def load_state_dict(self, sd: dict):
        self._need_optimizer_state()
        if self.scaled and "loss_scale" in sd:
            self.loss_scale = float(sd["loss_scale"])
        if "max_grad_norm" in sd:           # (dicts written before the key existed keep the constructor's value)
            self.max_grad_norm = self._checked_max_grad_norm(sd["max_grad_norm"])
        if set(sd["exp_avg"]) != set(self.m):
            raise KeyError(f"optimizer state does not match the trainable parameters: {sorted(set(sd['exp_avg']) ^ set(self.m))[:4]} ...")
        self.step_count = int(sd["step"])
        self.lr, self.wd, self.betas, self.eps = sd["lr"], sd["weight_decay"], tuple(sd["betas"]), sd["eps"]
        for n in self.m:
            self.m[n].copy_(sd["exp_avg"][n])
            self.v[n].copy_(sd["exp_avg_sq"][n])

    def _is_trainable(self, name: str) -> bool:
        if name.startswith("net.img_process.cnn.") and not self.train_cnn:
            return False            # train_cnn=False: fine-tune the trunk and heads only
        if name.startswith("value_head."):
            return False            # no gradient under the BC loss; normaliser buffers are not trained
        return True

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def loss_and_grads(self, img_u8, first, state_in, act_buttons, act_camera, global_frames: Optional[float] = None, debug: Optional[dict] = None,
                       on_trunk_grads=None, unscaled: bool = True, *, frame_weight=None, metrics: Optional[dict] = None, _weight_sum=None):
        """Forward (saving activations) + backward.  Returns (loss of this rank's frames, grads dict, state_out).
        global_frames: number of frames in the global (all-rank) batch the mean runs over (default: local); with frame_weight the global
        weight sum (it may then be a float).
        frame_weight: [B, T] finite, non-negative per-frame weights: loss = sum w nll / sum w and its gradient (0 = padding or a frame left out:
        whatever its image and labels hold, it adds exact zeros); sum w and min w are read on the host before anything is queued (one transfer) --
        ValueError on a negative or non-finite weight, and on sum w == 0 unless global_frames says other ranks carry weight.
        metrics: a dict this call fills (as `debug`): loss, nll_buttons, nll_camera, acc_buttons, acc_camera, entropy_buttons, entropy_camera
        (weighted means, lib/action_head.py:176-193), weight_sum, frames (rows with w > 0), frame_nll fp32 [B, T], frame_out fp32 [B, T, 8]
        (ops.bc_loss's records) -- device tensors, nothing synchronises.  With neither, the loss path is ops.nll_backward + a gather, as ever;
        otherwise ONE ops.bc_loss launch writes dz, the per-frame records the returned loss is formed from (_record_loss) and the totals behind the
        metrics and the reduction over ranks.
        unscaled=True: the gradients of the mean loss in both operand formats.  False (what step() uses): in the fp16 mode they are
        left multiplied by 1 / grad_unscale(global_frames) -- the optimiser launch folds that factor in, no extra pass.
        on_trunk_grads(g): called once the gradients of everything behind the CNN (88 % of the parameters) are final and
        before the CNN's backward starts -- the data-parallel step starts their all-reduce there."""
        if on_trunk_grads is not None and unscaled and self.scaled:
            # the callback (an asynchronous all-reduce in the data-parallel step) would see loss-SCALED gradients that this function then
            # multiplies in place while the collective may still be reading them
            raise ValueError("loss_and_grads: on_trunk_grads needs unscaled=False in the fp16 (loss-scaled) mode; apply grad_unscale() after the exchange")
        w, wsum = None, None
        if frame_weight is not None:
            w, wsum = (frame_weight, _weight_sum) if _weight_sum is not None else self._checked_weights(frame_weight, img_u8)
            if not global_frames and wsum == 0:
                raise ValueError("frame_weight: every weight is zero (the loss sum w nll / sum w is undefined)")
        S = self.forward_saving(img_u8, first, state_in)
        m = S["m"]
        ab = act_buttons.reshape(m).to(torch.int64).contiguous()
        ac = act_camera.reshape(m).to(torch.int64).contiguous()
        gf = global_frames or (m if w is None else wsum)
        # bf16: the gradient of the global mean.  fp16: loss_scale x the gradient of the SUM over frames (see __init__); grad_unscale()
        # is the factor that turns the returned gradients into those of the mean.
        scale = (self.loss_scale if self.scaled else 1.0 / gf) / self.engine.cfg["temperature"]
        if w is None and metrics is None:
            loss = -(S["lp_b"].gather(1, ab[:, None]) + S["lp_c"].gather(1, ac[:, None])).mean()
            dz = ops.nll_backward(S["lp_b"], S["lp_c"], ab, ac, S["ldz"], scale, dtype=self.dtype)
        else:       # one sweep over the log-probs: dz, the per-frame records and their fixed-order totals
            dz, frame_out, totals = ops.bc_loss(S["lp_b"], S["lp_c"], ab, ac, S["ldz"], scale, weight=w, dtype=self.dtype)
            loss = self._record_loss(frame_out, w, wsum)        # this rank's; NaN where its shard carries no weight (reduced_loss_and_grads sums the totals)
            self._bc_totals = totals
            if metrics is not None:
                self._fill_metrics(metrics, totals, frame_out, S["bsz"], S["t"])
                metrics["loss"] = loss
        g = self.backward_from(S, dz, on_trunk_grads=on_trunk_grads, debug=debug)
        if unscaled and self.scaled:
            f = self.grad_unscale(gf)
            for t_ in g.values():
                t_.mul_(f)
        return loss, g, S["state_out"]

    def grad_unscale(self, global_frames: float) -> float:
        """What loss_and_grads' gradients must be multiplied by to be d(mean loss)/d(parameter): 1 in bf16.  (global_frames: the global weight
        sum when the step carries frame weights.)"""
        return 1.0 / (self.loss_scale * global_frames) if self.scaled else 1.0

    @staticmethod
    def _checked_weights(frame_weight, img_u8):
        """[B, T] weights -> (fp32 [M] on the images' device, their fp64 sum as a host float).  The sum and the minimum come to the host in ONE
        transfer; a negative or non-finite weight raises ValueError (a NaN makes the minimum NaN, an infinity the sum infinite)."""
        m = img_u8.shape[0] * img_u8.shape[1]
        w = torch.as_tensor(frame_weight)
        if w.numel() != m:
            raise ValueError(f"frame_weight must hold one weight per frame ([{img_u8.shape[0]}, {img_u8.shape[1]}]), got {tuple(w.shape)}")
        w = w.reshape(m).to(device=img_u8.device, dtype=torch.float32).contiguous()
        w64 = w.to(torch.float64)
        wsum, wmin = torch.stack([w64.sum(), w64.min()]).tolist()
        if not (wmin >= 0.0) or wsum != wsum or wsum in (float("inf"), float("-inf")):
            raise ValueError(f"frame_weight must be finite and non-negative (min {wmin}, sum {wsum})")
        return w, wsum

    @staticmethod
    def _record_loss(frame_out, w, wsum):
        """sum w nll / sum w of one rank from the kernel's per-frame records, in the ARITHMETIC OF THE DEFAULT PATH: per frame nll_b + nll_c (the
        negated sum of the two picked log-probs, exactly), then torch's mean over the frames, then the factor M / sum w.  With every weight 1 each
        step is the default path's own -- w x is x, the mean of the negated values is the negated mean, the factor is 1.0 -- so frame_weight=ones (and
        metrics={} alone) returns the default path's loss bit for bit; the totals' fixed tree adds the same terms in another association and lands an
        ulp away, which is why the returned loss is not read from them (they feed the metrics and the reduction over ranks).  M floats per step."""
        nll = frame_out[:, 0] + frame_out[:, 1]
        if w is None:
            return nll.mean()
        wn = torch.where(w != 0, w * nll, torch.zeros_like(nll))          # a zero-weight frame counts an exact zero whatever its record holds
        return wn.mean() * (nll.numel() / wsum if wsum else float("nan"))

    @staticmethod
    def _fill_metrics(metrics: dict, totals, frame_out, bsz: int, t: int):
        """totals [8] (ops.bc_loss's, or their sum over ranks) + this rank's records -> the metrics dict; device arithmetic only."""
        ws = totals[6]
        metrics.update(loss=(totals[0] + totals[1]) / ws, nll_buttons=totals[0] / ws, nll_camera=totals[1] / ws,
                       entropy_buttons=totals[2] / ws, entropy_camera=totals[3] / ws, acc_buttons=totals[4] / ws, acc_camera=totals[5] / ws,
                       weight_sum=ws, frames=totals[7])
        if frame_out is not None:
            metrics.update(frame_nll=(frame_out[:, 0] + frame_out[:, 1]).view(bsz, t), frame_out=frame_out.view(bsz, t, 8))

    @torch.no_grad()
    def evaluate(self, img_u8, first, state_in, act_buttons, act_camera, *, frame_weight=None):
        """Forward-only loss and metrics of a [B, T] chunk -> (metrics dict as loss_and_grads fills it, state_out).  The inference forward
        (PolicyEngine.forward, nothing saved) + ops.bc_loss without dz: no activations, no optimiser state (works with optimizer_state=False)."""
        w = None
        if frame_weight is not None:
            w, wsum = self._checked_weights(frame_weight, img_u8)
            if wsum == 0:
                raise ValueError("frame_weight: every weight is zero (the loss sum w nll / sum w is undefined)")
        self.policy._ensure_packed()
        eng = self.engine
        bsz, t = img_u8.shape[:2]
        m = bsz * t
        out = eng.forward(img_u8, first, state_in, episode_starts=self.episode_starts)
        lp_b, lp_c = out["buttons"].reshape(m, eng.n_buttons), out["camera"].reshape(m, eng.n_camera)
        ab = act_buttons.reshape(m).to(torch.int64).contiguous()
        ac = act_camera.reshape(m).to(torch.int64).contiguous()
        _, frame_out, totals = ops.bc_loss(lp_b, lp_c, ab, ac, 0, 0.0, weight=w, dtype=self.dtype, want_dz=False)
        metrics: dict = {}
        self._fill_metrics(metrics, totals, frame_out, bsz, t)
        return metrics, out["state_out"]

    @torch.no_grad()
    def forward_saving(self, img_u8, first, state_in, mask: Optional[dict] = None) -> dict:
        """The policy forward with every activation the backward needs kept alive.  Returns the saved-state dict S:
        S["lp_b"] / S["lp_c"] fp32 [M, n] log-probs, S["logits"] fp32 [M, nb+nc+1] (last column: raw value), S["state_out"]."""
        pol, eng = self.policy, self.engine
        pol._ensure_packed()
        cfg, w = eng.cfg, eng.w
        bsz, t = img_u8.shape[:2]
        m = bsz * t
        hid, heads, maxlen = cfg["hidsize"], cfg["heads"], cfg["maxlen"]
        ratio = cfg["pointwise_ratio"]
        dev = img_u8.device
        nb, nc = eng.n_buttons, eng.n_camera
        frames = img_u8.reshape(m, *img_u8.shape[2:]).contiguous()

        # ---------------- forward, keeping what the backward needs ----------------
        outs, cnn_saved = [], []
        streams, main = self._chunk_streams((m + eng.cnn_chunk - 1) // eng.cnn_chunk)
        for ci, i in enumerate(range(0, m, eng.cnn_chunk)):
            with (torch.cuda.stream(streams[ci % len(streams)]) if streams else contextlib.nullcontext()):
                if self.train_cnn:
                    xn, sv = self._cnn_forward_saving(frames[i:i + eng.cnn_chunk])
                    cnn_saved.append(sv)
                else:
                    xn = eng._cnn_chunk(frames[i:i + eng.cnn_chunk])
                d32, _ = ops.linear(xn.view(xn.shape[0], -1), w["net.img_process.cnn.dense.w"], 256, splitk=DENSE_SPLITK)
                outs.append(d32)
                del xn
        for st in streams:
            main.wait_stream(st)
        d = outs[0] if len(outs) == 1 else torch.cat(outs, 0)                     # [M,256] pre-ReLU dense output
        pl = "net.img_process.linear."
        dt = self.dtype
        _, dn = ops.layernorm(d, w[pl + "g"], w[pl + "b"], relu_in=True, dtype=dt)          # 16-bit
        x, x16 = ops.linear(dn, w[pl + "w"], hid, relu=True, out_f32=True, out_bf16=True)
        x_lin16 = x16
        x_pre = None
        if cfg["use_pre_lstm_ln"]:     # MinecraftPolicy.pre_lstm_ln (lib/policy.py:202-203)
            x_pre = x
            x, _ = ops.layernorm(x_pre, w["prelstm.g"], w["prelstm.b"], out_f32=True, out_bf16=False, dtype=dt)
        episodes = EpisodeMasks(first, bsz, t, maxlen, self.episode_starts)      # the bookkeeping of PolicyEngine.forward: the same memories
        qlo = episodes.qlo
        saved: List[dict] = []
        state_out = []
        for l in range(cfg["n_layers"]):
            p = f"net.recurrent_layer.blocks.{l}."
            state_mask, (kmem, vmem) = state_in[l]
            memvalid, new_mask = episodes.layer(state_mask, dev)
            kmem, vmem = kmem.contiguous(), vmem.contiguous()
            x1, x1b = ops.layernorm(x, w[p + "ln1.g"], w[p + "ln1.b"], out_f32=True, dtype=dt)
            qkvr, _ = ops.linear(x1b, w[p + "qkvr.w"], eng.n_qkvr, bias=w[p + "qkvr.b"])
            att = ops.masked_attention(qkvr, kmem, vmem, memvalid, w[p + "b_nd"], bsz, t, heads, hid, dtype=dt, qlo=qlo)
            kout, vout = ops.kv_memory_update(qkvr, kmem, vmem, bsz, t, hid)
            x2, _ = ops.linear(att, w[p + "proj.w"], hid, bias=w[p + "proj.b"], res=x1)
            _, hb = ops.layernorm(x2, w[p + "ln2.g"], w[p + "ln2.b"], dtype=dt)
            _, h2 = ops.linear(hb, w[p + "mlp0.w"], hid * ratio, relu=True, out_f32=False, out_bf16=True)
            xo, _ = ops.linear(h2, w[p + "mlp1.w"], hid, bias=w[p + "mlp1.b"], res=x2)
            saved.append(dict(x=x, x1b=x1b, qkvr=qkvr, kmem=kmem, vmem=vmem, memvalid=memvalid, qlo=qlo, att=att, x2=x2, hb=hb, h2=h2))
            state_out.append((new_mask, (kout, vout)))
            x = xo
        x_trunk = x
        _, xb = ops.layernorm(x_trunk, w["last.g"], w["last.b"], relu_in=True, dtype=dt)
        y, y16 = ops.linear(xb, w["last.w"], hid, relu=True, out_f32=True, out_bf16=True)
        _, lb = ops.layernorm(y, w["final.g"], w["final.b"], dtype=dt)
        logits, _ = ops.linear(lb, w["heads.w"], nb + nc + 1, bias=w["heads.b"])
        temp = cfg["temperature"]
        mk = {h: (mask[h].reshape(m, n_).to(torch.uint8).contiguous() if mask is not None and mask.get(h) is not None else None)
              for h, n_ in (("buttons", nb), ("camera", nc))}
        lp_b = ops.log_softmax_cols(logits, 0, nb, temp, mask=mk["buttons"])
        lp_c = ops.log_softmax_cols(logits, nb, nc, temp, mask=mk["camera"])
        return dict(m=m, bsz=bsz, t=t, dev=dev, d=d, dn=dn, x_lin16=x_lin16, x_pre=x_pre, saved=saved, x_trunk=x_trunk, xb=xb, y=y, y16=y16, lb=lb,
                    logits=logits, lp_b=lp_b, lp_c=lp_c, cnn_saved=cnn_saved, state_out=state_out, ldz=_round_up(nb + nc + 1, 64), mask=mk)

    @torch.no_grad()
    def backward_from(self, S: dict, dz: torch.Tensor, on_trunk_grads=None, debug: Optional[dict] = None, value_grads: bool = False):
        """Backward of everything below the head logits.  dz: bf16 [M, ldz] = d loss / d (fused head logits).
        Consumes S (the CNN activations are released chunk by chunk).  value_grads: also return the value head's gradients
        (non-zero only when dz's value column is)."""
        pol, eng = self.policy, self.engine
        cfg, w = eng.cfg, eng.w
        P = {n: p.detach() for n, p in self.params.items()}
        m, bsz, t, dev = S["m"], S["bsz"], S["t"], S["dev"]
        hid, heads, maxlen = cfg["hidsize"], cfg["heads"], cfg["maxlen"]
        ratio = cfg["pointwise_ratio"]
        nb, nc = eng.n_buttons, eng.n_camera
        d, dn, x_lin16, saved, x_trunk, xb, y, y16, lb = (S[k] for k in ("d", "dn", "x_lin16", "saved", "x_trunk", "xb", "y", "y16", "lb"))
        cnn_saved = S["cnn_saved"]
        pl = "net.img_process.linear."
        g: Dict[str, torch.Tensor] = {}
        zeros = lambda n_: torch.zeros(n_, dtype=torch.float32, device=dev)
        nh = nb + nc + 1
        # heads (fused [buttons; camera; value] GEMM): dlat, dW, db
        wh = torch.cat([P["pi_head.buttons.linear_layer.weight"], P["pi_head.camera.linear_layer.weight"],
                        P["value_head.linear.weight"]], 0)
        dlat, _, dwh = linear_backward(dz, nh, lb, wh)
        if debug is not None:
            debug['dlatent'] = dlat.clone(); debug['latent'] = lb.float().clone(); debug['y'] = y.clone()
        dbh = zeros(nh)
        ops.column_sum_(dbh, dz, nh)
        g["pi_head.buttons.linear_layer.weight"], g["pi_head.camera.linear_layer.weight"] = dwh[:nb], dwh[nb:nb + nc]
        g["pi_head.buttons.linear_layer.bias"], g["pi_head.camera.linear_layer.bias"] = dbh[:nb], dbh[nb:nb + nc]
        if value_grads:
            g["value_head.linear.weight"], g["value_head.linear.bias"] = dwh[nb + nc:nh].clone(), dbh[nb + nc:nh].clone()
        del dz, dwh
        # final_ln
        g["net.final_ln.weight"], g["net.final_ln.bias"] = zeros(hid), zeros(hid)
        dy = ops.layernorm_backward(y, P["net.final_ln.weight"], dlat, g["net.final_ln.weight"], g["net.final_ln.bias"])
        # lastlayer: y = relu(xb Wl^T); gate dy by y > 0 while casting to the GEMM operand
        dy16 = ops.gate_cast(dy, hid, mask=y16)
        dxb, _, g["net.lastlayer.layer.weight"] = linear_backward(dy16, hid, xb, P["net.lastlayer.layer.weight"])
        g["net.lastlayer.norm.weight"], g["net.lastlayer.norm.bias"] = zeros(hid), zeros(hid)
        dx = ops.layernorm_backward(x_trunk, P["net.lastlayer.norm.weight"], dxb, g["net.lastlayer.norm.weight"],
                                    g["net.lastlayer.norm.bias"], relu_in=True)
        if debug is not None:
            debug['dy'] = dy.clone(); debug['dx_trunk'] = dx.clone(); debug['x_trunk'] = x_trunk.clone()
        del dy, dy16, dxb, dlat
        # transformer blocks, last to first
        for l in reversed(range(cfg["n_layers"])):
            p = f"net.recurrent_layer.blocks.{l}."
            o = p + "r.orc_block."
            s = saved[l]
            dout16 = ops.gate_cast(dx, hid, dtype=self.dtype)
            # mlp1: out = x2 + h2 W1^T + b1
            _, dh16, g[p + "mlp1.layer.weight"] = linear_backward(dout16, hid, s["h2"], P[p + "mlp1.layer.weight"], mask=s["h2"],
                                                                  dx_f32=False, dx_bf16_ld=hid * ratio)
            g[p + "mlp1.layer.bias"] = zeros(hid)
            ops.column_sum_(g[p + "mlp1.layer.bias"], dout16, hid)
            # mlp0: h2 = relu(hb W0^T)  (the ReLU gate was applied by the mask above)
            dhb, _, g[p + "mlp0.layer.weight"] = linear_backward(dh16, hid * ratio, s["hb"], P[p + "mlp0.layer.weight"])
            g[p + "mlp0.norm.weight"], g[p + "mlp0.norm.bias"] = zeros(hid), zeros(hid)
            dx2 = ops.layernorm_backward(s["x2"], P[p + "mlp0.norm.weight"], dhb, g[p + "mlp0.norm.weight"], g[p + "mlp0.norm.bias"], dx_add=dx)
            if debug is not None:
                debug[f'dout16_{l}'] = dout16.clone(); debug[f'dh16_{l}'] = dh16.clone(); debug[f'dhb_{l}'] = dhb.clone()
            del dh16, dhb, dout16
            # proj: x2 = x1 + att Wp^T + bp
            dx2_16 = ops.gate_cast(dx2, hid, dtype=self.dtype)
            datt, _, g[o + "proj_layer.weight"] = linear_backward(dx2_16, hid, s["att"], P[o + "proj_layer.weight"])
            g[o + "proj_layer.bias"] = zeros(hid)
            ops.column_sum_(g[o + "proj_layer.bias"], dx2_16, hid)
            # attention
            g[o + "b_nd"] = torch.zeros(10, maxlen, dtype=torch.float32, device=dev)
            dqkvr = ops.masked_attention_backward(s["qkvr"], s["kmem"], s["vmem"], s["memvalid"], w[p + "b_nd"], datt,
                                                  g[o + "b_nd"], bsz, t, heads, hid, qlo=s["qlo"])
            nq = eng.n_qkvr
            dq16 = ops.gate_cast(dqkvr, _round_up(nq, 64), dtype=self.dtype)
            wq = torch.cat([P[o + "q_layer.weight"], P[o + "k_layer.weight"], P[o + "v_layer.weight"], P[o + "r_layer.weight"]], 0)
            dx1, _, dwq = linear_backward(dq16, nq, s["x1b"], wq, res=dx2)   # dx1 = dx2 (skip) + dqkvr Wqkvr
            g[o + "q_layer.weight"], g[o + "k_layer.weight"] = dwq[:hid], dwq[hid:2 * hid]
            g[o + "v_layer.weight"], g[o + "r_layer.weight"] = dwq[2 * hid:3 * hid], dwq[3 * hid:]
            dbq = zeros(nq)
            ops.column_sum_(dbq, dq16, nq)
            g[o + "q_layer.bias"], g[o + "r_layer.bias"] = dbq[:hid], dbq[3 * hid:]
            g[p + "pre_r_ln.weight"], g[p + "pre_r_ln.bias"] = zeros(hid), zeros(hid)
            dx = ops.layernorm_backward(s["x"], P[p + "pre_r_ln.weight"], dx1, g[p + "pre_r_ln.weight"], g[p + "pre_r_ln.bias"])
            if debug is not None:
                debug[f'dx_block{l}'] = dx.clone(); debug[f'dx2_block{l}'] = dx2.clone(); debug[f'datt{l}'] = datt.clone(); debug[f'dqkvr{l}'] = dqkvr.clone()
                debug[f'dx1_block{l}'] = dx1.clone(); debug[f'dq16_{l}'] = dq16.clone(); debug[f'dx2_16_{l}'] = dx2_16.clone()
            del dx2, dx2_16, datt, dqkvr, dq16, dx1, dwq
        if cfg["use_pre_lstm_ln"]:
            g["net.pre_lstm_ln.weight"], g["net.pre_lstm_ln.bias"] = zeros(hid), zeros(hid)
            dx = ops.layernorm_backward(S["x_pre"], P["net.pre_lstm_ln.weight"], dx, g["net.pre_lstm_ln.weight"], g["net.pre_lstm_ln.bias"])
        # ImgObsProcess.linear: x = relu(dn Wlin^T)
        dx16 = ops.gate_cast(dx, hid, mask=x_lin16)
        ddn, _, g[pl + "layer.weight"] = linear_backward(dx16, hid, dn, P[pl + "layer.weight"])
        g[pl + "norm.weight"], g[pl + "norm.bias"] = zeros(256), zeros(256)
        dd = ops.layernorm_backward(d, P[pl + "norm.weight"], ddn, g[pl + "norm.weight"], g[pl + "norm.bias"], relu_in=True)
        if on_trunk_grads is not None:
            on_trunk_grads(g)
        if self.train_cnn:
            acc = self._cnn_backward_begin(P)
            n_acc = max(1, min(self.cnn_streams, len(cnn_saved)))
            accs = [acc] + [self._cnn_backward_accumulators(acc) for _ in range(n_acc - 1)]     # operands shared, accumulators per stream
            streams, main = self._chunk_streams(len(cnn_saved))                                   # (after the zero-fills above were enqueued)
            for ci, i in enumerate(range(0, m, eng.cnn_chunk)):
                with (torch.cuda.stream(streams[ci % len(streams)]) if streams else contextlib.nullcontext()):
                    self._cnn_backward_chunk(cnn_saved[ci], dd[i:i + eng.cnn_chunk].contiguous(), accs[ci % len(accs)])
                    cnn_saved[ci] = None
            for st in streams:
                main.wait_stream(st)
            self._cnn_backward_merge(accs)
            self._cnn_backward_finish(acc, P, g)
        return g

    def _chunk_streams(self, n_chunks: int):
        """-> (the side streams the CNN chunks alternate over -- [] = everything on the current stream --, the current stream);
        the side streams have been made to wait for the work enqueued so far."""
        main = torch.cuda.current_stream()
        n = min(self.cnn_streams, n_chunks)
        if n <= 1:
            return [], main
        while len(self._streams) < n:        # append only: chunk ci of an earlier forward_saving() must find ITS stream at index ci % n again
            self._streams.append(torch.cuda.Stream())
        for st in self._streams[:n]:
            st.wait_stream(main)
        return self._streams[:n], main

    def _cnn_backward_accumulators(self, acc):
        """A second set of zeroed accumulators next to `acc` (same read-only operands)."""
        z = torch.zeros_like
        other = dict(wt=acc["wt"], dense_wt=acc["dense_wt"], raw={}, n={s: (z(a), z(b)) for s, (a, b) in acc["n"].items()}, dense=None,
                     dense_dwT=z(acc["dense_dwT"]), dense_dg=z(acc["dense_dg"]), dense_db=z(acc["dense_db"]))
        return other

    def _cnn_backward_merge(self, accs):
        """Sum the per-stream accumulators into accs[0], in stream order."""
        a0 = accs[0]
        for a in accs[1:]:
            for q, r in a["raw"].items():
                if q in a0["raw"]:
                    for t0, t1 in zip(a0["raw"][q], r):
                        t0.add_(t1)
                else:
                    a0["raw"][q] = r
            for s, (dg_, db_) in a["n"].items():
                a0["n"][s][0].add_(dg_); a0["n"][s][1].add_(db_)
            for k in ("dense_dwT", "dense_dg", "dense_db"):
                a0[k].add_(a[k])
            if a.get("first") is not None:
                if a0.get("first") is None:
                    a0["first"] = a["first"]
                else:
                    a0["first"][0].add_(a["first"][0]); a0["first"][1].add_(a["first"][1])


    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def reduced_loss_and_grads(self, img_u8, first, state_in, act_buttons, act_camera, *, frame_weight=None, metrics: Optional[dict] = None):
        """This rank's shard of the batch -> (global mean loss, gradients of the GLOBAL mean loss summed over ranks, state_out).
        frame_weight / metrics: as loss_and_grads.  With weights the count the ranks agree on is sum_ranks sum w (fp64), the loss is
        sum_ranks(sum w nll) / that, and a rank whose shard carries no weight is legal while the global sum is positive; requested metrics
        are GLOBAL (the eight totals travel in the final reduction, next to the health flag); frame_nll / frame_out are this rank's frames.
        (fp16 mode: the gradients stay loss-scaled, i.e. are those of the mean divided by grad_unscale(global frames); step() hands
        that factor to the optimiser launch.)
        The loss gradient already carries 1 / global_frames, so the exchange is a plain sum, in two bucketed all-reduces:
        the trunk + head gradients (final before the CNN backward starts) travel over RCCL WHILE the CNN backward -- two
        thirds of the step's compute -- runs; the CNN's own gradients (a tenth of the bytes) follow at the end.  A rank
        that fails locally (e.g. out of memory) still joins every collective with zeros and reports it in the final
        (loss, healthy-rank count) reduction, so all ranks raise together instead of blocking in an all-reduce."""
        # (self.exchange = False: the local step only -- bench.py times it beside the full step to report how much of the exchange the CNN backward hides)
        world = dist.get_world_size() if dist.is_initialized() and getattr(self, "exchange", True) else 1
        m_local = img_u8.shape[0] * img_u8.shape[1]
        self._global_frames = m_local
        # force_exchange (VPT_DP_FORCE_EXCHANGE=1): take the data-parallel path in a ONE-rank group too -- the frame-count reduction, both arenas, the early exchange
        # under the CNN backward, the late one, the health reduction -- so that the whole step can be run (and timed) over the real transport on a 1-GPU box
        force = bool(getattr(self, "force_exchange", False)) and dist.is_initialized()
        fused = frame_weight is not None or metrics is not None      # the loss path through ops.bc_loss (its totals), else the unchanged default
        if world == 1 and not force:
            if not fused:
                return self.loss_and_grads(img_u8, first, state_in, act_buttons, act_camera, global_frames=m_local, unscaled=False)
            w, wsum = self._checked_weights(frame_weight, img_u8) if frame_weight is not None else (None, None)
            if wsum is not None:
                if wsum == 0:
                    raise ValueError("frame_weight: every weight is zero (the loss sum w nll / sum w is undefined)")
                self._global_frames = wsum
            return self.loss_and_grads(img_u8, first, state_in, act_buttons, act_camera, global_frames=self._global_frames, unscaled=False,
                                       frame_weight=w, metrics=metrics, _weight_sum=wsum)
        dev = img_u8.device
        # Shards may differ by one sequence when B % world != 0 (distributed.shard_range): the mean runs over the TRUE global
        # frame count, and the reported loss is the frame-weighted mean of the ranks' losses.  With frame weights the count is the global weight sum;
        # a rank whose weights are invalid still joins every collective (with zeros) and reports itself in the final reduction.
        err, w, wsum = None, None, None
        if frame_weight is not None:
            try:
                w, wsum = self._checked_weights(frame_weight, img_u8)
            except ValueError as e:
                err, wsum = e, 0.0
        count = torch.tensor([float(m_local) if frame_weight is None else wsum], dtype=torch.float64, device=dev)
        dist.all_reduce(count)
        if frame_weight is None:
            m_global = self._global_frames = int(round(float(count.item())))
        else:
            m_global = self._global_frames = float(count.item())
            if err is None and m_global == 0:
                err = ValueError("frame_weight: every weight of the global batch is zero (the loss sum w nll / sum w is undefined)")
        early = [n for n in self.trainable if not n.startswith("net.img_process.cnn.")]   # final before the CNN backward
        late = [n for n in self.trainable if n.startswith("net.img_process.cnn.")]
        pending, state = [], dict(early_sent=False)
        # the gradients live in two flat fp32 arenas that persist across steps (distributed.GradArena): each tensor is copied in once when it
        # is final, the collectives run in place on 64 MB slices of the arena, the optimiser reads the views -- no cat, no copy back
        akey = (tuple(early), tuple(late), tuple(tuple(self.params[n].shape) for n in early + late), str(dev))
        if self._arenas is None or self._arenas[0] != akey:      # rebuilt when the trainable set, a shape or the device changes
            self._arenas = (akey, tuple(D.GradArena(ns, [self.params[n].shape for n in ns], dev) for ns in (early, late)))
        arena_early, arena_late = self._arenas[1]

        def start_trunk_exchange(g):
            arena_early.adopt(g)
            pending.extend(arena_early.all_reduce_start(force))
            state["early_sent"] = True

        loss, grads, state_out = None, None, None
        local_metrics = {} if metrics is not None else None
        try:
            if err is not None:
                raise err
            if fused:
                loss, grads, state_out = self.loss_and_grads(img_u8, first, state_in, act_buttons, act_camera, global_frames=m_global,
                                                             on_trunk_grads=start_trunk_exchange, unscaled=False, frame_weight=w,
                                                             metrics=local_metrics, _weight_sum=wsum)
            else:
                loss, grads, state_out = self.loss_and_grads(img_u8, first, state_in, act_buttons, act_camera,
                                                             global_frames=m_global, on_trunk_grads=start_trunk_exchange, unscaled=False)
            arena_late.adopt(grads)
            pending.extend(arena_late.all_reduce_start(force))
        except Exception as e:          # e.g. out of memory on this rank: still take part in every collective (with zeros of
            err = e                     # the same shapes) so that the other ranks are not left blocked, then fail everywhere
            if not state["early_sent"]:
                arena_early.flat.zero_()
                pending.extend(arena_early.all_reduce_start(force))
            arena_late.flat.zero_()
            pending.extend(arena_late.all_reduce_start(force))
        D.bucketed_all_reduce_finish(pending)
        if fused:       # (this rank's eight totals, healthy): the loss and the metrics come from the totals' sum over ranks
            tail = torch.zeros(9, dtype=torch.float64, device=dev)
            if err is None:
                tail[:8] = self._bc_totals.to(torch.float64)
                tail[8] = 1.0
            dist.all_reduce(tail)
            if float(tail[8].item()) != world:
                raise RuntimeError(f"BC step failed on {'this' if err is not None else 'another'} rank: {err!r}")
            totals = tail[:8].to(torch.float32)
            if metrics is not None:
                self._fill_metrics(metrics, totals, None, 0, 0)
                metrics.update(frame_nll=local_metrics["frame_nll"], frame_out=local_metrics["frame_out"])
            return (totals[0] + totals[1]) / totals[6], grads, state_out
        tail = torch.tensor([0.0 if err is not None else float(loss) * m_local, 0.0 if err is not None else 1.0], device=dev)
        dist.all_reduce(tail)           # (sum over ranks of loss x local frames, number of healthy ranks)
        if float(tail[1].item()) != world:
            raise RuntimeError(f"BC step failed on {'this' if err is not None else 'another'} rank: {err!r}")
        return tail[0] / m_global, grads, state_out

    @torch.no_grad()
    def step(self, img_u8, first, state_in, act_buttons, act_camera, *, frame_weight=None, metrics: Optional[dict] = None):
        """One optimiser step on this rank's shard of the batch.  Returns (global mean loss, state_out).  frame_weight / metrics: as
        loss_and_grads (the weighted loss sum w nll / sum w over all ranks; global metrics)."""
        self._need_optimizer_state()
        if frame_weight is None and metrics is None:
            loss, grads, state_out = self.reduced_loss_and_grads(img_u8, first, state_in, act_buttons, act_camera)
        else:
            loss, grads, state_out = self.reduced_loss_and_grads(img_u8, first, state_in, act_buttons, act_camera, frame_weight=frame_weight, metrics=metrics)
        # the Adam launch (clipped when max_grad_norm is set) after the exchange: the norm is that of the summed global gradients, the same bits on every rank
        loss, _ = self._optimizer_tail(loss, grads, self.grad_unscale(self._global_frames), img_u8.device, metrics)
        return loss, state_out




def conv_dgrad_coef(stats_in: torch.Tensor, t12: torch.Tensor, n: int) -> torch.Tensor:
    """Per-frame (c0, c1) of the statistics terms of dx:  dx += c0 + c1 x,  c1 = -rstd^2 T1 / n,  c0 = -rstd T2 / n - c1 mu."""
    mu = stats_in[:, 0] / n
    rstd = torch.rsqrt((stats_in[:, 1] / n - mu * mu).clamp(min=0) + 1e-5)
    c1 = -(rstd * rstd) * t12[:, 0] / n
    c0 = -(rstd / n) * t12[:, 1] - c1 * mu
    return torch.stack([c0, c1], 1).float().contiguous()
