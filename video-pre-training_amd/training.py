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
from typing import List, Optional

import torch
import torch.distributed as dist

from . import distributed as D
from . import ops
from .cnn_training import _tap_sum, conv_param_grads  # noqa: F401  (conv_param_grads: this module's long-standing name for it)
from .engine import DENSE_SPLITK, EpisodeMasks, check_episode_starts
from .trainer_base import TrainerBase, _round_up, linear_backward  # noqa: F401  (linear_backward: this module's long-standing name for it)


class BCTrainer(TrainerBase):
    def __init__(self, policy, lr: float = 0.000181, weight_decay: float = 0.039428, betas=(0.9, 0.999), eps: float = 1e-8,
                 train_cnn: bool = True, optimizer_state: bool = True, loss_scale: Optional[float] = None,
                 scale_growth_interval: int = 200, episode_starts: str = "chunk", max_grad_norm: Optional[float] = None,
                 trainable=None, param_groups=None, decoupled_weight_decay: bool = False, adapters=None):
        """adapters: an adapters.LowRankAdapters built on this policy: its A / B tensors train on the frozen base; trainable=None then
        means "no base tensor" and strings add base tensors; evaluate() sees base + adapters (merged for the call, restored bit for bit after it).
        trainable / param_groups / decoupled_weight_decay: partial fine-tuning (TrainerBase._init_trainer): which tensors train --
        None = all this trainer trains, or parameter names / module prefixes such as ["pi_head", "net.lastlayer"], or a callable; selecting
        `value_head.*`, or `net.img_process.cnn.*` with train_cnn=False, raises ValueError --, per-group lr_scale / weight_decay, AdamW-style decay.
        The backward stops where training stops; with any CNN tensor trainable the whole CNN backward runs (no cut inside the CNN) and the frozen
        CNN tensors are dropped from the gradients.
        max_grad_norm: None (default: no clipping -- the reference's actual behaviour, its clip_grad_norm_ call receives an exhausted generator),
        5.0 (MAX_GRAD_NORM, what behavioural_cloning.py:38-40,121 meant) or float("inf") (measure the norm, never clip).  When set, step() takes the
        global l2 norm of the gradients of the mean loss on the device -- after the all-reduce, un-scaled: neither fp16's loss scale nor 1 / frames
        reaches the threshold -- and the Adam launch multiplies by torch's clip coefficient; `metrics` gains grad_norm, clip_coef and
        grad_norm_per_tensor, `last_grad_norm` keeps the norm.  A non-finite norm SKIPS the step on the device in both operand formats
        (skipped_steps; fp16 also halves its loss scale) where torch would write NaN into every parameter (TrainerBase._optimizer_tail).
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
        self._init_trainer(policy, lr, weight_decay, betas, eps, train_cnn, optimizer_state, loss_scale, scale_growth_interval, max_grad_norm,
                           trainable, param_groups, decoupled_weight_decay, adapters)
        self.episode_starts = check_episode_starts(episode_starts)
        # the autograd boundary's counterpart of loss_scale (lib/policy.py:_PolicyForwardFn.backward): where the largest incoming
        # gradient element is lifted to before it enters the 16-bit buffers; halved on every overflow it detects
        self.autograd_lift, self.autograd_overflows = 256.0, 0
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
        self.force_exchange = os.environ.get("VPT_DP_FORCE_EXCHANGE", "0") == "1"      # see reduced_loss_and_grads
        self._arenas = None      # (key, (GradArena trunk + heads, GradArena CNN)) of the data-parallel step, built on first use
        self._streams: List[torch.cuda.Stream] = []

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
            self._unscale_(g, gf)
        return loss, g, S["state_out"]

    @torch.no_grad()
    def evaluate(self, img_u8, first, state_in, act_buttons, act_camera, *, frame_weight=None):
        """Forward-only loss and metrics of a [B, T] chunk -> (metrics dict as loss_and_grads fills it, state_out).  The inference forward
        (PolicyEngine.forward, nothing saved) + ops.bc_loss without dz: no activations, no optimiser state (works with optimizer_state=False)."""
        w = None
        if frame_weight is not None:
            w, wsum = self._checked_weights(frame_weight, img_u8)
            if wsum == 0:
                raise ValueError("frame_weight: every weight is zero (the loss sum w nll / sum w is undefined)")
        eng = self.engine
        bsz, t = img_u8.shape[:2]
        m = bsz * t
        with self._adapters_applied():
            self.policy._ensure_packed()
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
        eng = self.engine
        self.policy._ensure_packed()
        cfg, w = eng.cfg, eng.w
        bsz, t = img_u8.shape[:2]
        m = bsz * t
        hid, heads = cfg["hidsize"], cfg["heads"]
        dev, dt = img_u8.device, self.dtype
        nb, nc = eng.n_buttons, eng.n_camera
        frames = img_u8.reshape(m, *img_u8.shape[2:]).contiguous()

        # ---------------- forward, keeping what the backward needs ----------------
        outs, cnn_saved = [], []
        streams, main = self._chunk_streams((m + eng.cnn_chunk - 1) // eng.cnn_chunk)
        for ci, i in enumerate(range(0, m, eng.cnn_chunk)):
            with (torch.cuda.stream(streams[ci % len(streams)]) if streams else contextlib.nullcontext()):
                if self.train_cnn:
                    xn, sv = self._cnn_forward_saving(frames[i:i + eng.cnn_chunk])
                    if self._cnn_backward:       # (a subset without a CNN tensor: the same forward, nothing of it kept)
                        cnn_saved.append(sv)
                    del sv
                else:
                    xn = eng._cnn_chunk(frames[i:i + eng.cnn_chunk])
                d32, _ = ops.linear(xn.view(xn.shape[0], -1), w["net.img_process.cnn.dense.w"], 256, splitk=DENSE_SPLITK)
                outs.append(d32)
                del xn
        for st in streams:
            main.wait_stream(st)
        d = outs[0] if len(outs) == 1 else torch.cat(outs, 0)                     # [M,256] pre-ReLU dense output
        episodes = EpisodeMasks(first, bsz, t, cfg["maxlen"], self.episode_starts)      # the bookkeeping of PolicyEngine.forward: the same memories
        qlo = episodes.qlo
        state_out = []

        def attend(l, p, qkvr):
            state_mask, (kmem, vmem) = state_in[l]
            memvalid, new_mask = episodes.layer(state_mask, dev)
            kmem, vmem = kmem.contiguous(), vmem.contiguous()
            att = ops.masked_attention(qkvr, kmem, vmem, memvalid, w[p + "b_nd"], bsz, t, heads, hid, dtype=dt, qlo=qlo)
            kout, vout = ops.kv_memory_update(qkvr, kmem, vmem, bsz, t, hid)
            state_out.append((new_mask, (kout, vout)))
            return att, dict(kmem=kmem, vmem=vmem, memvalid=memvalid, qlo=qlo)

        trunk = self._trunk_forward_saving(d, attend)       # no tiling / splitk: the row count decides ("auto"), part of this trainer's bits
        x_trunk = trunk["x_trunk"]
        _, xb = ops.layernorm(x_trunk, w["last.g"], w["last.b"], relu_in=True, dtype=dt)
        y, y16 = ops.linear(xb, w["last.w"], hid, relu=True, out_f32=True, out_bf16=True)
        _, lb = ops.layernorm(y, w["final.g"], w["final.b"], dtype=dt)
        logits, _ = ops.linear(lb, w["heads.w"], nb + nc + 1, bias=w["heads.b"])
        temp = cfg["temperature"]
        mk = {h: (mask[h].reshape(m, n_).to(torch.uint8).contiguous() if mask is not None and mask.get(h) is not None else None)
              for h, n_ in (("buttons", nb), ("camera", nc))}
        lp_b = ops.log_softmax_cols(logits, 0, nb, temp, mask=mk["buttons"])
        lp_c = ops.log_softmax_cols(logits, nb, nc, temp, mask=mk["camera"])
        return self._release_unread(dict(trunk, m=m, bsz=bsz, t=t, dev=dev, d=d, xb=xb, y=y, y16=y16, lb=lb, logits=logits, lp_b=lp_b, lp_c=lp_c,
                                         cnn_saved=cnn_saved, state_out=state_out, ldz=_round_up(nb + nc + 1, 64), mask=mk))

    def _attention_backward(self, S, l, datt, g):
        """The masked attention's backward; the relative-position bias b_nd is trained by it."""
        cfg = self.engine.cfg
        p = f"net.recurrent_layer.blocks.{l}."
        s = S["saved"][l]
        db_nd = g[p + "r.orc_block.b_nd"] = torch.zeros(10, cfg["maxlen"], dtype=torch.float32, device=S["dev"])
        return ops.masked_attention_backward(s["qkvr"], s["kmem"], s["vmem"], s["memvalid"], self.engine.w[p + "b_nd"], datt,
                                             db_nd, S["bsz"], S["t"], cfg["heads"], cfg["hidsize"], qlo=s["qlo"])

    @torch.no_grad()
    def backward_from(self, S: dict, dz: torch.Tensor, on_trunk_grads=None, debug: Optional[dict] = None, value_grads: bool = False):
        """Backward of everything below the head logits.  dz: bf16 [M, ldz] = d loss / d (fused head logits).
        Consumes S (the CNN activations are released chunk by chunk).  value_grads: also return the value head's gradients
        (non-zero only when dz's value column is).  With a trainable subset the trunk's walk stops at its cut (TrainerBase._trunk_backward); the CNN
        is not cut: when one of its tensors is trainable its backward runs whole and the frozen CNN tensors' gradients are dropped at the end."""
        eng = self.engine
        P = {n: p.detach() for n, p in self.params.items()}
        g, dd = self._trunk_backward(S, dz, P, value_grads=value_grads, debug=debug)
        if on_trunk_grads is not None:
            on_trunk_grads(g)
        if self.train_cnn and self._cnn_backward:
            m, cnn_saved = S["m"], S["cnn_saved"]
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
            if self._subset is not None:
                for n in [n for n in g if n.startswith("net.img_process.cnn.") and n not in self._subset]:
                    del g[n]
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
    def reduced_loss_and_grads(self, img_u8, first, state_in, act_buttons, act_camera, *, frame_weight=None, metrics: Optional[dict] = None,
                               micro_batches: int = 1):
        """This rank's shard of the batch -> (global mean loss, gradients of the GLOBAL mean loss summed over ranks, state_out).
        micro_batches=K > 1 (gradient accumulation): the shard's B sequences run as K contiguous row groups (micro_batch_rows) one
        after the other, each carrying the window's frame count, their gradients summed in order (the first adopted, then one ops.grad_accumulate_
        launch each) -- a micro-batch's activations are gone before the next forward, so the peak is that of B / K sequences.  Loss and metrics come
        from the micro-batches' totals summed in fp64 (the arithmetic of the data-parallel fused path; the loss path is always ops.bc_loss);
        frame_nll / frame_out / state_out are the row-wise concatenations.  Across ranks: ONE count reduction and ONE exchange per window.
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
        rows = self.micro_batch_rows(img_u8.shape[0], micro_batches) if micro_batches != 1 else None      # (ValueError before anything is queued)
        self._global_frames = m_local
        # force_exchange (VPT_DP_FORCE_EXCHANGE=1): take the data-parallel path in a ONE-rank group too -- the frame-count reduction, both arenas, the early exchange
        # under the CNN backward, the late one, the health reduction -- so that the whole step can be run (and timed) over the real transport on a 1-GPU box
        force = bool(getattr(self, "force_exchange", False)) and dist.is_initialized()
        fused = frame_weight is not None or metrics is not None or rows is not None      # the loss path through ops.bc_loss (its totals), else the unchanged default
        if world == 1 and not force:
            if rows is not None:
                w, wsum = self._checked_weights(frame_weight, img_u8) if frame_weight is not None else (None, None)
                if wsum is not None:
                    if wsum == 0:
                        raise ValueError("frame_weight: every weight is zero (the loss sum w nll / sum w is undefined)")
                    self._global_frames = wsum
                grads, totals, state_out = self._micro_batched(rows, img_u8, first, state_in, act_buttons, act_camera, w, self._global_frames, metrics)
                return (totals[0] + totals[1]) / totals[6], grads, state_out
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
        pending, state = [], dict(early_sent=False, accumulated=False)
        # the gradients live in two flat fp32 arenas that persist across steps (distributed.GradArena): each tensor is copied in once when it
        # is final, the collectives run in place on 64 MB slices of the arena, the optimiser reads the views -- no cat, no copy back
        akey = (tuple(early), tuple(late), tuple(tuple(self.params[n].shape) for n in early + late), str(dev))
        if self._arenas is None or self._arenas[0] != akey:      # rebuilt when the trainable set, a shape or the device changes
            self._arenas = (akey, tuple(D.GradArena(ns, [self.params[n].shape for n in ns], dev) for ns in (early, late)))
        arena_early, arena_late = self._arenas[1]

        def start_trunk_exchange(g):
            if state["accumulated"]:      # the window's earlier micro-batches are in the arena: add this one's trunk + head gradients to them
                arena_early.accumulate(g)
            else:
                arena_early.adopt(g)
            pending.extend(arena_early.all_reduce_start(force))
            state["early_sent"] = True

        def into_arenas(k, acc, g):       # micro-batches 0 .. K-2 whole, and the last one's CNN gradients: straight into the two arenas
            last = k == len(rows) - 1
            for arena in ((arena_late,) if last else (arena_early, arena_late)):
                (arena.accumulate if state["accumulated"] else arena.adopt)(g)
            state["accumulated"] = True
            return g if last else {n: g[n] for n in early + late}      # (the arenas' views)

        loss, grads, state_out = None, None, None
        local_metrics = {} if metrics is not None else None
        try:
            if err is not None:
                raise err
            if rows is not None:
                grads, self._bc_totals, state_out = self._micro_batched(rows, img_u8, first, state_in, act_buttons, act_camera, w, m_global, local_metrics,
                                                                        accumulate=into_arenas, on_last_trunk_grads=start_trunk_exchange)
            elif fused:
                loss, grads, state_out = self.loss_and_grads(img_u8, first, state_in, act_buttons, act_camera, global_frames=m_global,
                                                             on_trunk_grads=start_trunk_exchange, unscaled=False, frame_weight=w,
                                                             metrics=local_metrics, _weight_sum=wsum)
            else:
                loss, grads, state_out = self.loss_and_grads(img_u8, first, state_in, act_buttons, act_camera,
                                                             global_frames=m_global, on_trunk_grads=start_trunk_exchange, unscaled=False)
            if rows is None:
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

    def _micro_batched(self, rows, img_u8, first, state_in, act_buttons, act_camera, w, count, metrics, accumulate=None, on_last_trunk_grads=None):
        """The K > 1 window of reduced_loss_and_grads on this rank: loss_and_grads per row group with global_frames = `count` (the window's frame
        count or weight sum, all ranks'), w: the checked fp32 [M] weights or None -> (accumulated grads, the summed totals [8], state_out of all rows).
        `metrics` (when a dict) is filled from the summed totals and the concatenated records.  on_last_trunk_grads: loss_and_grads's callback, for the
        LAST micro-batch only (the data-parallel step starts its early exchange there); accumulate: TrainerBase._accumulated_window's."""
        bsz, t = img_u8.shape[:2]
        first = torch.as_tensor(first)
        ab, ac = act_buttons.reshape(bsz, t), act_camera.reshape(bsz, t)
        w_rows = w.view(bsz, t) if w is not None else None

        def run(k, lo, hi):
            local: dict = {}
            # (_weight_sum: the rows' own sum would only feed this micro-batch's own loss, which the window does not read -- no host transfer)
            _, g, s_out = self.loss_and_grads(img_u8[lo:hi], first[lo:hi], self._tree_rows(state_in, lo, hi), ab[lo:hi], ac[lo:hi], global_frames=count,
                                              on_trunk_grads=on_last_trunk_grads if k == len(rows) - 1 else None, unscaled=False,
                                              frame_weight=None if w_rows is None else w_rows[lo:hi].reshape(-1), metrics=local,
                                              _weight_sum=None if w_rows is None else count)
            return g, self._bc_totals, local["frame_out"].reshape(-1, 8), s_out

        grads, totals, records, states = self._accumulated_window(rows, run, accumulate)
        if metrics is not None:
            self._fill_metrics(metrics, totals, records, bsz, t)
        return grads, totals, self._tree_cat_rows(states)

    @torch.no_grad()
    def step(self, img_u8, first, state_in, act_buttons, act_camera, *, frame_weight=None, metrics: Optional[dict] = None, micro_batches: int = 1):
        """One optimiser step on this rank's shard of the batch.  Returns (global mean loss, state_out).  frame_weight / metrics: as
        loss_and_grads (the weighted loss sum w nll / sum w over all ranks; global metrics).  micro_batches=K: the shard runs as K row groups
        whose gradients are accumulated (reduced_loss_and_grads); ONE Adam launch, clip and loss-scale decision per window."""
        self._need_optimizer_state()
        if micro_batches != 1:
            loss, grads, state_out = self.reduced_loss_and_grads(img_u8, first, state_in, act_buttons, act_camera, frame_weight=frame_weight, metrics=metrics,
                                                                 micro_batches=micro_batches)
        elif frame_weight is None and metrics is None:
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
