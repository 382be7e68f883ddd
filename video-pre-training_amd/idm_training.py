"""Training of the inverse-dynamics model on MI355X: everything behind the CNN (the default), or the whole network from the pixels (train_cnn=True).

The IDM (lib/policy.py:342-467) is temporal Conv3d -> IMPALA CNN -> 256 -> hid linear -> transformer blocks with mask "none" -> ReLU -> final_ln ->
20 two-way button groups + 2 eleven-way camera groups.  About 99 % of its forward FLOPs are the per-frame CNN; by default that part stays frozen and runs
through the inference path with nothing saved.  The part that is always trained -- ImgObsProcess.linear, the transformer blocks, final_ln and the two heads --
holds all of the window-level reasoning.

    loss = sum_frames w (nll_buttons + nll_camera) / sum_frames w,   nll_* = -sum over the head's groups of log pi(label)
           (the negative of pi_head.logprob, lib/action_head.py:176-184,252-253, averaged over frames)

train_cnn=True is the first stage of the VPT method, training the IDM itself: the temporal conv (`net.conv3d_layer.*`) and the IMPALA CNN
(`net.img_process.cnn.*`, the dense layer included) get gradients too.  The CNN's saving forward and its backward are BCTrainer's own
(cnn_training.CnnTrainingMixin, one copy of the launch order) with stack 0 fed by the temporal conv's output: there `firstconv` is a normed 3x3 conv on
128 x 128 pixels, its dgrad returns dx0, and ops.conv3d_t5_backward turns (image, x0, dx0) into the temporal conv's weight and bias gradient.

The autograd boundary: a gradient-enabled `InverseActionPolicy.forward` is one autograd node (lib/policy.py:_IDMForwardFn) over forward_saving and
backward_from of an IDMTrainer(optimizer_state=False) the policy keeps; the incoming gradients of the two grouped log-prob tensors become dz in one launch
(ops.grouped_logprob_backward).  Any loss written through pi_head.logprob / entropy / kl_divergence then trains the IDM with `loss.backward()` and a torch
optimizer; IDMTrainer.step stays the fast path for the plain NLL (fused loss, one-launch Adam).

NOT built: data-parallel IDM steps, and chunk streams for the CNN backward (one stream).

The trunk's saving forward and backward, the optimiser state and the loss-scale bookkeeping are trainer_base.TrainerBase's, shared with BCTrainer.
The backward runs on the HIP kernels of the BC step (trainer_base.linear_backward, ops.layernorm_backward, ops.gate_cast, ops.column_sum_,
ops.adam_step_multi_) plus two of its own: ops.full_attention_backward (the mask-"none" attention) and ops.idm_loss (the grouped heads' loss,
gradient and metrics in one launch).  Every reduction has a fixed order: the same batch gives the same gradient bits."""
from typing import Dict, Optional

import torch

from . import ops
from .engine import DENSE_SPLITK, action_heads
from .trainer_base import TrainerBase

_FROZEN = ("net.conv3d_layer.", "net.img_process.cnn.")
_UNREACHED = ("net.lastlayer.",)       # computed and discarded by the reference (lib/policy.py:390-391): not part of the function that is trained


class IDMTrainer(TrainerBase):
    fused_qkv = "qkv"            # mask "none": no relative-position bias, r_layer is not in the fused projection (trainer_base.py)
    head_params = ("pi_head.buttons.linear_layer", "pi_head.camera.linear_layer")      # one [62, hid] matrix for the two backward GEMMs
    has_lastlayer = False        # computed and discarded by the reference: final_ln reads relu(x_trunk)
    final_ln_relu = True
    stack0_from_x0 = True        # the CNN's stack 0 is fed by the temporal conv (cnn_training.py)
    dense_tiling = "throughput"  # as IDMEngine: the MFMA GEMM whatever the row count (a one-window chunk of <= 8 frames would take the GEMV kernel)

    def __init__(self, policy, lr: float = 0.000181, weight_decay: float = 0.039428, betas=(0.9, 0.999), eps: float = 1e-8,
                 optimizer_state: bool = True, loss_scale: Optional[float] = None, scale_growth_interval: int = 200, train_cnn: bool = False,
                 max_grad_norm: Optional[float] = None, trainable=None, param_groups=None, decoupled_weight_decay: bool = False, adapters=None):
        """adapters: an adapters.LowRankAdapters built on this IDM (r_layer sits outside its fused projection and is not adaptable);
        trainable=None then means "no base tensor".
        trainable / param_groups / decoupled_weight_decay: partial fine-tuning as BCTrainer's (TrainerBase._init_trainer); selecting
        what this trainer does not train -- `net.lastlayer.*` (unreached), the empty `b_nd`, the CNN side with train_cnn=False -- raises ValueError.
        With any tensor of the temporal conv or the CNN trainable their whole backward runs and the frozen ones are dropped from the gradients.
        max_grad_norm: global-norm gradient clipping as BCTrainer's (None = off, the default; float("inf") = measure only; a non-finite norm skips
        the step on the device in both formats).
        policy: lib.policy.InverseActionPolicy on the GPU.  Trainable: `net.img_process.linear.*`, `net.pre_lstm_ln.*` (when configured), every
        `net.recurrent_layer.blocks.*` tensor, `net.final_ln.*`, `pi_head.buttons.*`, `pi_head.camera.*`.  train_cnn=False (default) freezes
        `net.conv3d_layer.*` and every `net.img_process.cnn.*` tensor (the dense layer included) and launches what it always launched.
        train_cnn=True trains those 49 tensors as well: per chunk of whole windows (the engine's cnn_chunk granularity) ops.conv3d_t5 with x0 kept, the
        saving CNN forward, the dense layer; backward per chunk dense -> stacks 2, 1, 0 -> dx0 -> ops.conv3d_t5_backward, on one stream.  It needs the
        pool-fused forward (VPT_BC_FUSED_POOL=0 raises).  The saving forward does not use the inference path's `n` and dense folds, so with
        train_cnn=True the log-probs equal IDMEngine.forward's to the parity bounds, not bit for bit (BCTrainer(train_cnn=True) has the same property);
        about 27 MB of activations per frame are kept on the 4x model.  (`r_layer.*` of a block is trainable by name but unreached -- mask "none" has no relative-position bias -- so its
        gradient is exact zeros and only weight decay moves it, as torch.optim.Adam would; `b_nd` is [10, 0]: nothing to train; `net.lastlayer.*`
        is computed and discarded by the reference and takes no part.)
        optimizer_state=False: gradients only, no Adam moments.  The fp16 mode uses BCTrainer's loss scaling unchanged (see there): `loss_scale`
        defaults to 256 (1 = off in bf16), the loss gradient is written as loss_scale / temperature x (softmax - one-hot) per frame, the optimiser
        launch un-scales, an overflowed step is skipped on the device, the scale halves then and doubles after `scale_growth_interval` clean steps."""
        self._init_trainer(policy, lr, weight_decay, betas, eps, train_cnn, optimizer_state, loss_scale, scale_growth_interval, max_grad_norm,
                           trainable, param_groups, decoupled_weight_decay, adapters)
        # the autograd boundary's counterpart of loss_scale (lib/policy.py:_IDMForwardFn.backward), as BCTrainer's: where the largest incoming
        # gradient element is lifted to before it enters the 16-bit buffers; halved on every overflow the boundary detects
        self.autograd_lift, self.autograd_overflows = 256.0, 0
        if self.train_cnn and not self.fused_pool:
            raise RuntimeError("IDMTrainer(train_cnn=True) needs the pool-fused forward (ops.conv3x3_pool_argmax): at 128 x 128 only the pooled entry of "
                               "the conv backward is built -- unset VPT_BC_FUSED_POOL=0")

    def _is_trainable(self, name: str) -> bool:
        if (name.startswith(_FROZEN) and not self.train_cnn) or name.startswith(_UNREACHED):
            return False
        return self.params[name].numel() > 0            # (b_nd is [10, maxlen = 0])

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def factored_labels(chunk: dict, n_camera_bins: int = 11):
        """A [B, T] chunk dict of SequenceBatcher / labeler.labelled_chunks (joint `act_buttons` / `act_camera`, int64 [B, T]) -> the IDM's labels
        (buttons int64 [B, T, 20], camera int64 [B, T, 2]) through ops.action_to_factored.  A convenience: the joint encoding has ALREADY collapsed
        mutually exclusive buttons (forward + back, the hotbar keys, ... lib/action_mapping.py), so what comes back is the policy's view of the
        action; labels taken straight from ActionTransformer.env2policy are the faithful ones for the IDM."""
        jb, jc = chunk["act_buttons"], chunk["act_camera"]
        bsz, t = jb.shape[:2]
        b, c = ops.action_to_factored(jb.reshape(-1).to(torch.int64).contiguous(), jc.reshape(-1).to(torch.int64).contiguous(), n_camera_bins)
        return b.view(bsz, t, 20), c.view(bsz, t, 2)

    def _checked_inputs(self, img_u8, buttons, camera, frame_weight, allow_zero_sum: bool = False):
        """Labels -> int64 [M, G] on the images' device, weights -> fp32 [M] (or None); the weights' sum and minimum and the labels' extrema come
        to the host in ONE transfer (one synchronisation per step).  ValueError on a label out of range, on a negative or non-finite weight and on
        all-zero weights (unless allow_zero_sum: a micro-batch of a window that carries weight elsewhere).  -> (buttons, camera, weights | None, weight sum)."""
        bsz, t = img_u8.shape[:2]
        m, dev = bsz * t, img_u8.device
        (gb, nb), (gc, nc) = self.engine.button_shape, self.engine.camera_shape
        ab, ac = torch.as_tensor(buttons), torch.as_tensor(camera)
        if ab.numel() != m * gb or ac.numel() != m * gc:
            raise ValueError(f"labels must be [{bsz}, {t}, {gb}] and [{bsz}, {t}, {gc}], got {tuple(ab.shape)} and {tuple(ac.shape)}")
        ab = ab.reshape(m, gb).to(device=dev, dtype=torch.int64).contiguous()
        ac = ac.reshape(m, gc).to(device=dev, dtype=torch.int64).contiguous()
        w = None
        probe = [ab.min(), ab.max(), ac.min(), ac.max()]
        if frame_weight is not None:
            w, wprobe = self._weights_on_device(frame_weight, img_u8)
            probe += wprobe
        vals = torch.stack([p.to(torch.float64) for p in probe]).tolist()
        if vals[0] < 0 or vals[1] >= nb:
            raise ValueError(f"button labels must lie in 0..{nb - 1} (found {int(vals[0])}..{int(vals[1])})")
        if vals[2] < 0 or vals[3] >= nc:
            raise ValueError(f"camera bins must lie in 0..{nc - 1} (found {int(vals[2])}..{int(vals[3])})")
        wsum = float(m)
        if w is not None:
            wsum = vals[4]
            self._check_weight_probe(wsum, vals[5])
            if wsum == 0 and not allow_zero_sum:
                raise ValueError("frame_weight: every weight is zero (the loss sum w nll / sum w is undefined)")
        return ab, ac, w, wsum

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward_saving(self, img_u8, mask: Optional[dict] = None) -> dict:
        """IDMEngine.forward with what the backward needs kept from the dense layer's pre-activation output `d` (fp32 [M, 256]) onward.  The frozen
        part in front of it runs exactly as the engine runs it (ops.conv3d_t5 per whole window, the CNN + dense layer in cnn_chunk pieces, nothing
        kept); behind it the same launches with the same tilings and split-K choice (the engine's, never the row count's), so the log-probs
        S["lp_b"] [M, 20, 2] / S["lp_c"] [M, 2, 11] equal IDMEngine.forward's bit for bit.
        train_cnn=True: the same chunks through the saving CNN forward (x0 and every CNN activation kept in S["cnn_saved"]; no `n` / dense folds, so
        the log-probs equal the engine's to the parity bounds only).
        mask: {"buttons": bool [B, T, 20, 2], "camera": bool [B, T, 2, 11]} (either entry optional), as IDMEngine.forward takes it: False -> the logit is
        the constant LOG0.  Kept in S["mask"] as {"buttons" / "camera": uint8 [M, G, n] or None} for the backward (None when no mask was given, and
        then the launches are the unmasked call's)."""
        eng = self.engine
        self.policy._ensure_packed()
        cfg, w = eng.cfg, eng.w
        bsz, t = img_u8.shape[:2]
        if t > ops.FULL_ATTENTION_MAX_T:
            raise NotImplementedError("the mask='none' attention kernels handle chunks of at most 160 frames")
        m = bsz * t
        hid, heads, dt = cfg["hidsize"], cfg["heads"], self.dtype
        lin = dict(tiling="throughput", splitk=eng.linear_splitk)       # the engine's choice, never the row count's
        frames = img_u8.reshape(m, *img_u8.shape[2:]).contiguous()
        wfrag, bias = w["conv3d"]
        outs, cnn_saved = [], []
        step = max(1, eng.cnn_chunk // t) * t if t <= eng.cnn_chunk else t
        for i in range(0, m, step):
            fr = frames[i:i + step]
            s0 = torch.zeros(fr.shape[0], 2, dtype=torch.float64, device=fr.device)
            x0 = ops.conv3d_t5(fr, wfrag, bias, eng.c3d_out, t, stats_out=s0)
            if self.train_cnn:
                xn, sv = self._cnn_forward_saving(fr, x0=x0, s_x0=s0)
                if self._cnn_backward:       # (a subset without a CNN-side tensor: the same forward, nothing of it kept)
                    cnn_saved.append(sv)
                del sv
                d32, _ = ops.linear(xn.view(xn.shape[0], -1), w["net.img_process.cnn.dense.w"], 256, splitk=DENSE_SPLITK, tiling=self.dense_tiling)
                outs.append(d32)
                del xn
            else:
                outs.append(eng._cnn_dense(None, x0=x0, s_x0=s0))
            del x0
        d = outs[0] if len(outs) == 1 else torch.cat(outs, 0)                        # [M, 256] pre-ReLU dense output: a constant of the backward
        trunk = self._trunk_forward_saving(d, lambda l, p, qkv: (ops.full_attention(qkv, bsz, t, heads, hid, dtype=dt), {}), **lin)
        _, lb = ops.layernorm(trunk["x_trunk"], w["final.g"], w["final.b"], relu_in=True, out_f32=False, dtype=dt)          # ReLU, then final_ln; no lastlayer
        lps, kept = {}, None
        for h, (groups, n) in (("buttons", eng.button_shape), ("camera", eng.camera_shape)):
            z, _ = ops.linear(lb, w[h + ".w"], groups * n, bias=w[h + ".b"], **lin)
            lps[h] = action_heads(z, ((h, 0, groups, n),), bsz, t, cfg["temperature"], mask)[h].view(m, groups, n)
        if mask is not None:
            kept = {h: (mask[h].reshape(m, groups, n).to(torch.uint8).contiguous() if mask.get(h) is not None else None)
                    for h, (groups, n) in (("buttons", eng.button_shape), ("camera", eng.camera_shape))}
        return self._release_unread(dict(trunk, m=m, bsz=bsz, t=t, dev=img_u8.device, d=d, lb=lb,
                                         lp_b=lps["buttons"], lp_c=lps["camera"], mask=kept, cnn_saved=cnn_saved, cnn_step=step))

    def _attention_backward(self, S, l, datt, g):
        """Mask "none": no memory, no relative-position bias -- nothing of the attention itself is trained."""
        cfg = self.engine.cfg
        return ops.full_attention_backward(S["saved"][l]["qkv"], datt, S["bsz"], S["t"], cfg["heads"], cfg["hidsize"])

    @torch.no_grad()
    def backward_from(self, S: dict, dz: torch.Tensor) -> Dict[str, torch.Tensor]:
        """dz: 16-bit [M, 64] = d loss / d (the two heads' logits, buttons first) -> the gradient of every trainable tensor.  Launch order: heads
        (dgrad, wgrad, bias sums) -> final_ln through its ReLU -> per block, last to first: mlp1, mlp0, its LayerNorm (+ skip), proj,
        ops.full_attention_backward, the fused QKV GEMM (+ skip), pre_r_ln -> pre_lstm_ln -> ImgObsProcess.linear and its LayerNorm; with
        train_cnn=True then per chunk of S["cnn_saved"] (released chunk by chunk): dense -> stacks 2, 1, 0 -> dx0 -> ops.conv3d_t5_backward, and the
        CNN's finish step."""
        P = {n: p.detach() for n, p in self.params.items()}
        g, dd = self._trunk_backward(S, dz, P)
        if self.train_cnn and self._cnn_backward:
            m, t, cnn_saved, step = S["m"], S["t"], S["cnn_saved"], S["cnn_step"]
            acc = self._cnn_backward_begin(P)
            c3d = (torch.zeros_like(P["net.conv3d_layer.layer.weight"], dtype=torch.float32), torch.zeros_like(P["net.conv3d_layer.layer.bias"], dtype=torch.float32))
            for ci, i in enumerate(range(0, m, step)):
                sv = cnn_saved[ci]
                dx0 = self._cnn_backward_chunk(sv, dd[i:i + step].contiguous(), acc)
                ops.conv3d_t5_backward(sv["img"], sv["stacks"][0]["x_prev"], dx0, t, out=c3d)
                cnn_saved[ci] = None
                del sv, dx0
            self._cnn_backward_finish(acc, P, g)
            g["net.conv3d_layer.layer.weight"], g["net.conv3d_layer.layer.bias"] = c3d
            if self._subset is not None:     # no cut inside the CNN: the frozen tensors of that side are dropped
                for n in [n for n in g if n.startswith(_FROZEN) and n not in self._subset]:
                    del g[n]
        return g

    @torch.no_grad()
    def loss_and_grads(self, img_u8, buttons, camera, *, frame_weight=None, metrics: Optional[dict] = None, unscaled: bool = True,
                       global_weight: Optional[float] = None, micro_batches: int = 1):
        """img_u8 uint8 [B, T, 128, 128, 3]; buttons int64 [B, T, 20] in {0, 1}; camera int64 [B, T, 2] in 0..10 -> (loss, grads of every trainable
        tensor).  frame_weight: [B, T] finite, non-negative (0 = a frame left out: exact zeros whatever it holds).  Labels out of range and bad
        weights raise ValueError before anything is queued (one host transfer).  metrics: a dict this call fills as BCTrainer.loss_and_grads does
        (loss, nll_* , entropy_*, acc_* = the fraction of groups whose arg-max is the label, weight_sum, frames, frame_nll, frame_out; device
        tensors).  unscaled=False (what step() uses): in the fp16 mode the gradients stay multiplied by 1 / grad_unscale(sum w).
        global_weight (default: this call's own frame count / weight sum): the count of a larger batch these frames are a part of -- the gradients
        are this part's share of the gradient of THAT batch's mean loss (BCTrainer's global_frames), and all-zero weights are then legal.
        micro_batches=K > 1 (gradient accumulation): the B sequences run as K row groups (micro_batch_rows) one after the other, each
        carrying the whole call's count, their gradients summed in order (ops.grad_accumulate_); the loss and the metrics come from the groups'
        totals summed in fp64, frame_nll / frame_out are the concatenations.  The inputs are checked once, for the whole batch."""
        rows = self.micro_batch_rows(img_u8.shape[0], micro_batches) if micro_batches != 1 else None
        ab, ac, w, wsum = self._checked_inputs(img_u8, buttons, camera, frame_weight, allow_zero_sum=global_weight is not None)
        count = wsum if global_weight is None else float(global_weight)
        self._weight_sum = count
        bsz, t = img_u8.shape[:2]
        if rows is None:
            g, totals, frame_out = self._loss_and_grads_checked(img_u8, ab, ac, w, count)
            loss = self._record_loss(frame_out, w, wsum)
        else:
            def run(k, lo, hi):
                f = slice(lo * t, hi * t)
                return self._loss_and_grads_checked(img_u8[lo:hi], ab[f], ac[f], None if w is None else w[f], count) + (None,)
            g, totals, frame_out, _ = self._accumulated_window(rows, run)
            loss = (totals[0] + totals[1]) / totals[6]
        self._idm_totals = totals
        if metrics is not None:
            self._fill_metrics(metrics, totals, frame_out, bsz, t)
            metrics["loss"] = loss
        if unscaled and self.scaled:
            self._unscale_(g, count)
        return loss, g

    def _loss_and_grads_checked(self, img_u8, ab, ac, w, count: float):
        """Forward, the fused loss and the backward of checked inputs (_checked_inputs) under the frame count `count` -> (grads -- in the fp16 mode
        multiplied by 1 / grad_unscale(count) --, ops.idm_loss's totals [8], its records [M, 8])."""
        S = self.forward_saving(img_u8)
        scale = (self.loss_scale if self.scaled else 1.0 / count) / self.engine.cfg["temperature"]
        dz, frame_out, totals = ops.idm_loss(S["lp_b"], S["lp_c"], ab, ac, scale, weight=w, dtype=self.dtype)
        return self.backward_from(S, dz), totals, frame_out

    @torch.no_grad()
    def evaluate(self, img_u8, buttons, camera, *, frame_weight=None) -> dict:
        """Forward-only loss and metrics of a [B, T] chunk: IDMEngine.forward (nothing saved) + ops.idm_loss without dz."""
        ab, ac, w, _ = self._checked_inputs(img_u8, buttons, camera, frame_weight)
        bsz, t = img_u8.shape[:2]
        with self._adapters_applied():
            self.policy._ensure_packed()
            out = self.engine.forward(img_u8)
        (gb, nb), (gc, nc) = self.engine.button_shape, self.engine.camera_shape
        lp_b, lp_c = out["buttons"].reshape(bsz * t, gb, nb), out["camera"].reshape(bsz * t, gc, nc)
        _, frame_out, totals = ops.idm_loss(lp_b, lp_c, ab, ac, 0.0, weight=w, dtype=self.dtype, want_dz=False)
        metrics: dict = {}
        self._fill_metrics(metrics, totals, frame_out, bsz, t)
        return metrics

    @torch.no_grad()
    def step(self, img_u8, buttons, camera, *, frame_weight=None, metrics: Optional[dict] = None, micro_batches: int = 1) -> float:
        """One Adam step (ops.adam_step_multi_: one launch for all tensors; in the fp16 mode it un-scales the gradients and leaves every tensor
        untouched when the overflow check fired; with max_grad_norm set the gradients are clipped by their global norm inside that launch and metrics gains
        grad_norm / clip_coef / grad_norm_per_tensor -- TrainerBase._optimizer_tail).  Returns the loss.  The policy's next predict / label_video sees the new weights.
        micro_batches=K: loss_and_grads's gradient accumulation over K row groups; one Adam launch, clip and loss-scale decision for the window."""
        self._need_optimizer_state()
        loss, grads = self.loss_and_grads(img_u8, buttons, camera, frame_weight=frame_weight, metrics=metrics, unscaled=False, micro_batches=micro_batches)
        loss, _ = self._optimizer_tail(loss, grads, self.grad_unscale(self._weight_sum), img_u8.device, metrics)
        return loss
