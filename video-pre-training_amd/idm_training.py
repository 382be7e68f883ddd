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

NOT built: data-parallel IDM steps, an autograd boundary for the IDM, and chunk streams for the CNN backward (one stream).

The backward runs on the HIP kernels of the BC step (training.linear_backward, ops.layernorm_backward, ops.gate_cast, ops.column_sum_,
ops.adam_step_multi_) plus two of its own: ops.full_attention_backward (the mask-"none" attention) and ops.idm_loss (the grouped heads' loss,
gradient and metrics in one launch).  Every reduction has a fixed order: the same batch gives the same gradient bits."""
from typing import Dict, List, Optional

import torch

from . import ops
from .cnn_training import CnnTrainingMixin
from .engine import DENSE_SPLITK, action_heads
from .training import BCTrainer, linear_backward

_FROZEN = ("net.conv3d_layer.", "net.img_process.cnn.")
_UNREACHED = ("net.lastlayer.",)       # computed and discarded by the reference (lib/policy.py:390-391): not part of the function that is trained


class IDMTrainer(CnnTrainingMixin):
    stack0_from_x0 = True        # the CNN's stack 0 is fed by the temporal conv (cnn_training.py)
    dense_tiling = "throughput"  # as IDMEngine: the MFMA GEMM whatever the row count (a one-window chunk of <= 8 frames would take the GEMV kernel)

    def __init__(self, policy, lr: float = 0.000181, weight_decay: float = 0.039428, betas=(0.9, 0.999), eps: float = 1e-8,
                 optimizer_state: bool = True, loss_scale: Optional[float] = None, scale_growth_interval: int = 200, train_cnn: bool = False,
                 max_grad_norm: Optional[float] = None):
        """max_grad_norm: global-norm gradient clipping as BCTrainer's (None = off, the default; float("inf") = measure only; a non-finite norm skips
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
        self.train_cnn = bool(train_cnn)
        self.max_grad_norm = self._checked_max_grad_norm(max_grad_norm)
        self.policy = policy
        self.engine = policy._engine
        self.dtype = self.engine.dtype
        self.scaled = self.engine.precision == "fp16"
        self.loss_scale = float(loss_scale) if loss_scale is not None else (256.0 if self.scaled else 1.0)
        self.scale_growth_interval, self._clean_steps, self.skipped_steps = int(scale_growth_interval), 0, 0
        self.lr, self.wd, self.betas, self.eps = lr, weight_decay, betas, eps
        self.step_count = 0
        self._cnn_flags_from_env()
        if self.train_cnn and not self.fused_pool:
            raise RuntimeError("IDMTrainer(train_cnn=True) needs the pool-fused forward (ops.conv3x3_pool_argmax): at 128 x 128 only the pooled entry of "
                               "the conv backward is built -- unset VPT_BC_FUSED_POOL=0")
        self.params: Dict[str, torch.nn.Parameter] = dict(policy.named_parameters())
        self.trainable = [n for n in self.params if self._is_trainable(n)]
        self.m = {n: torch.zeros_like(self.params[n], dtype=torch.float32) for n in self.trainable} if optimizer_state else {}
        self.v = {n: torch.zeros_like(self.params[n], dtype=torch.float32) for n in self.trainable} if optimizer_state else {}

    def _is_trainable(self, name: str) -> bool:
        if (name.startswith(_FROZEN) and not self.train_cnn) or name.startswith(_UNREACHED):
            return False
        return self.params[name].numel() > 0            # (b_nd is [10, maxlen = 0])

    # ---- checkpoint / resume: BCTrainer's keys ---------------------------------------------------
    def state_dict(self) -> dict:
        self._need_optimizer_state()
        return dict(step=self.step_count, lr=self.lr, weight_decay=self.wd, betas=tuple(self.betas), eps=self.eps,
                    loss_scale=self.loss_scale, train_cnn=self.train_cnn, max_grad_norm=self.max_grad_norm,
                    exp_avg={n: t.detach().clone() for n, t in self.m.items()},
                    exp_avg_sq={n: t.detach().clone() for n, t in self.v.items()})

    def _need_optimizer_state(self):
        if not self.m and self.trainable:
            raise RuntimeError("this IDMTrainer was built with optimizer_state=False (gradients only): step / state_dict / load_state_dict need the Adam moments")

    def load_state_dict(self, sd: dict):
        self._need_optimizer_state()
        if self.scaled and "loss_scale" in sd:
            self.loss_scale = float(sd["loss_scale"])
        if "max_grad_norm" in sd:
            self.max_grad_norm = self._checked_max_grad_norm(sd["max_grad_norm"])
        if set(sd["exp_avg"]) != set(self.m):
            raise KeyError(f"optimizer state does not match the trainable parameters: {sorted(set(sd['exp_avg']) ^ set(self.m))[:4]} ...")
        self.step_count = int(sd["step"])
        self.lr, self.wd, self.betas, self.eps = sd["lr"], sd["weight_decay"], tuple(sd["betas"]), sd["eps"]
        for n in self.m:
            self.m[n].copy_(sd["exp_avg"][n])
            self.v[n].copy_(sd["exp_avg_sq"][n])

    def grad_unscale(self, weight_sum: float) -> float:
        """What loss_and_grads(unscaled=False)'s gradients must be multiplied by to be d(loss)/d(parameter): 1 in bf16."""
        return 1.0 / (self.loss_scale * weight_sum) if self.scaled else 1.0

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

    def _checked_inputs(self, img_u8, buttons, camera, frame_weight):
        """Labels -> int64 [M, G] on the images' device, weights -> fp32 [M] (or None); the weights' sum and minimum and the labels' extrema come
        to the host in ONE transfer (one synchronisation per step).  ValueError on a label out of range, on a negative or non-finite weight and on
        all-zero weights.  -> (buttons, camera, weights | None, weight sum)."""
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
            w = torch.as_tensor(frame_weight)
            if w.numel() != m:
                raise ValueError(f"frame_weight must hold one weight per frame ([{bsz}, {t}]), got {tuple(w.shape)}")
            w = w.reshape(m).to(device=dev, dtype=torch.float32).contiguous()
            w64 = w.to(torch.float64)
            probe += [w64.sum(), w64.min()]
        vals = torch.stack([p.to(torch.float64) for p in probe]).tolist()
        if vals[0] < 0 or vals[1] >= nb:
            raise ValueError(f"button labels must lie in 0..{nb - 1} (found {int(vals[0])}..{int(vals[1])})")
        if vals[2] < 0 or vals[3] >= nc:
            raise ValueError(f"camera bins must lie in 0..{nc - 1} (found {int(vals[2])}..{int(vals[3])})")
        wsum = float(m)
        if w is not None:
            wsum, wmin = vals[4], vals[5]
            if not (wmin >= 0.0) or wsum != wsum or wsum in (float("inf"), float("-inf")):
                raise ValueError(f"frame_weight must be finite and non-negative (min {wmin}, sum {wsum})")
            if wsum == 0:
                raise ValueError("frame_weight: every weight is zero (the loss sum w nll / sum w is undefined)")
        return ab, ac, w, wsum

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward_saving(self, img_u8) -> dict:
        """IDMEngine.forward with what the backward needs kept from the dense layer's pre-activation output `d` (fp32 [M, 256]) onward.  The frozen
        part in front of it runs exactly as the engine runs it (ops.conv3d_t5 per whole window, the CNN + dense layer in cnn_chunk pieces, nothing
        kept); behind it the same launches with the same tilings and split-K choice (the engine's, never the row count's), so the log-probs
        S["lp_b"] [M, 20, 2] / S["lp_c"] [M, 2, 11] equal IDMEngine.forward's bit for bit.
        train_cnn=True: the same chunks through the saving CNN forward (x0 and every CNN activation kept in S["cnn_saved"]; no `n` / dense folds, so
        the log-probs equal the engine's to the parity bounds only)."""
        pol, eng = self.policy, self.engine
        pol._ensure_packed()
        cfg, w = eng.cfg, eng.w
        bsz, t = img_u8.shape[:2]
        if t > ops.FULL_ATTENTION_MAX_T:
            raise NotImplementedError("the mask='none' attention kernels handle chunks of at most 160 frames")
        m = bsz * t
        hid, heads, ratio = cfg["hidsize"], cfg["heads"], cfg["pointwise_ratio"]
        sk, dt, tl = eng.linear_splitk, self.dtype, "throughput"
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
                cnn_saved.append(sv)
                d32, _ = ops.linear(xn.view(xn.shape[0], -1), w["net.img_process.cnn.dense.w"], 256, splitk=DENSE_SPLITK, tiling=self.dense_tiling)
                outs.append(d32)
                del xn
            else:
                outs.append(eng._cnn_dense(None, x0=x0, s_x0=s0))
            del x0
        d = outs[0] if len(outs) == 1 else torch.cat(outs, 0)                        # [M, 256] pre-ReLU dense output: a constant of the backward
        pl = "net.img_process.linear."
        _, dn = ops.layernorm(d, w[pl + "g"], w[pl + "b"], relu_in=True, dtype=dt)
        x, x_lin16 = ops.linear(dn, w[pl + "w"], hid, relu=True, out_f32=True, out_bf16=True, tiling=tl, splitk=sk)
        x_pre = None
        if cfg["use_pre_lstm_ln"]:
            x_pre = x
            x, _ = ops.layernorm(x_pre, w["prelstm.g"], w["prelstm.b"], out_f32=True, out_bf16=False, dtype=dt)
        saved: List[dict] = []
        for l in range(cfg["n_layers"]):
            p = f"net.recurrent_layer.blocks.{l}."
            x1, x1b = ops.layernorm(x, w[p + "ln1.g"], w[p + "ln1.b"], out_f32=True, dtype=dt)
            qkv, _ = ops.linear(x1b, w[p + "qkv.w"], eng.n_qkvr, bias=w[p + "qkv.b"], tiling=tl, splitk=sk)
            att = ops.full_attention(qkv, bsz, t, heads, hid, dtype=dt)
            x2, _ = ops.linear(att, w[p + "proj.w"], hid, bias=w[p + "proj.b"], res=x1, tiling=tl, splitk=sk)      # x2 = x1 + proj (engine._block)
            _, hb = ops.layernorm(x2, w[p + "ln2.g"], w[p + "ln2.b"], dtype=dt)
            _, h2 = ops.linear(hb, w[p + "mlp0.w"], hid * ratio, relu=True, out_f32=False, out_bf16=True, tiling=tl, splitk=sk)
            xo, _ = ops.linear(h2, w[p + "mlp1.w"], hid, bias=w[p + "mlp1.b"], res=x2, tiling=tl, splitk=sk)
            saved.append(dict(x=x, x1b=x1b, qkv=qkv, att=att, x2=x2, hb=hb, h2=h2))
            x = xo
        x_trunk = x
        _, lb = ops.layernorm(x_trunk, w["final.g"], w["final.b"], relu_in=True, out_f32=False, dtype=dt)          # ReLU, then final_ln; no lastlayer
        lps = {}
        for h, (groups, n) in (("buttons", eng.button_shape), ("camera", eng.camera_shape)):
            z, _ = ops.linear(lb, w[h + ".w"], groups * n, bias=w[h + ".b"], tiling=tl, splitk=sk)
            lps[h] = action_heads(z, ((h, 0, groups, n),), bsz, t, cfg["temperature"])[h].view(m, groups, n)
        return dict(m=m, bsz=bsz, t=t, dev=img_u8.device, d=d, dn=dn, x_lin16=x_lin16, x_pre=x_pre, saved=saved, x_trunk=x_trunk, lb=lb,
                    lp_b=lps["buttons"], lp_c=lps["camera"], cnn_saved=cnn_saved, cnn_step=step)

    @torch.no_grad()
    def backward_from(self, S: dict, dz: torch.Tensor) -> Dict[str, torch.Tensor]:
        """dz: 16-bit [M, 64] = d loss / d (the two heads' logits, buttons first) -> the gradient of every trainable tensor.  Launch order: heads
        (dgrad, wgrad, bias sums) -> final_ln through its ReLU -> per block, last to first: mlp1, mlp0, its LayerNorm (+ skip), proj,
        ops.full_attention_backward, the fused QKV GEMM (+ skip), pre_r_ln -> pre_lstm_ln -> ImgObsProcess.linear and its LayerNorm; with
        train_cnn=True then per chunk of S["cnn_saved"] (released chunk by chunk): dense -> stacks 2, 1, 0 -> dx0 -> ops.conv3d_t5_backward, and the
        CNN's finish step."""
        eng = self.engine
        cfg = eng.cfg
        P = {n: p.detach() for n, p in self.params.items()}
        m, bsz, t, dev = S["m"], S["bsz"], S["t"], S["dev"]
        hid, heads, ratio = cfg["hidsize"], cfg["heads"], cfg["pointwise_ratio"]
        (gb, nb), (gc, nc) = eng.button_shape, eng.camera_shape
        nbt, nct = gb * nb, gc * nc
        nh = nbt + nct
        g: Dict[str, torch.Tensor] = {}
        zeros = lambda n_: torch.zeros(n_, dtype=torch.float32, device=dev)
        # heads: one [62, hid] matrix for the two backward GEMMs
        wh = torch.cat([P["pi_head.buttons.linear_layer.weight"], P["pi_head.camera.linear_layer.weight"]], 0)
        dlat, _, dwh = linear_backward(dz, nh, S["lb"], wh)
        dbh = zeros(nh)
        ops.column_sum_(dbh, dz, nh)
        g["pi_head.buttons.linear_layer.weight"], g["pi_head.camera.linear_layer.weight"] = dwh[:nbt], dwh[nbt:nh]
        g["pi_head.buttons.linear_layer.bias"], g["pi_head.camera.linear_layer.bias"] = dbh[:nbt], dbh[nbt:nh]
        del dz, dwh
        # final_ln(relu(x_trunk))
        g["net.final_ln.weight"], g["net.final_ln.bias"] = zeros(hid), zeros(hid)
        dx = ops.layernorm_backward(S["x_trunk"], P["net.final_ln.weight"], dlat, g["net.final_ln.weight"], g["net.final_ln.bias"], relu_in=True)
        del dlat
        for l in reversed(range(cfg["n_layers"])):
            p = f"net.recurrent_layer.blocks.{l}."
            o = p + "r.orc_block."
            s = S["saved"][l]
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
            del dh16, dhb, dout16
            # proj: x2 = x1 + att Wp^T + bp
            dx2_16 = ops.gate_cast(dx2, hid, dtype=self.dtype)
            datt, _, g[o + "proj_layer.weight"] = linear_backward(dx2_16, hid, s["att"], P[o + "proj_layer.weight"])
            g[o + "proj_layer.bias"] = zeros(hid)
            ops.column_sum_(g[o + "proj_layer.bias"], dx2_16, hid)
            # attention (mask "none": no memory, no relative-position bias -> r_layer is unreached)
            dqkv = ops.full_attention_backward(s["qkv"], datt, bsz, t, heads, hid)
            nq = eng.n_qkvr
            dq16 = ops.gate_cast(dqkv, (nq + 63) // 64 * 64, dtype=self.dtype)
            wq = torch.cat([P[o + "q_layer.weight"], P[o + "k_layer.weight"], P[o + "v_layer.weight"]], 0)
            dx1, _, dwq = linear_backward(dq16, nq, s["x1b"], wq, res=dx2)      # dx1 = dx2 (skip) + dqkv Wqkv
            g[o + "q_layer.weight"], g[o + "k_layer.weight"], g[o + "v_layer.weight"] = dwq[:hid], dwq[hid:2 * hid], dwq[2 * hid:3 * hid]
            g[o + "q_layer.bias"] = zeros(hid)
            ops.column_sum_(g[o + "q_layer.bias"], dq16, hid)
            g[o + "r_layer.weight"], g[o + "r_layer.bias"] = torch.zeros_like(P[o + "r_layer.weight"]), torch.zeros_like(P[o + "r_layer.bias"])
            g[p + "pre_r_ln.weight"], g[p + "pre_r_ln.bias"] = zeros(hid), zeros(hid)
            dx = ops.layernorm_backward(s["x"], P[p + "pre_r_ln.weight"], dx1, g[p + "pre_r_ln.weight"], g[p + "pre_r_ln.bias"])
            del dx2, dx2_16, datt, dqkv, dq16, dx1, dwq
        if cfg["use_pre_lstm_ln"]:
            g["net.pre_lstm_ln.weight"], g["net.pre_lstm_ln.bias"] = zeros(hid), zeros(hid)
            dx = ops.layernorm_backward(S["x_pre"], P["net.pre_lstm_ln.weight"], dx, g["net.pre_lstm_ln.weight"], g["net.pre_lstm_ln.bias"])
        # ImgObsProcess.linear: x = relu(dn Wlin^T); its LayerNorm sits on relu(d), d being the CNN's output (its gradient goes on only with train_cnn)
        pl = "net.img_process.linear."
        dx16 = ops.gate_cast(dx, hid, mask=S["x_lin16"])
        ddn, _, g[pl + "layer.weight"] = linear_backward(dx16, hid, S["dn"], P[pl + "layer.weight"])
        g[pl + "norm.weight"], g[pl + "norm.bias"] = zeros(256), zeros(256)
        dd = ops.layernorm_backward(S["d"], P[pl + "norm.weight"], ddn, g[pl + "norm.weight"], g[pl + "norm.bias"], relu_in=True)
        if self.train_cnn:
            cnn_saved, step = S["cnn_saved"], S["cnn_step"]
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
        return g

    @torch.no_grad()
    def loss_and_grads(self, img_u8, buttons, camera, *, frame_weight=None, metrics: Optional[dict] = None, unscaled: bool = True):
        """img_u8 uint8 [B, T, 128, 128, 3]; buttons int64 [B, T, 20] in {0, 1}; camera int64 [B, T, 2] in 0..10 -> (loss, grads of every trainable
        tensor).  frame_weight: [B, T] finite, non-negative (0 = a frame left out: exact zeros whatever it holds).  Labels out of range and bad
        weights raise ValueError before anything is queued (one host transfer).  metrics: a dict this call fills as BCTrainer.loss_and_grads does
        (loss, nll_* , entropy_*, acc_* = the fraction of groups whose arg-max is the label, weight_sum, frames, frame_nll, frame_out; device
        tensors).  unscaled=False (what step() uses): in the fp16 mode the gradients stay multiplied by 1 / grad_unscale(sum w)."""
        ab, ac, w, wsum = self._checked_inputs(img_u8, buttons, camera, frame_weight)
        S = self.forward_saving(img_u8)
        scale = (self.loss_scale if self.scaled else 1.0 / wsum) / self.engine.cfg["temperature"]
        dz, frame_out, totals = ops.idm_loss(S["lp_b"], S["lp_c"], ab, ac, scale, weight=w, dtype=self.dtype)
        loss = BCTrainer._record_loss(frame_out, w, wsum)
        if metrics is not None:
            BCTrainer._fill_metrics(metrics, totals, frame_out, S["bsz"], S["t"])
            metrics["loss"] = loss
        self._weight_sum = wsum
        g = self.backward_from(S, dz)
        if unscaled and self.scaled:
            f = self.grad_unscale(wsum)
            for t_ in g.values():
                t_.mul_(f)
        return loss, g

    @torch.no_grad()
    def evaluate(self, img_u8, buttons, camera, *, frame_weight=None) -> dict:
        """Forward-only loss and metrics of a [B, T] chunk: IDMEngine.forward (nothing saved) + ops.idm_loss without dz."""
        ab, ac, w, _ = self._checked_inputs(img_u8, buttons, camera, frame_weight)
        self.policy._ensure_packed()
        bsz, t = img_u8.shape[:2]
        out = self.engine.forward(img_u8)
        (gb, nb), (gc, nc) = self.engine.button_shape, self.engine.camera_shape
        lp_b, lp_c = out["buttons"].reshape(bsz * t, gb, nb), out["camera"].reshape(bsz * t, gc, nc)
        _, frame_out, totals = ops.idm_loss(lp_b, lp_c, ab, ac, 0.0, weight=w, dtype=self.dtype, want_dz=False)
        metrics: dict = {}
        BCTrainer._fill_metrics(metrics, totals, frame_out, bsz, t)
        return metrics

    @torch.no_grad()
    def step(self, img_u8, buttons, camera, *, frame_weight=None, metrics: Optional[dict] = None) -> float:
        """One Adam step (ops.adam_step_multi_: one launch for all tensors; in the fp16 mode it un-scales the gradients and leaves every tensor
        untouched when the overflow check fired; with max_grad_norm set the gradients are clipped by their global norm inside that launch and metrics gains
        grad_norm / clip_coef / grad_norm_per_tensor -- CnnTrainingMixin._optimizer_tail).  Returns the loss.  The policy's next predict / label_video sees the new weights."""
        self._need_optimizer_state()
        loss, grads = self.loss_and_grads(img_u8, buttons, camera, frame_weight=frame_weight, metrics=metrics, unscaled=False)
        loss, _ = self._optimizer_tail(loss, grads, self.grad_unscale(self._weight_sum), img_u8.device, metrics)
        return loss
