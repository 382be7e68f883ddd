"""The IMPALA CNN's training forward and backward, shared by the trainers (ONE copy of the launch order).

BCTrainer(train_cnn=True) feeds stack 0 from the uint8 image through the fused first conv (vpt_conv_first_kernel / vpt_conv_first_bwd_kernel);
IDMTrainer(train_cnn=True) feeds it from the temporal conv's output (x0, s_x0): there stack 0's `firstconv` is a normed 3x3 conv like the other
stacks' (first_conv_norm=True, lib/policy.py:360-363), takes the generic pool-fused branch, and its dgrad returns dx0 -- the gradient the temporal
conv's backward reads.  `stack0_from_x0` selects between the two; everything else is one code path.

A class that mixes this in provides: engine (a packed PolicyEngine / IDMEngine), dtype, and the flags of _cnn_flags_from_env()."""
import os

import torch

from . import ops, packing


class CnnTrainingMixin:
    stack0_from_x0 = False       # True: stack 0 is fed by (x0, s_x0) and is a normed conv (the inverse dynamics model)
    dense_tiling = "auto"        # ops.linear tiling of the dense layer's dgrad; "throughput": a frame's result does not depend on the chunk's frame count

    def _cnn_flags_from_env(self):
        # a block's conv1 -> conv0 backward through ONE dgrad epilogue (_block_backward); 0 = the round-4 path (A/B)
        self.gated_dgrad = os.environ.get("VPT_BC_GATED_DGRAD", "1") != "0"
        # stacks 1..: firstconv + max-pool as ONE pass that records the arg-max positions (ops.conv3x3_pool_argmax), its backward from the pooled
        # tensors alone (ops.conv_backward_prepare_pooled); 0 = conv -> vpt_pool_kernel with the pre-pool tensor kept (round 4, A/B)
        self.fused_pool = os.environ.get("VPT_BC_FUSED_POOL", "1") != "0"
        # ... and with it the second pass of the GroupNorm-`n` backward of stacks 1.. folded into that consumer (needs fused_pool); 0: two passes (A/B)
        self.fold_n_backward = os.environ.get("VPT_BC_FOLD_N_BWD", "1") != "0"
        # ... and stack 0's inside the first conv's backward kernel (ops.conv_first_backward(nfold=...), round 6); 0: two passes + the plain kernel (A/B)
        self.fold_n_backward0 = os.environ.get("VPT_BC_FOLD_N_BWD0", "1") != "0"

    # ------------------------------------------------------------------------------------------
    # IMPALA CNN: forward that keeps every activation (6.2 MB / frame on the 2x model: a 64 x 128 batch is 50 GB of
    # the 288 GB HBM, so nothing is recomputed), and the backward through the folded GroupNorm convolutions.
    # ------------------------------------------------------------------------------------------
    def _cnn_forward_saving(self, img: torch.Tensor, x0=None, s_x0=None):
        """PolicyEngine._cnn_chunk without in-place reuse; returns (xn, saved).  stack0_from_x0: (x0, s_x0) = the temporal conv's blocked output and
        its frame statistics feed stack 0's normed firstconv; `img` is only kept for the caller."""
        eng = self.engine
        cfg, w = eng.cfg, eng.w
        if self.stack0_from_x0 != (x0 is not None):
            raise ValueError("_cnn_forward_saving: (x0, s_x0) are given exactly when stack 0 is fed by the temporal conv")
        if self.stack0_from_x0 and not self.fused_pool:
            raise RuntimeError("training the CNN behind the temporal conv needs the pool-fused forward (ops.conv3x3_pool_argmax): at 128 x 128 only the "
                               "pooled entry of the conv backward is built -- unset VPT_BC_FUSED_POOL=0")
        f = img.shape[0]
        st = torch.zeros(24, f, 2, dtype=torch.float64, device=img.device)
        si = 0

        def nxt():
            nonlocal si
            si += 1
            return st[si - 1]

        sv = dict(img=img, stacks=[])
        x, s_x = x0, s_x0
        for s, c in enumerate(cfg["chans"]):
            p = f"net.img_process.cnn.stacks.{s}."
            rec = dict(x_prev=x, s_prev=s_x)
            s_pool = nxt()
            if s == 0 and not self.stack0_from_x0:
                pooled = ops.conv_first(img, w[p + "firstconv"], c, stats_out=s_pool)
            else:
                wpk, sa, sg = w[p + "firstconv"]
                if self.fused_pool:    # firstconv + ReLU + max-pool in one pass that also records where each maximum sits (round 5): no pre-pool tensor
                    pooled, rec["mask"] = ops.conv3x3_pool_argmax(x, wpk, sa, sg, s_x, c, stats_out=s_pool)
                else:
                    rec["pre"] = ops.conv3x3(x, wpk, sa, sg, s_x, c)
                    pooled, rec["argmax"] = ops.maxpool(rec["pre"], stats_out=s_pool, want_argmax=True)
            s_x = nxt()
            x = ops.frame_affine(pooled, w[p + "n.g"], w[p + "n.b"], s_pool, stats_out=s_x)
            rec.update(pooled=pooled, s_pool=s_pool, blocks=[])
            for b in range(2):
                wpk, sa, sg = w[f"{p}blocks.{b}.conv0"]
                s_y = nxt()
                y = ops.conv3x3(x, wpk, sa, sg, s_x, c, stats_out=s_y)
                wpk, sa, sg = w[f"{p}blocks.{b}.conv1"]
                s_n = nxt()
                xo = ops.conv3x3(y, wpk, sa, sg, s_y, c, res=x, stats_out=s_n)
                rec["blocks"].append(dict(x_in=x, s_in=s_x, y=y, s_y=s_y, x_out=xo))
                x, s_x = xo, s_n
            sv["stacks"].append(rec)
        sv["x_last"], sv["s_last"] = x, s_x
        p = "net.img_process.cnn.dense."
        return ops.frame_affine(x, w[p + "g"], w[p + "b"], s_x, per_element=True), sv

    def _conv_names(self):
        names = []
        for s in range(len(self.engine.cfg["chans"])):
            p = f"net.img_process.cnn.stacks.{s}."
            if s > 0 or self.stack0_from_x0:
                names.append(p + "firstconv")
            for b in range(2):
                for cv in range(2):
                    names.append(f"{p}blocks.{b}.conv{cv}")
        return names

    def _cnn_backward_begin(self, P):
        """Per-step operands of the CNN backward (transposed conv weights, dense W^T) and zeroed accumulators."""
        cfg = self.engine.cfg
        dev = next(iter(P.values())).device
        c2 = cfg["chans"][-1]
        acc = dict(wt={}, raw={}, n={}, dense=None)
        for q in self._conv_names():
            acc["wt"][q] = packing.pack_conv3x3_dgrad(P[q + ".layer.weight"].float(), P[q + ".norm.weight"].float(), dtype=self.dtype)
        pd = "net.img_process.cnn.dense."
        wd_blk = packing.chw_to_blocked_columns(P[pd + "layer.weight"].float(), c2, 16, 16)      # [256, K] in activation order
        acc["dense_wt"] = packing.pack_linear(wd_blk.t().contiguous(), dtype=self.dtype)                           # dgrad operand: N = K, K = 256
        k = wd_blk.shape[1]
        acc["dense_dwT"] = torch.zeros(k, 256, dtype=torch.float32, device=dev)
        acc["dense_dg"], acc["dense_db"] = torch.zeros(k, dtype=torch.float32, device=dev), torch.zeros(k, dtype=torch.float32, device=dev)
        for s, c in enumerate(cfg["chans"]):
            acc["n"][s] = (torch.zeros(c, dtype=torch.float32, device=dev), torch.zeros(c, dtype=torch.float32, device=dev))
        return acc

    def _conv_layer_backward(self, q, acc, dy, y, res, x_in, s_in, skip, need_dx=True, pool=None):
        """One GN -> conv3x3 -> ReLU (+res) layer: accumulates the raw weight-gradient pieces and returns dx (+skip).
        pool = (dpooled, argmax) when the layer feeds the stack's max-pool (dy is then None)."""
        _, sa, sg = self.engine.w[q]
        cin = x_in.shape[1] * 32
        r = self._raw_acc(acc, q, y.shape[1] * 32, cin, sa, sg)
        dacc, coef, _, _ = ops.conv_backward_prepare(dy, y, res, s_in, sa, sg, cin, dpooled=pool[0] if pool else None,
                                                     argmax=pool[1] if pool else None, d_sa=r[1], d_sg=r[2])
        ops.conv3x3_wgrad(dacc, x_in, out=r[0])
        if not need_dx:
            return None
        return ops.conv3x3_dgrad(dacc, acc["wt"][q], cin, skip=skip, xin=x_in, coef=coef)

    def _block_backward(self, p, b, blk, acc, dx):
        """CnnBasicBlock backward (lib/impala_cnn.py:50-52: x + conv1(conv0(x))): dx w.r.t. the block output -> dx w.r.t. its input.
        gated_dgrad (round 5, default): conv1's dgrad writes conv0's backward operand directly (ops.conv3x3_dgrad_gated: conv0 has no residual,
        its output is conv1's input, so its ReLU gate and rstd scale fit into that epilogue), and conv0's per-element prepare pass (read dy, read y,
        write dacc) becomes a reduction over the operand (ops.conv_backward_reduce: one read)."""
        q1, q0 = f"{p}blocks.{b}.conv1", f"{p}blocks.{b}.conv0"
        if not self.gated_dgrad:
            dy = self._conv_layer_backward(q1, acc, dx, blk["x_out"], blk["x_in"], blk["y"], blk["s_y"], None)
            return self._conv_layer_backward(q0, acc, dy, blk["y"], None, blk["x_in"], blk["s_in"], dx)
        w = self.engine.w
        x_in, y, x_out = blk["x_in"], blk["y"], blk["x_out"]
        c_in, c_mid = x_in.shape[1] * 32, y.shape[1] * 32
        # conv1 (residual layer): prepare -> wgrad -> gated dgrad
        _, sa1, sg1 = w[q1]
        r1 = self._raw_acc(acc, q1, x_out.shape[1] * 32, c_mid, sa1, sg1)
        dacc1, coef1, _, _ = ops.conv_backward_prepare(dx, x_out, x_in, blk["s_y"], sa1, sg1, c_mid, d_sa=r1[1], d_sg=r1[2])
        ops.conv3x3_wgrad(dacc1, y, out=r1[0])
        dacc0, gate_u = ops.conv3x3_dgrad_gated(dacc1, acc["wt"][q1], c_mid, y, coef1, blk["s_in"], c_in)
        del dacc1
        # conv0 (no residual): its operand exists already; sums only
        _, sa0, sg0 = w[q0]
        r0 = self._raw_acc(acc, q0, c_mid, c_in, sa0, sg0)
        coef0, _, _ = ops.conv_backward_reduce(dacc0, gate_u, blk["s_in"], sa0, sg0, c_in, d_sa=r0[1], d_sg=r0[2])
        ops.conv3x3_wgrad(dacc0, x_in, out=r0[0])
        return ops.conv3x3_dgrad(dacc0, acc["wt"][q0], c_in, skip=dx, xin=x_in, coef=coef0)

    @staticmethod
    def _raw_acc(acc, q, cout, cin, sa, sg):
        r = acc["raw"].get(q)
        if r is None:   # [dw_raw, d_sa, d_sg]: the kernels accumulate into them across the frame chunks
            r = acc["raw"][q] = [torch.zeros(cout, 9, cin, dtype=torch.float32, device=sa.device), torch.zeros_like(sa), torch.zeros_like(sg)]
        return r

    def _cnn_backward_chunk(self, sv, dd, acc):
        """dd: fp32 [f, 256] gradient w.r.t. the dense layer's pre-activation output for this chunk's frames.  stack0_from_x0: returns dx0, the
        gradient w.r.t. the temporal conv's output (stack 0's firstconv dgrad, its c0 + c1 x term applied); None otherwise."""
        eng = self.engine
        cfg, w = eng.cfg, eng.w
        pd = "net.img_process.cnn.dense."
        x_last, s_last = sv["x_last"], sv["s_last"]
        f = x_last.shape[0]
        k = x_last[0].numel()
        # dense: d = xn Wd^T.   dxn = dd Wd ;  dWd^T += xn^T dd  (GEMM rows = the K activations, reduction over frames)
        dd16 = ops.gate_cast(dd, 256, dtype=self.dtype)
        _, dxn = ops.linear(dd16, acc["dense_wt"], k, out_f32=False, out_bf16=True, tiling=self.dense_tiling)
        xn = ops.frame_affine(x_last, w[pd + "g"], w[pd + "b"], s_last, per_element=True)
        ops.linear_wgrad(xn.view(f, k), dd16, k, out=acc["dense_dwT"])      # dWd^T [K, 256] += xn^T dd
        del xn
        dx = ops.frame_affine_backward(x_last, dxn.view_as(x_last), w[pd + "g"], s_last, acc["dense_dg"], acc["dense_db"], per_element=True)
        del dxn
        for s in reversed(range(len(cfg["chans"]))):
            p = f"net.img_process.cnn.stacks.{s}."
            rec = sv["stacks"][s]
            for b in (1, 0):
                dx = self._block_backward(p, b, rec["blocks"][b], acc, dx)
            dgn, dbn = acc["n"][s]
            nfold = None
            conv_first = s == 0 and not self.stack0_from_x0       # the fused uint8 first conv (else: a normed conv like the other stacks')
            if conv_first and self.fold_n_backward0:
                # stack 0 (round 6): the reduction pass only; vpt_conv_first_bwd_kernel forms d(pooled) per element itself -- the pooled value it needs is the
                # window maximum its arg-max search finds anyway
                ab = ops.frame_affine_backward_reduce(rec["pooled"], dx, w[p + "n.g"], rec["s_pool"], dgn, dbn)
                c = cfg["chans"][0]
                acc["first"] = ops.conv_first_backward(sv["img"], w[p + "firstconv"], dx, c, out=acc.get("first"), nfold=(w[p + "n.g"], rec["s_pool"], ab))
                continue
            if "mask" in rec and self.fold_n_backward:
                # GroupNorm `n` backward: the reduction pass only; the consumer below forms d(pooled) from (G, pooled) per element itself
                nfold = (w[p + "n.g"], rec["s_pool"], ops.frame_affine_backward_reduce(rec["pooled"], dx, w[p + "n.g"], rec["s_pool"], dgn, dbn))
                dpooled = dx
            else:
                dpooled = ops.frame_affine_backward(rec["pooled"], dx, w[p + "n.g"], rec["s_pool"], dgn, dbn)
            if conv_first:
                c = cfg["chans"][0]
                acc["first"] = ops.conv_first_backward(sv["img"], w[p + "firstconv"], dpooled, c, out=acc.get("first"))
            elif "mask" in rec:
                q = p + "firstconv"
                _, sa, sg = w[q]
                x_prev = rec["x_prev"]
                c_prev = x_prev.shape[1] * 32
                r = self._raw_acc(acc, q, rec["pooled"].shape[1] * 32, c_prev, sa, sg)
                dacc, coef, _, _ = ops.conv_backward_prepare_pooled(dpooled, rec["pooled"], rec["mask"], rec["s_prev"], sa, sg, c_prev, d_sa=r[1], d_sg=r[2], nfold=nfold)
                ops.conv3x3_wgrad(dacc, x_prev, out=r[0])
                dx = ops.conv3x3_dgrad(dacc, acc["wt"][q], c_prev, xin=x_prev, coef=coef)
                del dacc
            else:
                dx = self._conv_layer_backward(p + "firstconv", acc, None, rec["pre"], None, rec["x_prev"], rec["s_prev"], None,
                                               pool=(dpooled, rec["argmax"]))
            del dpooled
        return dx if self.stack0_from_x0 else None

    def _cnn_backward_finish(self, acc, P, g):
        cfg = self.engine.cfg
        c2 = cfg["chans"][-1]
        for q, (dw_raw, d_sa, d_sg) in acc["raw"].items():
            dW, dgain, dbias = conv_param_grads(dw_raw, d_sa, d_sg, P[q + ".layer.weight"].float(), P[q + ".norm.weight"].float(),
                                                P[q + ".norm.bias"].float())
            g[q + ".layer.weight"], g[q + ".norm.weight"], g[q + ".norm.bias"] = dW, dgain, dbias
        if not self.stack0_from_x0:
            g["net.img_process.cnn.stacks.0.firstconv.layer.weight"] = ops.conv_first_grad_to_reference(acc["first"][0])
            g["net.img_process.cnn.stacks.0.firstconv.layer.bias"] = acc["first"][1]
        for s in range(len(cfg["chans"])):
            g[f"net.img_process.cnn.stacks.{s}.n.weight"], g[f"net.img_process.cnn.stacks.{s}.n.bias"] = acc["n"][s]
        pd = "net.img_process.cnn.dense."
        unblock = lambda v: v.view(c2 // 32, 16, 16, 32).permute(0, 3, 1, 2).reshape(-1).contiguous()
        g[pd + "norm.weight"], g[pd + "norm.bias"] = unblock(acc["dense_dg"]), unblock(acc["dense_db"])
        dwd = acc["dense_dwT"].t()                                                               # [256, K] in activation order
        g[pd + "layer.weight"] = dwd.reshape(256, c2 // 32, 16, 16, 32).permute(0, 1, 4, 2, 3).reshape(256, -1).contiguous()


# ---------------------------------------------------------------------------------------------------------
# host mapping of the folded-conv gradients to the reference's parameters (small tensors: [Cout, Cin, 3, 3])
# ---------------------------------------------------------------------------------------------------------
def _tap_sum(tab: torch.Tensor, cout: int) -> torch.Tensor:
    """[9 edge classes, >= cout] -> [cout, 3, 3]: for every tap, the sum over the edge classes in which it is inside the image."""
    # an index-sum, not a matrix product: `tab.t() @ M` dispatched to a Tensile / hipBLASLt GEMM (84 of them per BC step in the round-3
    # PMC survey) -- there is no vendor BLAS on the measured path
    m = packing.edge_tap_matrix(tab.device, tab.dtype)                      # [9 classes, 9 taps] of 0 / 1
    return (tab[:, :cout].t().unsqueeze(2) * m.unsqueeze(0)).sum(dim=1).view(cout, 3, 3)


def conv_param_grads(dw_raw: torch.Tensor, d_sa: torch.Tensor, d_sg: torch.Tensor, weight: torch.Tensor,
                     gain: torch.Tensor, bias: torch.Tensor):
    """Gradients of a GN -> conv layer's parameters from the kernels' outputs.
    Forward (vpt_conv3x3.hip): W' = W * gain[c];  v = rstd conv(W', x) + SA[e,o] - rstd mu SG[e,o],
    SG[e,o] = sum_{taps valid in e, c} W'[o,c,tap],  SA[e,o] = sum_{valid taps, c} W[o,c,tap] bias[c].
      dW'  = dw_raw (wgrad kernel, [Cout,9,Cin])  +  tap_sum(d_sg)  (broadcast over c)
      dW   = dW' * gain  +  bias[c] * tap_sum(d_sa)
      dgain[c] = sum_{o,tap} dW' W ;   dbias[c] = sum_{o,tap} W tap_sum(d_sa)
    Returns (dW [Cout,Cin,3,3], dgain [Cin], dbias [Cin])."""
    cout, cin = weight.shape[:2]
    dwp = dw_raw.view(cout, 3, 3, cin).permute(0, 3, 1, 2)                  # [Cout, Cin, 3, 3]
    dwp = dwp + _tap_sum(d_sg, cout).unsqueeze(1)
    ta = _tap_sum(d_sa, cout).unsqueeze(1)                                  # [Cout, 1, 3, 3]
    dW = dwp * gain.view(1, -1, 1, 1) + bias.view(1, -1, 1, 1) * ta
    dgain = (dwp * weight).sum(dim=(0, 2, 3))
    dbias = (weight * ta).sum(dim=(0, 2, 3))
    return dW.contiguous(), dgain, dbias
