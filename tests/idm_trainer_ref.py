"""fp64 autograd reference of the part of the IDM that IDMTrainer trains -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A restatement of oracle/vpt_oracle.py:idm_forward (lines 586-608: InverseActionNet.forward behind the CNN, lib/policy.py:374-392) that runs under
autograd in float64 and takes the dense layer's pre-activation output `d` [M, 256] as a CONSTANT: ImgObsProcess.linear (LayerNorm on relu(d),
linear, ReLU) -> optional pre_lstm_ln -> transformer blocks with mask "none" (softmax(Q K^T / d_head) V, no memory, no relative-position bias;
x2 = x1 + proj with x1 the LayerNorm's OUTPUT, lib/xf.py) -> ReLU -> final_ln -> 20 x 2 button and 2 x 11 camera log-softmax heads.

`rnd` (None = exact, or "bf16" / "fp16") rounds at the points where the HIP path rounds, as oracle/vpt_oracle_bf16.Rounding does for the policy:
every GEMM's weight operand and A operand (the LayerNorm outputs that feed a GEMM, the attention output, the MLP hidden activation, the latent in
front of the heads).  LayerNorm statistics, softmax, the residual stream, Q / K / V and the logits stay unrounded.  torch's casts are
straight-through under autograd, so autograd through this file with `rnd` set is the matched oracle of the trainer's gradients."""
import torch

from oracle import vpt_oracle as O

_DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def rounder(rnd):
    if rnd is None:
        return lambda t: t
    dt = _DT[rnd]
    return lambda t: t.to(dt).to(torch.float64)


def trainable_names(sd, cfg):
    """The tensors IDMTrainer trains, in state-dict order (b_nd is [10, 0] for the IDM: nothing to train)."""
    keep = ("net.img_process.linear.", "net.pre_lstm_ln.", "net.recurrent_layer.blocks.", "net.final_ln.", "pi_head.buttons.", "pi_head.camera.")
    return [k for k, v in sd.items() if k.startswith(keep) and v.numel() > 0]


def forward(sd, cfg, d, bsz, t, rnd=None):
    """sd: name -> float64 tensor (leaves or constants); d float64 [B*t, 256].  -> (lp_buttons [M, 20, 2], lp_camera [M, 2, n_bins])."""
    r = rounder(rnd)
    hid, heads = cfg["hidsize"], cfg["heads"]
    dh = hid // heads
    p = "net.img_process.linear."
    x = torch.relu(r(O.layer_norm(torch.relu(d), sd[p + "norm.weight"], sd[p + "norm.bias"])) @ r(sd[p + "layer.weight"]).t())
    if cfg.get("use_pre_lstm_ln"):
        x = O.layer_norm(x, sd["net.pre_lstm_ln.weight"], sd["net.pre_lstm_ln.bias"])
    x = x.reshape(bsz, t, hid)
    for l in range(cfg["n_layers"]):
        pfx = f"net.recurrent_layer.blocks.{l}."
        o = pfx + "r.orc_block."
        x1 = O.layer_norm(x, sd[pfx + "pre_r_ln.weight"], sd[pfx + "pre_r_ln.bias"])
        x1b = r(x1)
        q = x1b @ r(sd[o + "q_layer.weight"]).t() + sd[o + "q_layer.bias"]
        k = x1b @ r(sd[o + "k_layer.weight"]).t()
        v = x1b @ r(sd[o + "v_layer.weight"]).t()
        sp = lambda z: z.reshape(bsz, t, heads, dh).permute(0, 2, 1, 3)
        w_ = torch.softmax(torch.matmul(sp(q), sp(k).transpose(-1, -2)) * (1.0 / dh), dim=-1)
        a = r(torch.matmul(w_, sp(v)).permute(0, 2, 1, 3).reshape(bsz, t, hid))
        x2 = x1 + a @ r(sd[o + "proj_layer.weight"]).t() + sd[o + "proj_layer.bias"]
        hb = r(O.layer_norm(x2, sd[pfx + "mlp0.norm.weight"], sd[pfx + "mlp0.norm.bias"]))
        h = r(torch.relu(hb @ r(sd[pfx + "mlp0.layer.weight"]).t()))
        x = x2 + h @ r(sd[pfx + "mlp1.layer.weight"]).t() + sd[pfx + "mlp1.layer.bias"]
    lat = r(O.layer_norm(torch.relu(x), sd["net.final_ln.weight"], sd["net.final_ln.bias"])).reshape(bsz * t, hid)
    temp = cfg["temperature"]
    zb = (lat @ r(sd["pi_head.buttons.linear_layer.weight"]).t() + sd["pi_head.buttons.linear_layer.bias"]).reshape(bsz * t, -1, 2)
    zc = (lat @ r(sd["pi_head.camera.linear_layer.weight"]).t() + sd["pi_head.camera.linear_layer.bias"]).reshape(bsz * t, 2, -1)
    return torch.log_softmax(zb / temp, -1), torch.log_softmax(zc / temp, -1)


def loss_from_logprobs(lp_b, lp_c, buttons, camera, weight=None):
    """sum_r w_r (nll_b + nll_c)_r / sum_r w_r: the negative of pi_head.logprob (the groups' gathers summed, lib/action_head.py:176-184,252-253),
    averaged over the frames.  buttons int64 [M, 20], camera int64 [M, 2]."""
    nll = -(lp_b.gather(-1, buttons.unsqueeze(-1)).squeeze(-1).sum(-1) + lp_c.gather(-1, camera.unsqueeze(-1)).squeeze(-1).sum(-1))
    if weight is None:
        return nll.mean()
    w = weight.to(nll.dtype)
    return (w * nll).sum() / w.sum()


def loss_and_grads(sd, cfg, d, bsz, t, buttons, camera, weight=None, rnd=None):
    """-> (loss float, {name: float64 gradient} for trainable_names; a tensor the loss does not reach gets zeros)."""
    names = trainable_names(sd, cfg)
    leaves = {k: (v.detach().double().clone().requires_grad_(True) if k in names else v.detach().double()) for k, v in sd.items()
              if v.dtype.is_floating_point}
    with torch.enable_grad():
        lp_b, lp_c = forward(leaves, cfg, d.detach().double(), bsz, t, rnd=rnd)
        loss = loss_from_logprobs(lp_b, lp_c, buttons.reshape(bsz * t, -1), camera.reshape(bsz * t, -1), weight)
        grads = torch.autograd.grad(loss, [leaves[n] for n in names], allow_unused=True)
    return float(loss.detach()), {n: (g if g is not None else torch.zeros_like(leaves[n])) for n, g in zip(names, grads)}
