"""fp64 autograd reference of the WHOLE inverse dynamics model, from the pixels -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The oracle's own building blocks composed under autograd: oracle.vpt_oracle.conv3d_temporal (bytes / 255 -> Conv3d(5,1,1) + ReLU) ->
oracle.vpt_oracle.impala_cnn (stack 0's firstconv normed) -> tests/idm_trainer_ref.forward (everything behind the dense layer).  impala_cnn returns
relu(dense); idm_trainer_ref.forward applies the ReLU to its input `d` itself, and relu(relu(x)) = relu(x) with the same gate, so the composition is
oracle.vpt_oracle.idm_forward's function and gradient.

`rnd` ("bf16" / "fp16") is the matched oracle of IDMTrainer(train_cnn=True): it rounds where the HIP path rounds -- the temporal conv's weight operand
and stored output, then oracle.vpt_oracle_bf16.conv_fold (called, not restated) for every 3x3 conv with the pooled tensor, the GroupNorm `n` output and
the dense layer's normalised input stored in 16 bits and the dense weight as an operand, as oracle.vpt_oracle_bf16.policy_forward does for the policy;
behind the dense layer idm_trainer_ref.forward's own `rnd`.  Casts are straight-through under autograd.  Everything stays in float64 between the
rounding points (conv_fold builds its tables in torch's default dtype, which is float64 inside these functions)."""
import contextlib
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from oracle import vpt_oracle as O
from oracle import vpt_oracle_bf16 as OB
from tests import idm_trainer_ref as IR

CNN_PREFIXES = ("net.conv3d_layer.", "net.img_process.cnn.")


@contextlib.contextmanager
def _float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def trainable_names(sd, cfg):
    """The tensors IDMTrainer(train_cnn=True) trains, in state-dict order: the 49 of the temporal conv and the CNN, then idm_trainer_ref's."""
    behind = set(IR.trainable_names(sd, cfg))
    return [k for k, v in sd.items() if (k.startswith(CNN_PREFIXES) or k in behind) and v.numel() > 0]


def dense_output(sd, cfg, img_u8, rnd=None):
    """img_u8 uint8 [B, T, 128, 128, 3] -> relu(dense) float64 [B*T, 256] (module docstring)."""
    b, t = img_u8.shape[:2]
    if rnd is None:
        x0 = O.conv3d_temporal(sd, img_u8.double() / 255.0)
        return O.impala_cnn(sd, "net.img_process.cnn.", x0.reshape(b * t, *x0.shape[2:]))
    r = IR.rounder(rnd)
    rr = SimpleNamespace(w=r, a=r, t=r, winograd=False)
    # vpt_conv3d.hip: operands = raw bytes (exact in 16 bits) and op16(W); 1 / 255 and the bias in fp32; the output stored in 16 bits
    xb = img_u8.double().permute(0, 4, 1, 2, 3)
    y = F.conv3d(xb, r(sd["net.conv3d_layer.layer.weight"]), None, padding=(2, 0, 0)) / 255.0 + sd["net.conv3d_layer.layer.bias"].view(1, -1, 1, 1, 1)
    cur = r(torch.relu(y)).permute(0, 2, 1, 3, 4).reshape(b * t, -1, *img_u8.shape[2:4])            # [M, 128, H, W]
    for s in range(3):
        p = f"net.img_process.cnn.stacks.{s}."
        y = OB.conv_fold(sd, p + "firstconv.", cur, rnd=rr)
        y = r(F.max_pool2d(y, 3, 2, 1))
        cur = r(O.group_norm_1(y, sd[p + "n.weight"], sd[p + "n.bias"]))
        for blk in range(2):
            q = f"{p}blocks.{blk}."
            h = OB.conv_fold(sd, q + "conv0.", cur, rnd=rr)
            cur = OB.conv_fold(sd, q + "conv1.", h, res=cur, rnd=rr)
    p = "net.img_process.cnn.dense."
    xn = r(O.layer_norm(cur.reshape(b * t, -1), sd[p + "norm.weight"], sd[p + "norm.bias"]))
    return torch.relu(xn @ r(sd[p + "layer.weight"]).t())


def forward(sd, cfg, img_u8, rnd=None):
    """-> (lp_buttons [M, 20, 2], lp_camera [M, 2, n_bins]) float64."""
    b, t = img_u8.shape[:2]
    with _float64_default():
        return IR.forward(sd, cfg, dense_output(sd, cfg, img_u8, rnd), b, t, rnd=rnd)


def loss_and_grads(sd, cfg, img_u8, buttons, camera, weight=None, rnd=None):
    """-> (loss float, {name: float64 gradient} for trainable_names; a tensor the loss does not reach gets zeros)."""
    b, t = img_u8.shape[:2]
    names = trainable_names(sd, cfg)
    leaves = {k: (v.detach().double().clone().requires_grad_(True) if k in names else v.detach().double()) for k, v in sd.items()
              if v.dtype.is_floating_point}
    with torch.enable_grad():
        lp_b, lp_c = forward(leaves, cfg, img_u8, rnd=rnd)
        loss = IR.loss_from_logprobs(lp_b, lp_c, buttons.reshape(b * t, -1), camera.reshape(b * t, -1), weight)
        grads = torch.autograd.grad(loss, [leaves[n] for n in names], allow_unused=True)
    return float(loss.detach()), {n: (g if g is not None else torch.zeros_like(leaves[n])) for n, g in zip(names, grads)}


def grad_stats(grads, ref):
    """Per tensor with a non-zero reference: rel-L2 and cosine to `ref`, and the norm ratio -> dict(l2, cos, ratio: name -> float; l2_mean, cos_mean,
    cos_min, worst = the tensor with the largest rel-L2)."""
    l2, cos, ratio = {}, {}, {}
    for n, rf in ref.items():
        if float(rf.norm()) == 0.0:
            continue
        g = grads[n].detach().cpu().double().reshape(rf.shape)
        l2[n] = float((g - rf).norm() / rf.norm())
        cos[n] = float((g * rf).sum() / (g.norm() * rf.norm()).clamp(min=1e-300))
        ratio[n] = float(g.norm() / rf.norm())
    worst = max(l2, key=l2.get)
    return dict(l2=l2, cos=cos, ratio=ratio, l2_mean=sum(l2.values()) / len(l2), cos_mean=sum(cos.values()) / len(cos), cos_min=min(cos.values()),
                worst=(worst, l2[worst]))


def meets_table(stats, gb):
    """parity.GRAD_BOUNDS[mode] as tests/test_gpu_idm_training.py asserts it: the means and the worst tensor's cosine."""
    return stats["l2_mean"] < gb["l2_mean"] and stats["cos_mean"] > gb["cos_mean"] and stats["cos_min"] > gb["cos_min_small"]


# ---- the one batch both test files use: tiny IDM (tests/labeler_ref.tiny_idm: temperature 2), B = 2 windows of T = 6 structured frames ----
B, T = 2, 6


def batch():
    """-> (img uint8 [B, T, 128, 128, 3], buttons int64 [B, T, 20], camera int64 [B, T, 2]), seed 23."""
    from tests import parity as P
    g = torch.Generator().manual_seed(23)
    img = P.structured_frames(B, T, g)
    return img, torch.randint(0, 2, (B, T, 20), generator=g), torch.randint(0, 11, (B, T, 2), generator=g)


_REFERENCES = {}


def reference(rnd=None):
    """(loss, grads) of loss_and_grads on batch() for the tiny IDM, computed once per process and rounding mode."""
    if rnd not in _REFERENCES:
        from tests import labeler_ref
        _, cfg, sd = labeler_ref.tiny_idm()
        img, buttons, camera = batch()
        _REFERENCES[rnd] = loss_and_grads(sd, cfg, img, buttons, camera, rnd=rnd)
    return _REFERENCES[rnd]
