"""Freezing at the autograd boundary: after the reference's own idiom, `p.requires_grad = False`, the reference's loop --
get_output_for_observation -> get_logprob_of_action -> backward() (behavioural_cloning.py:99-119) -- runs the backward that stops where training
stops: the heads' gradients are those of the boundary with everything behind the (frozen) CNN trainable, bit for bit -- a trained CNN runs another
CNN forward, see the test --, everything frozen gets None, the engine is chosen by the set of
parameters that require grad (all of them: the engine the boundary always used), and a policy keeps at most four engines.  1x policy, two
frames, both operand formats.  Needs an MI355X."""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from vpt_amd.lib import policy as policy_module  # noqa: E402
from vpt_amd.lib.policy import MinecraftAgentPolicy  # noqa: E402
from vpt_amd.lib.types import minecraft_action_space  # noqa: E402
from oracle import vpt_oracle as O  # noqa: E402

DEV = "cuda"
N = 2


def _policy(precision):
    pk = O.policy_kwargs_for("1x")
    cfg = O.config_from_policy_kwargs(pk, dict(temperature=2.0))
    pol = MinecraftAgentPolicy(minecraft_action_space(), pk, dict(temperature=2.0), precision=precision)
    pol.load_state_dict(O.synthetic_state_dict(cfg, seed=0), strict=False)
    return pol.to(DEV)


def _loop(pol, img, tgt):
    """One pass of the reference's loop -> ({name: grad or None}, launch counts of the backward)."""
    pol.zero_grad(set_to_none=True)
    pd, _, _ = pol.get_output_for_observation({"img": img}, pol.initial_state(N), torch.zeros(N, dtype=torch.bool, device=DEV))
    loss = -pol.get_logprob_of_action(pd, tgt).mean()
    ops.TIMER.reset()
    ops.TIMER.enabled = True
    try:
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.TIMER.enabled = False
    counts = collections.Counter(rec[0] for rec in ops.TIMER.records)
    ops.TIMER.reset()
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in pol.named_parameters()}, counts, float(loss.detach())


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_heads_only_after_the_references_freezing_idiom(precision):
    pol = _policy(precision)
    g = torch.Generator().manual_seed(12)
    img = torch.randint(0, 256, (N, 128, 128, 3), generator=g, dtype=torch.uint8).to(DEV)
    tgt = {"buttons": torch.randint(0, 8641, (N, 1), generator=g).to(DEV), "camera": torch.randint(0, 121, (N, 1), generator=g).to(DEV)}
    full, c_full, loss_full = _loop(pol, img, tgt)
    assert list(pol._grad_engines) == [True]                 # every parameter requires grad: the engine keyed True, as ever
    eng_all = pol._grad_engines[True]
    assert eng_all._subset is None and eng_all.train_cnn
    heads = [n for n in full if n.startswith("pi_head.")]
    assert len(heads) == 4 and all(full[n] is not None for n in heads) and full["net.final_ln.weight"] is not None
    # The bit-for-bit reference is the all-trainable boundary BEHIND THE CNN (the engine keyed False): a frozen CNN runs the inference CNN path,
    # a trained one the saving path -- two sets of kernels whose outputs agree to the parity bounds only (BCTrainer's docstring) -- and freezing
    # everything but the heads freezes the CNN.  Against the engine keyed True the heads' gradients are compared and printed, not asserted.
    for n, p in pol.named_parameters():
        if n.startswith("net.img_process.cnn."):
            p.requires_grad = False
    ref, c_ref, loss_ref = _loop(pol, img, tgt)
    eng_trunk = pol._grad_engines[False]
    assert eng_trunk._subset is None and not eng_trunk.train_cnn and len(pol._grad_engines) == 2
    assert all(ref[n] is None for n in ref if n.startswith("net.img_process.cnn.")) and ref["net.final_ln.weight"] is not None
    for n, p in pol.named_parameters():                      # the reference's idiom
        if not n.startswith("pi_head."):
            p.requires_grad = False
    part, c_part, loss_part = _loop(pol, img, tgt)
    assert loss_part == loss_ref
    assert all(torch.equal(part[n], ref[n]) for n in heads)
    print(f"[{precision}] heads-only vs the engine keyed True (another CNN forward): max |diff| / max |g| = "
          f"{max(float((part[n] - full[n]).abs().max() / full[n].abs().max()) for n in heads):.3e}")
    assert [n for n in part if n not in heads and part[n] is not None] == []
    # the truncated backward: one linear wgrad (the fused heads'), no dgrad GEMM, no LayerNorm or attention backward
    assert c_part["vpt_linear_wgrad"] == 1 and c_full["vpt_linear_wgrad"] > 10, (c_part, c_full)
    assert c_part["vpt_linear_forward"] == 0 and c_part["vpt_layernorm_backward"] == 0
    assert not any(k.startswith("vpt_masked_attention_backward") for k in c_part)
    assert len(pol._grad_engines) == 3 and pol._grad_engines[True] is eng_all and pol._grad_engines[False] is eng_trunk
    for p in pol.parameters():
        p.requires_grad = True
    for n, p in pol.named_parameters():                      # (the value normaliser's statistics never required grad)
        if n.startswith("value_head.normalizer."):
            p.requires_grad = False
    again, c_again, _ = _loop(pol, img, tgt)
    assert pol._grad_engines[True] is eng_all and len(pol._grad_engines) == 3 and c_again == c_full
    assert all(torch.equal(again[n], full[n]) for n in heads)
    # six more distinct sets: the cache never holds more than four engines, the oldest go first
    assert policy_module.MAX_GRAD_ENGINES == 4
    n_layers = pol._cfg["n_layers"]
    for k in range(6):
        for n, p in pol.named_parameters():
            p.requires_grad = n.startswith("pi_head.") or n.startswith(f"net.recurrent_layer.blocks.{k % n_layers}.") or (k >= n_layers and n.startswith("net.final_ln."))
        got, _, _ = _loop(pol, img, tgt)
        assert len(pol._grad_engines) <= 4
        assert {n for n, t_ in got.items() if t_ is not None} == {n for n, p in pol.named_parameters() if p.requires_grad}
        assert all(torch.equal(got[n], ref[n]) for n in heads)
    assert len(pol._grad_engines) == 4 and True not in pol._grad_engines and False not in pol._grad_engines
