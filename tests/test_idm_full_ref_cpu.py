"""tests/idm_full_ref.py on the CPU: the composed fp64 reference is the oracle's IDM, its trainable set is the whole network in state-dict order, and
the rounding reference's own distance to fp64 -- the yardstick of tests/test_gpu_idm_full_training.py -- is measured on that test's batch.

Measured here (tiny IDM, temperature 2, B = 2, T = 6, parity.structured_frames seed 23), rounding reference against fp64 over the 91 reached tensors:
    bf16: loss 18.8665 (fp64 18.8704), mean rel-L2 0.345, mean cosine 0.929, worst cosine 0.689; worst tensor net.conv3d_layer.layer.bias, rel-L2 0.890
    fp16: loss 18.8711,                mean rel-L2 0.099, mean cosine 0.993, worst cosine 0.963; worst tensor net.conv3d_layer.layer.bias, rel-L2 0.285
Both meet parity.GRAD_BOUNDS[mode] (bf16: l2_mean 0.40, cos_mean 0.90, cos_min 0.40; fp16: 0.15, 0.985, 0.90), so the GPU test asserts that table too;
test_rounding_reference_meets_the_table pins that decision."""
import pytest
import torch

import vpt_amd  # noqa: F401
from oracle import vpt_oracle as O
from tests import idm_full_ref as F
from tests import labeler_ref
from tests import parity as P


def test_composed_forward_is_the_oracles_idm():
    _, cfg, sd = labeler_ref.tiny_idm()
    img = F.batch()[0]
    lp_b, lp_c = F.forward({k: v.double() for k, v in sd.items()}, cfg, img)
    ref = O.idm_forward(sd, cfg, img)               # float32
    assert float((lp_b.view(F.B, F.T, 20, 2) - ref["buttons"]).abs().max()) < 1e-4
    assert float((lp_c.view(F.B, F.T, 2, 11) - ref["camera"]).abs().max()) < 1e-4


def test_trainable_names_are_the_whole_network_in_state_dict_order():
    _, cfg, sd = labeler_ref.tiny_idm()
    names = F.trainable_names(sd, cfg)
    new = [n for n in names if n.startswith(F.CNN_PREFIXES)]
    assert new == [k for k in sd if k.startswith(F.CNN_PREFIXES)] and names[:len(new)] == new
    assert new[:2] == ["net.conv3d_layer.layer.weight", "net.conv3d_layer.layer.bias"]
    # stack 0's firstconv is normed here: norm.* and no bias
    assert "net.img_process.cnn.stacks.0.firstconv.norm.weight" in new and "net.img_process.cnn.stacks.0.firstconv.layer.bias" not in new
    assert len(new) == 2 + 3 * (3 + 2 + 4 * 3) + 3
    assert not any(n.startswith("net.lastlayer.") for n in names)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_rounding_reference_meets_the_table(mode):
    loss64, g64 = F.reference(None)
    loss_em, g_em = F.reference(mode)
    assert set(g64) == set(g_em)
    unreached = [n for n in g64 if float(g64[n].norm()) == 0.0]
    assert all(".r_layer." in n for n in unreached) and len(unreached) == 4, unreached
    st = F.grad_stats(g_em, g64)
    print(f"IDM full reference [{mode}]: loss fp64 {loss64:.5f}, rounding reference {loss_em:.5f}; over {len(st['l2'])} tensors mean rel-L2 {st['l2_mean']:.4f}, "
          f"mean cosine {st['cos_mean']:.5f}, worst cosine {st['cos_min']:.4f}, worst tensor {st['worst']}; GRAD_BOUNDS {P.GRAD_BOUNDS[mode]}")
    assert abs(loss_em - loss64) < 2e-2
    assert F.meets_table(st, P.GRAD_BOUNDS[mode]), st
    for n in g64:                                    # finite, and the temporal conv's taps all get a gradient
        assert bool(torch.isfinite(g_em[n]).all()), n
    assert bool((g64["net.conv3d_layer.layer.weight"].abs().amax((0, 1, 3, 4)) > 0).all())
