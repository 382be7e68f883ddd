"""Low-rank adapters, the parts that need no GPU: which modules a target selects and what it refuses, the parameter names and the
seeded initialisation, the stacked / block-diagonal index algebra of the fused projection against a dense torch restatement, the state dict's keys
and round trip, what a trainer's constructor accepts (on a fake built with object.__new__, as tests/test_trainer_base_cpu.py does), and the numpy
restatement of the merge against fp64 under (r + 2) 2^-24 (|W| + s sum |B||A|)."""
import math

import numpy as np
import pytest
import torch

import vpt_amd  # noqa: F401
from vpt_amd.adapters import LEAVES, LowRankAdapters, adaptable_modules, init_tensors, resolve_targets
from vpt_amd.trainer_base import stack_operands, unstack_gradients

from tests import lowrank_ref as R

HID, RATIO, LAYERS = 16, 4, 3
BLK = "net.recurrent_layer.blocks."


class FakePolicy:
    """The parameter names of the policy with tiny shapes (a LowRankAdapters reads named_parameters() / state_dict() only)."""

    def __init__(self, hid=HID, layers=LAYERS):
        p = {"net.img_process.cnn.dense.layer.weight": (8, 32), "net.img_process.linear.layer.weight": (hid, 8)}
        for l in range(layers):
            b = f"{BLK}{l}."
            p[b + "pre_r_ln.weight"] = (hid,)
            for c in "qkvr":
                p[f"{b}r.orc_block.{c}_layer.weight"] = (hid, hid)
            p[b + "r.orc_block.q_layer.bias"] = (hid,)
            p[b + "r.orc_block.proj_layer.weight"] = (hid, hid)
            p[b + "r.orc_block.proj_layer.bias"] = (hid,)
            p[b + "mlp0.norm.weight"] = (hid,)
            p[b + "mlp0.layer.weight"] = (hid * RATIO, hid)
            p[b + "mlp1.layer.weight"] = (hid, hid * RATIO)
            p[b + "mlp1.layer.bias"] = (hid,)
        p.update({"net.lastlayer.layer.weight": (hid, hid), "net.final_ln.weight": (hid,), "pi_head.buttons.linear_layer.weight": (5, hid),
                  "value_head.linear.weight": (1, hid)})
        g = torch.Generator().manual_seed(3)
        self.p = {n: torch.nn.Parameter(torch.randn(*s, generator=g)) for n, s in p.items()}

    def named_parameters(self):
        return list(self.p.items())

    def state_dict(self):
        return {n: t.detach() for n, t in self.p.items()}


NAMES = [n for n, _ in FakePolicy().named_parameters()]


def test_targets_select_adaptable_linears_by_prefix_and_by_name():
    every = adaptable_modules(NAMES)
    assert len(every) == LAYERS * len(LEAVES) and every[0] == BLK + "0.r.orc_block.q_layer" and every[6] == BLK + "0.mlp1.layer"
    assert resolve_targets(NAMES, ("net.recurrent_layer.blocks",)) == sorted(every)
    assert resolve_targets(NAMES, "net") == sorted(every)        # a prefix selects every adaptable linear under it
    one = resolve_targets(NAMES, (BLK + "1",))
    assert one == sorted(m for m in every if m.startswith(BLK + "1.")) and len(one) == 7
    assert resolve_targets(NAMES, (BLK + "2.mlp0", BLK + "0.r.orc_block.q_layer", BLK + "2.mlp0.layer")) == [BLK + "0.r.orc_block.q_layer", BLK + "2.mlp0.layer"]
    assert resolve_targets(NAMES, (BLK + "1.r",)) == [f"{BLK}1.r.orc_block.{c}_layer" for c in ("k", "proj", "q", "r", "v")]
    # the IDM's r_layer sits outside its fused projection: not adaptable there
    assert BLK + "0.r.orc_block.r_layer" not in adaptable_modules(NAMES, fused="qkv") and len(adaptable_modules(NAMES, fused="qkv")) == LAYERS * 6


@pytest.mark.parametrize("target", ["net.lastlayer", "net.img_process.linear", "pi_head", "value_head.linear", "net.img_process.cnn", "net.final_ln",
                                    BLK + "0.pre_r_ln", BLK + "0.mlp0.norm", BLK + "1.mlp1.layer.bias"])
def test_what_is_not_adaptable_raises(target):
    with pytest.raises(ValueError, match="is not adaptable"):
        resolve_targets(NAMES, (BLK + "0", target))


def test_other_target_refusals():
    with pytest.raises(ValueError, match="matches no module"):
        resolve_targets(NAMES, ("net.recurrent_layer.block",))
    with pytest.raises(ValueError, match="matches no module"):
        resolve_targets(NAMES, (BLK + "1", BLK + "7"))
    with pytest.raises(ValueError, match="is not adaptable"):
        resolve_targets(NAMES, (BLK + "0.r.orc_block.r_layer",), fused="qkv")
    with pytest.raises(ValueError, match="non-empty"):
        resolve_targets(NAMES, ("",))
    with pytest.raises(ValueError, match="selection is empty"):
        resolve_targets(NAMES, ())
    for bad in (0, 65, 2.5, -1):
        with pytest.raises(ValueError, match="rank must be an integer in 1..64"):
            LowRankAdapters(FakePolicy(), rank=bad)
    with pytest.raises(ValueError, match="alpha must be finite"):
        LowRankAdapters(FakePolicy(), alpha=float("nan"))


def test_names_shapes_and_seeded_init():
    pol = FakePolicy()
    ad = LowRankAdapters(pol, targets=(BLK + "1",), rank=4, alpha=8.0, seed=5)
    assert ad.scale == 2.0 and len(ad.params) == 14
    assert list(ad.params) == [m + sfx for m in sorted(ad.modules) for sfx in (".lora_A", ".lora_B")]
    assert ad.adapted_weights == [m + ".weight" for m in ad.modules]
    for m in ad.modules:
        n, k = pol.p[m + ".weight"].shape
        a, b = ad.pair(m)
        assert a.shape == (4, k) and b.shape == (n, 4) and a.dtype == b.dtype == torch.float32
        assert float(a.abs().max()) <= 1.0 / math.sqrt(k) and float(a.abs().max()) > 0.5 / math.sqrt(k) and not bool(b.any())
    # one CPU generator, drawn in name order: the same triple gives the same bits, another seed does not, and the draw does not depend on the device
    again = LowRankAdapters(FakePolicy(), targets=(BLK + "1",), rank=4, alpha=8.0, seed=5)
    assert all(torch.equal(ad.params[n], again.params[n]) for n in ad.params)
    other = LowRankAdapters(FakePolicy(), targets=(BLK + "1",), rank=4, seed=6)
    assert not torch.equal(ad.params[ad.modules[0] + ".lora_A"], other.params[ad.modules[0] + ".lora_A"])
    gen = torch.Generator().manual_seed(5)
    first = sorted(ad.modules)[0]
    k = pol.p[first + ".weight"].shape[1]
    assert torch.equal(ad.params[first + ".lora_A"], (torch.rand(4, k, generator=gen) * 2.0 - 1.0) * (1.0 / math.sqrt(k)))
    assert set(init_tensors({"b": (3, 8), "a": (2, 8)}, 2, 0)) == {"a.lora_A", "a.lora_B", "b.lora_A", "b.lora_B"}


def test_stacked_block_diagonal_algebra_equals_the_per_layer_sum():
    """sum_i s_i (x A_i^T) B_i^T at layer i's rows == (x a_stack^T) sb^T, and the gradients of the stacked operands hold each adapter's own
    gradient in A's rows / the DIAGONAL block; keeping an off-diagonal block would be another function."""
    g = torch.Generator().manual_seed(0)
    hid, m, ranks, scales = 16, 9, (24, 24, 24), (0.5, 2.0, 0.25)          # 72 -> R = 128: crosses one 64-wide step
    x = torch.randn(m, hid, generator=g, dtype=torch.float64)
    A = [torch.randn(r, hid, generator=g, dtype=torch.float64).float() for r in ranks]
    B = [torch.randn(hid, r, generator=g, dtype=torch.float64).float() for r in ranks]
    entries = [(A[0], B[0], scales[0], 0), (A[2], B[2], scales[2], 2 * hid)]          # q and v adapted, k and r not: 4 * hid rows
    a_stack, sb, spans = stack_operands(entries, 4 * hid, hid)
    assert a_stack.shape == (64, hid) and sb.shape == (4 * hid, 64) and spans == [(0, hid, 0, 24), (2 * hid, hid, 24, 24)]
    assert not bool(a_stack[48:].any()) and not bool(sb[:, 48:].any()) and not bool(sb[hid:2 * hid].any()) and not bool(sb[3 * hid:].any())
    assert not bool(sb[:hid, 24:48].any()) and not bool(sb[2 * hid:3 * hid, :24].any())            # the off-diagonal blocks are zero
    entries = [(A[i], B[i], scales[i], i * hid) for i in range(3)]
    a_stack, sb, spans = stack_operands(entries, 4 * hid, hid)
    assert a_stack.shape == (128, hid) and sb.shape == (4 * hid, 128)
    want = torch.zeros(m, 4 * hid, dtype=torch.float64)
    for i in range(3):
        want[:, i * hid:(i + 1) * hid] = scales[i] * (x @ A[i].double().t()) @ B[i].double().t()
    got = (x @ a_stack.double().t()) @ sb.double().t()
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    # autograd through the dense restatement against the unstacked gradients
    Ap = [a.double().requires_grad_() for a in A]
    Bp = [b.double().requires_grad_() for b in B]
    dy = torch.randn(m, 4 * hid, generator=g, dtype=torch.float64)
    y = torch.cat([scales[i] * (x @ Ap[i].t()) @ Bp[i].t() for i in range(3)] + [torch.zeros(m, hid, dtype=torch.float64)], 1)
    (y * dy).sum().backward()
    u = x @ a_stack.double().t()
    du = dy @ sb.double()
    pieces = unstack_gradients(du.t() @ x, dy.t() @ u, spans)
    for i, (da, db) in enumerate(pieces):
        assert torch.allclose(da, Ap[i].grad, rtol=1e-10, atol=1e-12) and torch.allclose(scales[i] * db, Bp[i].grad, rtol=1e-10, atol=1e-12)
    off = (dy.t() @ u)[:hid, 24:48]
    assert float(off.abs().max()) > 1.0          # the dropped blocks are not small: they belong to no parameter


def test_state_dict_keys_round_trip_and_refusals():
    pol = FakePolicy()
    ad = LowRankAdapters(pol, targets=(BLK + "0.mlp0", BLK + "2.r.orc_block.q_layer"), rank=3, alpha=6.0, seed=1)
    for t in ad.params.values():
        t.copy_(torch.randn(t.shape, generator=torch.Generator().manual_seed(t.numel())))
    sd = ad.state_dict()
    mods = [BLK + "0.mlp0.layer", BLK + "2.r.orc_block.q_layer"]
    assert set(sd) == {m + s for m in mods for s in (".lora_A", ".lora_B")} | {"rank", "alpha", "targets"}
    assert sd["rank"] == 3 and sd["alpha"] == 6.0 and sd["targets"] == mods
    assert all(sd[n].data_ptr() != ad.params[n].data_ptr() for n in ad.params)            # copies, not views
    fresh = LowRankAdapters(FakePolicy(), targets=mods, rank=3, alpha=1.0, seed=9)
    fresh.load_state_dict(sd)
    assert fresh.alpha == 6.0 and fresh.scale == 2.0 and all(torch.equal(fresh.params[n], ad.params[n]) for n in ad.params)
    assert ad.nbytes() == 4 * sum(t.numel() for t in ad.params.values())
    with pytest.raises(ValueError, match="another target set"):
        LowRankAdapters(FakePolicy(), targets=(BLK + "0.mlp0",), rank=3).load_state_dict(sd)
    with pytest.raises(ValueError, match="rank 3 does not fit"):
        LowRankAdapters(FakePolicy(), targets=mods, rank=4).load_state_dict(sd)
    with pytest.raises(ValueError, match="another policy shape"):
        LowRankAdapters(FakePolicy(hid=32), targets=mods, rank=3).load_state_dict(sd)
    with pytest.raises(ValueError, match="tensor names differ"):
        fresh.load_state_dict({k: v for k, v in sd.items() if not k.endswith("q_layer.lora_B")})
    with pytest.raises(ValueError, match="another policy object"):
        ad.merge_(FakePolicy())
    with pytest.raises(RuntimeError, match="not merged"):
        ad.unmerge_(pol)


def test_a_trainer_takes_adapters_plus_a_selection_and_refuses_adapted_weights():
    """_init_trainer's name logic on a fake (no engine, no device): trainable=None means no base tensor, strings add base tensors, an adapted weight
    is refused, adapter names resolve in param_groups, the cut is the lowest adapted level."""
    from vpt_amd.training import BCTrainer
    pol = FakePolicy()
    pol._engine = type("E", (), dict(cfg=dict(n_layers=LAYERS), dtype=torch.bfloat16, precision="bf16", cnn_streams=1, _QKV="qkvr"))()
    ad = LowRankAdapters(pol, targets=(BLK + "1", BLK + "2.mlp1"), rank=2)

    def make(**kw):
        tr = object.__new__(BCTrainer)
        tr._cnn_flags_from_env = lambda: None
        tr._init_trainer(pol, 1e-3, 0.0, (0.9, 0.999), 1e-8, False, True, None, 200, None, **kw)
        return tr

    tr = make(adapters=ad)
    assert tr.trainable == list(ad.params) and tr._cut == 3 and set(tr.m) == set(ad.params)
    assert all(tr.params[n] is ad.params[n] for n in ad.params)
    tr = make(adapters=ad, trainable=("pi_head", BLK + "2.mlp0"), param_groups=[dict(params=[BLK + "1.mlp0.layer.lora_A", "pi_head"], lr_scale=0.5)])
    assert tr.trainable == [BLK + "2.mlp0.norm.weight", BLK + "2.mlp0.layer.weight", "pi_head.buttons.linear_layer.weight"] + list(ad.params) and tr._cut == 3
    assert tr._group_of == {BLK + "1.mlp0.layer.lora_A": 0, "pi_head.buttons.linear_layer.weight": 0}
    assert sorted(tr.state_dict()["exp_avg"]) == sorted(tr.trainable)
    with pytest.raises(ValueError, match="frozen under an adapter"):
        make(adapters=ad, trainable=(BLK + "2.mlp1",))
    with pytest.raises(ValueError, match="frozen under an adapter"):
        make(adapters=ad, trainable=("net.recurrent_layer.blocks",))
    with pytest.raises(ValueError, match="match no parameter"):
        make(adapters=ad, trainable=(BLK + "1.mlp0.layer.lora_A",))          # adapters always train: they are not selectable base tensors
    with pytest.raises(ValueError, match="another policy object"):
        make(adapters=LowRankAdapters(FakePolicy(), rank=2))
    assert make().adapters is None and make()._subset is None              # the default: today's code path


@pytest.mark.parametrize("n,k,r", [(1, 1, 1), (3, 5, 16), (130, 257, 64), (7, 33, 4)])
def test_merge_restatement_within_the_fp64_bound(n, k, r):
    g = torch.Generator().manual_seed(n * 1000 + k + r)
    w = torch.randn(n, k, generator=g).numpy()
    a = ((torch.rand(r, k, generator=g) * 2 - 1) / math.sqrt(k)).numpy()
    b = torch.randn(n, r, generator=g).numpy()
    for s in (1.0, 16.0 / r, 0.3):
        out = R.merge_f32(w, a, b, s)
        assert out.dtype == np.float32 and out.shape == (n, k)
        out64, bnd = R.merge_ref(w, a, b, s)
        worst, msg = R.bound_ratio(torch.from_numpy(out), out64, bnd)
        assert msg is None, msg
        # a reference that leaves s out sits far outside
        if s != 1.0 and r >= 4:
            assert R.bound_ratio(torch.from_numpy(out), R.merge_ref(w, a, b, 1.0)[0], bnd)[0] > 100.0
    assert np.array_equal(R.merge_f32(w, a, np.zeros_like(b), 2.0), w)           # B = 0: the masters themselves
