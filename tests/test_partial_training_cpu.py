"""Partial fine-tuning, the parts that need no GPU: which names a selection picks (prefixes end at a `.` boundary), what it refuses,
how parameter groups resolve, what a fake trainer's checkpoint carries, and that both libraries export vpt_adam_step_groups under the unchanged ABI
number.  Fakes are built with object.__new__, as tests/test_trainer_base_cpu.py does."""
import ctypes
import os

import pytest
import torch

import vpt_amd  # noqa: F401
from vpt_amd import _native
from vpt_amd.idm_training import IDMTrainer
from vpt_amd.rl_training import PPOTrainer
from vpt_amd.trainer_base import TrainerBase, name_matches, resolve_param_groups, select_trainable
from vpt_amd.training import BCTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = [f"net.recurrent_layer.blocks.{l}.{leaf}" for l in (0, 1, 2, 10) for leaf in ("mlp0.layer.weight", "mlp1.layer.bias")]
NAMES = (["net.img_process.cnn.dense.layer.weight", "net.img_process.linear.layer.weight"] + BLOCKS +
         ["net.lastlayer.layer.weight", "net.final_ln.weight", "net.final_ln.bias", "pi_head.buttons.linear_layer.weight", "pi_head.camera.linear_layer.bias",
          "value_head.linear.weight", "value_head.linear.bias"])
BC_RULE = lambda n: not n.startswith("value_head.")


def test_a_prefix_ends_at_a_dot_boundary():
    assert name_matches("pi_head", "pi_head.camera.linear_layer.bias") and name_matches("pi_head.", "pi_head.camera.linear_layer.bias")
    assert name_matches("net.final_ln.bias", "net.final_ln.bias") and not name_matches("net.final_ln.bias", "net.final_ln.bias2")
    assert not name_matches("pi_hea", "pi_head.camera.linear_layer.bias") and not name_matches("net.final", "net.final_ln.weight")
    assert name_matches("net.recurrent_layer.blocks.1", "net.recurrent_layer.blocks.1.mlp0.layer.weight")
    assert not name_matches("net.recurrent_layer.blocks.1", "net.recurrent_layer.blocks.10.mlp0.layer.weight")
    got = select_trainable(NAMES, BC_RULE, ["net.recurrent_layer.blocks.1"])
    assert got == [n for n in NAMES if n.startswith("net.recurrent_layer.blocks.1.")] and len(got) == 2


def test_selection_keeps_parameter_order_and_none_is_the_rule():
    assert select_trainable(NAMES, BC_RULE, None) == [n for n in NAMES if BC_RULE(n)]
    got = select_trainable(NAMES, BC_RULE, ["pi_head", "net.final_ln.bias", "net.lastlayer"])
    assert got == ["net.lastlayer.layer.weight", "net.final_ln.bias", "pi_head.buttons.linear_layer.weight", "pi_head.camera.linear_layer.bias"]
    assert select_trainable(NAMES, BC_RULE, "pi_head") == got[2:]                     # a bare string is one selector, not its characters
    assert select_trainable(NAMES, BC_RULE, (s for s in ["pi_head"])) == got[2:]      # any iterable
    assert select_trainable(NAMES, BC_RULE, ["pi_head", "pi_head.camera"]) == got[2:]     # overlapping selectors: each name once
    # a callable filters inside the rule: accepting everything is the rule's own set, value head left out silently
    assert select_trainable(NAMES, BC_RULE, lambda n: True) == select_trainable(NAMES, BC_RULE, None)
    assert select_trainable(NAMES, BC_RULE, lambda n: n.endswith(".bias")) == [n for n in NAMES if n.endswith(".bias") and BC_RULE(n)]


def test_selection_refusals_name_the_offenders():
    with pytest.raises(ValueError, match=r"BCTrainer\(trainable=\): \['pi_heads', 'net\.final'\] match no parameter"):
        select_trainable(NAMES, BC_RULE, ["pi_head", "pi_heads", "net.final"], "BCTrainer")
    with pytest.raises(ValueError, match=r"does not train \['value_head\.linear\.weight', 'value_head\.linear\.bias'\]"):
        select_trainable(NAMES, BC_RULE, ["pi_head", "value_head"])
    with pytest.raises(ValueError, match="leaves no trainable parameter"):
        select_trainable(NAMES, BC_RULE, [])
    with pytest.raises(ValueError, match="leaves no trainable parameter"):
        select_trainable(NAMES, BC_RULE, lambda n: n.startswith("value_head."))
    with pytest.raises(ValueError, match="non-empty parameter names"):
        select_trainable(NAMES, BC_RULE, ["pi_head", ""])
    with pytest.raises(ValueError, match="non-empty parameter names"):
        select_trainable(NAMES, BC_RULE, ["pi_head", 3])


def test_the_trainers_rules_without_building_one():
    params = {n: torch.nn.Parameter(torch.zeros(0 if n.endswith("b_nd") else 2)) for n in NAMES + ["net.recurrent_layer.blocks.0.r.orc_block.b_nd",
                                                                                                   "net.conv3d_layer.layer.weight"]}
    bc = BCTrainer.rule_trainable(params, False)
    assert not any(n.startswith(("value_head.", "net.img_process.cnn.")) for n in bc) and "net.lastlayer.layer.weight" in bc
    assert "net.img_process.cnn.dense.layer.weight" in BCTrainer.rule_trainable(params, True)
    ppo = PPOTrainer.rule_trainable(params, False)
    assert set(ppo) - set(bc) == {"value_head.linear.weight", "value_head.linear.bias"}
    idm = IDMTrainer.rule_trainable(params, False)
    assert not any(n.startswith(("net.lastlayer.", "net.conv3d_layer.", "net.img_process.cnn.")) or n.endswith("b_nd") for n in idm)
    assert "net.conv3d_layer.layer.weight" in IDMTrainer.rule_trainable(params, True)
    with pytest.raises(ValueError, match=r"does not train \['net\.lastlayer\.layer\.weight'\]"):
        probe = object.__new__(IDMTrainer)
        probe.train_cnn, probe.params = False, params
        select_trainable(list(params), probe._is_trainable, ["net.lastlayer"], "IDMTrainer")


def test_unit_levels_follow_the_forward_order():
    import types
    tr = object.__new__(BCTrainer)
    tr.engine = types.SimpleNamespace(cfg=dict(n_layers=4))
    level = tr._unit_level
    order = ["net.img_process.cnn.dense.layer.weight", "net.img_process.linear.norm.bias", "net.pre_lstm_ln.weight", "net.recurrent_layer.blocks.0.pre_r_ln.bias",
             "net.recurrent_layer.blocks.3.r.orc_block.b_nd", "net.lastlayer.layer.weight", "net.final_ln.bias", "pi_head.camera.linear_layer.bias"]
    assert [level(n) for n in order] == [-1, 0, 1, 2, 5, 6, 7, 8] and level("value_head.linear.bias") == 8 and level("net.conv3d_layer.layer.bias") == -1
    assert TrainerBase._cut == -1 and TrainerBase._subset is None and TrainerBase.param_groups == () and not TrainerBase.decoupled_weight_decay


def test_param_groups_resolve_to_one_group_per_name():
    trainable = select_trainable(NAMES, BC_RULE, None)
    groups, owner = resolve_param_groups(NAMES, trainable, [dict(params=["pi_head"], lr_scale=0.1, weight_decay=0),
                                                             dict(params="net.recurrent_layer.blocks.1"), dict(params=["net.final_ln.bias"], weight_decay=0.5)])
    assert groups == [dict(params=["pi_head"], lr_scale=0.1, weight_decay=0.0), dict(params=["net.recurrent_layer.blocks.1"], lr_scale=1.0, weight_decay=None),
                      dict(params=["net.final_ln.bias"], lr_scale=1.0, weight_decay=0.5)]
    assert owner == {"pi_head.buttons.linear_layer.weight": 0, "pi_head.camera.linear_layer.bias": 0, "net.recurrent_layer.blocks.1.mlp0.layer.weight": 1,
                     "net.recurrent_layer.blocks.1.mlp1.layer.bias": 1, "net.final_ln.bias": 2}
    assert resolve_param_groups(NAMES, trainable, None) == ([], {}) and resolve_param_groups(NAMES, trainable, []) == ([], {})
    assert resolve_param_groups(NAMES, trainable, groups)[0] == groups         # what state_dict() carries resolves to itself


def test_param_group_refusals():
    trainable = select_trainable(NAMES, BC_RULE, ["pi_head", "net.final_ln"])
    with pytest.raises(ValueError, match=r"\['pi_head\.camera\.linear_layer\.bias'\] are in group 0 and in group 1"):
        resolve_param_groups(NAMES, trainable, [dict(params=["pi_head"]), dict(params=["pi_head.camera"])])
    with pytest.raises(ValueError, match=r"group 0 names tensors that are not trainable: \['net\.lastlayer\.layer\.weight'\]"):
        resolve_param_groups(NAMES, trainable, [dict(params=["net.lastlayer", "pi_head"])])
    with pytest.raises(ValueError, match=r"group 1: \['nowhere'\] match no parameter"):
        resolve_param_groups(NAMES, trainable, [dict(params=["pi_head"]), dict(params=["nowhere"])])
    with pytest.raises(ValueError, match="must be dict"):
        resolve_param_groups(NAMES, trainable, [dict(params=["pi_head"], lr=0.1)])
    with pytest.raises(ValueError, match="must be dict"):
        resolve_param_groups(NAMES, trainable, [["pi_head"]])
    with pytest.raises(ValueError, match="finite and non-negative"):
        resolve_param_groups(NAMES, trainable, [dict(params=["pi_head"], weight_decay=float("nan"))])


def _fake(names, groups=None, decoupled=False, subset=True):
    tr = object.__new__(BCTrainer)
    tr.params = {n: torch.nn.Parameter(torch.zeros(3)) for n in NAMES}
    tr.trainable = list(names)
    if subset:
        tr._subset = frozenset(names)
    tr.param_groups, tr._group_of = resolve_param_groups(NAMES, tr.trainable, groups)
    tr.decoupled_weight_decay = decoupled
    tr.scaled, tr.loss_scale, tr.train_cnn, tr.max_grad_norm = False, 1.0, False, None
    tr.step_count, tr.lr, tr.wd, tr.betas, tr.eps = 0, 1e-3, 0.01, (0.9, 0.999), 1e-8
    tr.m = {n: torch.full((3,), 0.5) for n in names}
    tr.v = {n: torch.full((3,), 0.25) for n in names}
    return tr


def test_checkpoint_carries_names_groups_and_flag():
    heads = [n for n in NAMES if n.startswith("pi_head.")]
    groups = [dict(params=["pi_head.camera"], lr_scale=0.5, weight_decay=None)]
    sd = _fake(heads, groups, decoupled=True).state_dict()
    assert sd["trainable"] == heads and sd["param_groups"] == groups and sd["decoupled_weight_decay"] is True and set(sd["exp_avg"]) == set(heads)
    dst = _fake(heads)
    dst.load_state_dict(sd)
    assert dst.param_groups == groups and dst.decoupled_weight_decay and dst._group_of == {"pi_head.camera.linear_layer.bias": 0}
    # a dict without them leaves the constructor's values in place; a default trainer writes the dict it always wrote
    plain = _fake(heads).state_dict()
    assert "param_groups" not in plain and "decoupled_weight_decay" not in plain
    keep = _fake(heads, groups, decoupled=True)
    keep.load_state_dict(plain)
    assert keep.param_groups == groups and keep.decoupled_weight_decay
    assert "trainable" not in _fake(heads, subset=False).state_dict()
    with pytest.raises(KeyError, match="optimizer state does not match the trainable parameters"):
        _fake(heads + ["net.final_ln.bias"]).load_state_dict(sd)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_both_libraries_export_the_groups_entry_point_under_abi_5(fmt):
    lib = _native.load(fmt)
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    assert lib.vpt_adam_step_groups.argtypes == [P, P, I, L, I, F, F, F, F, I, P, P, P]
    assert int(lib.vpt_abi_version()) == 5 == _native.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "vpt_hip.h")).read()
    assert "int vpt_adam_step_groups(const void* table, const void* groups, int ntensors, int64_t total_blocks, int step, float beta1, float beta2," in hdr
    assert "behavioural_cloning.py:63-67" in hdr[hdr.index("/* Parameter groups"):hdr.index("int vpt_adam_step_groups(")]
    assert hasattr(ctypes.CDLL(_native._LIB_PATHS[fmt]), "vpt_adam_step_groups")
    # argument errors are refused without a launch
    assert lib.vpt_adam_step_groups(None, None, 3, 3, 1, 0.9, 0.999, 1e-8, 1.0, 0, None, None, None) != 0
    assert b"vpt_adam_step_groups" in lib.vpt_last_error()
    assert lib.vpt_adam_step_groups(None, None, 0, 0, 0, 0.9, 0.999, 1e-8, 1.0, 0, None, None, None) != 0        # step counts from 1
