"""The host code the three trainers share (trainer_base.TrainerBase) on CPU tensors: the frame-weight check, the record-based loss, grad_unscale and
the optimiser-state checkpoint.  Fakes are built with object.__new__ (as tests/test_distributed_cpu.py does): no policy, no engine, no GPU."""
import types

import pytest
import torch

import vpt_amd  # noqa: F401
from vpt_amd.idm_training import IDMTrainer
from vpt_amd.rl_training import PPOTrainer
from vpt_amd.trainer_base import TrainerBase
from vpt_amd.training import BCTrainer

TRAINERS = (BCTrainer, PPOTrainer, IDMTrainer)
B, T = 3, 5
IMG = types.SimpleNamespace(shape=(B, T, 128, 128, 3), device=torch.device("cpu"))     # _checked_weights reads the frame count and the device only


def test_the_three_trainers_share_one_base():
    assert all(issubclass(c, TrainerBase) for c in TRAINERS) and issubclass(PPOTrainer, BCTrainer) and not issubclass(IDMTrainer, BCTrainer)
    for name in ("state_dict", "load_state_dict", "_need_optimizer_state", "grad_unscale", "_optimizer_tail", "_checked_weights", "_record_loss",
                 "_fill_metrics", "_trunk_backward", "_trunk_forward_saving"):
        assert all(getattr(c, name) is getattr(TrainerBase, name) for c in TRAINERS), name


# ---- frame weights ----------------------------------------------------------------------------------------------------------------------
def test_checked_weights_returns_fp32_flat_weights_and_their_fp64_sum():
    g = torch.Generator().manual_seed(5)
    fw = torch.rand(B, T, generator=g, dtype=torch.float64).t().contiguous().t()       # [B, T], not contiguous
    w, wsum = BCTrainer._checked_weights(fw, IMG)
    assert w.dtype == torch.float32 and tuple(w.shape) == (B * T,) and w.is_contiguous()
    assert torch.equal(w, fw.reshape(-1).to(torch.float32))
    assert isinstance(wsum, float) and wsum == float(w.to(torch.float64).sum())
    w2, wsum2 = IDMTrainer._checked_weights(fw.tolist(), IMG)                          # anything torch.as_tensor takes
    assert torch.equal(w2, w) and wsum2 == wsum


def test_checked_weights_device_and_host_halves_are_the_whole():
    fw = torch.arange(B * T, dtype=torch.float32).view(B, T)
    w, probe = TrainerBase._weights_on_device(fw, IMG)
    assert len(probe) == 2 and all(p.dtype == torch.float64 and p.dim() == 0 for p in probe)
    assert [float(p) for p in probe] == [float(fw.sum()), 0.0] and torch.equal(w, fw.reshape(-1))
    TrainerBase._check_weight_probe(*[float(p) for p in probe])


@pytest.mark.parametrize("bad, message", [
    (torch.ones(B, T + 1), rf"frame_weight must hold one weight per frame \(\[{B}, {T}\]\), got \({B}, {T + 1}\)"),
    (torch.ones(B, T).index_put((torch.tensor(1), torch.tensor(2)), torch.tensor(-0.5)), r"frame_weight must be finite and non-negative \(min -0\.5, sum 13\.5\)"),
    (torch.ones(B, T).index_put((torch.tensor(0), torch.tensor(0)), torch.tensor(float("nan"))), r"frame_weight must be finite and non-negative \(min nan, sum nan\)"),
    (torch.ones(B, T).index_put((torch.tensor(2), torch.tensor(4)), torch.tensor(float("inf"))), r"frame_weight must be finite and non-negative \(min 1\.0, sum inf\)"),
], ids=["count", "negative", "nan", "inf"])
def test_checked_weights_rejects(bad, message):
    with pytest.raises(ValueError, match=message):
        BCTrainer._checked_weights(bad, IMG)


def test_all_zero_weights_pass_the_check_and_the_callers_raise():
    w, wsum = BCTrainer._checked_weights(torch.zeros(B, T), IMG)
    assert wsum == 0 and not w.any()
    tr = object.__new__(BCTrainer)
    tr.scaled = False
    with pytest.raises(ValueError, match="frame_weight: every weight is zero"):        # raised before the forward: nothing else of the trainer is read
        tr.loss_and_grads(IMG, None, None, None, None, frame_weight=torch.zeros(B, T))
    with pytest.raises(ValueError, match="frame_weight: every weight is zero"):
        tr.evaluate(IMG, None, None, None, None, frame_weight=torch.zeros(B, T))
    idm = object.__new__(IDMTrainer)
    idm.engine = types.SimpleNamespace(button_shape=(20, 2), camera_shape=(2, 11))
    labels = torch.zeros(B, T, 20, dtype=torch.int64), torch.zeros(B, T, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="frame_weight: every weight is zero"):
        idm._checked_inputs(IMG, *labels, torch.zeros(B, T))
    with pytest.raises(ValueError, match=r"frame_weight must be finite and non-negative \(min -1\.0, sum 13\.0\)"):
        idm._checked_inputs(IMG, *labels, torch.ones(B, T).index_put((torch.tensor(0), torch.tensor(0)), torch.tensor(-1.0)))
    ab, ac, w, wsum = idm._checked_inputs(IMG, *labels, torch.full((B, T), 0.5))
    assert wsum == 0.5 * B * T and w.dtype == torch.float32 and tuple(ab.shape) == (B * T, 20) and tuple(ac.shape) == (B * T, 2)
    assert idm._checked_inputs(IMG, *labels, None)[2:] == (None, float(B * T))


# ---- the loss from the per-frame records ------------------------------------------------------------------------------------------------------
def test_record_loss_with_unit_weights_is_the_default_paths_mean_bit_for_bit():
    m = 37
    frame_out = torch.randn(m, 8, generator=torch.Generator().manual_seed(9))
    ref = (frame_out[:, 0] + frame_out[:, 1]).mean()
    assert torch.equal(TrainerBase._record_loss(frame_out, None, None), ref)
    assert torch.equal(TrainerBase._record_loss(frame_out, torch.ones(m), float(m)), ref)


def test_record_loss_counts_an_exact_zero_for_a_zero_weight_frame():
    m = 6
    frame_out = torch.rand(m, 8, generator=torch.Generator().manual_seed(10))
    w = torch.tensor([1.0, 0.0, 2.0, 0.5, 0.0, 1.0])
    clean = TrainerBase._record_loss(frame_out, w, float(w.sum()))
    dirty = frame_out.clone()
    dirty[1, :2], dirty[4, 0] = float("nan"), float("inf")
    assert torch.equal(TrainerBase._record_loss(dirty, w, float(w.sum())), clean) and torch.isfinite(clean)
    assert torch.isnan(TrainerBase._record_loss(frame_out, torch.zeros(m), 0.0))       # a shard without weight: NaN, the reduction over ranks decides


# ---- fp16 loss scaling ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", TRAINERS)
def test_grad_unscale(cls):
    tr = object.__new__(cls)
    tr.scaled, tr.loss_scale = False, 256.0
    assert tr.grad_unscale(40) == 1.0
    tr.scaled = True
    assert tr.grad_unscale(40) == 1.0 / (256.0 * 40)
    g = {"a": torch.full((3,), 512.0), "b": torch.ones(2, 2)}
    keep = {k: v.data_ptr() for k, v in g.items()}
    tr._unscale_(g, 2.0)
    assert torch.equal(g["a"], torch.ones(3)) and torch.equal(g["b"], torch.full((2, 2), 1.0 / 512.0)) and keep == {k: v.data_ptr() for k, v in g.items()}


# ---- checkpoint ----------------------------------------------------------------------------------------------------------------------------------
_NAMES = ("net.final_ln.weight", "pi_head.camera.linear_layer.bias")


def _fake(cls, seed=None, optimizer_state=True, max_grad_norm=None):
    tr = object.__new__(cls)
    tr.params = {n: torch.nn.Parameter(torch.zeros(s)) for n, s in zip(_NAMES, ((4,), (3, 2)))}
    tr.trainable = list(_NAMES)
    tr.scaled, tr.loss_scale, tr.train_cnn, tr.max_grad_norm = True, 256.0, False, max_grad_norm
    tr.step_count, tr.lr, tr.wd, tr.betas, tr.eps = 0, 1e-3, 0.0, (0.9, 0.999), 1e-8
    g = torch.Generator().manual_seed(seed or 0)
    fill = (lambda p: torch.randn(p.shape, generator=g)) if seed is not None else torch.zeros_like
    tr.m = {n: fill(p) for n, p in tr.params.items()} if optimizer_state else {}
    tr.v = {n: fill(p) for n, p in tr.params.items()} if optimizer_state else {}
    return tr


@pytest.mark.parametrize("cls", TRAINERS)
def test_checkpoint_round_trip(cls):
    src = _fake(cls, seed=3, max_grad_norm=5.0)
    src.step_count, src.lr, src.wd, src.betas, src.eps, src.loss_scale = 17, 2e-4, 0.04, [0.8, 0.99], 1e-6, 64.0
    sd = src.state_dict()
    assert list(sd) == ["step", "lr", "weight_decay", "betas", "eps", "loss_scale", "train_cnn", "max_grad_norm", "exp_avg", "exp_avg_sq"]
    assert sd["betas"] == (0.8, 0.99) and sd["exp_avg"][_NAMES[0]].data_ptr() != src.m[_NAMES[0]].data_ptr()
    dst = _fake(cls)
    dst.load_state_dict(sd)
    assert (dst.step_count, dst.lr, dst.wd, dst.betas, dst.eps, dst.loss_scale, dst.max_grad_norm) == (17, 2e-4, 0.04, (0.8, 0.99), 1e-6, 64.0, 5.0)
    for n in _NAMES:
        assert torch.equal(dst.m[n], src.m[n]) and torch.equal(dst.v[n], src.v[n]) and dst.m[n].data_ptr() != sd["exp_avg"][n].data_ptr()
    # a dict written before max_grad_norm existed keeps the constructor's value; bf16 ignores a stored loss scale
    old = {k: v for k, v in sd.items() if k != "max_grad_norm"}
    dst = _fake(cls, max_grad_norm=2.5)
    dst.scaled, dst.loss_scale = False, 1.0
    dst.load_state_dict(old)
    assert dst.max_grad_norm == 2.5 and dst.loss_scale == 1.0 and dst.step_count == 17
    with pytest.raises(ValueError, match="max_grad_norm must be positive"):
        _fake(cls).load_state_dict(dict(sd, max_grad_norm=0.0))


@pytest.mark.parametrize("cls", TRAINERS)
def test_checkpoint_rejects_other_parameters_and_gradient_only_trainers(cls):
    sd = _fake(cls, seed=4).state_dict()
    other = dict(sd, exp_avg={("renamed" if n == _NAMES[1] else n): t for n, t in sd["exp_avg"].items()})
    with pytest.raises(KeyError, match="optimizer state does not match the trainable parameters"):
        _fake(cls).load_state_dict(other)
    bare = _fake(cls, optimizer_state=False)
    for call in (bare.state_dict, lambda: bare.load_state_dict(sd), bare._need_optimizer_state):
        with pytest.raises(RuntimeError, match=f"this {cls.__name__} was built with optimizer_state=False"):
            call()
