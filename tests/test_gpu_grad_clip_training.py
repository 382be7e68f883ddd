"""max_grad_norm of BCTrainer / PPOTrainer / IDMTrainer on the GPU, both operand formats: measure-only leaves the step bit-identical, a clipped step is
the hand-run sequence loss_and_grads -> ops.grad_norm -> ops.adam_step_multi_ on pre-multiplied gradients, the norm is torch's to the derived bound
and does not see the loss scale, a non-finite norm skips the step on the device, checkpoints carry the threshold, and the data-parallel path reports
the local path's norm.  1x policy (temperature 2), B = 2, T = 4; the tiny IDM of tests/test_gpu_idm_training.py.  Needs an MI355X."""
import copy
import os
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from vpt_amd.idm_training import IDMTrainer  # noqa: E402
from vpt_amd.rl_training import PPOTrainer  # noqa: E402
from vpt_amd.training import BCTrainer  # noqa: E402
from vpt_amd.lib.policy import InverseActionPolicy, MinecraftAgentPolicy  # noqa: E402
from vpt_amd.lib.types import idm_action_space, minecraft_action_space  # noqa: E402
from oracle import vpt_oracle as O  # noqa: E402
from tests import grad_norm_ref as GR  # noqa: E402
from tests import labeler_ref as LR  # noqa: E402
from tests import parity as P  # noqa: E402

DEV = "cuda"
NB, NC = 8641, 121
B, T = 2, 4
INF = float("inf")


def _policy(precision):
    pk = O.policy_kwargs_for("1x")
    cfg = O.config_from_policy_kwargs(pk, dict(temperature=2.0))
    sd = O.synthetic_state_dict(cfg, seed=0)
    pol = MinecraftAgentPolicy(minecraft_action_space(), pk, dict(temperature=2.0), precision=precision)
    pol.load_state_dict(sd, strict=False)
    return pol.to(DEV)


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def trainer_1x(request):
    pol = _policy(request.param)
    return pol, copy.deepcopy(pol.state_dict())


def _batch():
    g = torch.Generator().manual_seed(29)
    img = torch.randint(0, 256, (B, T, 128, 128, 3), generator=g, dtype=torch.uint8).to(DEV)
    first = torch.zeros(B, T, dtype=torch.bool, device=DEV)
    return img, first, torch.randint(0, NB, (B, T), generator=g).to(DEV), torch.randint(0, NC, (B, T), generator=g).to(DEV)


def _args(pol, batch):
    img, first, ab, ac = batch
    return img, first, pol.initial_state(B), ab, ac


def _snapshot(pol, tr):
    return ({k: v.detach().clone() for k, v in pol.named_parameters()}, {k: v.clone() for k, v in tr.m.items()}, {k: v.clone() for k, v in tr.v.items()})


def _same(a, b):
    return [k for part_a, part_b in zip(a, b) for k in part_a if not torch.equal(part_a[k], part_b[k])]


def _hand_clipped_step(tr, grads, grad_scale, max_norm, flag=None):
    """ops.grad_norm -> gradients pre-multiplied in torch as (g * grad_scale) * coef -> the UNCLIPPED ops.adam_step_multi_ with grad_scale = 1."""
    names = [n for n in tr.trainable if n in grads]
    flat = [grads[n].contiguous().view(-1) for n in names]
    norm_out, per = ops.grad_norm(flat, scale=grad_scale, max_norm=max_norm, per_tensor=True, flag=flag)
    gs = torch.tensor(grad_scale, dtype=torch.float32, device=DEV)
    pre = [(g * gs) * norm_out[1] for g in flat]
    ops.adam_step_multi_([tr.params[n].data.view(-1) for n in names], pre, [tr.m[n].view(-1) for n in names], [tr.v[n].view(-1) for n in names],
                         tr.step_count + 1, lr=tr.lr, beta1=tr.betas[0], beta2=tr.betas[1], eps=tr.eps, weight_decay=tr.wd, grad_scale=1.0)
    return norm_out, per, names


_MEASURED = {}


def _measured(pol, sd):
    """Once per format: two unclipped steps, the same two steps with max_grad_norm=inf, and ops.grad_norm of the first step's unscaled gradients."""
    key = pol.precision
    if key in _MEASURED:
        return _MEASURED[key]
    batch = _batch()
    out = dict(batch=batch)
    try:
        for tag, kw in (("plain", {}), ("inf", dict(max_grad_norm=INF))):
            pol.load_state_dict(sd)
            tr = BCTrainer(pol, **kw)
            losses, mets, snaps = [], [], []
            for _ in range(2):
                met = {}
                loss, _ = tr.step(*_args(pol, batch), metrics=met)
                losses.append(loss)
                mets.append(met)
                snaps.append(_snapshot(pol, tr))
            out[tag] = dict(losses=losses, metrics=mets, snaps=snaps, tr=tr)
        pol.load_state_dict(sd)
        tr = BCTrainer(pol, optimizer_state=False)
        _, g, _ = tr.loss_and_grads(*_args(pol, batch), unscaled=True, metrics={})      # (metrics: the fused loss launch step(metrics=...) takes)
        names = [n for n in tr.trainable if n in g]
        out["names"] = names
        out["grads"] = {n: g[n].clone() for n in names}
        out["norm_out"], out["per"] = ops.grad_norm([g[n].contiguous().view(-1) for n in names], per_tensor=True)
        torch.cuda.synchronize()
    finally:
        pol.load_state_dict(sd)
    _MEASURED[key] = out
    return out


def test_measure_only_is_bit_identical_and_reports_the_norm(trainer_1x):
    """(g) max_grad_norm=inf: two steps give parameters, moments and loss torch.equal to a trainer built without the argument; metrics["grad_norm"] is
    ops.grad_norm of loss_and_grads(unscaled=True)'s gradients (same table order: bit for bit)."""
    pol, sd = trainer_1x
    M = _measured(pol, sd)
    assert M["plain"]["losses"] == M["inf"]["losses"]
    for s0, s1 in zip(M["plain"]["snaps"], M["inf"]["snaps"]):
        assert not _same(s0, s1), _same(s0, s1)[:4]
    assert "grad_norm" not in M["plain"]["metrics"][0] and M["plain"]["tr"].last_grad_norm is None
    met = M["inf"]["metrics"][0]
    assert torch.equal(met["grad_norm"], M["norm_out"][0]) and float(met["clip_coef"]) == 1.0 and float(met["grad_norm"]) > 0
    assert list(met["grad_norm_per_tensor"]) == M["names"] and len(M["names"]) >= 120
    assert torch.equal(torch.stack([met["grad_norm_per_tensor"][n] for n in M["names"]]), M["per"])
    assert torch.equal(M["inf"]["tr"].last_grad_norm, M["inf"]["metrics"][1]["grad_norm"])
    assert M["inf"]["tr"].step_count == 2 and M["inf"]["tr"].skipped_steps == 0
    print(f"[{pol.precision}] gradient norm of the first step {float(met['grad_norm']):.6f}, of the second {float(M['inf']['metrics'][1]['grad_norm']):.6f}")
    with pytest.raises(ValueError, match="max_grad_norm"):
        BCTrainer(pol, max_grad_norm=0.0)


def test_clipped_step_is_the_hand_run_sequence(trainer_1x):
    """(h) max_grad_norm = half the measured norm, weight decay 0: the step equals loss_and_grads(unscaled=False) -> ops.grad_norm -> ops.adam_step_multi_ on
    pre-multiplied gradients bit for bit and differs from the unclipped step.  Update sizes: on Adam's FIRST step (m = v = 0, wd = 0) an element moves by
    lr g' / (|g'| + eps) with g' = c g, so clipped / unclipped = c (|g| + eps) / (c |g| + eps), which lies in [c, 1] -- Adam renormalises: the ratio is c only
    where |g| << eps and 1 where |g| >> eps.  Per tensor the update norms therefore satisfy c <= clipped / unclipped <= 1 (c ~ 1/2: "within a factor two above
    half"), up to the rounding of p - p0 in fp32: |p| < 4 and lr = 1.81e-4 give 2^-24 x 4 / 1.81e-4 < 2e-3 relative, taken as 1e-2.
    (i) torch.nn.utils.clip_grad_norm_ in fp64 on the same gradients gives a norm within the derived bound of the trainer's."""
    pol, sd = trainer_1x
    M = _measured(pol, sd)
    batch = M["batch"]
    half = float(M["norm_out"][0]) / 2
    m = B * T
    start = {k: v.detach().clone() for k, v in pol.named_parameters()}
    try:
        tr_h = BCTrainer(pol, weight_decay=0.0)
        _, grads, _ = tr_h.loss_and_grads(*_args(pol, batch), unscaled=False, metrics={})
        norm_h, per_h, names = _hand_clipped_step(tr_h, grads, tr_h.grad_unscale(m), half)
        hand = _snapshot(pol, tr_h)
        scale32 = float(torch.tensor(tr_h.grad_unscale(m), dtype=torch.float32))
        ps = [torch.nn.Parameter(torch.zeros(grads[n].numel(), dtype=torch.float64, device=DEV)) for n in names]
        for p_, n in zip(ps, names):
            p_.grad = grads[n].double().view(-1) * scale32
        t_norm = float(torch.nn.utils.clip_grad_norm_(ps, half))

        pol.load_state_dict(sd)
        tr_c = BCTrainer(pol, weight_decay=0.0, max_grad_norm=half)
        met = {}
        tr_c.step(*_args(pol, batch), metrics=met)
        clipped = _snapshot(pol, tr_c)

        pol.load_state_dict(sd)
        tr_u = BCTrainer(pol, weight_decay=0.0)
        tr_u.step(*_args(pol, batch), metrics={})
        plain = _snapshot(pol, tr_u)
        torch.cuda.synchronize()
    finally:
        pol.load_state_dict(sd)
    assert not _same(clipped, hand), _same(clipped, hand)[:4]
    assert torch.equal(met["grad_norm"], norm_h[0]) and torch.equal(met["clip_coef"], norm_h[1])
    assert torch.equal(met["grad_norm"], M["norm_out"][0])                  # the same weights and batch as the measured step
    c = float(met["clip_coef"])
    assert abs(c - 0.5) < 1e-6 and tr_c.step_count == 1 and tr_c.skipped_steps == 0
    ratios = []
    for n in names:
        du = float((plain[0][n] - start[n]).double().norm())
        dc = float((clipped[0][n] - start[n]).double().norm())
        if du == 0.0:
            assert dc == 0.0, n
            continue
        ratios.append(dc / du)
        assert not torch.equal(clipped[1][n], plain[1][n]) and not torch.equal(clipped[2][n], plain[2][n]), n      # the moments: x c and x c^2
        assert c * (1 - 1e-2) <= dc / du <= 1 + 1e-2, (n, dc / du)
    err = abs(float(met["grad_norm"]) - t_norm) / t_norm
    print(f"[{pol.precision}] clip coefficient {c!r}; update-norm ratios clipped / unclipped in [{min(ratios):.4f}, {max(ratios):.4f}] over {len(ratios)} tensors; "
          f"norm vs clip_grad_norm_ in fp64: err / bound = {err / GR.BOUND:.3f}")
    assert err <= GR.BOUND


def test_fp16_threshold_does_not_see_the_loss_scale():
    """(i) two fp16 trainers with loss scales 256 and 1024 report norms no further apart than their gradient sets are: | |a| - |b| | <= |a - b|, measured
    here on loss_and_grads(unscaled=True) of the two, plus the kernel's bound on each norm."""
    pol = _policy("fp16")
    sd = copy.deepcopy(pol.state_dict())
    batch = _batch()
    norms, sets = {}, {}
    for ls in (256.0, 1024.0):
        pol.load_state_dict(sd)
        tr = BCTrainer(pol, loss_scale=ls, max_grad_norm=INF)
        _, g, _ = tr.loss_and_grads(*_args(pol, batch), unscaled=True, metrics={})
        sets[ls] = {n: g[n].double().clone() for n in tr.trainable if n in g}
        met = {}
        tr.step(*_args(pol, batch), metrics=met)
        norms[ls] = float(met["grad_norm"])
        assert tr.skipped_steps == 0 and tr.loss_scale == ls
    torch.cuda.synchronize()
    d = float(torch.sqrt(sum(((sets[256.0][n] - sets[1024.0][n]) ** 2).sum() for n in sets[256.0])))
    print(f"fp16 norms at loss scale 256 / 1024: {norms[256.0]:.6f} / {norms[1024.0]:.6f}, distance of the gradient sets {d:.3e}")
    assert abs(norms[256.0] - norms[1024.0]) <= d + 2 * GR.BOUND * norms[256.0]
    assert d < 0.05 * norms[256.0]                       # (the sets themselves agree: the bound above is not vacuous)


def test_nonfinite_norm_skips_the_step_in_both_formats():
    """(j) fp16 with an absurd loss scale and clipping on: skipped, parameters unchanged, scale halved, skipped_steps == 1.  bf16: an inf planted in one
    gradient on the hand-run route through ops (the flag given to adam_step_multi_ with max_grad_norm) leaves every tensor untouched; torch would have
    written NaN into every parameter."""
    batch = _batch()
    pol = _policy("fp16")
    tr = BCTrainer(pol, lr=1e-4, weight_decay=0.0, loss_scale=2.0 ** 30, max_grad_norm=5.0)
    before = {k: v.detach().clone() for k, v in pol.named_parameters()}
    met = {}
    tr.step(*_args(pol, batch), metrics=met)
    torch.cuda.synchronize()
    assert tr.skipped_steps == 1 and tr.step_count == 0 and tr.loss_scale == 2.0 ** 29
    assert float(met["clip_coef"]) == 0.0 and not bool(torch.isfinite(met["grad_norm"]))
    assert all(torch.equal(v.detach(), before[k]) for k, v in pol.named_parameters())
    assert all(float(x.abs().max()) == 0.0 for x in tr.m.values()) and all(float(x.abs().max()) == 0.0 for x in tr.v.values())
    del pol, tr
    pol = _policy("bf16")
    tr = BCTrainer(pol, max_grad_norm=5.0)
    before = _snapshot(pol, tr)
    _, grads, _ = tr.loss_and_grads(*_args(pol, batch), unscaled=False)
    names = [n for n in tr.trainable if n in grads]
    last = grads[names[-1]]
    last[(-1,) * last.dim()] = INF
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    norm_out = torch.empty(4, device=DEV)
    ops.adam_step_multi_([tr.params[n].data.view(-1) for n in names], [grads[n].contiguous().view(-1) for n in names],
                         [tr.m[n].view(-1) for n in names], [tr.v[n].view(-1) for n in names], 1, lr=tr.lr, weight_decay=tr.wd,
                         found_inf=flag, max_grad_norm=5.0, norm_out=norm_out)
    torch.cuda.synchronize()
    assert int(flag) == 1 and float(norm_out[1]) == 0.0 and float(norm_out[2]) == 1.0
    assert not _same(_snapshot(pol, tr), before)
    # ... and through step(): a bf16 trainer whose norm is not finite counts a skipped step and keeps its loss scale of 1
    tr._optimizer_tail(torch.zeros((), device=DEV), grads, 1.0, DEV)
    assert tr.skipped_steps == 1 and tr.step_count == 0 and tr.loss_scale == 1.0 and not _same(_snapshot(pol, tr), before)


def _ppo_inputs(pol, batch):
    g = torch.Generator().manual_seed(31)
    img, first, ab, ac = batch
    adv = (torch.rand(B, T, generator=g) - 0.3).to(DEV)
    target = torch.randn(B, T, generator=g).to(DEV)
    tr = PPOTrainer(pol, optimizer_state=False, train_cnn=False, normalize_advantages=False, update_value_normalizer=False)
    met, _ = tr.evaluate(img, first, pol.initial_state(B), ab, ac, torch.zeros(B, T, device=DEV), adv, target)
    old = met["frame_out"][..., 8].clone() - 0.1
    return lambda: (img, first, pol.initial_state(B), ab, ac, old, adv, target)


def test_ppo_clipped_step_is_the_hand_run_sequence(trainer_1x):
    """(k) PPOTrainer: one clipped step == loss_and_grads(unscaled=False) -> ops.grad_norm -> Adam on pre-multiplied gradients, the value head included."""
    pol, sd = trainer_1x
    args = _ppo_inputs(pol, _batch())
    kw = dict(update_value_normalizer=False, entropy_coef=0.01)
    try:
        tr_m = PPOTrainer(pol, max_grad_norm=INF, **kw)
        met = {}
        tr_m.step(*args(), metrics=met)
        half = float(met["grad_norm"]) / 2
        pol.load_state_dict(sd)
        tr_h = PPOTrainer(pol, **kw)
        _, grads, _ = tr_h.loss_and_grads(*args(), unscaled=False)
        norm_h, _, names = _hand_clipped_step(tr_h, grads, tr_h.grad_unscale(tr_h._global_frames), half)
        hand = _snapshot(pol, tr_h)
        pol.load_state_dict(sd)
        tr_c = PPOTrainer(pol, max_grad_norm=half, **kw)
        met_c = {}
        tr_c.step(*args(), metrics=met_c)
        clipped = _snapshot(pol, tr_c)
        torch.cuda.synchronize()
    finally:
        pol.load_state_dict(sd)
    assert "value_head.linear.weight" in names and "value_head.linear.weight" in met_c["grad_norm_per_tensor"]
    assert not _same(clipped, hand), _same(clipped, hand)[:4]
    assert torch.equal(met_c["grad_norm"], norm_h[0]) and torch.equal(met_c["clip_coef"], norm_h[1]) and abs(float(norm_h[1]) - 0.5) < 1e-6
    assert torch.equal(met_c["grad_norm"], met["grad_norm"]) and "pg_loss" in met_c


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_idm_clipped_step_is_the_hand_run_sequence(precision):
    """(k) IDMTrainer, the tiny IDM, B = 2, T = 12."""
    kw, cfg, sd = LR.tiny_idm()
    pol = InverseActionPolicy(idm_action_space(), pi_head_kwargs=dict(temperature=LR.TEMPERATURE), idm_net_kwargs=kw, precision=precision)
    pol.load_state_dict(sd, strict=False)
    pol = pol.to(DEV)
    g = torch.Generator().manual_seed(21)
    img = P.structured_frames(2, 12, g).to(DEV)
    buttons, camera = torch.randint(0, 2, (2, 12, 20), generator=g).to(DEV), torch.randint(0, 11, (2, 12, 2), generator=g).to(DEV)
    tr_m = IDMTrainer(pol, max_grad_norm=INF)
    met = {}
    tr_m.step(img, buttons, camera, metrics=met)
    half = float(met["grad_norm"]) / 2
    pol.load_state_dict(sd, strict=False)
    tr_h = IDMTrainer(pol)
    _, grads = tr_h.loss_and_grads(img, buttons, camera, unscaled=False)
    norm_h, _, names = _hand_clipped_step(tr_h, grads, tr_h.grad_unscale(tr_h._weight_sum), half)
    hand = _snapshot(pol, tr_h)
    pol.load_state_dict(sd, strict=False)
    tr_c = IDMTrainer(pol, max_grad_norm=half)
    met_c = {}
    tr_c.step(img, buttons, camera, metrics=met_c)
    torch.cuda.synchronize()
    assert not _same(_snapshot(pol, tr_c), hand)
    assert torch.equal(met_c["grad_norm"], norm_h[0]) and torch.equal(met_c["clip_coef"], norm_h[1]) and abs(float(norm_h[1]) - 0.5) < 1e-6
    assert torch.equal(met_c["grad_norm"], met["grad_norm"]) and list(met_c["grad_norm_per_tensor"]) == names
    state = tr_c.state_dict()
    assert state["max_grad_norm"] == half
    tr2 = IDMTrainer(pol)
    tr2.load_state_dict(state)
    assert tr2.max_grad_norm == half


def test_state_dict_round_trip(trainer_1x):
    """(l) state_dict carries max_grad_norm; a dict without the key keeps the constructor's value."""
    pol, sd = trainer_1x
    tr = BCTrainer(pol, max_grad_norm=5.0)
    state = tr.state_dict()
    assert state["max_grad_norm"] == 5.0 and BCTrainer(pol).state_dict()["max_grad_norm"] is None
    tr2 = BCTrainer(pol)
    tr2.load_state_dict(state)
    assert tr2.max_grad_norm == 5.0
    tr2.load_state_dict(dict(state, max_grad_norm=None))
    assert tr2.max_grad_norm is None
    old = {k: v for k, v in state.items() if k != "max_grad_norm"}
    tr3 = BCTrainer(pol, max_grad_norm=INF)
    tr3.load_state_dict(old)
    assert tr3.max_grad_norm == INF
    tr4 = PPOTrainer(pol, max_grad_norm=2.5)
    assert tr4.max_grad_norm == 2.5 and tr4.state_dict()["max_grad_norm"] == 2.5


def _rccl_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        pol = _policy("bf16")
        sd = copy.deepcopy(pol.state_dict())
        batch = _batch()
        res = []
        for force in (False, True):
            pol.load_state_dict(sd)
            tr = BCTrainer(pol, max_grad_norm=1.0)
            tr.force_exchange = force
            met = {}
            tr.step(*_args(pol, batch), metrics=met)
            torch.cuda.synchronize()
            assert (tr._arenas is not None) == force
            res.append((met["grad_norm"].clone(), met["clip_coef"].clone(), {k: v.detach().clone() for k, v in pol.named_parameters()}))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and 0 < float(res[0][1]) < 1
        assert all(torch.equal(res[0][2][k], res[1][2][k]) for k in res[0][2])
        with open(os.path.join(out_dir, "ok"), "w") as f:
            f.write(f"{float(res[0][0])!r}")
    finally:
        dist.destroy_process_group()


def test_data_parallel_path_reports_the_local_norm():
    """(l) the whole data-parallel step over RCCL in a one-rank group (force_exchange): the Adam call sits after the exchange, so grad_norm, the
    coefficient and the clipped parameters are the local path's, bit for bit."""
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_rccl_worker, args=(1, 29571, d), nprocs=1, join=True)
        assert float(open(os.path.join(d, "ok")).read()) > 0
