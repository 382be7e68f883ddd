"""The weighted BC loss on the GPU: vpt_bc_loss_kernel (ops.bc_loss) against its host twin packing.bc_loss_metrics, bit for bit against
vpt_nll_bwd_kernel (ops.nll_backward) and against torch autograd; then BCTrainer's frame_weight / metrics / evaluate, in both operand formats, and
the two-rank step with weights.  Needs an MI355X.  The head widths are the real ones: 8641 is odd (rows are not 16-byte aligned) and
8641 + 121 + 1 is padded to 8768; the second kernel shape (300 + 7 -> 320) has fewer elements than two sweeps of the workgroup and a camera head
narrower than a wave."""
import os
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops, packing  # noqa: E402
from vpt_amd.training import BCTrainer  # noqa: E402
from vpt_amd.lib.policy import MinecraftAgentPolicy  # noqa: E402
from vpt_amd.lib.types import minecraft_action_space  # noqa: E402
from oracle import vpt_oracle as O  # noqa: E402

DEV = "cuda"
TEMP = 2.0
WEIGHTS = [1.0, 0.0, 0.3, 1.0, 2.0, 0.5]
SHAPES = {"heads": (8641, 121, 8768), "small": (300, 7, 320)}
METRIC_KEYS = {"loss", "nll_buttons", "nll_camera", "acc_buttons", "acc_camera", "entropy_buttons", "entropy_camera", "weight_sum", "frames",
               "frame_nll", "frame_out"}


def _l2(a, ref):
    return float((a - ref).norm() / ref.norm().clamp(min=1e-30))


# ---------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------
_CASES = {}


def _case(shape):
    """Seeded inputs of one shape (built once): logits, log-probs as test_nll_backward makes them, labels with one hit and one miss placed by hand."""
    if shape in _CASES:
        return _CASES[shape]
    nb, nc, ldz = SHAPES[shape]
    g = torch.Generator().manual_seed(1)
    m = 6
    zb, zc = torch.randn(m, nb, generator=g) * 2, torch.randn(m, nc, generator=g) * 2
    ab, ac = torch.randint(0, nb, (m,), generator=g), torch.randint(0, nc, (m,), generator=g)
    lb, lc = torch.log_softmax(zb / TEMP, -1), torch.log_softmax(zc / TEMP, -1)
    for lp in (lb, lc):                                 # no row has two equal maxima: the arg-max is unambiguous
        top = lp.topk(2, dim=-1).values
        assert bool((top[:, 0] > top[:, 1]).all())
    ab[2], ac[2] = lb[2].argmax(), lc[2].argmax()       # on the arg-max
    ab[3], ac[3] = (lb[3].argmax() + 1) % nb, (lc[3].argmax() + 1) % nc     # off it
    w = torch.tensor(WEIGHTS)
    c = dict(nb=nb, nc=nc, ldz=ldz, m=m, zb=zb, zc=zc, lb=lb.to(DEV), lc=lc.to(DEV), ab=ab.to(DEV), ac=ac.to(DEV), w=w.to(DEV),
             scale=1.0 / (float(w.double().sum()) * TEMP))
    c["twin"] = packing.bc_loss_metrics(c["lb"], c["lc"], c["ab"], c["ac"], c["w"])
    _CASES[shape] = c
    return c


@pytest.mark.parametrize("shape", list(SHAPES))
def test_records_and_totals_match_the_host_twin(shape):
    """1a.  Slots 0, 1, 4, 5, 6 are single picked values or flags: exact.  Entropies and totals: every summand of a row's entropy is non-negative, a
    thread adds at most 34 terms, the tree about 10 levels, expf is good to 2 ulp -> about 50 x 2^-24 = 3e-6 from fp64; 1e-4 leaves a factor of 30."""
    c = _case(shape)
    _, frame_out, totals = ops.bc_loss(c["lb"], c["lc"], c["ab"], c["ac"], c["ldz"], c["scale"], weight=c["w"], want_dz=False)
    torch.cuda.synchronize()
    f_ref, t_ref = c["twin"]
    assert frame_out.dtype == totals.dtype == torch.float32 and tuple(frame_out.shape) == (c["m"], 8) and tuple(totals.shape) == (8,)
    exact = [0, 1, 4, 5, 6, 7]
    assert torch.equal(frame_out[:, exact].double(), f_ref[:, exact].float().double()), (frame_out[:, exact], f_ref[:, exact])
    assert frame_out[2, 4:6].tolist() == [1.0, 1.0] and frame_out[3, 4:6].tolist() == [0.0, 0.0]
    ent_err = float(((frame_out[:, 2:4].double() - f_ref[:, 2:4]).abs() / f_ref[:, 2:4].abs()).max())
    tot_err = float(((totals.double() - t_ref).abs() / t_ref.abs().clamp(min=1e-30)).max())
    print(f"bc_loss[{shape}] vs the fp64 twin: entropies rel {ent_err:.2e}, totals rel {tot_err:.2e}")
    assert ent_err < 1e-4 and tot_err < 1e-4
    assert float(totals[7]) == 5.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_dz_equals_nll_backward_bit_for_bit(shape, dtype):
    """1b.  A row of weight v is vpt_nll_bwd_kernel's row at scale' = fp32(scale) * fp32(v) -- one fp32 multiply, then the same expression."""
    c = _case(shape)
    dz, _, _ = ops.bc_loss(c["lb"], c["lc"], c["ab"], c["ac"], c["ldz"], c["scale"], weight=c["w"], dtype=dtype, want_frames=False, want_totals=False)
    dz1, _, _ = ops.bc_loss(c["lb"], c["lc"], c["ab"], c["ac"], c["ldz"], c["scale"], dtype=dtype, want_frames=False, want_totals=False)
    assert dz.dtype == dtype and tuple(dz.shape) == (c["m"], c["ldz"])
    for v in sorted(set(WEIGHTS)):
        ref = ops.nll_backward(c["lb"], c["lc"], c["ab"], c["ac"], c["ldz"], float(np.float32(c["scale"]) * np.float32(v)), dtype=dtype)
        rows = [i for i, x in enumerate(WEIGHTS) if x == v]
        assert torch.equal(dz[rows], ref[rows]), v
        if v == 1.0:
            assert torch.equal(dz1, ref)                # weight=None: all ones
    assert float(dz[:, c["nb"] + c["nc"]:].float().abs().max()) == 0.0        # value column and padding
    assert float(dz[1].float().abs().max()) == 0.0


def test_zero_weight_row_with_garbage_is_harmless():
    """1c.  A zero-weight row of NaN log-probs with labels -1 and nb + 5: its dz row is zero, the totals are finite and equal those of the call
    without the row.  The row is the LAST one, so that both calls add the other rows' records in the same association (vpt_slab_sum's tree is a
    function of the row count: a removed middle row would regroup the others) and the comparison is exact; a garbage row in the middle is held to its own
    clean-but-zero-weight counterpart, exactly, and to the twin."""
    c = _case("heads")
    nb, nc = c["nb"], c["nc"]
    order = [0, 2, 3, 4, 5, 1]                                    # the zero-weight row last
    lb, lc, ab, ac, w = (c[k][order].clone() for k in ("lb", "lc", "ab", "ac", "w"))
    assert float(w[5]) == 0.0
    lb[5], lc[5], ab[5], ac[5] = float("nan"), float("nan"), -1, nb + 5
    dz, _, totals = ops.bc_loss(lb, lc, ab, ac, c["ldz"], c["scale"], weight=w, want_frames=False)
    _, _, t_without = ops.bc_loss(lb[:5].contiguous(), lc[:5].contiguous(), ab[:5].contiguous(), ac[:5].contiguous(), c["ldz"], c["scale"],
                                  weight=w[:5].contiguous(), want_dz=False, want_frames=False)
    torch.cuda.synchronize()
    assert float(dz[5].float().abs().max()) == 0.0 and not bool(torch.isnan(dz.float()).any())
    assert bool(torch.isfinite(totals).all()) and torch.equal(totals, t_without), (totals, t_without)
    # ... and in the middle (row 1 of the usual order)
    lb, lc, ab, ac = (c[k].clone() for k in ("lb", "lc", "ab", "ac"))
    _, _, t_clean = ops.bc_loss(lb, lc, ab, ac, c["ldz"], c["scale"], weight=c["w"], want_dz=False, want_frames=False)
    lb[1], lc[1], ab[1], ac[1] = float("nan"), float("nan"), -1, nb + 5
    dz, _, t_mid = ops.bc_loss(lb, lc, ab, ac, c["ldz"], c["scale"], weight=c["w"], want_frames=False)
    torch.cuda.synchronize()
    assert float(dz[1].float().abs().max()) == 0.0 and not bool(torch.isnan(dz.float()).any())
    assert bool(torch.isfinite(t_mid).all()) and torch.equal(t_mid, t_clean)
    assert float(((t_mid.double() - c["twin"][1]).abs() / c["twin"][1].abs()).max()) < 1e-4


def test_same_call_same_bits():
    """1d.  No atomics anywhere: ten runs, one result."""
    c = _case("heads")
    first = None
    for _ in range(10):
        out = ops.bc_loss(c["lb"], c["lc"], c["ab"], c["ac"], c["ldz"], c["scale"], weight=c["w"])
        torch.cuda.synchronize()
        if first is None:
            first = out
        else:
            assert all(torch.equal(a, b) for a, b in zip(out, first))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_dz_is_the_gradient_of_the_weighted_mean(shape):
    """1e.  Against torch.autograd.grad of sum w nll / sum w with respect to the logits; test_nll_backward's bound for a 16-bit dz."""
    c = _case(shape)
    nb, nc = c["nb"], c["nc"]
    zb, zc = c["zb"].clone().requires_grad_(True), c["zc"].clone().requires_grad_(True)
    w, ab, ac = torch.tensor(WEIGHTS), c["ab"].cpu(), c["ac"].cpu()
    lb, lc = torch.log_softmax(zb / TEMP, -1), torch.log_softmax(zc / TEMP, -1)
    nll = -(lb.gather(1, ab[:, None]) + lc.gather(1, ac[:, None]))[:, 0]
    gb, gc = torch.autograd.grad((w * nll).sum() / w.sum(), [zb, zc])
    dz, _, _ = ops.bc_loss(c["lb"], c["lc"], c["ab"], c["ac"], c["ldz"], c["scale"], weight=c["w"], want_frames=False, want_totals=False)
    torch.cuda.synchronize()
    dz = dz.cpu().float()
    eb, ec = _l2(dz[:, :nb], gb), _l2(dz[:, nb:nb + nc], gc)
    print(f"bc_loss[{shape}] dz vs autograd: rel-L2 buttons {eb:.2e}, camera {ec:.2e}")
    assert eb < 6e-3 and ec < 6e-3


def test_launcher_errors():
    c = _case("small")
    with pytest.raises(RuntimeError, match="ldz"):
        ops.bc_loss(c["lb"], c["lc"], c["ab"], c["ac"], 256, c["scale"], weight=c["w"])
    from vpt_amd import _native
    from vpt_amd._native import ptr
    import ctypes
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    totals = torch.empty(8, device=DEV)
    with pytest.raises(RuntimeError, match="workspace"):          # totals without a workspace
        _native.call("vpt_bc_loss", ptr(c["lb"]), ptr(c["lc"]), ptr(c["ab"]), ptr(c["ac"]), None, None, None, ptr(totals), None,
                     c["m"], c["nb"], c["nc"], c["ldz"], ctypes.c_float(1.0), stream)
    with pytest.raises(RuntimeError, match="M must be positive"):
        _native.call("vpt_bc_loss", ptr(c["lb"]), ptr(c["lc"]), ptr(c["ab"]), ptr(c["ac"]), None, None, None, None, None,
                     0, c["nb"], c["nc"], c["ldz"], ctypes.c_float(1.0), stream)


# ---------------------------------------------------------------------------------------------------------
# trainer level
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["bf16", "fp16"])
def trainer_1x(request):
    pk = O.policy_kwargs_for("1x")
    cfg = O.config_from_policy_kwargs(pk, dict(temperature=2.0))
    sd = O.synthetic_state_dict(cfg, seed=0)
    pol = MinecraftAgentPolicy(minecraft_action_space(), pk, dict(temperature=2.0), precision=request.param)
    pol.load_state_dict(sd, strict=False)
    return pol.to(DEV), cfg, sd


B, T = 2, 6
_BATCH = {}


def _batch():
    if not _BATCH:
        g = torch.Generator().manual_seed(5)
        _BATCH.update(img=torch.randint(0, 256, (B, T, 128, 128, 3), generator=g, dtype=torch.uint8).to(DEV),
                      first=torch.zeros(B, T, dtype=torch.bool, device=DEV),
                      ab=torch.randint(0, 8641, (B, T), generator=g).to(DEV), ac=torch.randint(0, 121, (B, T), generator=g).to(DEV),
                      w=torch.tensor([[1.0, 0.3, 0.0, 1.0, 0.3, 1.0], [0.0, 1.0, 1.0, 0.3, 0.0, 0.3]]).to(DEV))     # every row: a zero and a non-zero
    return _BATCH


def _args(pol, bt):
    return bt["img"], bt["first"], pol.initial_state(B), bt["ab"], bt["ac"]


@pytest.mark.parametrize("train_cnn", [False, True])
def test_weighted_step_is_the_parents_pieces_bit_for_bit(trainer_1x, train_cnn):
    """2a.  forward_saving -> dz assembled row by row from ops.nll_backward (one call per distinct weight, as in 1b) -> backward_from must be,
    tensor for tensor, what loss_and_grads(frame_weight=w) returns; the loss is the twin's on the saved log-probs."""
    pol, cfg, sd = trainer_1x
    tr = BCTrainer(pol, train_cnn=train_cnn, optimizer_state=False)
    bt = _batch()
    w = bt["w"]
    wsum = float(w.double().sum())
    m = B * T
    S = tr.forward_saving(bt["img"], bt["first"], pol.initial_state(B))
    ab, ac = bt["ab"].reshape(m), bt["ac"].reshape(m)
    _, t_twin = packing.bc_loss_metrics(S["lp_b"], S["lp_c"], ab, ac, w.reshape(m))
    loss_twin = float((t_twin[0] + t_twin[1]) / t_twin[6])
    scale = (tr.loss_scale if tr.scaled else 1.0 / wsum) / cfg["temperature"]
    dz_ref = torch.empty(m, S["ldz"], dtype=tr.dtype, device=DEV)
    for v in sorted(set(w.reshape(m).tolist())):
        rows = (w.reshape(m) == v).nonzero()[:, 0]
        dz_ref[rows] = ops.nll_backward(S["lp_b"], S["lp_c"], ab, ac, S["ldz"], float(np.float32(scale) * np.float32(v)), dtype=tr.dtype)[rows]
    g_ref = tr.backward_from(S, dz_ref)
    loss, grads, _ = tr.loss_and_grads(*_args(pol, bt), frame_weight=w, unscaled=False)
    torch.cuda.synchronize()
    assert set(grads) == set(g_ref) and len(grads) >= 60
    bad = [k for k in g_ref if not torch.equal(grads[k], g_ref[k])]
    assert not bad, bad[:6]
    print(f"weighted BC loss [{pol.precision}]: trainer {float(loss):.7f}, fp64 twin {loss_twin:.7f}")
    assert abs(float(loss) - loss_twin) <= 1e-5 * abs(loss_twin)


def test_padding_content_is_irrelevant(trainer_1x):
    """2b.  The last two frames of every row carry zero weight.  They are causally last (no kept frame's forward sees them) and their dz rows are
    exact zeros (exact zeros into every sum of the backward): random images and labels there -- in range in one call, -1 in the other -- change
    not one bit of the loss or of any gradient."""
    pol, cfg, sd = trainer_1x
    tr = BCTrainer(pol, train_cnn=True, optimizer_state=False)
    bt = _batch()
    w = bt["w"].clone()
    w[:, -2:] = 0.0
    w[:, 0] = 1.0
    g = torch.Generator().manual_seed(9)
    res = []
    for labels_in_range in (True, False):
        img, ab, ac = bt["img"].clone(), bt["ab"].clone(), bt["ac"].clone()
        img[:, -2:] = torch.randint(0, 256, (B, 2, 128, 128, 3), generator=g, dtype=torch.uint8).to(DEV)
        if labels_in_range:
            ab[:, -2:] = torch.randint(0, 8641, (B, 2), generator=g).to(DEV)
            ac[:, -2:] = torch.randint(0, 121, (B, 2), generator=g).to(DEV)
        else:
            ab[:, -2:], ac[:, -2:] = -1, -1
        loss, grads, _ = tr.loss_and_grads(img, bt["first"], pol.initial_state(B), ab, ac, frame_weight=w)
        torch.cuda.synchronize()
        res.append((loss.clone(), {k: v.clone() for k, v in grads.items()}))
    (l0, g0), (l1, g1) = res
    assert bool(torch.isfinite(l0)) and torch.equal(l0, l1), (l0, l1)
    bad = [k for k in g0 if not torch.equal(g0[k], g1[k])]
    assert not bad, bad[:6]
    assert all(bool(torch.isfinite(v).all()) for v in g0.values())


_DEFAULTS = {}


def _default_and_ones(trainer_1x):
    """The three calls of 2c on one batch, once per operand format."""
    pol, cfg, sd = trainer_1x
    if pol.precision not in _DEFAULTS:
        tr = BCTrainer(pol, train_cnn=True, optimizer_state=False)
        bt = _batch()
        keep = lambda r: (r[0].clone(), {k: v.clone() for k, v in r[1].items()})
        r_def = keep(tr.loss_and_grads(*_args(pol, bt)))
        r_one = keep(tr.loss_and_grads(*_args(pol, bt), frame_weight=torch.ones(B, T)))
        metrics = {}
        r_met = keep(tr.loss_and_grads(*_args(pol, bt), metrics=metrics))
        S = tr.forward_saving(bt["img"], bt["first"], pol.initial_state(B))
        _, t64 = packing.bc_loss_metrics(S["lp_b"], S["lp_c"], bt["ab"].reshape(-1), bt["ac"].reshape(-1))
        torch.cuda.synchronize()
        _DEFAULTS[pol.precision] = (r_def, r_one, r_met, metrics, float((t64[0] + t64[1]) / t64[6]))
    return _DEFAULTS[pol.precision]


def test_defaults_untouched(trainer_1x):
    """2c, gradients and metrics.  frame_weight=None, metrics=None (ops.nll_backward + gather + mean, as before) returns the gradients of
    frame_weight=ones bit for bit, and so does metrics={} alone, which fills the dict."""
    (l_def, g_def), (l_one, g_one), (l_met, g_met), metrics, _ = _default_and_ones(trainer_1x)
    bad = [k for k in g_def if not torch.equal(g_def[k], g_one[k]) or not torch.equal(g_def[k], g_met[k])]
    assert not bad, bad[:6]
    assert set(metrics) == METRIC_KEYS and all(isinstance(v, torch.Tensor) and v.is_cuda for v in metrics.values())
    assert tuple(metrics["frame_nll"].shape) == (B, T) and tuple(metrics["frame_out"].shape) == (B, T, 8)
    assert float(metrics["weight_sum"]) == B * T == float(metrics["frames"]) and torch.equal(metrics["loss"], l_met)
    assert abs(float(metrics["nll_buttons"] + metrics["nll_camera"]) - float(l_met)) < 1e-5
    assert 0.0 <= float(metrics["acc_buttons"]) <= 1.0 and 0.0 < float(metrics["entropy_camera"]) < float(np.log(121)) + 1e-3
    assert torch.equal(l_one, l_met)


def test_default_loss_equals_the_all_ones_weighted_loss(trainer_1x):
    """2c, the loss: torch.equal between the default path's loss (torch's mean over the frames of lp_b[label] + lp_c[label], negated) and the
    loss of frame_weight=ones.  Exact by construction: the weighted loss is formed from the kernel's per-frame records in the default path's own
    arithmetic (BCTrainer._record_loss) -- w x is x, the mean of the negated values is the negated mean, the factor M / sum w is 1.0.  (Read
    from the totals' fixed tree the same twelve terms land one ulp away: 13.812507629 against 13.812506676 in bf16.)"""
    (l_def, _), (l_one, _), _, _, l64 = _default_and_ones(trainer_1x)
    print(f"BC loss [{trainer_1x[0].precision}]: default path {float(l_def):.9f}, frame_weight=ones {float(l_one):.9f}, fp64 of the same log-probs {l64:.9f}")
    assert torch.equal(l_def, l_one), (float(l_def), float(l_one), l64)


def test_evaluate_is_forward_only(trainer_1x):
    """2d.  On a trainer without optimiser state; its loss against loss_and_grads' on the same batch at test_bc_gradients_vs_oracle's bound across
    forward paths (the inference forward folds its norms differently from forward_saving)."""
    pol, cfg, sd = trainer_1x
    tr = BCTrainer(pol, train_cnn=True, optimizer_state=False)
    bt = _batch()
    metrics, state_out = tr.evaluate(*_args(pol, bt), frame_weight=bt["w"])
    loss, _, state_ref = tr.loss_and_grads(*_args(pol, bt), frame_weight=bt["w"])
    torch.cuda.synchronize()
    assert set(metrics) == METRIC_KEYS
    print(f"evaluate [{pol.precision}]: loss {float(metrics['loss']):.5f}, loss_and_grads {float(loss):.5f}")
    assert abs(float(metrics["loss"]) - float(loss)) < 2e-2
    assert float(metrics["weight_sum"]) == pytest.approx(float(bt["w"].sum()), rel=1e-6) and float(metrics["frames"]) == float((bt["w"] > 0).sum())
    assert len(state_out) == len(state_ref)
    for (m0, (k0, v0)), (m1, (k1, v1)) in zip(state_out, state_ref):
        assert m0.shape == m1.shape and m0.dtype == m1.dtype and k0.shape == k1.shape and v0.shape == v1.shape and k0.dtype == k1.dtype
    m_plain, _ = tr.evaluate(*_args(pol, bt))
    assert float(m_plain["weight_sum"]) == B * T


def test_step_with_weights(trainer_1x):
    """2e.  Six weighted steps on a fixed batch lower the weighted loss (test_bc_step_reduces_loss's criterion); no fp16 step is skipped; invalid
    weights are refused before anything runs."""
    pol, cfg, sd = trainer_1x
    pol.load_state_dict(sd, strict=False)
    tr = BCTrainer(pol, lr=1e-4, weight_decay=0.0, train_cnn=True)
    bt = _batch()
    losses = []
    try:
        for _ in range(6):
            loss, _ = tr.step(*_args(pol, bt), frame_weight=bt["w"])
            losses.append(loss)
        torch.cuda.synchronize()
        for bad in (-1.0, float("nan")):
            w = bt["w"].clone()
            w[1, 2] = bad
            with pytest.raises(ValueError):
                tr.step(*_args(pol, bt), frame_weight=w)
        with pytest.raises(ValueError):
            tr.step(*_args(pol, bt), frame_weight=torch.zeros(B, T))
        assert tr.step_count == 6
    finally:
        pol.load_state_dict(sd, strict=False)
    print(f"weighted BC losses on a fixed batch [{pol.precision}]:", [round(l, 3) for l in losses])
    assert losses[-1] < losses[0] - 0.2 and all(b_ < a_ + 0.05 for a_, b_ in zip(losses, losses[1:]))
    assert tr.skipped_steps == 0


# ---------------------------------------------------------------------------------------------------------
# two ranks (gloo, both on cuda:0)
# ---------------------------------------------------------------------------------------------------------
SCALARS = sorted(METRIC_KEYS - {"frame_nll", "frame_out"})


def _dp_make():
    from vpt_amd import configs
    pol = MinecraftAgentPolicy(minecraft_action_space(), configs.policy_kwargs_for("1x"), dict(temperature=2.0), precision="bf16")
    configs.randomize_(pol, 0)
    return pol.to("cuda")


def _dp_batch():
    g = torch.Generator().manual_seed(34)
    b, t = 4, 5
    img = torch.randint(0, 256, (b, t, 128, 128, 3), generator=g, dtype=torch.uint8)
    first = torch.zeros(b, t, dtype=torch.bool)
    first[1, 0] = True
    w = torch.tensor([[1.0, 0.3, 1.0, 1.0, 0.3], [0.3, 0.3, 1.0, 0.3, 1.0], [1.0, 1.0, 1.0, 0.3, 1.0], [0.0] * 5])    # sequence 3: no weight at all
    return img, first, torch.randint(0, 8641, (b, t), generator=g), torch.randint(0, 121, (b, t), generator=g), w


def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    import __graft_entry__ as ge
    ge.build()
    from vpt_amd import distributed as D
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pol = _dp_make()
        tr = BCTrainer(pol, train_cnn=True, weight_decay=0.0)
        img, first, ab, ac, w = _dp_batch()
        b0, b1 = D.shard_range(img.shape[0], rank, world)
        sl = slice(b0, b1)
        args = lambda: (img[sl].cuda(), first[sl].cuda(), pol.initial_state(b1 - b0), ab[sl].cuda(), ac[sl].cuda())
        metrics = {}
        loss, grads, _ = tr.reduced_loss_and_grads(*args(), frame_weight=w[sl].cuda(), metrics=metrics)
        torch.cuda.synchronize()
        saved = dict(loss=float(loss), grads={k: v.cpu().clone() for k, v in grads.items()}, metrics={k: float(metrics[k]) for k in SCALARS},
                     frame_shape=tuple(metrics["frame_out"].shape))
        tr.step(*args(), frame_weight=w[sl].cuda())
        torch.cuda.synchronize()
        saved["params"] = {k: v.detach().cpu() for k, v in pol.named_parameters()}
        torch.save(saved, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_two_rank_weighted_step_matches_single_process():
    """2f.  Shards of different weight sums (one sequence without any weight): the count the ranks agree on is the global sum w, the gradients are
    bit for bit the in-process sum of the shards, the loss and the metrics are the whole batch's."""
    import torch.multiprocessing as mp
    from vpt_amd import distributed as D
    pol = _dp_make()
    tr = BCTrainer(pol, train_cnn=True, weight_decay=0.0, optimizer_state=False)
    img, first, ab, ac, w = _dp_batch()
    b = img.shape[0]
    wsum = float(w.double().sum())
    sums = [float(w[slice(*D.shard_range(b, r, 2))].double().sum()) for r in range(2)]
    assert sums[0] != sums[1] and min(sums) > 0 and float(w[3].sum()) == 0
    m1 = {}
    loss1, grads1, _ = tr.reduced_loss_and_grads(img.cuda(), first.cuda(), pol.initial_state(b), ab.cuda(), ac.cuda(), frame_weight=w.cuda(), metrics=m1)
    torch.cuda.synchronize()
    grads1 = {k: v.cpu().clone() for k, v in grads1.items()}
    shard_sum = None
    for rank in range(2):
        b0, b1 = D.shard_range(b, rank, 2)
        sl = slice(b0, b1)
        _, gs, _ = tr.loss_and_grads(img[sl].cuda(), first[sl].cuda(), pol.initial_state(b1 - b0), ab[sl].cuda(), ac[sl].cuda(), global_frames=wsum,
                                     unscaled=False, frame_weight=w[sl].cuda())
        torch.cuda.synchronize()
        gs = {k: v.cpu().clone() for k, v in gs.items()}
        shard_sum = gs if shard_sum is None else {k: shard_sum[k] + gs[k] for k in shard_sum}
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_dp_worker, args=(2, 29577, d), nprocs=2, join=True)
        r0, r1 = torch.load(os.path.join(d, "rank0.pt")), torch.load(os.path.join(d, "rank1.pt"))
    assert abs(r0["loss"] - float(loss1)) < 1e-4 and abs(r0["loss"] - r1["loss"]) < 1e-6
    errs, not_bitwise = [], []
    for k, g1 in grads1.items():
        assert torch.equal(r0["grads"][k], r1["grads"][k]), k
        if not torch.equal(r0["grads"][k].reshape(shard_sum[k].shape), shard_sum[k]):
            not_bitwise.append(k)
        if float(g1.norm()) == 0:
            continue
        errs.append((float((r0["grads"][k].reshape(g1.shape) - g1).norm() / g1.norm()), k))
    errs.sort(reverse=True)
    print(f"2-rank weighted BC gradients: bit-identical to the in-process sum of the shards on {len(grads1) - len(not_bitwise)} of {len(grads1)} tensors; "
          f"vs the whole batch worst rel-L2 {errs[0][0]:.3e} ({errs[0][1]})")
    assert not not_bitwise, not_bitwise[:6]
    assert errs[0][0] < 1e-3, errs[0]
    for k in r0["params"]:
        assert torch.equal(r0["params"][k], r1["params"][k]), k
    for r in (r0, r1):                                     # global metrics on both ranks; the per-frame records are the rank's own frames
        assert r["frame_shape"] == (2, 5, 8)
        for k in SCALARS:
            want = float(m1[k])
            assert abs(r["metrics"][k] - want) <= 1e-5 * max(1.0, abs(want)), (k, r["metrics"][k], want)
    assert r0["metrics"]["weight_sum"] == pytest.approx(wsum, rel=1e-6) and r0["metrics"]["frames"] == 15.0
