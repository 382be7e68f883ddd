"""vpt_rl_loss_kernel (ops.rl_loss) on the GPU against the gate-pinned fp64 reference tests/rl_loss_ref.py with derived bounds, bit for bit against
vpt_bc_loss_kernel where the two must coincide, zero-weight rows, reproducibility, the optional inputs.  Needs an MI355X.  Shapes: the real heads
(5 x 8641 + 121: 34 sweeps of the workgroup, rows that are not 16-byte aligned, the value column, ldz = 8768) and 300 x 70 + 11 (more than 256 rows:
the slab sum's second slice; heads shorter than a workgroup)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from tests import rl_loss_ref as R  # noqa: E402

DEV = "cuda"
SHAPES = {"heads": (5, 8641, 121, 8768), "small": (300, 70, 11, 128)}
COEF = dict(kl_coef=0.3, entropy_coef=0.02, value_coef=0.5)
ZERO = dict(kl_coef=0.0, entropy_coef=0.0, value_coef=0.0)
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
_CASES = {}


def _case(shape, nan_rows=True):
    """Seeded inputs of one shape (built once per variant), on the device; the raw value sits in the last column of a [M, nb + nc + 1] buffer, as in
    the trainer (the kernel reads it through a row stride)."""
    key = (shape, nan_rows)
    if key not in _CASES:
        m, nb, nc, ldz = SHAPES[shape]
        c = R.make_case(m, nb, nc, nan_rows=nan_rows)
        g = {k: c[k].to(DEV) for k in ("lb", "lc", "qb", "qc", "ab", "ac", "old", "adv", "target", "vnorm", "w")}
        buf = torch.full((m, nb + nc + 1), float("nan"), device=DEV)
        buf[:, nb + nc] = c["value"].to(DEV)
        g["value"] = buf[:, nb + nc]
        _CASES[key] = (c, g, ldz)
    return _CASES[key]


def _run(g, ldz, dtype=torch.bfloat16, scale=None, prior=True, value=True, temperature=None, c=None, **kw):
    opts = dict(clip=c["clip"], temperature=c["temperature"] if temperature is None else temperature, dtype=dtype, weight=g["w"])
    opts.update(kw)
    return ops.rl_loss(g["lb"], g["lc"], g["ab"], g["ac"], opts.pop("old", g["old"]), opts.pop("adv", g["adv"]), ldz,
                       c["scale"] if scale is None else scale, prior_buttons=g["qb"] if prior else None, prior_camera=g["qc"] if prior else None,
                       value=g["value"] if value else None, value_target=g["target"] if value else None, vnorm=g["vnorm"] if value else None, **opts)


def _device_expf_error(c, frame_out):
    """The largest relative error (in u = 2^-24) of the DEVICE's expf over the arguments this test hands it -- every finite log-prob of the live rows
    and every lp - old_lp -- measured through the kernel itself: with one class per head, lp_camera = 0 and old_log_prob = 0, slot 6 of the record
    is expf(argument)."""
    live = c["w"] != 0
    lp = frame_out[:, 8].cpu()
    args = torch.cat([c["lb"][live].reshape(-1), c["lc"][live].reshape(-1), (lp - c["old"])[live]])
    args = args[torch.isfinite(args)].contiguous()
    n = args.numel()
    z = torch.zeros(n, device=DEV)
    zi = torch.zeros(n, dtype=torch.int64, device=DEV)
    _, fo, _ = ops.rl_loss(args.to(DEV).reshape(n, 1), z.reshape(n, 1), zi, zi, z, torch.ones(n, device=DEV), 0, 1.0, want_dz=False, want_totals=False)
    torch.cuda.synchronize()
    return R.exp_rel_error_u(args.double(), fo[:, 6].cpu())


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_outputs_against_the_fp64_reference_with_the_kernels_own_clip_flags(shape, fmt):
    """(a)  dz, frame_out and totals inside the bounds derived in tests/rl_loss_ref.py (the device's expf error measured over this test's own
    arguments and doubled); max err / bound is printed per quantity.  Wrong references -- the KL the other way round, K left out of the gradient, the
    value gradient one column to the left -- are far outside."""
    c, g, ldz = _case(shape)
    dz, frame_out, totals = _run(g, ldz, DT[fmt], c=c, **COEF)
    torch.cuda.synchronize()
    m, nb, nc = c["m"], c["nb"], c["nc"]
    assert dz.dtype == DT[fmt] and tuple(dz.shape) == (m, ldz) and tuple(frame_out.shape) == (m, 16) and tuple(totals.shape) == (16,)
    live = c["w"] != 0
    clipped = frame_out[:, 7].cpu().bool() & live
    exact, rho, dist = R.exact_clip_flags(c)
    assert float(dist.min()) > 1e-3 and torch.equal(clipped, exact)             # inputs away from 1 +- clip: the recorded flags are the exact rule's
    measured = _device_expf_error(c, frame_out)
    ref = R.reference(c, clipped, e_exp=2 * measured, **COEF)
    rt = R.ratios(dz, frame_out, totals, ref, fmt)
    print(f"rl_loss[{shape}, {fmt}] device expf: largest relative error {measured:.3f} u over the test's arguments (bound used: twice that)")
    print(f"rl_loss[{shape}, {fmt}] max err / bound: {rt}")
    assert rt.pop("dz_pad") == 0.0                                               # columns beyond nb + nc + 1
    assert all(v <= 1.0 for v in rt.values()), rt
    assert float(dz[~live.to(DEV)].float().abs().max()) == 0.0 and not bool(torch.isnan(dz.float()).any())
    assert bool(torch.isfinite(totals).all()) and float(totals[11]) == float(live.sum()) and float(totals[12:].abs().max()) == 0.0
    assert float(frame_out[:, 12:][live.to(DEV)].abs().max()) == 0.0
    for mut in ("kl_swap", "no_K", "value_left"):
        bad = R.ratios(dz, frame_out, totals, R.reference(c, clipped, e_exp=2 * measured, mutate=mut, **COEF), fmt)
        print(f"    mutated reference {mut}: dz err / bound {bad['dz']:.1f}")
        assert bad["dz"] > 50.0, (mut, bad)


@pytest.mark.parametrize("temperature", [1.0, 2.0])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_policy_columns_equal_bc_loss_bit_for_bit(shape, fmt, temperature):
    """(b)  kl_coef = entropy_coef = value_coef = 0, advantage = 1, old_log_prob = a previous call's recorded lp (rho = expf(0) = 1 exactly):
    c = -1 and dz[:, :nb + nc] is vpt_bc_loss_kernel's dz at the same scale and weight (temperature 1; at temperature 2 the BC kernel, whose caller
    folds 1 / T into the scale, is given scale / 2 -- a power of two, exact)."""
    c, g, ldz = _case(shape)
    nbc = c["nb"] + c["nc"]
    ones = torch.ones(c["m"], device=DEV)
    _, f0, _ = _run(g, ldz, DT[fmt], c=c, temperature=temperature, adv=ones, want_dz=False, want_totals=False, **ZERO)
    dz, f1, _ = _run(g, ldz, DT[fmt], c=c, temperature=temperature, adv=ones, old=f0[:, 8].contiguous(), want_totals=False, **ZERO)
    ref, _, _ = ops.bc_loss(g["lb"], g["lc"], g["ab"], g["ac"], ldz, c["scale"] / temperature, weight=g["w"], dtype=DT[fmt], want_frames=False,
                            want_totals=False)
    torch.cuda.synchronize()
    live = (c["w"] != 0).to(DEV)
    assert bool((f1[:, 6][live] == 1.0).all()) and bool((f1[:, 7][live] == 0.0).all())
    assert torch.equal(dz[:, :nbc], ref[:, :nbc])
    assert float(dz[:, nbc:].float().abs().max()) == 0.0 and float(ref[live][:, :nbc].float().abs().max()) > 0.0


def test_zero_weight_rows_with_garbage_change_nothing():
    """(c)  NaN in the log-probs, the prior, the advantage and the target of the w = 0 rows (one in the middle, one last): exact zeros in their dz
    rows, and totals that equal, bit for bit, those of the same call with clean values in those rows."""
    for shape in SHAPES:
        (c, g, ldz), (c0, g0, _) = _case(shape, True), _case(shape, False)
        dead = (c["w"] == 0).to(DEV)
        assert int(dead.sum()) >= 1 and bool(torch.isnan(g["lb"][dead]).all()) and bool(torch.isnan(g["qb"][dead]).all())
        assert bool(torch.isnan(g["adv"][dead]).all()) and bool(torch.isnan(g["target"][dead]).all()) and bool(torch.isfinite(g0["lb"][dead]).any())
        dz, fo, totals = _run(g, ldz, c=c, **COEF)
        dz0, fo0, totals0 = _run(g0, ldz, c=c0, **COEF)
        torch.cuda.synchronize()
        assert float(dz[dead].float().abs().max()) == 0.0 and not bool(torch.isnan(dz.float()).any())
        assert bool(torch.isfinite(totals).all()) and torch.equal(totals, totals0)
        assert torch.equal(dz, dz0) and torch.equal(fo[~dead], fo0[~dead])


def test_same_call_same_bits():
    """(d)  No atomics anywhere: ten runs, one result, on all three outputs."""
    for shape in SHAPES:
        c, g, ldz = _case(shape, False)
        first = None
        for _ in range(10):
            out = _run(g, ldz, c=c, **COEF)
            torch.cuda.synchronize()
            if first is None:
                first = out
            else:
                assert all(torch.equal(a, b) for a, b in zip(out, first))


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_optional_inputs(fmt):
    """(e)  prior = NULL equals kl_coef = 0 with a prior supplied: dz bit for bit, and every record / total except the two KL slots, which the
    call with a prior still fills (the KL metric of a run that does not penalise it) and the call without leaves 0.  value = NULL leaves the value
    column and the value slot 0 and changes nothing else.  weight = NULL is weight = ones."""
    c, g, ldz = _case("small", False)
    nbc = c["nb"] + c["nc"]
    coef = dict(COEF, kl_coef=0.0)
    dz_n, fo_n, t_n = _run(g, ldz, DT[fmt], c=c, prior=False, **coef)
    dz_p, fo_p, t_p = _run(g, ldz, DT[fmt], c=c, prior=True, **coef)
    dz_v, fo_v, t_v = _run(g, ldz, DT[fmt], c=c, value=False, **COEF)
    dz_f, fo_f, t_f = _run(g, ldz, DT[fmt], c=c, **COEF)
    dz_w, fo_w, t_w = _run(g, ldz, DT[fmt], c=c, weight=None, **COEF)
    dz_1, fo_1, t_1 = _run(g, ldz, DT[fmt], c=c, weight=torch.ones_like(g["w"]), **COEF)
    torch.cuda.synchronize()
    keep = [k for k in range(16) if k not in (1, 2)]
    assert torch.equal(dz_n, dz_p) and torch.equal(fo_n[:, keep], fo_p[:, keep]) and torch.equal(t_n[keep], t_p[keep])
    assert float(fo_n[:, 1:3].abs().max()) == 0.0 and float(t_n[1:3].abs().max()) == 0.0 and float(t_p[1]) > 0.0 and float(t_p[2]) > 0.0
    assert float(dz_v[:, nbc].float().abs().max()) == 0.0 and float(fo_v[:, 5].abs().max()) == 0.0 and float(t_v[5]) == 0.0
    assert float(dz_f[:, nbc].float().abs().max()) > 0.0
    keep = [k for k in range(16) if k != 5]
    assert torch.equal(dz_v[:, :nbc], dz_f[:, :nbc]) and torch.equal(fo_v[:, keep], fo_f[:, keep]) and torch.equal(t_v[keep], t_f[keep])
    assert torch.equal(dz_w, dz_1) and torch.equal(fo_w, fo_1) and torch.equal(t_w, t_1)


def test_validation_errors():
    c, g, ldz = _case("small", False)
    with pytest.raises(RuntimeError, match="ldz"):
        _run(g, c["nb"] + c["nc"], c=c, **COEF)                                   # no room for the value column
    with pytest.raises(ValueError, match="both"):
        ops.rl_loss(g["lb"], g["lc"], g["ab"], g["ac"], g["old"], g["adv"], ldz, 1.0, prior_buttons=g["qb"])
    with pytest.raises(ValueError, match="rows"):
        ops.rl_loss(g["lb"], g["lc"], g["ab"][:5].contiguous(), g["ac"], g["old"], g["adv"], ldz, 1.0)
    with pytest.raises(ValueError, match="value_target"):
        ops.rl_loss(g["lb"], g["lc"], g["ab"], g["ac"], g["old"], g["adv"], ldz, 1.0, value=g["value"])
