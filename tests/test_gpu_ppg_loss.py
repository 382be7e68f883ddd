"""vpt_ppg_aux_loss_kernel (ops.ppg_aux_loss) on the GPU against the fp64 reference tests/ppg_loss_ref.py with derived bounds, bit for bit against
vpt_rl_loss_kernel where the two must coincide, the identity teacher, zero-weight rows, reproducibility, the optional inputs.  Needs an MI355X.
Shapes: the real heads (5 x 8641 + 121: 34 sweeps of the workgroup, rows that are not 16-byte aligned, ldz = 8768), 300 x 70 + 11 (more than 256
rows: the slab sum's second slice; heads narrower than a workgroup and than a wave) and 1 x 1 + 1 (one-class heads, one row)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from tests import ppg_loss_ref as R  # noqa: E402

DEV = "cuda"
SHAPES = {"heads": (5, 8641, 121, 8768), "small": (300, 70, 11, 128), "one": (1, 1, 1, 64)}
COEF = dict(clone_coef=0.7, value_coef=0.5)
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
_CASES = {}
_EXPF = {}


def _case(shape, temperature=2.0, nan_rows=True):
    """Seeded inputs of one shape (built once per variant), on the device; the raw value sits in the last column of a [M, nb + nc + 1] buffer, as in
    the trainer (the kernel reads it through a row stride)."""
    key = (shape, temperature, nan_rows)
    if key not in _CASES:
        m, nb, nc, ldz = SHAPES[shape]
        c = R.make_case(m, nb, nc, temperature=temperature, nan_rows=nan_rows)
        g = {k: c[k].to(DEV) for k in ("lb", "lc", "mb", "mc", "target", "vnorm", "w")}
        buf = torch.full((m, nb + nc + 1), float("nan"), device=DEV)
        buf[:, nb + nc] = c["value"].to(DEV)
        g["value"] = buf[:, nb + nc]
        _CASES[key] = (c, g, ldz)
    return _CASES[key]


def _run(g, ldz, c, dtype=torch.bfloat16, value=True, **kw):
    opts = dict(temperature=c["temperature"], dtype=dtype, weight=g["w"])
    opts.update(kw)
    return ops.ppg_aux_loss(g["lb"], g["lc"], opts.pop("mb", g["mb"]), opts.pop("mc", g["mc"]), ldz, opts.pop("scale", c["scale"]),
                            value=g["value"] if value else None, value_target=g["target"] if value else None, vnorm=g["vnorm"] if value else None, **opts)


def _device_expf_error(key, c):
    """The largest relative error (in u = 2^-24) of the DEVICE's expf over the arguments this test hands it -- every finite log-prob of the policy
    and of the teacher on the live rows -- measured through the kernel itself: a head with one class makes S (slot 3 of the record) equal to
    expf(m_0).  Once per case."""
    if key not in _EXPF:
        args = R.exp_arguments(c)
        n = args.numel()
        z = torch.zeros(n, 1, device=DEV)
        _, fo, _ = ops.ppg_aux_loss(z, z, args.to(DEV).reshape(n, 1), z, 0, 1.0, want_dz=False, want_totals=False)
        torch.cuda.synchronize()
        _EXPF[key] = R.exp_rel_error_u(args.double(), fo[:, 3].cpu())
    return _EXPF[key]


@pytest.mark.parametrize("temperature", [1.0, 2.0])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_outputs_against_the_fp64_reference(shape, fmt, temperature):
    """(a)  dz, frame_out and totals inside the bounds derived in tests/ppg_loss_ref.py (the device's expf error measured over this test's own
    arguments and doubled); max err / bound is printed per quantity.  Wrong references -- the KL the other way round, 1 / T left out, the value
    gradient one column to the left -- fail the same assertion wherever they are another reference at all: a one-class head has p = o = 1 and no
    policy gradient either way, and at T = 1 there is no 1 / T to leave out (those mutants are asserted to BE the reference there)."""
    c, g, ldz = _case(shape, temperature)
    dz, frame_out, totals = _run(g, ldz, c, DT[fmt], **COEF)
    torch.cuda.synchronize()
    m, nb, nc = c["m"], c["nb"], c["nc"]
    assert dz.dtype == DT[fmt] and tuple(dz.shape) == (m, ldz) and tuple(frame_out.shape) == (m, 8) and tuple(totals.shape) == (8,)
    live = c["w"] != 0
    measured = _device_expf_error((shape, temperature), c)
    ref = R.reference(c, e_exp=2 * measured, **COEF)
    rt = R.ratios(dz, frame_out, totals, ref, fmt)
    print(f"ppg_aux_loss[{shape}, {fmt}, T={temperature}] device expf: largest relative error {measured:.3f} u over the test's arguments (bound used: twice that)")
    print(f"ppg_aux_loss[{shape}, {fmt}, T={temperature}] max err / bound: {rt}")
    assert rt.pop("dz_pad") == 0.0                                               # columns beyond nb + nc + 1
    assert all(v <= 1.0 for v in rt.values()), rt
    if int((~live).sum()):
        assert float(dz[~live.to(DEV)].float().abs().max()) == 0.0
    assert not bool(torch.isnan(dz.float()).any())
    assert bool(torch.isfinite(totals).all()) and float(totals[6]) == float(live.sum()) and float(totals[7]) == 0.0
    assert float(frame_out[:, 7][live.to(DEV)].abs().max()) == 0.0
    if shape != "one":
        assert 0.05 < float(totals[0] / totals[5]) < 5.0 and 0.05 < float(totals[1] / totals[5]) < 5.0        # D is of order 1
    failed = []
    for mut in R.MUTATIONS:
        bad_ref = R.reference(c, e_exp=2 * measured, mutate=mut, **COEF)
        if torch.equal(bad_ref["dz"], ref["dz"]):
            continue
        bad = R.ratios(dz, frame_out, totals, bad_ref, fmt)
        print(f"    mutated reference {mut}: dz err / bound {bad['dz']:.1f}")
        bad.pop("dz_pad")
        assert not all(v <= 1.0 for v in bad.values()), (mut, bad)
        assert not bad["dz"] <= 1.0, (mut, bad)
        failed.append(mut)
    assert failed == (["value_left"] if shape == "one" else [mu for mu in R.MUTATIONS if mu != "no_temp" or temperature != 1.0]), failed


@pytest.mark.parametrize("temperature", [1.0, 2.0])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_hot_teacher_is_the_bc_anchor_of_rl_loss_bit_for_bit(shape, fmt, temperature):
    """(b)  A one-hot teacher (m = 0 at the label, -inf elsewhere), clone_coef = 1, no value: the policy columns are ops.rl_loss's in its BC-anchor
    configuration (kl_coef = entropy_coef = value_coef = 0, A = 1, old_log_prob = its own recorded lp, rho = 1), torch.equal; D_b and D_c are the
    negated log-probs of the labels, exactly, and their fp32 sum is that kernel's -lp."""
    c, g, ldz = _case(shape, temperature, nan_rows=False)
    m, nb, nc = c["m"], c["nb"], c["nc"]
    gen = torch.Generator().manual_seed(5)
    ab, ac = torch.randint(0, nb, (m,), generator=gen).to(DEV), torch.randint(0, nc, (m,), generator=gen).to(DEV)
    if m > 2:
        ab[2], ac[2] = 0, 0                                                      # row 2 has classes of probability 0: keep the label on a live one
    mb, mc = torch.full((m, nb), -float("inf"), device=DEV), torch.full((m, nc), -float("inf"), device=DEV)
    mb[torch.arange(m), ab], mc[torch.arange(m), ac] = 0.0, 0.0
    ones, zeros = torch.ones(m, device=DEV), torch.zeros(m, device=DEV)
    rl = dict(weight=g["w"], clip=0.2, kl_coef=0.0, entropy_coef=0.0, value_coef=0.0, temperature=temperature, dtype=DT[fmt], want_totals=False)
    _, f0, _ = ops.rl_loss(g["lb"], g["lc"], ab, ac, zeros, ones, ldz, c["scale"], want_dz=False, **rl)
    ref, f1, _ = ops.rl_loss(g["lb"], g["lc"], ab, ac, f0[:, 8].contiguous(), ones, ldz, c["scale"], **rl)
    dz, fo, _ = _run(g, ldz, c, DT[fmt], value=False, mb=mb, mc=mc, clone_coef=1.0, temperature=temperature, want_totals=False)
    torch.cuda.synchronize()
    live = (c["w"] != 0).to(DEV)
    assert bool((f1[:, 6][live] == 1.0).all()) and bool((f1[:, 7][live] == 0.0).all())
    assert torch.equal(dz[:, :nb + nc], ref[:, :nb + nc])
    assert float(dz[:, nb + nc:].float().abs().max()) == 0.0
    if shape != "one":
        assert float(ref[live][:, :nb + nc].float().abs().max()) > 0.0
    assert torch.equal(fo[:, 0], -g["lb"].gather(1, ab[:, None])[:, 0]) and torch.equal(fo[:, 1], -g["lc"].gather(1, ac[:, None])[:, 0])
    assert torch.equal(fo[:, 0] + fo[:, 1], -f1[:, 8])
    assert bool((fo[:, 3] == 1.0).all()) and bool((fo[:, 4] == 1.0).all())          # the one-hot teacher's mass


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_policy_as_its_own_teacher_gives_exact_zeros(shape, fmt):
    """(c)  old = the same tensors as lp: D_b = D_c = 0 exactly and the policy columns of dz are exact zeros (the value column is not)."""
    c, g, ldz = _case(shape, nan_rows=False)
    nbc = c["nb"] + c["nc"]
    dz, fo, totals = _run(g, ldz, c, DT[fmt], mb=g["lb"], mc=g["lc"], **COEF)
    torch.cuda.synchronize()
    assert float(fo[:, :2].abs().max()) == 0.0 and float(totals[:2].abs().max()) == 0.0
    assert float(dz[:, :nbc].float().abs().max()) == 0.0 and float(dz[:, nbc].float().abs().max()) > 0.0
    assert float((fo[:, 3:5] - 1.0).abs().max()) < 1e-4


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_zero_weight_rows_with_garbage_change_nothing(fmt):
    """(d)  NaN in the log-probs, the teacher, the value and the target of the w = 0 rows (the last row; with 300 rows many in the middle too): exact
    zeros in their dz rows, and totals that equal, bit for bit, those of the same call with clean values in those rows."""
    for shape, n_dead in (("heads", 1), ("small", 40)):
        (c, g, ldz), (c0, g0, _) = _case(shape, 2.0, True), _case(shape, 2.0, False)
        dead = (c["w"] == 0).to(DEV)
        assert int(dead.sum()) >= n_dead and bool(torch.isnan(g["lb"][dead]).all()) and bool(torch.isnan(g["mb"][dead]).all())
        assert bool(torch.isnan(g["value"][dead]).all()) and bool(torch.isnan(g["target"][dead]).all()) and bool(torch.isfinite(g0["lb"][dead]).any())
        dz, fo, totals = _run(g, ldz, c, DT[fmt], **COEF)
        dz0, fo0, totals0 = _run(g0, ldz, c0, DT[fmt], **COEF)
        torch.cuda.synchronize()
        assert float(dz[dead].float().abs().max()) == 0.0 and not bool(torch.isnan(dz.float()).any())
        assert bool(torch.isfinite(totals).all()) and torch.equal(totals, totals0)
        assert torch.equal(dz, dz0) and torch.equal(fo[~dead], fo0[~dead])


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_same_call_same_bits(fmt):
    """(e)  No atomics anywhere: ten runs, one result, on all three outputs."""
    for shape in SHAPES:
        c, g, ldz = _case(shape, 2.0, False)
        first = None
        for _ in range(10):
            out = _run(g, ldz, c, DT[fmt], **COEF)
            torch.cuda.synchronize()
            if first is None:
                first = out
            else:
                assert all(torch.equal(a, b) for a, b in zip(out, first))


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_optional_inputs(fmt):
    """(f)  value = None leaves the value column and the value slot 0 and changes nothing else; clone_coef = 0 leaves the policy columns 0, the value
    column and every record unchanged; want_dz = False still fills the records; weight = None is weight = ones; 65537 rows with totals are refused
    before any launch."""
    c, g, ldz = _case("small", 2.0, False)
    nbc = c["nb"] + c["nc"]
    dz_f, fo_f, t_f = _run(g, ldz, c, DT[fmt], **COEF)
    dz_v, fo_v, t_v = _run(g, ldz, c, DT[fmt], value=False, **COEF)
    dz_0, fo_0, t_0 = _run(g, ldz, c, DT[fmt], **dict(COEF, clone_coef=0.0))
    dz_c, fo_c, t_c = _run(g, ldz, c, DT[fmt], **dict(COEF, value_coef=0.0))
    none, fo_n, t_n = _run(g, ldz, c, DT[fmt], want_dz=False, **COEF)
    dz_w, fo_w, t_w = _run(g, ldz, c, DT[fmt], weight=None, **COEF)
    dz_1, fo_1, t_1 = _run(g, ldz, c, DT[fmt], weight=torch.ones_like(g["w"]), **COEF)
    only_dz = _run(g, ldz, c, DT[fmt], want_frames=False, want_totals=False, **COEF)
    torch.cuda.synchronize()
    keep = [k for k in range(8) if k != 2]
    assert float(dz_v[:, nbc].float().abs().max()) == 0.0 and float(fo_v[:, 2].abs().max()) == 0.0 and float(t_v[2]) == 0.0
    assert float(dz_f[:, nbc].float().abs().max()) > 0.0 and float(t_f[2]) > 0.0
    assert torch.equal(dz_v[:, :nbc], dz_f[:, :nbc]) and torch.equal(fo_v[:, keep], fo_f[:, keep]) and torch.equal(t_v[keep], t_f[keep])
    assert float(dz_0[:, :nbc].float().abs().max()) == 0.0 and float(dz_f[:, :nbc].float().abs().max()) > 0.0
    assert torch.equal(dz_0[:, nbc:], dz_f[:, nbc:]) and torch.equal(fo_0, fo_f) and torch.equal(t_0, t_f)
    assert float(dz_c[:, nbc:].float().abs().max()) == 0.0 and torch.equal(dz_c[:, :nbc], dz_f[:, :nbc]) and torch.equal(fo_c, fo_f)
    assert none is None and torch.equal(fo_n, fo_f) and torch.equal(t_n, t_f)
    assert torch.equal(dz_w, dz_1) and torch.equal(fo_w, fo_1) and torch.equal(t_w, t_1)
    assert only_dz[1] is None and only_dz[2] is None and torch.equal(only_dz[0], dz_f)
    big = torch.zeros(65537, 1, device=DEV)
    with pytest.raises(RuntimeError, match="65536"):
        ops.ppg_aux_loss(big, big, big, big, 64, 1.0, dtype=DT[fmt])
    torch.cuda.synchronize()


def test_validation_errors():
    c, g, ldz = _case("small", 2.0, False)
    with pytest.raises(RuntimeError, match="ldz"):
        _run(g, c["nb"] + c["nc"], c, **COEF)                                     # no room for the value column
    with pytest.raises(ValueError, match="old_buttons and old_camera"):
        ops.ppg_aux_loss(g["lb"], g["lc"], g["mb"], None, ldz, 1.0)
    with pytest.raises(ValueError, match="shapes"):
        ops.ppg_aux_loss(g["lb"], g["lc"], g["mb"][:, :5].contiguous(), g["mc"], ldz, 1.0)
    with pytest.raises(ValueError, match="rows"):
        ops.ppg_aux_loss(g["lb"], g["lc"], g["mb"], g["mc"], ldz, 1.0, weight=g["w"][:5].contiguous())
    with pytest.raises(ValueError, match="value_target"):
        ops.ppg_aux_loss(g["lb"], g["lc"], g["mb"], g["mc"], ldz, 1.0, value=g["value"])
    with pytest.raises(ValueError, match="temperature"):
        ops.ppg_aux_loss(g["lb"], g["lc"], g["mb"], g["mc"], ldz, 1.0, temperature=0.0)
