"""vpt_logsoftmax_kernel<4|16>, vpt_nll_bwd_kernel, vpt_bc_loss_kernel (dz, nll, entropies), vpt_heads_bwd_kernel and vpt_act_epilogue_kernel against the
fp64 reference of tests/action_head_ref.py under its derived per-element bounds, through vpt_amd.ops.  Needs an MI355X.  The log-softmax shapes are the
smallest that reach each path: the launch rule's edges (M 63 | 64, n 1024 | 1025), the register / tail edge of each wave count (n 2304 | 2305, 9216 | 9217),
the training head (65 x 8641 of a 8763-wide row) and the camera head at col0 = 8641; T = 1.7, logits of spread 12 with one row shifted by +80 and one by
-80.  Selected indices are compared exactly: tests/test_action_head_ref_cpu.py asserts that every row of these cases wins by more than twice the score
bound.  Every check prints `max err / bound`."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from tests import action_head_ref as R  # noqa: E402

DEV = "cuda"
RATIOS = {}
LSM = [(label, c) for label, c in R.lsm_cases() if not label.startswith("tie")]


def _note(res):
    for k, v in res.items():
        RATIOS[k] = max(RATIOS.get(k, 0.0), v)


def _dev(t):
    return t.to(DEV) if t is not None else None


def _same_bits(a, b):
    """Tuples of tensors (or None) equal bit for bit (NaN == NaN)."""
    return all((x is None and y is None) or torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def _head_forward(c, z=None, noise=None, rng=None):
    """-> (lp, action | None, action_logp | None) on the device."""
    z = _dev(c.z) if z is None else z
    if c.act == "none":
        return ops.log_softmax_cols(z, c.col0, c.n, c.T, mask=_dev(c.mask)), None, None
    return ops.log_softmax_cols(z, c.col0, c.n, c.T, mask=_dev(c.mask), noise=noise, want_action=True, rng=rng)


def _check_head(label, c, got):
    """lp under its bound, the selected indices the reference's, action_logp bit-equal to lp[row, action]."""
    o = R.compute(c)
    lp, ac, alp = got
    w, msg = R.check("lp", lp.cpu(), o.lp, o.b_lp)
    print(f"log_softmax {label}: NW {c.nw}, max err / bound: lp {w:.4f}")
    _note({f"log_softmax NW {c.nw} lp": w})
    assert msg is None, f"{label}: {msg}"
    if c.act != "none":
        assert ac.dtype == torch.int64 and torch.equal(ac.cpu(), o.action), f"{label}: rows {(ac.cpu() != o.action).nonzero()[:, 0].tolist()} select another index"
        assert _same_bits((alp,), (lp.gather(1, ac[:, None])[:, 0],)), f"{label}: action_logp is not lp[row, action]"


@pytest.mark.parametrize("i", range(len(LSM)), ids=[label.replace(" ", "_") for label, _ in LSM])
def test_log_softmax_action_head(i):
    label, c = LSM[i]
    z = _dev(c.z)
    if label.endswith("action rng"):
        # the in-kernel draw: bit-equal to the noise path fed the same uniforms, which are the host restatement's (so the CPU test's margin holds for them)
        st = ops.new_rng_state(DEV, seed=R.RNG_SEED)
        st[1] = R.RNG_STEP
        got = _head_forward(c, z, rng=(st, R.RNG_STREAM))
        u = ops.uniform_noise(st, R.RNG_STREAM, c.M, c.n)
        again = _head_forward(c, z, noise=u)
        torch.cuda.synchronize()
        assert torch.equal(u.cpu(), c.noise) and int(st[1]) == R.RNG_STEP
        assert _same_bits(got, again), f"{label}: the in-kernel draw and the noise path differ"
    else:
        got = _head_forward(c, z, noise=_dev(c.noise))
        again = _head_forward(c, z, noise=_dev(c.noise))
        torch.cuda.synchronize()
        assert _same_bits(got, again), f"{label}: the same call twice gives other bits"
    _check_head(label, c, got)


@pytest.mark.parametrize("name,m,n,i,j", R.TIES, ids=[t[0].replace(" ", "_") for t in R.TIES])
def test_ties_take_the_first_maximum(name, m, n, i, j):
    for higher_wins in (False, True):
        c = R.tie_case(m, n, i, j, higher_wins)
        got = _head_forward(c)
        torch.cuda.synchronize()
        want = j if higher_wins else i
        assert bool((got[1] == want).all()), f"{name}: columns {i} and {j}{' (the higher one a step above)' if higher_wins else ' equal'}: selected {got[1].tolist()}, expected {want}"
        _check_head(f"tie: {name}", c, got)


def _dz_check(name, fmt, label, dz, o, c, res, fails):
    key = f"{name} dz {fmt}"
    res[key], msg = R.check(key, dz.cpu(), o.dz, R.bound16(o.dz, o.b_dz, fmt))
    fails += [f"{label}: {msg}"] if msg else []
    if not R.bit_zero(dz[:, c.nb + c.nc + (1 if name == "heads" else 0):]):
        fails.append(f"{label}: {key}: a padding column is not +0")


@pytest.mark.parametrize("m", R.HEAD_ROWS)
@pytest.mark.parametrize("nb,nc,ldz", R.HEAD_SHAPES)
def test_nll_backward_and_bc_loss(nb, nc, ldz, m):
    fails = []
    for v in ((0, 1, 2) if m == 1 else (0,)):
        c = R.head_case(m, nb, nc, ldz, variant=v)
        label = f"nb {nb} nc {nc} ldz {ldz} M {m} labels {v}"
        lb, lc, ab, ac, w = _dev(c.lp_b), _dev(c.lp_c), _dev(c.act_b), _dev(c.act_c), _dev(c.weight)
        on, ob = R.compute(c, kind="nll"), R.compute(c, kind="bc")
        res = {}
        for fmt in ("bf16", "fp16"):
            dz = ops.nll_backward(lb, lc, ab, ac, ldz, c.scale, dtype=R.DT[fmt])
            dz2 = ops.nll_backward(lb, lc, ab, ac, ldz, c.scale, dtype=R.DT[fmt])
            bdz, frames, _ = ops.bc_loss(lb, lc, ab, ac, ldz, c.scale, weight=w, dtype=R.DT[fmt])
            bdz2, frames2, _ = ops.bc_loss(lb, lc, ab, ac, ldz, c.scale, weight=w, dtype=R.DT[fmt])
            torch.cuda.synchronize()
            assert dz.dtype == R.DT[fmt] and torch.equal(dz.view(torch.int16), dz2.view(torch.int16)) and torch.equal(bdz.view(torch.int16), bdz2.view(torch.int16))
            assert _same_bits((frames,), (frames2,))
            _dz_check("nll", fmt, label, dz, on, c, res, fails)
            _dz_check("bc", fmt, label, bdz, ob, c, res, fails)
            res["bc ent"], msg = R.check("bc ent", frames[:, 2:4].cpu(), ob.ent, ob.b_ent)
            fails += [f"{label}: {msg}"] if msg else []
            if not torch.equal(frames[:, 0:2].cpu().double(), ob.nll):
                fails.append(f"{label}: bc nll is not -lp[label] exactly")
            if not torch.equal(frames[:, 6].cpu(), c.weight):
                fails.append(f"{label}: the frame record's weight")
        print(f"nll / bc_loss {label}: max err / bound: " + "  ".join(f"{k} {x:.4f}" for k, x in res.items()))
        _note(res)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("m", R.HEAD_ROWS)
@pytest.mark.parametrize("nb,nc,ldz", R.HEAD_SHAPES)
def test_heads_backward(nb, nc, ldz, m):
    fails = []
    for gs, drop, mask in R.HEADS_CONFIGS:
        c = R.head_case(m, nb, nc, ldz, mask=mask, grad_scale=gs, drop=drop)
        label = f"nb {nb} nc {nc} ldz {ldz} M {m} grad_scale {gs} None {drop} mask {mask}"
        o = R.compute(c, kind="heads")
        args = (_dev(c.lp_b), _dev(c.lp_c), _dev(c.g_b), _dev(c.g_c), _dev(c.g_v), ldz, c.T)
        res = {}
        for fmt in ("bf16", "fp16"):
            kw = dict(mask_buttons=_dev(c.mask_b), mask_camera=_dev(c.mask_c), dtype=R.DT[fmt], grad_scale=gs)
            dz, dz2 = ops.heads_logprob_backward(*args, **kw), ops.heads_logprob_backward(*args, **kw)
            torch.cuda.synchronize()
            assert dz.dtype == R.DT[fmt] and torch.equal(dz.view(torch.int16), dz2.view(torch.int16))
            _dz_check("heads", fmt, label, dz, o, c, res, fails)
            for g, sl in ((c.g_b, slice(0, nb)), (c.g_c, slice(nb, nb + nc)), (c.g_v, slice(nb + nc, nb + nc + 1))):
                if g is None and not R.bit_zero(dz[:, sl]):
                    fails.append(f"{label}: {fmt}: the block of a None gradient is not +0")
            for mk, off in ((c.mask_b, 0), (c.mask_c, nb)):
                if mk is not None and not R.bit_zero(dz[:, off:off + mk.shape[1]][_dev(mk) == 0]):
                    fails.append(f"{label}: {fmt}: a masked element is not +0")
        print(f"heads_backward {label}: max err / bound: " + "  ".join(f"{k} {x:.4f}" for k, x in res.items()))
        _note(res)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("m", [1, 5, 64])
def test_act_epilogue_is_exact(m):
    c = R.act_case(m)
    o = R.compute(c)
    ab, ac, lb, lc, logits = _dev(c.act_b), _dev(c.act_c), _dev(c.lp_b), _dev(c.lp_c), _dev(c.logits)
    st = ops.new_rng_state(DEV, seed=5)
    keep, flag = ops.act_epilogue(ab, ac, lb, lc, logits, c.vcol, c.scale, c.shift, rng_state=st)
    keep2, flag2 = ops.act_epilogue(ab, ac, lb, lc, logits, c.vcol, c.scale, c.shift)
    torch.cuda.synchronize()
    assert st.tolist() == [5, 1], "one launch advances the step counter by exactly one"
    assert torch.equal(keep, keep2) and int(flag) == 0 and int(flag2) == 0
    b2, c2, lp, vd, v = (t.cpu() for t in ops.unpack_act_keep(keep))
    assert torch.equal(b2, c.act_b) and torch.equal(c2, c.act_c)
    assert _same_bits((lp, vd, v), (o.log_prob, o.vpred, o.vraw)), (lp, o.log_prob, vd, o.vpred)
    assert bool((keep.cpu()[:, 2] >> 32 == 0).all())
    for launch in range(2):
        ops.act_epilogue(ab, ac, lb, lc, logits, c.vcol, c.scale, c.shift, rng_state=st)
    assert st.tolist() == [5, 3]
    for row in sorted({0, m // 2, m - 1}):
        for which in (0, 1):
            bad = [lb.clone(), lc.clone()]
            bad[which][row] = float("nan")
            _, flag = ops.act_epilogue(ab, ac, bad[0], bad[1], logits, c.vcol, c.scale, c.shift)
            assert int(flag) == 1, f"a NaN log-prob in row {row} of {m} does not set the flag"
    assert st.tolist() == [5, 3], "a launch without rng_state leaves the counter alone"
    _note({"act_epilogue (exact: differing elements)": 0.0})


@pytest.mark.parametrize("shape", [(3, 65, 65, 0), (64, 2305, 2305, 0)], ids=["registers", "tail"])
def test_a_nan_logit_selects_index_zero_and_reports_nan(shape):
    """One NaN logit makes the row's every score NaN: the action is 0 (torch.argmax of an all-NaN row), action_logp NaN (vpt_act_epilogue's flag reports it)
    and every other row keeps the bits of a call without the NaN."""
    c = R.lsm_case(*shape, act="det")
    clean = _head_forward(c)
    row = 1
    c.z[row, c.col0 + c.n // 2] = float("nan")
    lp, ac, alp = _head_forward(c)
    torch.cuda.synchronize()
    assert int(ac[row]) == 0 and math.isnan(float(alp[row])) and bool(torch.isnan(lp[row]).all())
    others = [r for r in range(c.M) if r != row]
    assert _same_bits(tuple(t[others] for t in (lp, ac, alp)), tuple(t[others] for t in clean))
    assert bool(((ac >= 0) & (ac < c.n)).all())


def test_a_noise_row_of_zeros_selects_index_zero():
    """-log(0) = inf: every score of the row is -inf, none compares greater than the start value: index 0 (torch.argmax of an all--inf row), finite log-probs."""
    c = R.lsm_case(64, 2305, act="noise")
    c.noise[2] = 0.0
    lp, ac, alp = _head_forward(c, noise=_dev(c.noise))
    torch.cuda.synchronize()
    assert int(ac[2]) == 0 and bool(torch.isfinite(alp).all()) and bool(torch.isfinite(lp).all())
    assert _same_bits((alp,), (lp.gather(1, ac[:, None])[:, 0],))
    o = R.compute(c)
    rows = [r for r in range(c.M) if r != 2]
    assert torch.equal(ac.cpu()[rows], o.action[rows])


def test_print_worst_ratios():
    """Not a check: the table profiles/action_head_fp64_ratios.md quotes (run the module with -s)."""
    for key in sorted(RATIOS):
        print("worst err / bound: action head", key, f"{RATIOS[key]:.4f}")
