"""The low-rank adapter kernels and GEMM compositions on an MI355X, both operand formats:
vpt_lowrank_merge_kernel bit-equal to its float32 numpy restatement and inside the fp64 bound; trainer_base.adapted_linear /
adapted_linear_backward in isolation, on every epilogue combination the trunk uses, held to the two instruments of tests/lowrank_ref.py -- THE
exact result on integer operands, and the derived two-stage bound on real values -- plus the B = 0 anchor (bit-equal to ops.linear) and two
mutated references (s left out; the fused projection's off-diagonal blocks kept) that must sit at least 100 x outside the bound."""
import functools
import itertools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from vpt_amd.trainer_base import _round_up, adapted_linear, adapted_linear_backward, linear_backward, stack_operands, unstack_gradients  # noqa: E402
from tests import lowrank_ref as R  # noqa: E402

DEV = "cuda"
D = torch.float64
FMTS = ["bf16", "fp16"]
SHAPES = list(itertools.product((5, 70, 300), (64, 192), (136, 256), (1, 4, 16)))          # (M, K, n, r)
FUSED = (70, 64, 256, 24)            # q, k, v adapted with r = 24 (72 -> R = 128: crosses one 64-wide step), r_layer not; hid = 64

#            bias   relu   res    mask   f32    16-bit  padded 16-bit stride
FORWARD = {"bias+skip": (True, False, True, False, True, False, False),        # proj / mlp1 (the fused projection: bias alone)
           "relu16": (False, True, False, False, False, True, False)}          # mlp0
DGRAD = {"gate16": (False, False, False, True, False, True, True),             # mlp1's dgrad through mlp0's ReLU gate, 16-bit, padded row stride
         "skip": (False, False, True, False, True, False, False)}              # the fused projection's dgrad + the skip
EPILOGUES = dict(FORWARD, **DGRAD)


# ---- the merge -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(1, 1), (3, 5), (130, 257)])
@pytest.mark.parametrize("r", [1, 16, 64])
def test_merge_equals_its_numpy_restatement_and_meets_the_fp64_bound(n, k, r):
    g = torch.Generator().manual_seed(100 * n + k + r)
    w = torch.randn(n, k, generator=g)
    a = (torch.rand(r, k, generator=g) * 2 - 1) / math.sqrt(k)
    b = torch.randn(n, r, generator=g)
    for s in (16.0 / r, 0.3):
        out = ops.lowrank_merge(w.to(DEV), a.to(DEV), b.to(DEV), s).cpu()
        want = torch.from_numpy(R.merge_f32(w.numpy(), a.numpy(), b.numpy(), s))
        assert torch.equal(out, want), f"(n, K, r, s) = {(n, k, r, s)}: {int((out != want).sum())} of {out.numel()} elements differ from the float32 restatement"
        out64, bnd = R.merge_ref(w.numpy(), a.numpy(), b.numpy(), s)
        worst, msg = R.bound_ratio(out, out64, bnd)
        assert msg is None, msg
    wd = w.to(DEV)
    assert ops.lowrank_merge(wd, a.to(DEV), b.to(DEV), 0.3, out=wd) is wd and torch.equal(wd.cpu(), want)          # in place
    with pytest.raises(ValueError):
        ops.lowrank_merge(w.to(DEV), a.to(DEV), b[:, :0].contiguous().to(DEV), 1.0)


# ---- one adapted GEMM: operands --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(kind, fmt, m, k, n, r, fused=False):
    """Operands of one adapted linear on both sides, computed once and never modified.  kind "int": x, A in {-1, +1}, B, W, dy, bias, res from
    linear_ref.ints, s a power of two; "real": randn rounded to the format (W ~ K^-1/2, A ~ U(-K^-1/2, K^-1/2), B ~ N(0, 1/4)), s = 8 / r or 0.5."""
    g = torch.Generator().manual_seed(m + 3 * n + 7 * k + 11 * r + (0 if kind == "int" else 1))
    dt = R.DT[fmt]
    np_ = _round_up(n, 64)
    blocks = [(i * 64, 64) for i in range(3)] if fused else [(0, n)]
    if kind == "int":
        s = 0.5 if r == 4 else 2.0
        x, w, dy = R.signs(g, m, k), R.ints(g, n, k), R.ints(g, m, n)
        As, Bs = [R.signs(g, r, k) for _ in blocks], [R.ints(g, ni, r) for _, ni in blocks]
        bias, res_n, res_k, mask_k = R.ints(g, n), R.ints(g, m, n), R.ints(g, m, k), R.ints(g, m, k)
    else:
        s = 0.5 if fused else 8.0 / r
        x, w, dy = R.reals(g, fmt, m, k).float(), R.reals(g, fmt, n, k, scale=k ** -0.5).float(), R.reals(g, fmt, m, n).float()
        As = [(torch.rand(r, k, generator=g) * 2 - 1) * k ** -0.5 for _ in blocks]
        Bs = [torch.randn(ni, r, generator=g) * 0.5 for _, ni in blocks]
        bias, res_n, res_k, mask_k = torch.randn(n, generator=g), torch.randn(m, n, generator=g), torch.randn(m, k, generator=g), torch.randn(m, k, generator=g)
    a_stack, sb, spans = stack_operands([(a, b, s, row0) for a, b, (row0, _) in zip(As, Bs, blocks)], n, k)
    dyp = torch.zeros(m, np_)
    dyp[:, :n] = dy
    mask16 = mask_k.to(dt)
    c = dict(kind=kind, fmt=fmt, dt=dt, m=m, k=k, n=n, r=r, np=np_, s=s, spans=spans, As=As, Bs=Bs, blocks=blocks,
             x=x, w=w, dy=dyp, a_stack=a_stack, sb=sb, bias=bias, res_n=res_n, res_k=res_k, mask_k=mask16,
             a16=R.rnd16(a_stack, fmt), sb16=R.rnd16(sb, fmt), w16=R.rnd16(w, fmt))
    c.update(X=x.to(dt).to(DEV), W=w.to(DEV), WPK=ops.pack_linear(w.to(DEV), dtype=dt), DY=dyp.to(dt).to(DEV), A=a_stack.to(DEV), SB=sb.to(DEV),
             BIAS=bias.to(DEV), RES_N=res_n.to(DEV), RES_K=res_k.to(DEV), MASK_K=mask16.to(DEV))
    return c


def _forward(c, row, sb=None):
    bias, relu, res, mask, f32, b16, _ = row
    o32, o16, u16 = adapted_linear(c["X"], c["WPK"], c["n"], c["A"], c["SB"] if sb is None else sb, bias=c["BIAS"] if bias else None,
                                   res=c["RES_N"] if res else None, relu=relu, out_f32=f32, out_bf16=b16)
    torch.cuda.synchronize()
    return (o32.cpu() if o32 is not None else None), (o16.cpu() if o16 is not None else None), u16


def _forward_ref(c, row, sb16=None):
    bias, relu, res, _, _, _, _ = row
    return R.adapted_ref(c["x"], c["w16"], c["a16"], c["sb16"] if sb16 is None else sb16, c["fmt"], bias=c["bias"] if bias else None, relu=relu,
                         res=c["res_n"] if res else None)


def _backward(c, row, u16):
    _, _, res, mask, f32, b16, padded = row
    ld = (c["k"] + 64 if padded else c["k"]) if b16 else None
    dx32, dx16, dw, da, db = adapted_linear_backward(c["DY"], c["n"], c["X"], c["W"], c["A"], c["SB"], u16, res=c["RES_K"] if res else None,
                                                     mask=c["MASK_K"] if mask else None, dx_f32=f32, dx_bf16_ld=ld)
    torch.cuda.synchronize()
    assert dw is None          # a frozen adapted weight launches no [n, K] wgrad GEMM
    return (dx32.cpu() if dx32 is not None else None), (dx16.cpu() if dx16 is not None else None), da.cpu(), db.cpu()


def _backward_ref(c, row, du16_exact=None):
    """dx of one dgrad row as an adapted linear over (dy, W^T, (sB)^T, A^T): stage one is du = dy (sB)."""
    _, _, res, mask, _, _, _ = row
    wt = torch.zeros(c["k"], c["np"], dtype=D)
    wt[:, :c["n"]] = c["w16"].t()
    sbt = torch.zeros(c["sb16"].shape[1], c["np"], dtype=D)
    sbt[:, :c["n"]] = c["sb16"].t()
    return R.adapted_ref(c["dy"], wt, sbt, c["a16"].t(), c["fmt"], mask=c["mask_k"] if mask else None, res=c["res_k"] if res else None)


# ---- the exact-integer instrument ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(EPILOGUES))
def test_adapted_linear_is_exact_on_integers(fmt, name):
    row, fails = EPILOGUES[name], []
    for m, k, n, r in SHAPES + [FUSED]:
        c = _case("int", fmt, m, k, n, r, fused=(m, k, n, r) == FUSED)
        what = f"{name} (M, K, n, r) = {(m, k, n, r)} {fmt}"
        u = c["x"].to(D) @ c["a16"].t()                       # |u| <= K <= 256: exact in both formats
        o32, o16, u16 = _forward(c, FORWARD.get(name, FORWARD["bias+skip"]))
        fails.append(R.exact_failure(u16.cpu(), u, what + " u16"))
        if name in FORWARD:
            y = _forward_ref(c, row)[0]
            fails += [R.exact_failure(o, y, what) for o in (o32, o16) if o is not None]
            assert (o32 is not None) == row[4] and (o16 is not None) == row[5]
            continue
        dx32, dx16, da, db = _backward(c, row, u16)
        dy, x = c["dy"].to(D), c["x"].to(D)
        du16 = R.rnd16(dy[:, :c["n"]] @ c["sb16"], fmt)       # the ONE rounding of the exact du; everything after it is exact again
        fails.append(R.exact_failure(da, du16.t() @ x, what + " d a_stack"))
        fails.append(R.exact_failure(db, dy[:, :c["n"]].t() @ u, what + " dy^T u16"))
        dx = dy[:, :c["n"]] @ c["w16"] + du16 @ c["a16"]
        if row[3]:
            dx = torch.where(c["mask_k"].to(D) > 0, dx, torch.zeros_like(dx))
        if row[2]:
            dx = dx + c["res_k"].to(D)
        if dx32 is not None:
            fails.append(R.exact_failure(dx32, dx, what + " dx"))
        if dx16 is not None:
            fails.append(R.exact_failure(dx16[:, :k], dx, what + " dx16"))
            if dx16.shape[1] != k + 64 or bool(dx16[:, k:].any()):
                fails.append(what + f": the padded columns of dx16 {tuple(dx16.shape)} must exist and be zero")
    fails = [f for f in fails if f]
    assert not fails, "\n".join(fails[:8])


# ---- real values under the derived bound -----------------------------------------------------------------------------------------------------------
def _ratio(fails, out, y64, bnd, what):
    worst, msg = R.bound_ratio(out, y64, bnd)
    if msg:
        fails.append(f"{what}: {msg}")
    return worst


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(EPILOGUES))
def test_adapted_linear_meets_the_two_stage_bound(fmt, name):
    row, fails, worst = EPILOGUES[name], [], 0.0
    for m, k, n, r in SHAPES + [FUSED]:
        c = _case("real", fmt, m, k, n, r, fused=(m, k, n, r) == FUSED)
        what = f"{name} (M, K, n, r) = {(m, k, n, r)} {fmt}"
        o32, o16, u16 = _forward(c, FORWARD.get(name, FORWARD["bias+skip"]))
        if name in FORWARD:
            y, bnd, u64, du = _forward_ref(c, row)
            worst = max(worst, _ratio(fails, u16.cpu(), u64, du, what + " u16"))
            if o32 is not None:
                worst = max(worst, _ratio(fails, o32, y, bnd, what))
            if o16 is not None:
                worst = max(worst, _ratio(fails, o16, y, bnd + R.ulp16(y, fmt), what + " 16-bit"))
            continue
        dx32, dx16, da, db = _backward(c, row, u16)
        dx, bnd, du64, ddu = _backward_ref(c, row)
        if dx32 is not None:
            worst = max(worst, _ratio(fails, dx32, dx, bnd, what + " dx"))
        if dx16 is not None:
            worst = max(worst, _ratio(fails, dx16[:, :k], dx, bnd + R.ulp16(dx, fmt), what + " dx16"))
            if bool(dx16[:, k:].any()):
                fails.append(what + ": padded columns of dx16 not zero")
        da64, da_b = R.da_ref(du64, ddu, c["x"])
        worst = max(worst, _ratio(fails, da, da64, da_b, what + " d a_stack"))
        u64, du = R.stage_one(c["x"].to(D), c["a16"], 1, fmt)
        db64, db_b = R.db_ref(c["dy"], u64, du, c["n"])
        worst = max(worst, _ratio(fails, db, db64, db_b, what + " dy^T u16"))
    print(f"{name} {fmt}: worst error / bound = {worst:.3f}")
    assert not fails, "\n".join(fails[:8])


@pytest.mark.parametrize("fmt", FMTS)
def test_zero_b_is_the_unadapted_linear_bit_for_bit(fmt):
    """The anchor: with B = 0 the extra slice is exact zeros -- forward and dgrad equal ops.linear / linear_backward on every epilogue row, at the
    weight-streaming kernel's row count (5) and the MFMA GEMM's (70, 300)."""
    for m, k, n, r in [(5, 64, 136, 4), (70, 192, 256, 16), (300, 192, 136, 1)]:
        c = _case("real", fmt, m, k, n, r)
        zero = torch.zeros_like(c["SB"])
        for name, row in FORWARD.items():
            bias, relu, res, _, f32, b16, _ = row
            o32, o16, u16 = _forward(c, row, sb=zero)
            p32, p16 = ops.linear(c["X"], c["WPK"], n, bias=c["BIAS"] if bias else None, res=c["RES_N"] if res else None, relu=relu, out_f32=f32, out_bf16=b16)
            for got, want in ((o32, p32), (o16, p16)):
                assert (got is None) == (want is None) and (got is None or torch.equal(got, want.cpu())), (name, m, k, n, r)
        for name, row in DGRAD.items():
            _, _, res, mask, f32, b16, padded = row
            ld = (k + 64 if padded else k) if b16 else None
            kw = dict(res=c["RES_K"] if res else None, mask=c["MASK_K"] if mask else None, dx_f32=f32, dx_bf16_ld=ld)
            d32, d16, _, da, db = adapted_linear_backward(c["DY"], n, c["X"], c["W"], c["A"], zero, u16, **kw)
            q32, q16, _ = linear_backward(c["DY"], n, c["X"], c["W"], need_dw=False, **kw)
            for got, want in ((d32, q32), (d16, q16)):
                assert (got is None) == (want is None) and (got is None or torch.equal(got, want)), (name, m, k, n, r)
            assert not bool(da.any())            # du16 = dy (s 0) = 0: every dA is exact zeros


@pytest.mark.parametrize("fmt", FMTS)
def test_mutated_references_sit_far_outside_the_bound(fmt):
    """The fused case (three adapters, r = 24, s = 0.5): a reference with s left out, and one with the off-diagonal blocks of sB kept (every
    layer's B applied to every layer's u), each at least 100 x outside the bound that the kernels meet -- forward and dB."""
    m, k, n, r = FUSED
    c = _case("real", fmt, m, k, n, r, fused=True)
    row = FORWARD["bias+skip"]
    o32, _, u16 = _forward(c, row)
    y, bnd, u64, du = _forward_ref(c, row)
    assert R.bound_ratio(o32, y, bnd)[1] is None
    no_s = R.rnd16(c["sb"] / c["s"], fmt)
    dense = torch.zeros_like(c["sb"])
    for (row0, ni, _, _), b in zip(c["spans"], c["Bs"]):
        for (_, _, c0, rr) in c["spans"]:
            dense[row0:row0 + ni, c0:c0 + rr] = b * c["s"]
    for what, sb16 in (("s left out", no_s), ("off-diagonal blocks kept", R.rnd16(dense, fmt))):
        ym, bm, _, _ = _forward_ref(c, row, sb16=sb16)
        worst = R.bound_ratio(o32, ym, bnd)[0]
        print(f"forward, {what} ({fmt}): {worst:.0f} x the bound")
        assert worst >= 100.0, (what, worst)
    # dB: s times the diagonal blocks of dy^T u16; without s, or taken from an off-diagonal block, it is another tensor
    _, _, da, db = _backward(c, DGRAD["skip"], u16)
    db64, db_b = R.db_ref(c["dy"], u64, du, n)
    pieces = unstack_gradients(da, db, c["spans"])
    for i, ((row0, ni, c0, rr), (_, dbi)) in enumerate(zip(c["spans"], pieces)):
        got = dbi * c["s"]
        want, bnd_i = c["s"] * db64[row0:row0 + ni, c0:c0 + rr], c["s"] * db_b[row0:row0 + ni, c0:c0 + rr] + R.U32 * (c["s"] * db64[row0:row0 + ni, c0:c0 + rr]).abs()
        assert R.bound_ratio(got, want, bnd_i)[1] is None
        assert R.bound_ratio(dbi, want, bnd_i)[0] >= 100.0                                  # s left out
        j = (i + 1) % 3
        off = db[row0:row0 + ni, c["spans"][j][2]:c["spans"][j][2] + rr] * c["s"]
        assert R.bound_ratio(off, want, bnd_i)[0] >= 100.0                                  # an off-diagonal block taken for the diagonal one
