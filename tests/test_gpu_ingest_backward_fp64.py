"""The backward of the ingest side -- vpt_conv_first_bwd_kernel<false / true>, vpt_affine_bwd_reduce / apply / elem_kernel, vpt_pool_bwd_kernel -- held per
element to the fp64 references and derived bounds of tests/ingest_backward_ref.py (its docstring has the derivations and the counted summation lengths;
tests/test_ingest_backward_ref_cpu.py pins them on the CPU).  Both operand formats.  Needs an MI355X.

conv_first   Operands for which the never-stored pre-pool tensor is known exactly on the CPU (weights k 2^-12, bias j 2^-14 - 2: every fp32 partial sum is
             exact), so the forward must reproduce the pooled tensor BIT FOR BIT and the arg-max routing, ties included, is determined.  Blocky images (one byte
             triple per 4 x 4 block: over a quarter of the windows are live AND tied, every window offset wins) and random ones; integer gradients (db exact;
             dW exact on the one-tile launch) and real ones.  16 x 16 x 128 (one tile, one slab row), 3 x 48 x 80 x 160 (two channel tiles, the second partial),
             2 x 16 x 48 x 32 (one valid wave) and the PERSISTENT case: 48 x 80 frames in a number that follows from the device's CU count, so that the launch
             has more tiles than its 2 workgroups per CU, the working workgroups sweep two tiles, ranges begin inside frames and some workgroups get no tile.
             Plain and NFOLD (pool_stats / pool_ab computed on the CPU from the exact pooled tensor: the kernel is judged alone), `out=`, two calls.
frame_affine 16 pixels (most lanes idle), 60 (clamped duplicates), 1600 (two pixel chunks), 300 slab rows (two vpt_slab_sum slices); per element with one
             frame slice and with eight of which the last two are empty.  With and without dx_add and pre-filled dgain / dbias; integer dy with power-of-two
             gains (dbias and ab[:, 0] exact); a constant frame.
max-pool     few-level inputs with plateaus and all-zero windows: bit for bit against the kernel's own fp32 order; the forward's arg-max codes agree.

Every check prints `worst err / bound`; test_print_worst_ratios prints the table.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops, packing  # noqa: E402
from tests import ingest_backward_ref as B  # noqa: E402
from tests import ingest_ref as R  # noqa: E402

DEV = "cuda"
D = torch.float64
FMTS = ["bf16", "fp16"]
WORST = {}


def _bits(t):
    return t.contiguous().view(torch.int16)


def _blocked(t64, fmt):
    return packing.nchw_to_blocked(t64.float(), dtype=R.DT[fmt]).to(DEV)


def _check(got, ref, bound, what, group):
    """Every element against its bound; the worst ratio goes to the table under `group`."""
    worst, msg = R.failure(got.detach().cpu().to(D), ref, bound, what)
    print(f"{what}: worst err / bound {worst:.3f}")
    WORST[group] = max(WORST.get(group, 0.0), worst)
    assert msg is None, msg


def _leaves(got, ref, bound):
    return bool((R.ratio(got.detach().cpu().to(D), ref, bound) > 1.0).any())


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- conv_first ---------------------------------------------------------------------------------------------------------------------------------------------
def _conv_first_operands(c, fmt):
    return c["img"].to(DEV), packing.pack_conv_first(c["weight"], c["bias"], dtype=R.DT[fmt]).to(DEV)


def _nfold_dev(c):
    gain, st, ab = c["nfold"]
    return gain.to(DEV), st.to(DEV), ab.to(DEV)


def _check_conv_first_backward(c, fmt, style, what):
    img, wf = _conv_first_operands(c, fmt)
    cout, n = c["cout"], c["n"]
    rows = B.slab_rows(c["frames"], c["h"], c["w"], _cus())
    # the forward reproduces the exact pooled tensor: round-to-nearest-even of an exact fp32 sum, the premise of everything below
    st = torch.zeros(c["frames"], 2, dtype=D, device=DEV)
    y = ops.conv_first(img, wf, cout, stats_out=st)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y.cpu()), _bits(packing.nchw_to_blocked(c["pooled"].float(), dtype=R.DT[fmt]))), f"{what}: the forward is not the exact pooled tensor"
    sums, mags = R.frame_sums(c["pooled"])
    _check(st, sums, R.sum_bound(R.N_ADD_CONV_FIRST_STATS, mags), f"{what} forward stats_out", "conv_first forward stats_out")
    dp = _blocked(c["d"], fmt)
    for key, nfold in (("plain", None), ("folded", _nfold_dev(c))):
        ref = c[key]
        b_dw, b_db = B.conv_first_backward_bounds(ref, n, rows)
        dw, db = ops.conv_first_backward(img, wf, dp, cout, nfold=nfold)
        torch.cuda.synchronize()
        _check(dw, ref["dW"], b_dw, f"{what} {key} dW", f"conv_first backward {key} dW")
        _check(db, ref["db"], b_db, f"{what} {key} db", f"conv_first backward {key} db")
        if style[1] == "int" and key == "plain":
            assert bool((ref["db_abs"] < B.EXACT_LIMIT).all())
            assert torch.equal(db.cpu(), ref["db"].float()), f"{what}: db of integer gradients is not exact"
            if rows == 1:
                assert torch.equal(dw.cpu(), B.dw_exact_one_tile(ref)), f"{what}: dW of the one-tile launch is not fl32(S * fl32(1 / 255))"
        # two calls, the same bits
        dw2, db2 = ops.conv_first_backward(img, wf, dp, cout, nfold=nfold)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), f"{what} {key}: two calls differ"
        # out=: accumulation onto what the destination holds
        g = torch.Generator().manual_seed(5)
        dw0, db0 = torch.randn(cout, 27, generator=g), torch.randn(cout, generator=g)
        out = (dw0.to(DEV), db0.to(DEV))
        ops.conv_first_backward(img, wf, dp, cout, out=out, nfold=nfold)
        torch.cuda.synchronize()
        b_dw, b_db = B.conv_first_backward_bounds(ref, n, rows, prior=(dw0.to(D), db0.to(D)))
        _check(out[0], dw0.to(D) + ref["dW"], b_dw, f"{what} {key} dW out=", f"conv_first backward {key} dW")
        _check(out[1], db0.to(D) + ref["db"], b_db, f"{what} {key} db out=", f"conv_first backward {key} db")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("style", B.STYLES, ids=lambda s: "-".join(s))
@pytest.mark.parametrize("name", list(B.CONV_FIRST_BWD_CASES))
def test_conv_first_backward_fp64(name, style, fmt):
    c = B.conv_first_bwd_case(*B.CONV_FIRST_BWD_CASES[name], fmt, *style)
    _check_conv_first_backward(c, fmt, style, f"conv_first backward {name} {'-'.join(style)} {fmt}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("style", B.STYLES, ids=lambda s: "-".join(s))
def test_conv_first_backward_persistent_loop_fp64(style, fmt):
    """More tiles than the grid of two workgroups per CU: T = 15 * frames > grid, so the working workgroups sweep ceil(T / grid) = 2 consecutive tiles; 2 does
    not divide a frame's 15, so ranges begin inside frames and cross from one frame into the next; ceil(T / 2) < grid, so the last workgroups get no tile and
    write zero slab rows.  Asserted, not assumed: on a device where the conditions cannot hold the test fails."""
    cus = _cus()
    frames, tiles, grid = B.persistent_backward_frames(cus)
    per = -(-tiles // grid)
    working = -(-tiles // per)
    print(f"conv_first backward persistent {fmt}: {cus} CUs, grid {grid}, {frames} frames, T = {tiles} tiles, {per} per workgroup, {working} working workgroups")
    assert tiles > grid and per >= 2 and 15 % per != 0 and working < grid, (cus, frames, tiles, grid, per, working)
    c = B.conv_first_bwd_case(frames, *B.PERSISTENT_BWD_HW_COUT, fmt, *style)
    _check_conv_first_backward(c, fmt, style, f"conv_first backward persistent {'-'.join(style)} {fmt}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["one_tile", "nt2_partial"])
def test_conv_first_backward_mutated_reference_leaves_the_bound(name, fmt):
    """The kernel must NOT agree with a reference that takes the last maximum, lets a zero maximum pass its gradient, drops window offset 8, exchanges the two
    pooled-row pairs of a half tile, or (NFOLD) swaps A and B."""
    c = B.conv_first_bwd_case(*B.CONV_FIRST_BWD_CASES[name], fmt, "blocky", "real")
    img, wf = _conv_first_operands(c, fmt)
    rows = B.slab_rows(c["frames"], c["h"], c["w"], _cus())
    dp = _blocked(c["d"], fmt)
    plain = ops.conv_first_backward(img, wf, dp, c["cout"])
    fold = ops.conv_first_backward(img, wf, dp, c["cout"], nfold=_nfold_dev(c))
    torch.cuda.synchronize()
    for mutate in B.MUTATIONS + ("swap_ab",):
        folded = mutate == "swap_ab"
        mut = B.conv_first_backward_ref(c["img"], c["w16"], c["bh"], c["bl"], c["d"], fmt, nfold=c["nfold"] if folded else None, mutate=mutate)
        b_dw, b_db = B.conv_first_backward_bounds(mut, c["n"], rows)
        dw, db = fold if folded else plain
        r = max(float(R.ratio(dw.cpu().to(D), mut["dW"], b_dw).max()), float(R.ratio(db.cpu().to(D), mut["db"], b_db).max()))
        print(f"conv_first backward {name} {fmt}: err / bound against the `{mutate}` reference {r:.3g}")
        assert r > 1, f"the kernel agrees with the `{mutate}` reference"


# ---- frame_affine -------------------------------------------------------------------------------------------------------------------------------------------
def _vec(v, c):
    """A per-channel or per-element (C,H,W order) vector in the order the kernels index it."""
    return packing.chw_to_blocked_vector(v, c["c"], c["h"], c["w"]) if c["per_element"] else v


def _run_affine(c, fmt, with_add):
    n = c["gain"].numel()
    if with_add:
        dgain, dbias = _vec(c["prior"][0], c).to(DEV), _vec(c["prior"][1], c).to(DEV)
    else:
        dgain, dbias = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    dx = ops.frame_affine_backward(_blocked(c["x"], fmt), _blocked(c["dy"], fmt), _vec(c["gain"], c).to(DEV), c["stats_in"].to(DEV), dgain, dbias,
                                   per_element=c["per_element"], dx_add=_blocked(c["dx_add"], fmt) if with_add else None)
    torch.cuda.synchronize()
    return packing.blocked_to_nchw(dx.cpu(), c["c"], c["h"], c["w"]).to(D), dgain.cpu(), dbias.cpu()


def _check_affine(c, fmt, what):
    for key, with_add in (("plain", False), ("added", True)):
        r = c[key]
        dx, dgain, dbias = _run_affine(c, fmt, with_add)
        _check(dx, r["dx"], r["b_dx"], f"{what} {key} dx", "frame_affine backward dx")
        _check(dgain, _vec(r["dgain"], c), _vec(r["b_dgain"], c), f"{what} {key} dgain", "frame_affine backward dgain")
        _check(dbias, _vec(r["dbias"], c), _vec(r["b_dbias"], c), f"{what} {key} dbias", "frame_affine backward dbias")
        dx2, dgain2, dbias2 = _run_affine(c, fmt, with_add)
        assert torch.equal(dx, dx2) and torch.equal(dgain, dgain2) and torch.equal(dbias, dbias2), f"{what} {key}: two calls differ"
    if not c["per_element"]:
        n = c["gain"].numel()
        dgain, dbias = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        ab = ops.frame_affine_backward_reduce(_blocked(c["x"], fmt), _blocked(c["dy"], fmt), c["gain"].to(DEV), c["stats_in"].to(DEV), dgain, dbias)
        torch.cuda.synchronize()
        _check(ab, c["plain"]["ab"], c["plain"]["b_ab"], f"{what} ab", "frame_affine backward ab")
        return ab.cpu(), dbias.cpu()
    return None, _run_affine(c, fmt, False)[2]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("kind", ["real", "constant"])
@pytest.mark.parametrize("name", list(B.AFFINE_BWD_CASES))
def test_frame_affine_backward_fp64(name, kind, fmt):
    _check_affine(B.affine_bwd_case(name, fmt, kind), fmt, f"frame_affine backward {name} {kind} {fmt}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(B.AFFINE_BWD_CASES))
def test_frame_affine_backward_exact_sums(name, fmt):
    """Integer dy, gains in {1/2, 1, 2}: every partial sum of dbias and of ab[:, 0] is exact in fp32 (conditions asserted on the reference), so both are BIT exact
    in whatever order the kernel adds; everything else is held to its bound."""
    c = B.affine_bwd_case(name, fmt, "exact")
    r = c["plain"]
    assert bool((r["abs_dy"] < B.EXACT_LIMIT).all()) and bool((2.0 * r["abs_dyg"] < B.EXACT_LIMIT).all())
    ab, dbias = _check_affine(c, fmt, f"frame_affine backward {name} exact {fmt}")
    assert torch.equal(dbias.to(D), _vec(r["dbias"], c)), "dbias of integer gradients is not exact"
    if ab is not None:
        assert torch.equal(ab[:, 0], r["ab"][:, 0]), "ab[:, 0] of integer gradients and power-of-two gains is not exact"


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["clamped", "elem_partial"])
def test_frame_affine_backward_mutated_reference_leaves_the_bound(name, fmt):
    c = B.affine_bwd_case(name, fmt, "real")
    dx, _, _ = _run_affine(c, fmt, True)
    for mutate in ("no_add", "gain_octet", "swap_ab"):
        mut = B.affine_backward_ref(c["x"], c["dy"], c["gain"], c["stats_in"], fmt, c["per_element"], dx_add=c["dx_add"], prior=c["prior"], mutate=mutate)
        r = float(R.ratio(dx, mut["dx"], mut["b_dx"]).max())
        print(f"frame_affine backward {name} {fmt}: err / bound against the `{mutate}` reference {r:.3g}")
        assert r > 1, f"the kernel agrees with the `{mutate}` reference"


# ---- max-pool -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("i", range(len(B.POOL_CASES)))
def test_maxpool_backward_bit_exact(i, fmt):
    c = B.pool_case(i, fmt)
    pre = _blocked(c["pre"], fmt)
    pooled, am = ops.maxpool(pre, want_argmax=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(pooled.cpu()), _bits(packing.nchw_to_blocked(c["pooled"].float(), dtype=R.DT[fmt])))
    am = packing.blocked_to_nchw(am.cpu(), c["c"], c["h"] // 2, c["w"] // 2).long()
    live = c["pooled"] > 0
    assert torch.equal(am[live], c["argmax"][live]), "the forward's arg-max codes differ from the first maximum in scan order"
    assert bool((am[~live] == 15).all()), "an all-zero window does not carry code 15"
    dpre = ops.maxpool_backward(pre, pooled, _blocked(c["d"], fmt))
    torch.cuda.synchronize()
    got = packing.blocked_to_nchw(dpre.cpu(), c["c"], c["h"], c["w"]).to(R.DT[fmt])
    same = _bits(got) == _bits(c["dpre"])
    WORST["max-pool backward (share of elements that differ)"] = max(WORST.get("max-pool backward (share of elements that differ)", 0.0), 1.0 - same.double().mean().item())
    assert bool(same.all()), f"{int((~same).sum())} of {same.numel()} elements differ; first at {tuple((~same).nonzero()[0].tolist())}"


def test_print_worst_ratios():
    print("\nworst err / bound over every check of this file")
    for k in sorted(WORST):
        print(f"  {k:60s} {WORST[k]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
