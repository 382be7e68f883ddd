"""tests/ingest_backward_ref.py is the gradient, plain fp32 arithmetic meets its bounds, and its cases are what they claim to be -- shown on the CPU, before a
GPU sees any of it (tests/test_gpu_ingest_backward_fp64.py is the GPU half).

a. Every reference equals fp64 autograd on the same rounded operands to 1e-9: conv -> ReLU -> max_pool2d for conv_first (plain, and behind oracle
   group_norm_1 for the NFOLD chain), oracle group_norm_1 / layer_norm for frame_affine (both gain kinds, dx_add), max_pool2d for the pool.
b. A plain fp32 evaluation of each formula (torch fp32, torch's own summation order) lies inside every bound.
c. The case conditions hold on the reference alone: exact operands, sums below 2^24 units, the shares of live / tied windows and of every window offset in the
   blocky cases, integer-gradient sums below 2^24 wherever the GPU test demands bit equality, all-zero windows and plateaus in the pool cases.
d. The mutated references differ from the true one by more than the bound somewhere (a mutation nothing can see would prove nothing on the GPU).
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import vpt_oracle as O
from tests import ingest_backward_ref as B
from tests import ingest_ref as R
from tests.cnn_backward_ref import maxpool_backward_ref

D = torch.float64
FMTS = ["bf16", "fp16"]
CUS = 256                                   # the slab-row count of the bounds here; the GPU test takes the device's
SMALL = ["one_tile", "one_wave"]            # every style of these runs here in a second; nt2_partial once


def _close(a, b, what=""):
    assert bool(((a - b).abs() <= 1e-9 * b.abs().max().clamp(min=1e-300)).all()), f"{what}: {(a - b).abs().max().item():.3e} against {b.abs().max().item():.3e}"


def _inside(y, y64, bound, what):
    worst, msg = R.failure(y, y64, bound, what)
    print(f"{what}: worst err / bound {worst:.3f}")
    assert msg is None, msg


def _outside(y, y64, bound):
    return bool((R.ratio(y, y64, bound) > 1.0).any())


def _case(name, fmt, style):
    return B.conv_first_bwd_case(*B.CONV_FIRST_BWD_CASES[name], fmt, *style)


# ---- a. the references are the gradient --------------------------------------------------------------------------------------------------------------------
def _conv_first_autograd(c, fmt, folded):
    """fp64 autograd of conv -> ReLU -> (16-bit rounding, straight through) -> max_pool2d [-> group_norm_1] -> (dW [Cout, 27] (kh, kw, ch), db)."""
    w = c["w16"].to(D).requires_grad_(True)            # W16 = W / 255 against the raw bytes: exact in fp64, so ties stay ties; d / dW = (d / dW16) / 255
    b = (c["bh"].to(D) + c["bl"].to(D)).requires_grad_(True)
    y = torch.relu(F.conv2d(c["img"].permute(0, 3, 1, 2).to(D), w, b, padding=1))
    y = y + (c["pre"] - y.detach())
    p = F.max_pool2d(y, 3, 2, 1)
    # torch routes the gradient of an all-zero window to its first element, where the ReLU then stops it; the reference's `<= 0 passes nothing` is the same
    if folded:
        gain = c["nfold"][0].to(D)
        p = O.group_norm_1(p, gain, torch.zeros_like(gain))
    gw, gb = torch.autograd.grad((p * c["d"]).sum(), [w, b])
    return gw.permute(0, 2, 3, 1).reshape(-1, 27) / 255.0, gb


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("style", B.STYLES)
@pytest.mark.parametrize("name", SMALL)
def test_conv_first_backward_ref_is_autograd(name, style, fmt):
    c = _case(name, fmt, style)
    for key, folded in (("plain", False), ("folded", True)):
        gw, gb = _conv_first_autograd(c, fmt, folded)
        _close(c[key]["dW"], gw, f"{key} dW")
        _close(c[key]["db"], gb, f"{key} db")


@pytest.mark.parametrize("fmt", FMTS)
def test_conv_first_backward_ref_is_autograd_two_channel_tiles(fmt):
    c = _case("nt2_partial", fmt, ("blocky", "real"))
    for key, folded in (("plain", False), ("folded", True)):
        gw, gb = _conv_first_autograd(c, fmt, folded)
        _close(c[key]["dW"], gw, f"{key} dW")
        _close(c[key]["db"], gb, f"{key} db")


def _affine_autograd(c, with_add):
    x = c["x"].clone().requires_grad_(True)
    gain = c["gain"].to(D).requires_grad_(True)
    bias = torch.zeros_like(gain).requires_grad_(True)
    if c["per_element"]:
        y = O.layer_norm(x.reshape(c["frames"], -1), gain, bias).reshape(x.shape)
    else:
        y = O.group_norm_1(x, gain, bias)
    gx, gg, gb = torch.autograd.grad((y * c["dy"]).sum(), [x, gain, bias])
    if with_add:
        return gx + c["dx_add"], gg + c["prior"][0].to(D), gb + c["prior"][1].to(D)
    return gx, gg, gb


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("kind", ["real", "exact"])
@pytest.mark.parametrize("name", list(B.AFFINE_BWD_CASES))
def test_affine_backward_ref_is_autograd(name, kind, fmt):
    c = B.affine_bwd_case(name, fmt, kind)
    for key, with_add in (("plain", False), ("added", True)):
        gx, gg, gb = _affine_autograd(c, with_add)
        r = c[key]
        _close(r["dx"], gx, "dx"); _close(r["dgain"], gg, "dgain"); _close(r["dbias"], gb, "dbias")


@pytest.mark.parametrize("i", range(len(B.POOL_CASES)))
def test_pool_backward_fp32_routes_as_autograd(i):
    """The four-term fp32 sum rounded once lies within one 16-bit ulp of the fp64 gradient, and the routing is maxpool_backward_ref's and autograd's."""
    for fmt in FMTS:
        c = B.pool_case(i, fmt)
        pre = c["pre"].clone().requires_grad_(True)
        (want,) = torch.autograd.grad((F.max_pool2d(pre, 3, 2, 1) * c["d"]).sum(), [pre])
        assert torch.equal(want, maxpool_backward_ref(c["d"], c["pre"]))
        assert torch.equal(B.fold_parts(B.route_parts(c["d"], c["pre"]), c["h"], c["w"]), want)
        got = c["dpre"].to(D)
        assert bool(((got - want).abs() <= R.ulp16(want, fmt) + 3 * R.U32 * maxpool_backward_ref(c["d"].abs(), c["pre"])).all())


# ---- b. fp32 arithmetic lies inside every bound -------------------------------------------------------------------------------------------------------------
def _emu_conv_first(c, fmt, folded):
    f32 = torch.float32
    d = c["d"].to(f32)
    if folded:
        gain, st, ab = c["nfold"]
        n = c["cout"] * (c["h"] // 2) * (c["w"] // 2)
        m = (st[:, 0] / n)
        var = (st[:, 1] / n - m * m).clamp(min=0)
        mean, rstd = m.to(f32).view(-1, 1, 1, 1), (1.0 / torch.sqrt(var.to(f32) + torch.tensor(O.NORM_EPS, dtype=f32))).view(-1, 1, 1, 1)
        a_, b_ = (ab[:, 0] / n).to(f32).view(-1, 1, 1, 1), (ab[:, 1] / n).to(f32).view(-1, 1, 1, 1)
        xh = (c["pooled"].to(f32) - mean) * rstd
        d = (rstd * (d * gain.view(1, -1, 1, 1) - a_ - xh * b_)).to(R.DT[fmt]).to(f32)
        _inside(d, c["folded"]["dP"], c["folded"]["b_dP"], f"conv_first backward {fmt} dP")
    live = (c["pooled"] > 0).to(f32)
    gr = maxpool_backward_ref((d * live).to(D), c["pre"]).to(f32)          # (at most four 16-bit values per pixel: their sum is exact in fp32 here or not,
    h, w = c["h"], c["w"]                                                  # either is a legitimate fp32 evaluation)
    xp = F.pad(c["img"].permute(0, 3, 1, 2).to(f32), (1, 1, 1, 1))
    dw = torch.stack([torch.einsum("fohw,fchw->oc", gr, xp[:, :, kh:kh + h, kw:kw + w]) for kh in range(3) for kw in range(3)], 1).reshape(-1, 27)
    return dw * torch.tensor(1.0, dtype=f32).div(255.0), gr.sum((0, 2, 3))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("style", B.STYLES)
@pytest.mark.parametrize("name", SMALL)
def test_conv_first_backward_emulation_inside_the_bound(name, style, fmt):
    c = _case(name, fmt, style)
    rows = B.slab_rows(c["frames"], c["h"], c["w"], CUS)
    for key in ("plain", "folded"):
        dw, db = _emu_conv_first(c, fmt, key == "folded")
        b_dw, b_db = B.conv_first_backward_bounds(c[key], c["n"], rows)
        _inside(dw, c[key]["dW"], b_dw, f"conv_first backward {name} {style} {fmt} {key} dW")
        _inside(db, c[key]["db"], b_db, f"conv_first backward {name} {style} {fmt} {key} db")


def _emu_affine(c, fmt, with_add):
    f32 = torch.float32
    fr = c["frames"]
    n = c["c"] * c["h"] * c["w"]
    st = c["stats_in"]
    m = st[:, 0] / n
    var = (st[:, 1] / n - m * m).clamp(min=0)
    mean, rstd = m.to(f32).view(-1, 1, 1, 1), (1.0 / torch.sqrt(var.to(f32) + torch.tensor(O.NORM_EPS, dtype=f32))).view(-1, 1, 1, 1)
    shape = (1, c["c"], c["h"], c["w"]) if c["per_element"] else (1, c["c"], 1, 1)
    g = c["gain"].view(shape)
    x, dy = c["x"].to(f32), c["dy"].to(f32)
    xh = (x - mean) * rstd
    dg = dy * g
    ab = torch.stack([dg.reshape(fr, -1).sum(1), (dg * xh).reshape(fr, -1).sum(1)], 1)
    a_, b_ = (ab[:, 0].double() / n).to(f32).view(-1, 1, 1, 1), (ab[:, 1].double() / n).to(f32).view(-1, 1, 1, 1)
    dx = rstd * (dg - a_ - xh * b_)
    over = (0,) if c["per_element"] else (0, 2, 3)
    dgain, dbias = (dy * xh).sum(over).reshape(-1), dy.sum(over).reshape(-1)
    if with_add:
        dx = dx + c["dx_add"].to(f32)
        dgain, dbias = dgain + c["prior"][0], dbias + c["prior"][1]
    return ab, dx.to(R.DT[fmt]), dgain, dbias


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("kind", ["real", "exact", "constant"])
@pytest.mark.parametrize("name", list(B.AFFINE_BWD_CASES))
def test_affine_backward_emulation_inside_the_bound(name, kind, fmt):
    c = B.affine_bwd_case(name, fmt, kind)
    for key, with_add in (("plain", False), ("added", True)):
        ab, dx, dgain, dbias = _emu_affine(c, fmt, with_add)
        r = c[key]
        what = f"affine backward {name} {kind} {fmt} {key}"
        _inside(ab, r["ab"], r["b_ab"], what + " ab")
        _inside(dx, r["dx"], r["b_dx"], what + " dx")
        _inside(dgain, r["dgain"], r["b_dgain"], what + " dgain")
        _inside(dbias, r["dbias"], r["b_dbias"], what + " dbias")


# ---- c. the cases are what they claim to be ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("style", B.STYLES)
@pytest.mark.parametrize("name", list(B.CONV_FIRST_BWD_CASES))
def test_conv_first_backward_case_conditions(name, style, fmt):
    c = _case(name, fmt, style)
    assert torch.equal(c["w16"].to(D), c["k"].to(D) * 2.0 ** -12), "W16 != k 2^-12"
    assert torch.equal(c["bh"].to(D) + c["bl"].to(D), c["j"].to(D) * 2.0 ** -14 - 2.0), "bh + bl != bias"
    assert bool((c["bl"].float() != 0).any()), "no bias has a low half"
    assert c["units"] < B.EXACT_LIMIT, c["units"]
    live, tied, wins = B.routing_shares(c["pre"])
    print(f"{name} {style} {fmt}: sum of magnitudes {c['units']:.3g} units, live {live:.3f}, tied and live {tied:.3f}, offsets {[round(v, 3) for v in wins.tolist()]}")
    if style[0] == "blocky":
        assert 0.4 <= live <= 0.9 and tied >= 0.15 and bool((wins >= 0.01).all()), (live, tied, wins)
    if style[1] == "int":
        assert bool((c["plain"]["db_abs"] < B.EXACT_LIMIT).all())
        assert bool((c["d"] == 0).any()) and bool((c["d"] == c["d"].round()).all())
        if name == "one_tile":
            B.dw_exact_one_tile(c["plain"])          # asserts |S| < 2^24 and that S is an integer


@pytest.mark.parametrize("fmt", FMTS)
def test_persistent_backward_case(fmt):
    """On CU counts around the MI355X's 256: T > grid, two tiles per working workgroup, ranges that begin inside frames, workgroups without a tile; and the
    integer sums of the persistent case at 256 CUs are below 2^24."""
    for cus in (64, 228, 256, 304):
        frames, tiles, grid = B.persistent_backward_frames(cus)
        per = -(-tiles // grid)
        assert tiles == 15 * frames and tiles > grid and per == 2 and 15 % per != 0 and -(-tiles // per) < grid
    frames, _, _ = B.persistent_backward_frames(CUS)
    c = B.conv_first_bwd_case(frames, *B.PERSISTENT_BWD_HW_COUT, fmt, "blocky", "int")
    assert c["units"] < B.EXACT_LIMIT and bool((c["plain"]["db_abs"] < B.EXACT_LIMIT).all())


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(B.AFFINE_BWD_CASES))
def test_affine_backward_exact_case_conditions(name, fmt):
    c = B.affine_bwd_case(name, fmt, "exact")
    r = c["plain"]
    assert bool((r["abs_dy"] < B.EXACT_LIMIT).all()) and bool((2.0 * r["abs_dyg"] < B.EXACT_LIMIT).all())      # in units of the smallest gain, 1/2
    assert bool((c["dy"] == c["dy"].round()).all()) and set(c["gain"].tolist()) <= {0.5, 1.0, 2.0}
    assert torch.equal(r["dbias"], r["dbias"].round()) and torch.equal(2 * r["ab"][:, 0], (2 * r["ab"][:, 0]).round())
    x = B.affine_bwd_case(name, fmt, "constant")["x"]
    assert float(x[0].var()) == 0.0


def test_affine_backward_chains():
    assert B.slab_chain(1) == 3 and B.slab_chain(256) == 66 and B.slab_chain(300) == 66 + 3
    assert [B.affine_elem_slices(f) for f in (1, 15, 16, 17, 511, 512)] == [1, 1, 8, 8, 8, 32]
    assert B.affine_bwd_case("two_slices", "bf16", "real")["plain"]["n_add"] == 22 + 69
    assert B.affine_bwd_case("elem_slices", "bf16", "real")["plain"]["n_add"] == 3 + B.slab_chain(8)
    assert 8 * 3 - 17 >= 2 * 3      # 17 frames in eight slices of three: slices 6 and 7 are empty


def test_pool_cases_have_plateaus_and_zero_windows():
    for i in range(len(B.POOL_CASES)):
        c = B.pool_case(i, "bf16")
        win = B.windows(c["pre"])
        mx = win.max(dim=2, keepdim=True).values
        assert bool((mx == 0).any()), f"case {i}: no all-zero window"
        assert bool((((win == mx).sum(2, keepdim=True) > 1) & (mx > 0)).any()), f"case {i}: no plateau"
        assert c["pre"].unique().numel() <= 8


# ---- d. the mutations are visible ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("mutate", B.MUTATIONS + ("swap_ab",))
def test_conv_first_backward_mutations_fall_outside(mutate, fmt):
    c = _case("one_tile", fmt, ("blocky", "real"))
    key, nfold = ("folded", c["nfold"]) if mutate == "swap_ab" else ("plain", None)
    mut = B.conv_first_backward_ref(c["img"], c["w16"], c["bh"], c["bl"], c["d"], fmt, nfold=nfold, mutate=mutate)
    b_dw, _ = B.conv_first_backward_bounds(mut, c["n"], 1)
    assert _outside(c[key]["dW"], mut["dW"], b_dw), mutate


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("mutate", ["no_add", "gain_octet", "swap_ab"])
def test_affine_backward_mutations_fall_outside(mutate, fmt):
    for name in ("clamped", "elem_small"):
        c = B.affine_bwd_case(name, fmt, "real")
        mut = B.affine_backward_ref(c["x"], c["dy"], c["gain"], c["stats_in"], fmt, c["per_element"], dx_add=c["dx_add"], prior=c["prior"], mutate=mutate)
        assert _outside(c["added"]["dx"], mut["dx"], mut["b_dx"]), (mutate, name)
