"""tests/ingest_ref.py is the operation, plain fp32 arithmetic meets its bounds, and the bounds see the defects they are there for -- shown on the CPU,
before a GPU sees any of it (tests/test_gpu_ingest_fp64.py is the GPU half).

a. With weights that are already representable (and a bias whose two halves are exact) each reference equals the plain fp64 torch chain of the operation:
   F.conv2d(x / 255, W, b) -> relu -> max_pool2d, oracle conv3d_temporal, oracle group_norm_1 / layer_norm -- to 1e-12 of the tensor's magnitude, so the
   reference is pinned to the operation and not to itself.
b. An emulation of each kernel (fp32 accumulation of the same operands, then the format's rounding) lies inside the bound at EVERY element of every GPU
   case that runs here in a second.  A bound plain fp32 cannot meet would be wrong.
c. Mutations of the emulation -- one input byte zeroed at (H-1, W-1, 2) and at (0, 0, 0) of every frame, the output scaled by 255 / 256, a temporal tap
   admitted one frame past the sequence end (and the indexed kernel's window clamps and src), the affine's gain taken from the next channel block, the
   fp16-subnormal weights of conv_first flushed to zero -- each fall outside the bound somewhere.  The round-one
   criterion (max |d| / max |ref| against the fp32 chain, at its bf16 limit) ACCEPTS the 255 / 256 scale: the reason this file exists, recorded as a test."""
import pytest
import torch
import torch.nn.functional as F

import vpt_amd  # noqa: F401
from vpt_amd import packing
from oracle import vpt_oracle as O
from tests import ingest_ref as R

D = torch.float64
FMTS = ["bf16", "fp16"]
OLD_LIMIT_BF16 = {"conv_first": 1.5e-2, "conv3d": 1.5e-2, "affine": 8e-3}      # tests/test_gpu_kernels.py: max |a - b| / max |b|


def _close(a, b):
    """1e-12 relative to the tensor's magnitude (elements near zero are differences of O(1) terms)."""
    return bool(((a - b).abs() <= 1e-12 * b.abs().max()).all())


def _old_relerr(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


# ---- emulations: fp32 accumulation of the kernel's operands, rounded to the format -----------------------------------------------------------------------
def emu_conv_first(img, w16, bh, bl, fmt, scale=1.0):
    pre = F.conv2d(img.permute(0, 3, 1, 2).float(), w16.float(), padding=1) + bh.float().view(1, -1, 1, 1) + bl.float().view(1, -1, 1, 1)
    return (F.max_pool2d(torch.relu(pre), 3, 2, 1) * scale).to(R.DT[fmt])


def emu_conv3d(img, src, lo, hi, w16, bias, fmt, scale=1.0):
    taps = R.conv3d_taps(img, src, lo, hi).float()
    acc = torch.einsum("ocd,sdhwc->sohw", w16.float().reshape(-1, 3, 5), taps)
    y = torch.relu(acc * torch.tensor(1.0 / 255.0, dtype=torch.float32) + bias.float().view(1, -1, 1, 1))
    return (y * scale).to(R.DT[fmt])


def emu_affine(c, fmt, gain=None, scale=1.0):
    """vpt_affine_kernel's order: mean, rstd and shift = -mean * rstd in fp32, then (x * rstd + shift) * g + b (without the fmas: two roundings more)."""
    n = c["c"] * c["h"] * c["w"]
    m = c["stats_in"][:, 0] / n
    var = (c["stats_in"][:, 1] / n - m * m).clamp(min=0)
    mean = m.float()
    rstd = 1.0 / torch.sqrt(var.float() + torch.tensor(O.NORM_EPS, dtype=torch.float32))
    shift = (-mean * rstd).view(-1, 1, 1, 1)
    shape = (1, c["c"], c["h"], c["w"]) if c["per_element"] else (1, c["c"], 1, 1)
    g = (c["gain"] if gain is None else gain).view(shape)
    y = (c["x"].float() * rstd.view(-1, 1, 1, 1) + shift) * g + c["bias"].view(shape)
    return (y * scale).to(R.DT[fmt])


def _inside(y, c, what):
    worst, msg = R.failure(y, c["y64"], c["bound"], what)
    print(f"{what}: worst err / bound {worst:.3f}")
    assert msg is None, msg
    return worst


def _outside(y, c):
    return bool((R.ratio(y, c["y64"], c["bound"]) > 1.0).any())


def _zero_byte(img, y, x, ch):
    out = img.clone()
    out[:, y, x, ch] = 0
    return out


# ---- a. the references are the operation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_conv_first_ref_is_the_unrounded_operation(fmt):
    c = R.conv_first_case(*R.CONV_FIRST_CASES["nt2_partial"], fmt)
    weight = c["w16"].float() * 255.0                      # exact: 8- or 11-bit significand times 255
    bias = c["bh"].float() + c["bl"].float()               # exact: the two halves span at most 23 bits
    w16, bh, bl = R.conv_first_operands(weight, bias, fmt)
    assert torch.equal(w16, c["w16"])                      # such weights pack to themselves
    assert torch.equal(bh.double() + bl.double(), bias.double())      # and the two halves carry this bias exactly
    x = c["img"].permute(0, 3, 1, 2).to(D) / 255.0
    want = F.max_pool2d(torch.relu(F.conv2d(x, c["w16"].to(D) * 255.0, bias.to(D), padding=1)), 3, 2, 1)
    assert _close(c["y64"], want)


@pytest.mark.parametrize("fmt", FMTS)
def test_reference_operands_are_what_the_packing_stores(fmt):
    """The fragments the kernels read hold exactly the reference's operands: W16 at k < 27, bh / bl at k = 27 / 28 (conv_first), op16(W) at k = dt * 3 + ch and
    the fp32 bias (conv3d_t5); everything else is zero."""
    c = R.conv_first_case(*R.CONV_FIRST_CASES["nt2_partial"], fmt)
    cout = c["cout"]
    frag = packing.pack_conv_first(c["weight"], c["bias"], dtype=R.DT[fmt])
    nt = frag.shape[0]
    slots = frag.view(nt, 4, 2, 2, 32, 8).permute(0, 1, 4, 2, 3, 5).reshape(nt * 128, 32)
    rows = torch.zeros(nt * 128, 32, dtype=R.DT[fmt])
    rows[:, packing.CONV_FIRST_SLOT_K] = slots
    want = torch.zeros_like(rows)
    want[:cout, :27] = c["w16"].permute(0, 2, 3, 1).reshape(cout, 27)
    want[:cout, 27], want[:cout, 28] = c["bh"], c["bl"]
    assert torch.equal(rows.view(torch.int16), want.view(torch.int16))
    c = R.conv3d_case("t7_nt2", fmt)
    cout = c["cout"]
    frag, bp = packing.pack_conv3d_t5(c["weight"], c["bias"], dtype=R.DT[fmt])
    nt = frag.shape[0]
    rows = frag.view(nt, 4, 2, 32, 8).permute(0, 1, 3, 2, 4).reshape(nt * 128, 16)
    want = torch.zeros_like(rows)
    want[:cout, :15] = c["w16"].reshape(cout, 3, 5).permute(0, 2, 1).reshape(cout, 15)
    assert torch.equal(rows.view(torch.int16), want.view(torch.int16))
    assert torch.equal(bp[:cout], c["bias"]) and not bool(bp[cout:].any())


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(R.CONV3D_CASES))
def test_conv3d_ref_is_the_oracle(name, fmt):
    c = R.conv3d_case(name, fmt)
    bsz = c["frames"] // c["t"]
    sd = {"net.conv3d_layer.layer.weight": c["w16"].to(D), "net.conv3d_layer.layer.bias": c["bias"].to(D)}
    x = c["img"].reshape(bsz, c["t"], c["h"], c["w"], 3).to(D) / 255.0
    want = O.conv3d_temporal(sd, x).reshape(c["frames"], c["h"], c["w"], c["cout"]).permute(0, 3, 1, 2)
    assert _close(c["y64"], want)


@pytest.mark.parametrize("fmt", FMTS)
def test_conv3d_indexed_ref_is_the_oracle_on_gathered_windows(fmt):
    """Every slot equals the centre frame of the oracle's conv over the slot's own window [max(lo, 0), min(hi, n_img)) taken as one sequence."""
    c = R.conv3d_indexed_case(160, fmt)
    sd = {"net.conv3d_layer.layer.weight": c["w16"].to(D), "net.conv3d_layer.layer.bias": c["bias"].to(D)}
    for j, (s, lo, hi) in enumerate(R.CONV3D_INDEXED_SLOTS):
        lo, hi = max(lo, 0), min(hi, R.CONV3D_INDEXED_IMG)
        want = O.conv3d_temporal(sd, c["img"][lo:hi].to(D)[None] / 255.0)[0, s - lo].permute(2, 0, 1)
        assert _close(c["y64"][j], want), j


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(R.AFFINE_CASES))
def test_affine_ref_is_the_oracle(name, fmt):
    c = R.affine_case(name, fmt)
    x, g, b = c["x"].to(D), c["gain"].to(D), c["bias"].to(D)
    if c["per_element"]:
        want = O.layer_norm(x.reshape(c["frames"], -1), g, b).reshape(x.shape)
    else:
        want = O.group_norm_1(x, g, b)
    assert _close(c["y64"], want)


# ---- b. fp32 arithmetic lies inside every bound ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(R.CONV_FIRST_CASES))
def test_conv_first_emulation_inside_the_bound(name, fmt):
    c = R.conv_first_case(*R.CONV_FIRST_CASES[name], fmt)
    y = emu_conv_first(c["img"], c["w16"], c["bh"], c["bl"], fmt)
    _inside(y, c, f"conv_first {name} {fmt}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(R.CONV3D_CASES))
def test_conv3d_emulation_inside_the_bound(name, fmt):
    c = R.conv3d_case(name, fmt)
    y = emu_conv3d(c["img"], *R.conv3d_windows(c["frames"], c["t"]), c["w16"], c["bias"], fmt)
    _inside(y, c, f"conv3d {name} {fmt}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("cout", R.CONV3D_INDEXED_COUT)
def test_conv3d_indexed_emulation_inside_the_bound(cout, fmt):
    c = R.conv3d_indexed_case(cout, fmt)
    y = emu_conv3d(c["img"], c["src"], c["lo"], c["hi"], c["w16"], c["bias"], fmt)
    _inside(y, c, f"conv3d indexed {cout} {fmt}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(R.AFFINE_CASES))
def test_affine_emulation_inside_the_bound(name, fmt):
    c = R.affine_case(name, fmt)
    _inside(emu_affine(c, fmt), c, f"affine {name} {fmt}")


# ---- c. the bounds see the defects; the old criterion does not ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(R.CONV_FIRST_CASES))
def test_conv_first_mutations_fall_outside(name, fmt):
    c = R.conv_first_case(*R.CONV_FIRST_CASES[name], fmt)
    ops_ = (c["w16"], c["bh"], c["bl"], fmt)
    assert _outside(emu_conv_first(_zero_byte(c["img"], c["h"] - 1, c["w"] - 1, 2), *ops_), c), "last byte of the frame dropped"
    assert _outside(emu_conv_first(_zero_byte(c["img"], 0, 0, 0), *ops_), c), "first byte of the frame dropped"
    scaled = emu_conv_first(c["img"], *ops_, scale=255.0 / 256.0)
    assert _outside(scaled, c), "255 / 256 scale"
    if fmt == "fp16":       # W / 255 below 2^-14 is subnormal in fp16 (4-5 % of these weights): a matrix unit that flushed them would be seen
        w16 = c["w16"]
        flushed = torch.where(w16.float().abs() < 2.0 ** -14, torch.zeros_like(w16), w16)
        assert not torch.equal(flushed, w16) and _outside(emu_conv_first(c["img"], flushed, c["bh"], c["bl"], fmt), c), "subnormal weights flushed"
    if fmt == "bf16":
        old_ref = F.max_pool2d(torch.relu(F.conv2d(c["img"].permute(0, 3, 1, 2).float() / 255.0, c["weight"], c["bias"], padding=1)), 3, 2, 1)
        err = _old_relerr(scaled.float(), old_ref)
        print(f"conv_first {name}: 255 / 256 scale, old criterion {err:.2e}, {float((R.ratio(scaled, c['y64'], c['bound']) > 1).double().mean()):.1%} of the elements outside the bound")
        assert err < OLD_LIMIT_BF16["conv_first"]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(R.CONV3D_CASES))
def test_conv3d_mutations_fall_outside(name, fmt):
    c = R.conv3d_case(name, fmt)
    win = R.conv3d_windows(c["frames"], c["t"])
    ops_ = (c["w16"], c["bias"], fmt)
    assert _outside(emu_conv3d(_zero_byte(c["img"], c["h"] - 1, c["w"] - 1, 2), *win, *ops_), c)
    assert _outside(emu_conv3d(_zero_byte(c["img"], 0, 0, 0), *win, *ops_), c)
    scaled = emu_conv3d(c["img"], *win, *ops_, scale=255.0 / 256.0)
    assert _outside(scaled, c)
    if c["frames"] > c["t"]:        # more than one sequence: the frame behind a sequence's end exists
        src, lo, hi = win
        assert _outside(emu_conv3d(c["img"], src, lo, hi + 1, *ops_), c), "a tap one frame past the sequence end"
    if fmt == "bf16":
        bsz = c["frames"] // c["t"]
        sd = {"net.conv3d_layer.layer.weight": c["weight"], "net.conv3d_layer.layer.bias": c["bias"]}
        old_ref = O.conv3d_temporal(sd, c["img"].reshape(bsz, c["t"], c["h"], c["w"], 3).float() / 255.0).reshape(c["frames"], c["h"], c["w"], -1).permute(0, 3, 1, 2)
        assert _old_relerr(scaled.float(), old_ref) < OLD_LIMIT_BF16["conv3d"]


def test_conv3d_tap_past_the_end_is_tested():
    assert any(b > 1 for b, *_ in R.CONV3D_CASES.values())


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("cout", R.CONV3D_INDEXED_COUT)
def test_conv3d_indexed_mutations_fall_outside(cout, fmt):
    """The clamps and both window edges: without the clamp of hi (lo) the taps of the next (previous) frame come in, with the window ignored all five do."""
    c = R.conv3d_indexed_case(cout, fmt)
    ops_ = (c["w16"], c["bias"], fmt)
    assert _outside(emu_conv3d(c["img"], c["src"], c["lo"], c["hi"] + 1, *ops_), c)
    assert _outside(emu_conv3d(c["img"], c["src"], c["lo"] - 1, c["hi"], *ops_), c)
    assert _outside(emu_conv3d(c["img"], torch.arange(len(c["src"])), c["lo"], c["hi"], *ops_), c), "src ignored"


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(R.AFFINE_CASES))
def test_affine_mutations_fall_outside(name, fmt):
    c = R.affine_case(name, fmt)
    scaled = emu_affine(c, fmt, scale=255.0 / 256.0)
    assert _outside(scaled, c)
    n = c["h"] * c["w"] if c["per_element"] else 1
    assert _outside(emu_affine(c, fmt, gain=torch.roll(c["gain"], 32 * n)), c), "gain of the next channel block"
    if fmt == "bf16":
        x = c["x"].float()
        old_ref = O.layer_norm(x.reshape(c["frames"], -1), c["gain"], c["bias"]).reshape(x.shape) if c["per_element"] else O.group_norm_1(x, c["gain"], c["bias"])
        assert _old_relerr(scaled.float(), old_ref) < OLD_LIMIT_BF16["affine"]


@pytest.mark.parametrize("fmt", FMTS)
def test_stats_instrument_sees_a_lost_lane(fmt):
    """unrounded_stats_bound: the exact sums pass with nothing to spare being needed, the sums without one thread's 32 values do not."""
    c = R.affine_case("full_partial", fmt)
    st, _ = R.frame_sums(c["y64"])
    allowed = R.unrounded_stats_bound(c["y64"], c["acc"], R.N_ADD_AFFINE_STATS)
    flat = c["y64"].reshape(c["frames"], -1).clone()
    flat[:, :32] = 0
    st_lost = torch.stack([flat.sum(1), (flat * flat).sum(1)], 1)
    assert bool(((st_lost - st).abs() > allowed).all())


def test_persistent_frames():
    """The persistent case's frame count on CU counts around the MI355X's 256: 3 cap < T <= 4 cap, so four tiles per workgroup, no multiple of a frame's 15."""
    for cus in (64, 228, 256, 304):
        frames, tiles, cap = R.persistent_frames(cus)
        assert cap == 4 * cus and 3 * cap < tiles <= 4 * cap and tiles == 15 * frames
        assert -(-tiles // cap) == 4
