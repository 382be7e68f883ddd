"""The kernels every frame passes through first -- vpt_conv_first_kernel, vpt_conv3d_t5_kernel and its indexed twin, vpt_affine_kernel -- held per element to the
fp64 references and derived bounds of tests/ingest_ref.py (its docstring has the derivations and the counted summation lengths; tests/test_ingest_ref_cpu.py
pins them on the CPU).  Both operand formats.  Needs an MI355X.

Shapes are the smallest at which each path of the kernels can go wrong:

conv_first   16 x 16: ONE tile that touches all four borders (top / left zero records, the clamped first and last records of cf_rec_fix); 48 x 80 x 160: seams both
             ways, non-square, two channel tiles with one valid wave in the second; 16 x 48 x 32: one valid wave, column seams only; and the PERSISTENT case:
             48 x 80 frames (15 tiles) in a number that follows from the device's CU count, so that the launch has more tiles than the grid's cap of four workgroups
             per CU, every workgroup runs four tiles (advance / fetch one ahead / stage / convert of the NEXT tile's borders), and the ranges begin and end inside
             frames.
conv3d_t5    T = 1, 2, 4 (windows shorter than the five taps), 5, 7; one-chunk frames (H * W = 256) and two chunks; cout = 32 (three of four channel blocks
             skipped), 128, 160 (NT = 2, partial).  The indexed kernel against the fp64 reference DIRECTLY, on a fixed slot list: src not monotonic and repeated,
             windows clipped left, right and both, lo < 0 and hi > n_img (clamped), a window wider than five frames.
frame_affine partial 1024-item blocks (768 and 1200 items: the clamped loads and the `item < per_frame` guard), per channel and per element, and a constant frame.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops, packing  # noqa: E402
from tests import ingest_ref as R  # noqa: E402

DEV = "cuda"
D = torch.float64
FMTS = ["bf16", "fp16"]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check(y_blocked, c, what):
    """Every stored element against the bound -> the tensor in NCHW, fp64."""
    y = packing.blocked_to_nchw(y_blocked.cpu(), *c["y64"].shape[1:]).double()
    worst, msg = R.failure(y, c["y64"], c["bound"], what)
    print(f"{what}: worst err / bound {worst:.3f}")
    assert msg is None, msg
    return y


def _check_sums(got, want, allowed, what):
    """fp64 sums from the kernel against fp64 sums of the reference tensor, element-wise allowed error."""
    err = (got.cpu() - want).abs()
    worst = torch.where(err == 0, torch.zeros_like(err), err / allowed).max().item()
    print(f"{what}: worst err / allowed {worst:.3f}")
    assert bool((err <= allowed).all()) and bool(torch.isfinite(got).all()), f"{what}: worst err / allowed {worst:.3f}\n{got.cpu()}\n{want}"


# ---- conv_first ----------------------------------------------------------------------------------------------------------------------------------------
def _conv_first(c, fmt, img, out_gain=None, chs=False):
    wf = packing.pack_conv_first(c["weight"], c["bias"], dtype=R.DT[fmt]).to(DEV)
    frames = img.shape[0]
    st = torch.zeros(frames, 2, dtype=D, device=DEV)
    chs_out = torch.zeros(frames, c["cout"], 2, dtype=D, device=DEV) if chs else None
    y = ops.conv_first(img, wf, c["cout"], stats_out=st, out_gain=out_gain, chs_out=chs_out)
    torch.cuda.synchronize()
    return y, st, chs_out


def _check_conv_first(c, fmt, what):
    """Every check of a conv_first case -> (img on the device, y, st, y_chs, st_chs, chs) of the plain launch and of the one with gain and channel sums
    (None without the latter)."""
    cout, ph, pw = c["cout"], c["h"] // 2, c["w"] // 2
    img = c["img"].to(DEV)
    gain = c["gain"].to(DEV)
    y, st, _ = _conv_first(c, fmt, img)
    y_nchw = _check(y, c, what)
    sums, mags = R.frame_sums(y_nchw)                     # of the STORED, unscaled tensor
    allowed = R.sum_bound(R.N_ADD_CONV_FIRST_STATS, mags)
    _check_sums(st, sums, allowed, f"{what} stats_out")
    # out_gain: the stored tensor is op16(float(y) * gain) of the kernel's own ungained output; the statistics stay those of the unscaled tensor
    y2, st2, _ = _conv_first(c, fmt, img, out_gain=gain)
    want2 = (y.float() * gain.view(1, cout // 32, 1, 1, 32)).to(R.DT[fmt])
    assert torch.equal(_bits(y2), _bits(want2)), f"{what}: out_gain is not one rounding of y * gain"
    _check_sums(st2, sums, allowed, f"{what} stats_out with out_gain")
    if cout > 128:
        return img, y, st, None, None, None
    # chs_out: the same bits, the per-channel sums of the STORED (scaled) tensor
    y3, st3, chs = _conv_first(c, fmt, img, out_gain=gain, chs=True)
    assert torch.equal(_bits(y3), _bits(y2)), f"{what}: chs_out changes the output"
    _check_sums(st3, sums, allowed, f"{what} stats_out with chs_out")
    y4, _, _ = _conv_first(c, fmt, img, chs=True)
    assert torch.equal(_bits(y4), _bits(y)), f"{what}: chs_out changes the ungained output"
    s = packing.blocked_to_nchw(y3.cpu(), cout, ph, pw).double().reshape(c["frames"], cout, -1)
    ch_sums = torch.stack([s.sum(2), (s * s).sum(2)], 2)
    ch_mags = torch.stack([s.abs().sum(2), (s * s).sum(2)], 2)
    group, n_groups = R.conv_first_chs_group(c["h"], c["w"], cout)
    _check_sums(chs, ch_sums, R.sum_bound(2 * group + 5, ch_mags) + n_groups * 2.0 ** -53 * ch_mags, f"{what} chs_out")     # (+ one fp64 atomic per group)
    return img, y, st, y3, st3, chs


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(R.CONV_FIRST_CASES))
def test_conv_first_fp64(name, fmt):
    c = R.conv_first_case(*R.CONV_FIRST_CASES[name], fmt)
    _check_conv_first(c, fmt, f"conv_first {name} {fmt}")


@pytest.mark.parametrize("fmt", FMTS)
def test_conv_first_persistent_loop_fp64(fmt):
    """More tiles than the grid's cap (4 workgroups per CU), on non-square frames: T = 15 * frames with 3 cap < T <= 4 cap, so every workgroup runs a range of
    ceil(T / cap) = 4 consecutive tiles; 4 is no multiple of a frame's 15, so ranges begin and end inside frames and cross from one frame into the next.  The
    conditions are asserted, not assumed: on a device where they cannot hold the test fails.  Three single-frame launches (the first frame, a middle one whose
    tiles begin inside a workgroup's range, the last) must equal the big launch bit for bit, output and statistics."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    frames, tiles, cap = R.persistent_frames(cus)
    per = -(-tiles // cap)
    print(f"conv_first persistent {fmt}: {cus} CUs, cap {cap} workgroups, {frames} frames, T = {tiles} tiles, {per} tiles per workgroup")
    assert tiles > cap and per % 15 != 0, (cus, frames, tiles, cap, per)
    h, w, cout = R.PERSISTENT_HW_COUT
    c = R.conv_first_case(frames, h, w, cout, fmt)
    img, y, st, y3, st3, chs = _check_conv_first(c, fmt, f"conv_first persistent {fmt}")
    mid = next(f for f in range(frames // 2, frames) if (15 * f) % per != 0)
    gain = c["gain"].to(DEV)
    for f in (0, mid, frames - 1):
        y1, st1, _ = _conv_first(c, fmt, img[f:f + 1])
        assert torch.equal(_bits(y1), _bits(y[f:f + 1])) and torch.equal(st1, st[f:f + 1]), f"frame {f} depends on the launch it is part of"
        y1, st1, chs1 = _conv_first(c, fmt, img[f:f + 1], out_gain=gain, chs=True)
        assert torch.equal(_bits(y1), _bits(y3[f:f + 1])) and torch.equal(st1, st3[f:f + 1]) and torch.equal(chs1, chs[f:f + 1]), \
            f"frame {f} (gain, channel sums) depends on the launch it is part of"


# ---- conv3d_t5 -----------------------------------------------------------------------------------------------------------------------------------------
def _check_conv3d_stats(st, c, what):
    sums, _ = R.frame_sums(c["y64"])
    _check_sums(st, sums, R.unrounded_stats_bound(c["y64"], c["acc"], R.N_ADD_CONV3D_STATS), f"{what} stats_out")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(R.CONV3D_CASES))
def test_conv3d_t5_fp64(name, fmt):
    c = R.conv3d_case(name, fmt)
    wfrag, bp = packing.pack_conv3d_t5(c["weight"], c["bias"], dtype=R.DT[fmt])
    st = torch.zeros(c["frames"], 2, dtype=D, device=DEV)
    y = ops.conv3d_t5(c["img"].to(DEV), wfrag.to(DEV), bp.to(DEV), c["cout"], c["t"], stats_out=st)
    torch.cuda.synchronize()
    _check(y, c, f"conv3d_t5 {name} {fmt}")
    _check_conv3d_stats(st, c, f"conv3d_t5 {name} {fmt}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("cout", R.CONV3D_INDEXED_COUT)
def test_conv3d_t5_indexed_fp64(cout, fmt):
    """Against the fp64 reference itself, not against the plain kernel on gathered windows: an error common to both kernels shows."""
    c = R.conv3d_indexed_case(cout, fmt)
    wfrag, bp = packing.pack_conv3d_t5(c["weight"], c["bias"], dtype=R.DT[fmt])
    st = torch.zeros(len(c["src"]), 2, dtype=D, device=DEV)
    y = ops.conv3d_t5_indexed(c["img"].to(DEV), c["src"].to(DEV), c["lo"].to(DEV), c["hi"].to(DEV), wfrag.to(DEV), bp.to(DEV), cout, stats_out=st)
    torch.cuda.synchronize()
    _check(y, c, f"conv3d_t5_indexed {cout} {fmt}")
    _check_conv3d_stats(st, c, f"conv3d_t5_indexed {cout} {fmt}")


# ---- frame_affine --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(R.AFFINE_CASES))
def test_frame_affine_fp64(name, fmt):
    c = R.affine_case(name, fmt)
    gain, bias = c["gain"], c["bias"]
    if c["per_element"]:      # the reference's C,H,W order -> the blocked order the kernel indexes
        gain, bias = (packing.chw_to_blocked_vector(v, c["c"], c["h"], c["w"]) for v in (gain, bias))
    st = torch.zeros(c["frames"], 2, dtype=D, device=DEV)
    z = ops.frame_affine(packing.nchw_to_blocked(c["x"].float(), dtype=R.DT[fmt]).to(DEV), gain.to(DEV), bias.to(DEV), c["stats_in"].to(DEV),
                         stats_out=st, per_element=c["per_element"])
    torch.cuda.synchronize()
    _check(z, c, f"frame_affine {name} {fmt}")
    sums, _ = R.frame_sums(c["y64"])
    _check_sums(st, sums, R.unrounded_stats_bound(c["y64"], c["acc"], R.N_ADD_AFFINE_STATS), f"frame_affine {name} {fmt} stats_out")


@pytest.mark.parametrize("value", [2.0, 1.5])
@pytest.mark.parametrize("fmt", FMTS)
def test_frame_affine_constant_frame(fmt, value):
    """One frame of 32 x 8 x 8 = 2^11 equal values: the mean is the value and the variance is exactly 0 in fp64 (n is a power of two), rstd = rsqrt(eps) ~ 316.
    value = 2.0: mean * rstd is exact in fp32, the kernel's fma(x, rstd, -mean * rstd) is exactly 0 and the output is op16(bias[c]) BIT FOR BIT.
    value = 1.5: fl32(1.5 * rstd) may round, which leaves up to 2^-25 * 1.5 * rstd * |g| in front of the bias -- inside the bound (its `m * r * g` term is what
    allows for it), so that value is held to the bound, where y64 = bias exactly."""
    dt = R.DT[fmt]
    g = torch.Generator().manual_seed(7)
    gain = 1 + 0.2 * torch.randn(32, generator=g)
    bias = 0.1 * torch.randn(32, generator=g)
    x = torch.full((1, 32, 8, 8), value).to(dt)
    stats_in, _ = R.frame_sums(x)
    y64, bound, _ = R.affine_ref(x, stats_in, gain, bias, fmt)
    assert torch.equal(y64, bias.double().view(1, 32, 1, 1).expand(1, 32, 8, 8))
    z = ops.frame_affine(packing.nchw_to_blocked(x.float(), dtype=dt).to(DEV), gain.to(DEV), bias.to(DEV), stats_in.to(DEV))
    torch.cuda.synchronize()
    z = packing.blocked_to_nchw(z.cpu(), 32, 8, 8)
    if value == 2.0:
        assert torch.equal(_bits(z.to(dt)), _bits(bias.to(dt).view(1, 32, 1, 1).expand(1, 32, 8, 8)))
    worst, msg = R.failure(z.double(), y64, bound, f"frame_affine constant {value} {fmt}")
    assert msg is None, msg
