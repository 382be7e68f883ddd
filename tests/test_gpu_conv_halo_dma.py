"""The halo-DMA instantiations of vpt_conv3x3_kernel (forward modes 0, 1, 5 and the pool-fused mode 4 on an even count of 32-channel blocks: two
dense halo images filled by buffer loads to LDS, a four-slot weight ring, two-tap steps) against the register-staged instantiation the launch
function keeps for every other case.  Needs an MI355X.

The K order of every accumulator is the same in both, so outputs and frame statistics must agree BIT FOR BIT -- no tolerance anywhere in this file.
The kept path is reached through the launch function's own selector, forced with vpt_conv3x3_set_halo_dma(0) (a test hook of the library, like
vpt_conv3x3_set_trace; a negative argument restores the shipped selection, which every test does).

  * bitwise: (16, 16) one tile with every border, (32, 32) interior tile seams, (16, 48) column seams; cin 64 / 128 = one / two passes of the loop;
    cout 128 / 160 = the second with an odd count of 32-channel blocks (a wave with one valid block); three frames; both operand formats.
  * odd block count: cin = 96 takes the kept path whatever the selector says and meets the fp64 bound of tests/test_gpu_conv_mfma16.py.
  * NaN surround: the new path zero-fills the padding through the buffer resource's range check alone.  The input is a view into a larger allocation
    whose other elements hold NaN bit patterns: any padding chunk that is read instead of zero-filled turns the output into NaN."""
import contextlib
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import _native, ops, packing  # noqa: E402
from tests import test_gpu_conv_mfma16 as M16  # noqa: E402

DEV = "cuda"
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
FRAMES = 3


@contextlib.contextmanager
def halo_dma(fmt, on):
    lib = _native.load(fmt)
    lib.vpt_conv3x3_set_halo_dma.argtypes, lib.vpt_conv3x3_set_halo_dma.restype = [ctypes.c_int], ctypes.c_int
    lib.vpt_conv3x3_set_halo_dma(-1 if on else 0)      # -1: the shipped selection, 0: the register-staged path everywhere
    try:
        yield
    finally:
        lib.vpt_conv3x3_set_halo_dma(-1)


def _operands(h, w, cin, cout, fmt, seed):
    dt = DT[fmt]
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(cout, cin, 3, 3, generator=g) * (1.6 / (cin * 9) ** 0.5)
    gain = 1 + 0.2 * torch.randn(cin, generator=g)
    bias = 0.1 * torch.randn(cin, generator=g)
    x = (torch.relu(torch.randn(FRAMES, cin, h, w, generator=g)) + 0.2 * torch.randn(FRAMES, cin, h, w, generator=g)).to(dt)
    res = torch.randn(FRAMES, cout, h, w, generator=g).to(dt)
    wpk, sa, sg = ops.pack_conv3x3(W.to(DEV), gain.to(DEV), bias.to(DEV), dtype=dt)
    flat = x.double().reshape(FRAMES, -1)
    st_in = torch.stack([flat.sum(1), (flat * flat).sum(1)], 1).contiguous().to(DEV)
    return dict(cout=cout, wpk=wpk, sa=sa, sg=sg, st_in=st_in, xb=packing.nchw_to_blocked(x.float(), dtype=dt).to(DEV),
                resb=packing.nchw_to_blocked(res.float(), dtype=dt).to(DEV),
                kk=(0.3 * torch.randn(FRAMES, 9, sa.shape[1], generator=g)).to(DEV), rs=(0.5 + torch.rand(FRAMES, generator=g)).to(DEV),
                rsc=(0.5 + torch.rand(FRAMES, generator=g)).to(DEV), rb=(0.3 * torch.randn(FRAMES, cout, generator=g)).to(DEV))


def _run_modes(c, xb=None):
    """{mode: (output, frame statistics)} of modes 0, 1, 5 and 4 through the launch function's current selection (mode 4: the pooled tensor of the
    convolution and its seam pass; modes 0, 1, 5 write no masks, and mode 7 keeps the register-staged path)."""
    xb = c["xb"] if xb is None else xb
    out = {}
    for mode in (0, 1, 5):
        st = torch.zeros(FRAMES, 2, dtype=torch.float64, device=DEV)
        if mode == 5:
            y = ops.conv3x3_folded(xb, c["wpk"], c["sa"], c["sg"], c["st_in"], c["cout"], kk_frame=c["kk"], rs_frame=c["rs"], res=c["resb"],
                                   res_scale=c["rsc"], res_bias=c["rb"], stats_out=st)
        else:
            y = ops.conv3x3(xb, c["wpk"], c["sa"], c["sg"], c["st_in"], c["cout"], res=c["resb"] if mode == 1 else None, stats_out=st)
        out[mode] = (y, st)
    st4 = torch.zeros(FRAMES, 2, dtype=torch.float64, device=DEV)
    out[4] = (ops.conv3x3_pool(xb, c["wpk"], c["sa"], c["sg"], c["st_in"], c["cout"], stats_out=st4), st4)
    torch.cuda.synchronize()
    return out


def _assert_bitwise(got, want, what):
    for mode in want:
        y, st = got[mode]
        y0, st0 = want[mode]
        neq = y.view(torch.int16) != y0.view(torch.int16)
        assert not bool(neq.any()), f"{what} mode {mode}: {int(neq.sum())} of {neq.numel()} outputs differ; first at {neq.nonzero()[0].tolist()}"
        assert torch.equal(st.view(torch.int64), st0.view(torch.int64)), f"{what} mode {mode}: frame statistics differ: {st.tolist()} / {st0.tolist()}"


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("cout", [128, 160])
@pytest.mark.parametrize("cin", [64, 128])
@pytest.mark.parametrize("hw", [(16, 16), (32, 32), (16, 48)])
def test_halo_dma_bitwise_against_the_kept_path(hw, cin, cout, fmt):
    c = _operands(hw[0], hw[1], cin, cout, fmt, seed=hw[0] * 1000 + hw[1] * 10 + cin + cout)
    with halo_dma(fmt, False):
        want = _run_modes(c)
    with halo_dma(fmt, True):
        got = _run_modes(c)
    _assert_bitwise(got, want, f"{hw} cin {cin} cout {cout} {fmt}")


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_odd_block_count_takes_the_kept_path(fmt):
    """cin = 96 (three channel blocks): same bits with the selector on and off, and the fp64 bound of the project's forward reference."""
    c = M16._case("loop_once", fmt)
    mean, rstd = M16._mean_rstd(c)
    y64 = torch.relu(rstd * c["conv"] + c["sa_e"].unsqueeze(0) - rstd * mean * c["sg_e"].unsqueeze(0))
    ys = []
    for on in (True, False):
        with halo_dma(fmt, on):
            st = torch.zeros(c["frames"], 2, dtype=torch.float64, device=DEV)
            ys.append((ops.conv3x3(c["xb"], c["wpk"], c["sa"], c["sg"], c["st_in"], c["cout"], stats_out=st), st))
            torch.cuda.synchronize()
    assert torch.equal(ys[0][0].view(torch.int16), ys[1][0].view(torch.int16)) and torch.equal(ys[0][1], ys[1][1])
    M16._check(c, fmt, ys[0][0], y64, rstd, f"conv3x3 cin 96 {fmt}")
    M16._check_stats(ys[0][1], ys[0][0], f"conv3x3 cin 96 {fmt}")


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("hw", [(16, 16), (32, 32)])
def test_nan_surround_padding_is_zero(hw, fmt):
    c = _operands(hw[0], hw[1], 64, 128, fmt, seed=77 + hw[0])
    n = c["xb"].numel()
    pad = 64 * 1024                                    # elements in front and behind: more than any halo row of these shapes
    big = torch.full((n + 2 * pad,), float("nan"), dtype=DT[fmt], device=DEV)
    big[pad:pad + n] = c["xb"].reshape(-1)
    view = big[pad:pad + n].view(c["xb"].shape)
    assert bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[pad + n:]).all())
    with halo_dma(fmt, True):
        want = _run_modes(c)
        got = _run_modes(c, xb=view)
    for mode, (y, st) in got.items():
        assert bool(torch.isfinite(y.float()).all()), f"mode {mode}: {int((~torch.isfinite(y.float())).sum())} non-finite outputs: padding was read, not zero-filled"
        assert bool(torch.isfinite(st).all())
    _assert_bitwise(got, want, f"NaN surround {hw} {fmt}")
