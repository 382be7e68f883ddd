"""The forward modes of vpt_conv3x3_kernel on the 16x16x32 MFMA loop with the exchange-free epilogue, held to an fp64 convolution
of the SAME 16-bit-rounded operands (W' = op16(W * gain), x as stored), so only the kernel's own arithmetic is judged.  Needs an MI355X.

Bound per element, derived and not tuned (K = 9 * Cin):

    |y - y64| <= ulp16(y64) + (K + 8) * 2^-24 * rstd * conv(|W'|, |x|)

one unit in the last place of the stored format, plus the worst-case fp32 accumulation error of K products and the epilogue's few
operations.  Shapes are the smallest at which each code path of the kernel can go wrong: one channel block (zeroed accumulators, no loop),
two (first + last block, loop body never runs), three (loop body once); a wave with one valid 32-cout block (cout = 96), two channel
tiles with the second partial (cout = 160); one tile with all nine edge classes, seams in one direction only, interior tiles."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops, packing  # noqa: E402
from tests import cnn_forward_ref as R  # noqa: E402

DEV = "cuda"
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
MANT = {"bf16": 7, "fp16": 10}
EMIN = {"bf16": -126, "fp16": -14}

#        name        frames h   w   cin cout
CASES = {"one_block": (1, 16, 16, 32, 96),      # cin = 32: one channel block; cout = 96: a wave with one valid block; all nine edge classes in one tile
         "two_blocks": (1, 48, 16, 64, 160),    # cin = 64: first + last block; cout = 160: second channel tile partial; row seams only
         "loop_once": (1, 16, 80, 96, 128),     # cin = 96: loop body once; column seams only
         "interior": (2, 64, 64, 64, 128)}      # interior tiles, 2 frames, whole 32-row bands


def _ulp16(v, fmt):
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** EMIN[fmt]))).clamp(min=EMIN[fmt])
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT[fmt])


def _edge_class(h, w):
    ey = torch.ones(h, dtype=torch.long); ey[0] = 0; ey[-1] = 2
    ex = torch.ones(w, dtype=torch.long); ex[0] = 0; ex[-1] = 2
    return ey.view(h, 1) * 3 + ex.view(1, w)          # [h, w]


@functools.lru_cache(maxsize=None)
def _case(name, fmt):
    """Operands on the device + the fp64 pieces every test of the case shares (computed once, never modified)."""
    frames, h, w, cin, cout = CASES[name]
    dt = DT[fmt]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    W = torch.randn(cout, cin, 3, 3, generator=g) * (1.6 / (cin * 9) ** 0.5)
    gain = 1 + 0.2 * torch.randn(cin, generator=g)
    bias = 0.1 * torch.randn(cin, generator=g)
    x = (torch.relu(torch.randn(frames, cin, h, w, generator=g)) + 0.2 * torch.randn(frames, cin, h, w, generator=g)).to(dt)
    res = torch.randn(frames, cout, h, w, generator=g).to(dt)
    wpk, sa, sg = ops.pack_conv3x3(W.to(DEV), gain.to(DEV), bias.to(DEV), dtype=dt)
    w16 = (W * gain.view(1, -1, 1, 1)).to(dt).double()             # W' = op16(W * gain): what the packed image holds
    x64 = x.double()
    flat = x64.reshape(frames, -1)
    st_in = torch.stack([flat.sum(1), (flat * flat).sum(1)], 1).contiguous()
    conv = F.conv2d(x64, w16, padding=1)                           # [F, cout, h, w]
    conv_abs = F.conv2d(x64.abs(), w16.abs(), padding=1)
    e = _edge_class(h, w)
    sa_e = sa.cpu().double()[:, :cout][e]                          # [h, w, cout]
    sg_e = sg.cpu().double()[:, :cout][e]
    return dict(frames=frames, h=h, w=w, cin=cin, cout=cout, dt=dt, wpk=wpk, sa=sa, sg=sg, st_in=st_in.to(DEV), st_in_cpu=st_in,
                xb=packing.nchw_to_blocked(x.float(), dtype=dt).to(DEV), resb=packing.nchw_to_blocked(res.float(), dtype=dt).to(DEV),
                res64=res.double(), conv=conv, conv_abs=conv_abs, e=e,
                sa_e=sa_e.permute(2, 0, 1), sg_e=sg_e.permute(2, 0, 1))


def _mean_rstd(c):
    n = c["cin"] * c["h"] * c["w"]
    m = c["st_in_cpu"][:, 0] / n
    var = (c["st_in_cpu"][:, 1] / n - m * m).clamp(min=0)
    mean = m.float().double()
    rstd = 1.0 / torch.sqrt(var.float().double() + 1e-5)
    return mean.view(-1, 1, 1, 1), rstd.view(-1, 1, 1, 1)


def _check(c, fmt, y_blocked, y64, rstd, what):
    y = packing.blocked_to_nchw(y_blocked.cpu(), c["cout"], c["h"], c["w"]).double()
    k = 9 * c["cin"]
    bound = _ulp16(y64, fmt) + (k + 8) * 2.0 ** -24 * rstd * c["conv_abs"]
    err = (y - y64).abs()
    worst = (err / bound).max().item()
    print(f"{what}: max |y - y64| = {err.max().item():.3e}, max err / bound = {worst:.3f}")
    assert worst <= 1.0, f"{what}: {int((err > bound).sum())} of {err.numel()} elements beyond the bound (worst ratio {worst:.3f})"


def _check_stats(st_out, y_blocked, what):
    """The kernel sums the values it STORED: against the fp64 sums of its own output, within the fp32 summation error of one tile (tests/cnn_forward_ref.py,
    N_ADD_FWD16: the counted chain of the 16-row instantiations, halo DMA included)."""
    want, allowed = R.stored_stats_ref(y_blocked.cpu(), R.N_ADD_FWD16)
    worst, msg = R.stats_failure(st_out, want, allowed, f"{what} stats_out")
    print(f"{what} stats_out: worst err / bound {worst:.4f}")
    assert msg is None, msg


@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_conv3x3_fp64(name, fmt, use_res):
    """Modes 0 (no residual) and 1 (residual) against the fp64 convolution; frame statistics to the derived summation bound."""
    c = _case(name, fmt)
    mean, rstd = _mean_rstd(c)
    y64 = torch.relu(rstd * c["conv"] + c["sa_e"].unsqueeze(0) - rstd * mean * c["sg_e"].unsqueeze(0))
    if use_res:
        y64 = y64 + c["res64"]
    st_out = torch.zeros(c["frames"], 2, dtype=torch.float64, device=DEV)
    y = ops.conv3x3(c["xb"], c["wpk"], c["sa"], c["sg"], c["st_in"], c["cout"], res=c["resb"] if use_res else None, stats_out=st_out)
    torch.cuda.synchronize()
    _check(c, fmt, y, y64, rstd, f"conv3x3 {name} {fmt} res={use_res}")
    _check_stats(st_out, y, f"conv3x3 {name} {fmt} res={use_res}")


@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["one_block", "two_blocks", "interior"])
def test_conv3x3_folded_fp64(name, fmt, use_res):
    """Per-frame epilogue table (kk_frame, rs_frame) alone (mode 0) and with the residual through a per-frame affine
    res_scale * res + res_bias (mode 5):  out = relu(rs * acc + kk_frame[f][e][o]) + res_scale[f] * res + res_bias[f][o]."""
    c = _case(name, fmt)
    frames, cout = c["frames"], c["cout"]
    g = torch.Generator().manual_seed(5)
    kk = 0.3 * torch.randn(frames, 9, c["sa"].shape[1], generator=g)
    rs = 0.5 + torch.rand(frames, generator=g)
    rsc = 0.5 + torch.rand(frames, generator=g)
    rb = 0.3 * torch.randn(frames, cout, generator=g)
    rstd = rs.double().view(-1, 1, 1, 1)
    kk_e = kk.double()[:, :, :cout][:, c["e"]].permute(0, 3, 1, 2)          # [F, cout, h, w]
    y64 = torch.relu(rstd * c["conv"] + kk_e)
    if use_res:
        y64 = y64 + rsc.double().view(-1, 1, 1, 1) * c["res64"] + rb.double().view(frames, cout, 1, 1)
    st_out = torch.zeros(frames, 2, dtype=torch.float64, device=DEV)
    y = ops.conv3x3_folded(c["xb"], c["wpk"], c["sa"], c["sg"], c["st_in"], cout, kk_frame=kk.to(DEV), rs_frame=rs.to(DEV),
                           res=c["resb"] if use_res else None, res_scale=rsc.to(DEV) if use_res else None,
                           res_bias=rb.to(DEV) if use_res else None, stats_out=st_out)
    torch.cuda.synchronize()
    _check(c, fmt, y, y64, rstd, f"conv3x3_folded {name} {fmt} res={use_res}")
    _check_stats(st_out, y, f"conv3x3_folded {name} {fmt} res={use_res}")


@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_pool_fused_equals_conv_then_pool(name, fmt, masks):
    """Modes 4 (inference) and 7 (training, arg-max masks): the pooled tensor equals mode 0 followed by ops.maxpool BIT FOR BIT."""
    c = _case(name, fmt)
    pre = ops.conv3x3(c["xb"], c["wpk"], c["sa"], c["sg"], c["st_in"], c["cout"])
    st_a = torch.zeros(c["frames"], 2, dtype=torch.float64, device=DEV)
    want = ops.maxpool(pre, stats_out=st_a)
    st_b = torch.zeros(c["frames"], 2, dtype=torch.float64, device=DEV)
    mask = None
    if masks:
        got, mask = ops.conv3x3_pool_argmax(c["xb"], c["wpk"], c["sa"], c["sg"], c["st_in"], c["cout"], stats_out=st_b)
    else:
        got = ops.conv3x3_pool(c["xb"], c["wpk"], c["sa"], c["sg"], c["st_in"], c["cout"], stats_out=st_b)
    torch.cuda.synchronize()
    neq = got.view(torch.int16) != want.view(torch.int16)
    assert not bool(neq.any()), f"{int(neq.sum())} of {neq.numel()} pooled values differ; first at {neq.nonzero()[0].tolist()}"
    assert torch.allclose(st_a, st_b, rtol=1e-6, atol=1e-3), (st_a, st_b)
    if masks:      # bit 8 - k set = window position k = 3 (dy + 1) + (dx + 1) differs from the maximum or lies outside the image, derived from mode 0's output
        h, w = c["h"], c["w"]
        p = F.pad(pre.view(torch.int16).cpu().to(torch.int32).permute(0, 1, 4, 2, 3), (1, 1, 1, 1), value=-1)   # post-ReLU patterns are >= 0
        mx = want.view(torch.int16).cpu().to(torch.int32).permute(0, 1, 4, 2, 3)
        want_mask = torch.zeros_like(mx)
        for k in range(9):
            win = p[..., k // 3:k // 3 + h:2, k % 3:k % 3 + w:2]
            want_mask |= (win != mx).to(torch.int32) << (8 - k)
        got_mask = mask.cpu().to(torch.int32).permute(0, 1, 4, 2, 3) & 0x1ff
        assert torch.equal(got_mask, want_mask), f"{int((got_mask != want_mask).sum())} arg-max masks differ"


@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_32_row_tiles_equal_16_row_tiles(fmt, use_res):
    """The eight-wave 32-row tiles run the same per-pixel program as the 16-row tiles: bit-identical outputs."""
    c = _case("interior", fmt)
    res = c["resb"] if use_res else None
    y16 = ops.conv3x3(c["xb"], c["wpk"], c["sa"], c["sg"], c["st_in"], c["cout"], res=res, tiling="throughput")
    y32 = ops.conv3x3(c["xb"], c["wpk"], c["sa"], c["sg"], c["st_in"], c["cout"], res=res, tiling="throughput32")
    torch.cuda.synchronize()
    assert torch.equal(y16.view(torch.int16), y32.view(torch.int16))
