"""The kernels behind the CNN gradients -- vpt_conv_bwd_prep_kernel (dy, dy + res, arg-max bytes), vpt_conv_bwd_prep_pooled_kernel,
vpt_conv_backward_reduce, vpt_conv3x3_dgrad_kernel modes 2 / 3 / 6 and vpt_conv_wgrad_kernel<16|32|64> with its reduce -- held per element to the
fp64 reference of tests/cnn_backward_ref.py on the SAME stored 16-bit tensors, in both operand formats.  Needs an MI355X.

The forward runs once per case on the GPU (ops.conv3x3) so that the stored output has realistic gates; every backward op and the reference
then read the same stored tensors, so both open exactly the same ReLU gates (prepare: y - res > 0; pooled: P > 0; gated dgrad: xin > 0) and
only the kernel's arithmetic is judged.  The dgrad and wgrad operand is the reference's dacc rounded to 16 bits (the kernels take any operand).

Every bound is derived in the docstring of tests/cnn_backward_ref.py (u = 2^-24; tests/test_cnn_backward_ref_cpu.py shows that plain fp32
arithmetic meets them) and none is a fitted constant:
    dacc     ulp16 + 4u |dacc|   (+ 3u rstd sum|routed| for the pooled entries), zero pattern exact above the format's smallest subnormal
    dx       ulp16 + (9 Cout + 8) u convT(|dacc|, |W'|) + 8u (|skip| + |c0| + |c1 xin|);   gated: fp32 part x rstd0, zero pattern of xin
    dw_raw   (n + g + 2) u sum|dacc||x|, n = frames H W, g = frame groups;  with `out=` + u |out| for the reduce kernel's final add
    d_sa, d_sg, T1, T2, gate_u   n u sum|terms| + u |value| (+ the fp32 factor of every term where there is one);  coef: propagated
Each check prints `max err / bound` and asserts <= 1, naming the worst element's frame, channel block, pixel, edge class and tile position.
In fp16 dY is scaled by 1e-2 (the loss scale's job in training: the gradients must stay inside the format).

Shapes (frames, H, W, cin, cout) are the smallest that reach each path; the dgrad main loop runs over cout blocks, its output tile over cin:
    one_block   one cout block (no loop), an output wave with one valid 32-channel block, all nine edge classes in one tile
    two_blocks  first + last block, a second output tile that is partial, row seams only, H != W
    loop_once   loop body once, column seams only
    interior    interior tiles, two frames
The block cases (gated dgrad + reduce) take cin = cout = the case's cin (96, 160, 128), which keeps the partial output tiles in the gated epilogue."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import _native, ops, packing  # noqa: E402
from vpt_amd.training import conv_param_grads  # noqa: E402
from tests import cnn_backward_ref as R  # noqa: E402

DEV = "cuda"
#        name         frames h   w   cin  cout
CASES = {"one_block": (1, 16, 16, 96, 32),
         "two_blocks": (1, 48, 16, 160, 64),
         "loop_once": (1, 16, 80, 128, 96),
         "interior": (2, 64, 64, 128, 64)}
BLOCK_CASES = ["one_block", "two_blocks", "interior"]
POOL_CASES = ["one_block", "interior"]
#               frames h   w   cin  cout  out=
WGRAD_SHAPES = [(3, 16, 16, 96, 160, False),     # three cin blocks: the last pair half empty; partial second cout tile
                (2, 48, 32, 32, 128, False),     # H != W, one cin block
                (1, 64, 64, 64, 32, False),      # one cout block of four
                (33, 8, 16, 256, 256, False),    # 8 tiles, 17 frame groups of 2, the last holding one frame: the f1 = min(...) clamp, the reduce over groups
                (2, 16, 16, 64, 64, True)]       # out= given and pre-filled: the kernel adds


def _nchw(t, c, h, w):
    return packing.blocked_to_nchw(t.cpu(), c, h, w).double()


def _blocked(t, dt):
    return packing.nchw_to_blocked(t.float(), dtype=dt).to(DEV)


def _layer_params(g, cin, cout):
    W = torch.randn(cout, cin, 3, 3, generator=g) * (1.6 / (cin * 9) ** 0.5)
    return W, 1 + 0.2 * torch.randn(cin, generator=g), 0.1 * torch.randn(cin, generator=g)


def _act(g, dt, *shape, scale=1.0):
    return (scale * torch.randn(*shape, generator=g)).to(dt)


@functools.lru_cache(maxsize=None)
def _case(name, fmt):
    """Operands on the device, the GPU forward's stored outputs and their fp64 copies (computed once, never modified)."""
    frames, h, w, cin, cout = CASES[name]
    dt = R.DT[fmt]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    W, gain, bias = _layer_params(g, cin, cout)
    x = (torch.relu(torch.randn(frames, cin, h, w, generator=g)) + 0.2 * torch.randn(frames, cin, h, w, generator=g)).to(dt)
    gs = 1e-2 if fmt == "fp16" else 1.0
    res, dy, skip = _act(g, dt, frames, cout, h, w), _act(g, dt, frames, cout, h, w, scale=gs), _act(g, dt, frames, cin, h, w, scale=gs)
    dp = _act(g, dt, frames, cout, h // 2, w // 2, scale=gs)
    wpk, sa, sg = ops.pack_conv3x3(W.to(DEV), gain.to(DEV), bias.to(DEV), dtype=dt)
    st = R.stats_of(x)
    c = dict(frames=frames, h=h, w=w, cin=cin, cout=cout, dt=dt, W=W, gain=gain, bias=bias, wpk=wpk, sa=sa, sg=sg, sa64=sa.cpu().double(), sg64=sg.cpu().double(),
             wt=packing.pack_conv3x3_dgrad(W.to(DEV), gain.to(DEV), dtype=dt), w16=(W * gain.view(1, -1, 1, 1)).to(dt).double(),
             st=st, st_dev=st.to(DEV), x64=x.double(), res64=res.double(), dy64=dy.double(), skip64=skip.double(), dp64=dp.double(),
             xb=_blocked(x, dt), resb=_blocked(res, dt), dyb=_blocked(dy, dt), skipb=_blocked(skip, dt), dpb=_blocked(dp, dt))
    c["yb"] = {False: ops.conv3x3(c["xb"], wpk, sa, sg, c["st_dev"], cout), True: ops.conv3x3(c["xb"], wpk, sa, sg, c["st_dev"], cout, res=c["resb"])}
    torch.cuda.synchronize()
    c["y64"] = {k: _nchw(v, cout, h, w) for k, v in c["yb"].items()}
    return c


@functools.lru_cache(maxsize=None)
def _prepare_reference(name, fmt, use_res):
    c = _case(name, fmt)
    return R.prepare_ref(c["dy64"], c["y64"][use_res], c["res64"] if use_res else None, c["st"], c["sa64"], c["sg64"], c["cin"], fp32_stats=True)


def _check_zero_pattern(what, got, want, fmt):
    small = want.abs() < R.tiny16(fmt)
    bad = ((got == 0) != (want == 0)) & ~small
    if bool(bad.any()):
        idx = [int(i) for i in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {int(bad.sum())} elements are zero on one side only; first at {R.describe(idx, tuple(want.shape), 'nchw')}: "
                             f"got {float(got[tuple(idx)])} want {float(want[tuple(idx)])}")


def _check_prepare(what, c, fmt, r, outs, factor_u=0, dacc=True):
    """outs = (dacc blocked or None, coef, d_sa, d_sg, t12) from the GPU against the namespace r of prepare_ref / reduce_ref."""
    cout, h, w = c["cout"], c["h"], c["w"]
    if dacc:
        got = _nchw(outs[0], cout, h, w)
        _check_zero_pattern(f"{what} dacc", got, r.dacc, fmt)
        R.check(f"{what} dacc", got, r.dacc, R.bound_dacc(r, fmt), "nchw")
    b = R.bounds_tables(r, c["frames"], cout * h * w, factor_u)
    coef, d_sa, d_sg, t12 = (t.cpu().double() for t in outs[1:])
    R.check(f"{what} d_sa", d_sa[:, :cout], r.d_sa, b.d_sa, "table")
    R.check(f"{what} d_sg", d_sg[:, :cout], r.d_sg, b.d_sg, "table")
    assert not bool(d_sa[:, cout:].any()) and not bool(d_sg[:, cout:].any()), f"{what}: the tables' padding columns must stay zero"
    R.check(f"{what} T1", t12[:, 0], r.T1, b.T1)
    R.check(f"{what} T2", t12[:, 1], r.T2, b.T2)
    R.check(f"{what} coef", coef, r.coef, b.coef)


@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_prepare_fp64(name, fmt, use_res):
    """vpt_conv_bwd_prep_kernel<dy> and <dy, res> + the finish and sum kernels."""
    c = _case(name, fmt)
    r = _prepare_reference(name, fmt, use_res)
    outs = ops.conv_backward_prepare(c["dyb"], c["yb"][use_res], c["resb"] if use_res else None, c["st_dev"], c["sa"], c["sg"], c["cin"], want_t12=True)
    torch.cuda.synchronize()
    _check_prepare(f"prepare {name} {fmt} res={use_res}", c, fmt, r, outs)


@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", POOL_CASES)
def test_prepare_pooled_fp64(name, fmt, masks):
    """The pooled entries: the arg-max bytes of ops.maxpool (vpt_conv_bwd_prep_kernel<no dy>) and the 9-bit masks of ops.conv3x3_pool_argmax
    (vpt_conv_bwd_prep_pooled_kernel), against torch's first-maximum routing on the stored pre-pool tensor."""
    c = _case(name, fmt)
    pre = c["yb"][False]
    r = R.prepare_ref(None, c["y64"][False], None, c["st"], c["sa64"], c["sg64"], c["cin"], dpooled=c["dp64"], fp32_stats=True)
    if masks:
        pooled, mask = ops.conv3x3_pool_argmax(c["xb"], c["wpk"], c["sa"], c["sg"], c["st_dev"], c["cout"])
        outs = ops.conv_backward_prepare_pooled(c["dpb"], pooled, mask, c["st_dev"], c["sa"], c["sg"], c["cin"], want_t12=True)
    else:
        _, am = ops.maxpool(pre, want_argmax=True)
        outs = ops.conv_backward_prepare(None, pre, None, c["st_dev"], c["sa"], c["sg"], c["cin"], dpooled=c["dpb"], argmax=am, want_t12=True)
    torch.cuda.synchronize()
    _check_prepare(f"prepare pooled {name} {fmt} masks={masks}", c, fmt, r, outs)


@functools.lru_cache(maxsize=None)
def _dgrad_reference(name, fmt):
    """(the operand: the reference's dacc rounded to 16 bits, its fp32 coefficients, R.dgrad_ref without skip, conv^T of the magnitudes)."""
    c = _case(name, fmt)
    r = _prepare_reference(name, fmt, True)
    dacc16, coef = r.dacc.to(c["dt"]), r.coef.float()
    return (dacc16, coef) + R.dgrad_ref(dacc16.double(), c["w16"], None, c["x64"], coef)


@pytest.mark.parametrize("use_skip", [False, True])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_dgrad_fp64(name, fmt, use_skip):
    """vpt_conv3x3_dgrad_kernel modes 2 (no skip) and 3 (skip) on the reference's operand rounded to 16 bits."""
    c = _case(name, fmt)
    dacc16, coef, dx0, conv_abs = _dgrad_reference(name, fmt)
    dx = ops.conv3x3_dgrad(_blocked(dacc16, c["dt"]), c["wt"], c["cin"], skip=c["skipb"] if use_skip else None, xin=c["xb"], coef=coef.to(DEV))
    torch.cuda.synchronize()
    skip = c["skip64"] if use_skip else None
    dx64 = dx0 if skip is None else dx0 + skip
    R.check(f"dgrad {name} {fmt} skip={use_skip}", _nchw(dx, c["cin"], c["h"], c["w"]), dx64, R.bound_dx(dx64, fmt, c["cout"], conv_abs, skip, coef, c["x64"]), "nchw")


@functools.lru_cache(maxsize=None)
def _block(name, fmt):
    """A residual block x + conv1(conv0(x)) with ch = the case's cin: GPU forward, conv1's reference operand, fp64 copies."""
    frames, h, w, ch, _ = CASES[name]
    dt = R.DT[fmt]
    g = torch.Generator().manual_seed(7 + sum(map(ord, name)))
    (W0, g0, b0), (W1, g1, b1) = _layer_params(g, ch, ch), _layer_params(g, ch, ch)
    x = (torch.relu(torch.randn(frames, ch, h, w, generator=g)) + 0.2 * torch.randn(frames, ch, h, w, generator=g)).to(dt)
    dout = _act(g, dt, frames, ch, h, w, scale=1e-2 if fmt == "fp16" else 1.0)
    wpk0, sa0, sg0 = ops.pack_conv3x3(W0.to(DEV), g0.to(DEV), b0.to(DEV), dtype=dt)
    wpk1, sa1, sg1 = ops.pack_conv3x3(W1.to(DEV), g1.to(DEV), b1.to(DEV), dtype=dt)
    xb = _blocked(x, dt)
    st_x = R.stats_of(x)
    st_y_dev = torch.zeros(frames, 2, dtype=torch.float64, device=DEV)
    yb = ops.conv3x3(xb, wpk0, sa0, sg0, st_x.to(DEV), ch, stats_out=st_y_dev)
    ob = ops.conv3x3(yb, wpk1, sa1, sg1, st_y_dev, ch, res=xb)
    torch.cuda.synchronize()
    y64, out64 = _nchw(yb, ch, h, w), _nchw(ob, ch, h, w)
    st_y = R.stats_of(y64)                      # the statistics of the STORED tensor, which is what the forward accumulates
    r1 = R.prepare_ref(dout.double(), out64, x.double(), st_y, sa1.cpu().double(), sg1.cpu().double(), ch, fp32_stats=True)
    return dict(frames=frames, h=h, w=w, cin=ch, cout=ch, dt=dt, sa0=sa0, sg0=sg0, sa0_64=sa0.cpu().double(), sg0_64=sg0.cpu().double(),
                wt1=packing.pack_conv3x3_dgrad(W1.to(DEV), g1.to(DEV), dtype=dt), w16_1=(W1 * g1.view(1, -1, 1, 1)).to(dt).double(),
                yb=yb, y64=y64, st_x=st_x, st_x_dev=st_x.to(DEV), dacc1=r1.dacc.to(dt), coef1=r1.coef.float())


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", BLOCK_CASES)
def test_gated_dgrad_and_reduce_fp64(name, fmt):
    """vpt_conv3x3_dgrad_kernel mode 6 (conv0's operand rstd0 (conv^T + c0 + c1 xin) [xin > 0] and gate_u) and, on the operand it stored,
    vpt_conv_bwd_prep_kernel<pre-gated> = ops.conv_backward_reduce."""
    b = _block(name, fmt)
    ch, h, w = b["cin"], b["h"], b["w"]
    dacc0, gate_u = ops.conv3x3_dgrad_gated(_blocked(b["dacc1"], b["dt"]), b["wt1"], ch, b["yb"], b["coef1"].to(DEV), b["st_x_dev"], ch)
    outs = ops.conv_backward_reduce(dacc0, gate_u, b["st_x_dev"], b["sa0"], b["sg0"], ch, want_t12=True)
    torch.cuda.synchronize()
    want, want_u, conv_abs, rstd0, abs_u = R.dgrad_gated_ref(b["dacc1"].double(), b["w16_1"], b["y64"], b["coef1"], b["st_x"], ch, fp32_stats=True)
    got = _nchw(dacc0, ch, h, w)
    _check_zero_pattern(f"gated dgrad {name} {fmt}", got, want, fmt)
    R.check(f"gated dgrad {name} {fmt}", got, want, R.bound_dx(want, fmt, ch, conv_abs, None, b["coef1"], b["y64"], scale=rstd0), "nchw")
    R.check(f"gated dgrad {name} {fmt} gate_u", gate_u.cpu(), want_u, R.bound_sum(ch * h * w, abs_u, want_u))
    r0 = R.reduce_ref(got, gate_u.cpu(), b["st_x"], b["sa0_64"], b["sg0_64"], ch, fp32_stats=True)
    _check_prepare(f"reduce {name} {fmt}", b, fmt, r0, (None,) + tuple(outs), factor_u=8, dacc=False)


@functools.lru_cache(maxsize=None)
def _wgrad_operands(i, fmt):
    frames, h, w, cin, cout, _ = WGRAD_SHAPES[i]
    g = torch.Generator().manual_seed(140 + i)
    dacc, x = _act(g, R.DT[fmt], frames, cout, h, w, scale=1e-2 if fmt == "fp16" else 1.0), _act(g, R.DT[fmt], frames, cin, h, w)
    return dacc, x, R.wgrad_ref(dacc.double(), x.double())


def _wgrad_groups(fmt, frames, cin, cout):
    return _native.load(fmt).vpt_conv3x3_wgrad_scratch_floats(frames, cin, cout) // (cout * 9 * cin)      # scratch = [groups][Cout][9][Cin]


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("i", range(len(WGRAD_SHAPES)))
def test_wgrad_fp64(i, fmt):
    """vpt_conv_wgrad_kernel<W> + vpt_conv_wgrad_reduce_kernel per (cout, tap, cin)."""
    frames, h, w, cin, cout, prefill = WGRAD_SHAPES[i]
    dacc, x, (dw64, dw_abs) = _wgrad_operands(i, fmt)
    groups = _wgrad_groups(fmt, frames, cin, cout)
    if i == 3:
        assert groups == 17, groups
    bound = R.bound_dw(frames * h * w, groups, dw_abs)
    out = None
    if prefill:
        out0 = torch.randn(cout, 9, cin, generator=torch.Generator().manual_seed(5))
        out = out0.to(DEV)
        dw64 = dw64 + out0.double()
        bound = bound + R.U * dw64.abs()       # vpt_conv_wgrad_reduce_kernel: `*d = *d + s`, one more fp32 addition
    got = ops.conv3x3_wgrad(_blocked(dacc, R.DT[fmt]), _blocked(x, R.DT[fmt]), out=out)
    torch.cuda.synchronize()
    assert out is None or got.data_ptr() == out.data_ptr()
    R.check(f"wgrad {WGRAD_SHAPES[i][:5]} {fmt} groups={groups}", got.cpu(), dw64, bound, "dw")


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["one_block", "interior"])
def test_param_grads_fp64(name, fmt):
    """prepare -> wgrad -> training.conv_param_grads on the GPU's outputs against the same host mapping of the reference's outputs, with the
    kernels' bounds propagated through it: the mapping is linear with coefficients W, gain, bias, so its value at (bounds, |W|, |gain|, |bias|)
    bounds the error of (dW, dgain, dbias).  The tight companion of test_conv_layer_param_grads."""
    c = _case(name, fmt)
    cout, h, w, frames = c["cout"], c["h"], c["w"], c["frames"]
    r = _prepare_reference(name, fmt, True)
    dacc, _, d_sa, d_sg = ops.conv_backward_prepare(c["dyb"], c["yb"][True], c["resb"], c["st_dev"], c["sa"], c["sg"], c["cin"])
    dw_raw = ops.conv3x3_wgrad(dacc, c["xb"])
    torch.cuda.synchronize()
    dw64, dw_abs = R.wgrad_ref(_nchw(dacc, cout, h, w), c["x64"])            # the wgrad reference reads the operand the kernel read
    # ... which differs from the reference's own operand by the dacc bound: |d dw| <= sum bound_dacc |x|
    dacc_slack, _ = R.wgrad_ref(R.bound_dacc(r, fmt), c["x64"].abs())
    b = R.bounds_tables(r, frames, cout * h * w)
    Wd, gd, bd = c["W"].double(), c["gain"].double(), c["bias"].double()
    got = conv_param_grads(dw_raw.cpu().double(), d_sa.cpu().double(), d_sg.cpu().double(), Wd, gd, bd)
    want = conv_param_grads(R.wgrad_ref(r.dacc, c["x64"])[0].contiguous(), r.d_sa, r.d_sg, Wd, gd, bd)
    b_dw = R.bound_dw(frames * h * w, _wgrad_groups(fmt, frames, c["cin"], cout), dw_abs) + dacc_slack
    bounds = conv_param_grads(b_dw.contiguous(), b.d_sa, b.d_sg, Wd.abs(), gd.abs(), bd.abs())
    for g_, w_, b_, what in zip(got, want, bounds, ("dW", "dgain", "dbias")):
        R.check(f"param grads {name} {fmt} {what}", g_, w_, b_)
