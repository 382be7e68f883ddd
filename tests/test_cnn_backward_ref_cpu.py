"""tests/cnn_backward_ref.py is the true gradient, and its bounds admit plain fp32 arithmetic -- proved on the CPU, before a GPU sees either.

One GN -> conv3x3 -> ReLU (+ res) layer in fp64 torch, with the weights W' = op16(W * gain) where the kernels use them rounded (straight-through:
the gradient flows to W and gain as if unrounded, which is what training.conv_param_grads maps).  Three things are shown per case:

1. The reference chain (prepare_ref -> dgrad_ref, wgrad_ref -> conv_param_grads) fed the layer's output equals torch.autograd.grad w.r.t.
   x, W, gain and bias to 1e-9 of the gradient's largest magnitude.
2. Fed the STORED output y16 = op16(forward) it opens exactly the same gates -- inputs are picked so that no pre-activation lies within one
   16-bit ulp (at the stored value) of zero: `res` is zero where it would; checked, next seed otherwise, at most MAX_SEEDS, count printed --
   so dz, dacc and the edge-table sums are the same numbers.  T1 = sum dz (v - SA) is the one quantity that reads the VALUE v = y16 - res and
   not only its sign (as vpt_conv_bwd_prep_kernel does): it moves by at most sum |dz| ulp16(y16) / 2, asserted.  The layer's output itself is
   never 16-bit representable, so item 1 cannot be stated on y16 for T1 and what hangs on it (c1, c0).
3. The same quantities evaluated in fp32 (torch.float32 convolutions and sums on the same 16-bit operands, results rounded to 16 bits where the
   kernels store 16 bits) lie inside the bounds the GPU test uses.  A bound that plain fp32 arithmetic cannot meet would be wrong.

A two-layer block goes through dgrad_gated_ref and reduce_ref (conv1 -> conv0 as training.py chains them), the pooled entry against
max_pool2d autograd with a plateau for the first-maximum rule, and one 16 x 48 image has H != W."""
import functools

import pytest
import torch
import torch.nn.functional as F

import vpt_amd  # noqa: F401
from vpt_amd import packing
from vpt_amd.training import conv_param_grads
from tests import cnn_backward_ref as R

MAX_SEEDS = 8
#         name     frames h   w   cin cout res
CASES = {"plain": (2, 16, 16, 64, 96, False),
         "res": (2, 16, 16, 96, 32, True),
         "wide": (1, 16, 48, 32, 64, True)}


def _tables(W, gain, bias, fmt):
    """SA, SG [9, Cout] in fp64 from the master weights (packing.pack_conv3x3 stores their fp32 roundings)."""
    cout = W.shape[0]
    m = packing.edge_tap_matrix(W.device)
    sg_tap = R.op16(W * gain.view(1, -1, 1, 1), fmt).sum(1).view(cout, 9)
    sa_tap = (W * bias.view(1, -1, 1, 1)).sum(1).view(cout, 9)
    return m @ sa_tap.t(), m @ sg_tap.t()


def _pre_activation(x, W, gain, bias, fmt):
    """GroupNorm(1, Cin) -> conv3x3 (zero padding AFTER the norm) with W' = op16(W gain) straight-through, before the ReLU."""
    f, cin, h, w = x.shape
    flat = x.reshape(f, -1)
    mu = flat.mean(1).view(f, 1, 1, 1)
    rstd = 1.0 / torch.sqrt(flat.var(1, unbiased=False).view(f, 1, 1, 1) + R.EPS)
    wg = W * gain.view(1, -1, 1, 1)
    w_st = wg + (R.op16(wg.detach(), fmt) - wg.detach())
    return F.conv2d((x - mu) * rstd, w_st, padding=1) + F.conv2d(bias.view(1, cin, 1, 1).expand(1, cin, h, w), W, padding=1)


def _params(g, cin, cout):
    W = (torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * (1.6 / (cin * 9) ** 0.5)).requires_grad_(True)
    gain = (1 + 0.2 * torch.randn(cin, generator=g, dtype=torch.float64)).requires_grad_(True)
    bias = (0.1 * torch.randn(cin, generator=g, dtype=torch.float64)).requires_grad_(True)
    return W, gain, bias


def _acts(g, fmt, *shape, scale=1.0):
    return R.op16(scale * torch.randn(*shape, generator=g, dtype=torch.float64), fmt)


@functools.lru_cache(maxsize=None)
def _layer(name, fmt):
    frames, h, w, cin, cout, use_res = CASES[name]
    for tried in range(1, MAX_SEEDS + 1):
        g = torch.Generator().manual_seed(1000 * tried + sum(map(ord, name)))
        W, gain, bias = _params(g, cin, cout)
        x = R.op16(torch.relu(torch.randn(frames, cin, h, w, generator=g, dtype=torch.float64)) + 0.2 * torch.randn(frames, cin, h, w, generator=g, dtype=torch.float64), fmt)
        x.requires_grad_(True)
        dY = _acts(g, fmt, frames, cout, h, w, scale=1e-2 if fmt == "fp16" else 1.0)
        pre = _pre_activation(x, W, gain, bias, fmt)
        res = None
        if use_res:
            res = _acts(g, fmt, frames, cout, h, w)
            near = pre.detach().abs() <= R.ulp16(R.op16(torch.relu(pre.detach()) + res, fmt), fmt)
            res = torch.where(near, torch.zeros_like(res), res)       # picked inputs: no residual where the stored sum would swallow the pre-activation
        y = torch.relu(pre) + (res if use_res else 0)
        y16 = R.op16(y.detach(), fmt)
        margin = pre.detach().abs() > R.ulp16(y16, fmt)
        v16 = y16 - res if use_res else y16
        if bool(margin.all()) and torch.equal(v16 > 0, pre.detach() > 0):
            break
    else:
        raise AssertionError(f"{name} {fmt}: no seed of {MAX_SEEDS} keeps every pre-activation one 16-bit ulp from zero")
    print(f"{name} {fmt}: {tried} seed(s) tried (cap {MAX_SEEDS})")
    gx, gW, gg, gb = torch.autograd.grad((y * dY).sum(), [x, W, gain, bias])
    sa, sg = _tables(W.detach(), gain.detach(), bias.detach(), fmt)
    return dict(frames=frames, h=h, w=w, cin=cin, cout=cout, tried=tried, x=x.detach(), W=W.detach(), gain=gain.detach(), bias=bias.detach(), res=res, dY=dY,
                y=y.detach(), y16=y16, sa=sa, sg=sg, w16=R.op16(W.detach() * gain.detach().view(1, -1, 1, 1), fmt), st=R.stats_of(x.detach()), grads=(gx, gW, gg, gb))


def _close(a, b, what):
    scale = float(b.abs().max())
    diff = (a - b).abs()
    err = float(diff.max())
    at = [int(i) for i in torch.unravel_index(diff.reshape(-1).argmax(), diff.shape)]
    print(f"{what}: max |difference| / max |gradient| = {err / scale:.2e}")
    assert err <= 1e-9 * scale, f"{what}: {err:.3e} at index {at} against a largest magnitude of {scale:.3e}"


def _class_sums(t):
    """[F, C, H, W] -> [F, 9, C] sums over the pixels of each edge class, by slicing (independent of cnn_backward_ref.edge_class)."""
    rows = (t[:, :, :1], t[:, :, 1:-1], t[:, :, -1:])
    return torch.stack([r[..., sl].sum((2, 3)) for r in rows for sl in (slice(0, 1), slice(1, -1), slice(-1, None))], 1)


def _chain(c, r):
    dx, _ = R.dgrad_ref(r.dacc, c["w16"], None, c["x"], r.coef)
    dw_raw, _ = R.wgrad_ref(r.dacc, c["x"])
    return (dx,) + conv_param_grads(dw_raw.contiguous(), r.d_sa, r.d_sg, c["W"], c["gain"], c["bias"])


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_reference_is_the_fp64_gradient(name, fmt):
    c = _layer(name, fmt)
    assert c["tried"] <= MAX_SEEDS
    r = R.prepare_ref(c["dY"], c["y"], c["res"], c["st"], c["sa"], c["sg"], c["cin"])
    for got, want, what in zip(_chain(c, r), c["grads"], ("dx", "dW", "dgain", "dbias")):
        _close(got, want, f"{name} {fmt} {what}")
    # the stored output: the same gates, hence the same dz, operand and table sums; T1 within the rounding of the values it reads
    r16 = R.prepare_ref(c["dY"], c["y16"], c["res"], c["st"], c["sa"], c["sg"], c["cin"])
    assert torch.equal(r16.dz, r.dz) and torch.equal(r16.dacc, r.dacc)
    assert torch.equal(r16.d_sa, r.d_sa) and torch.equal(r16.d_sg, r.d_sg) and torch.equal(r16.T2, r.T2)
    moved = (r16.T1 - r.T1).abs()
    allowed = (r.dz.abs() * R.ulp16(c["y16"], fmt) / 2).sum((1, 2, 3))
    print(f"{name} {fmt}: T1 moved by {float((moved / allowed).max()):.3f} of the stored values' rounding")
    assert bool((moved <= allowed).all())
    for got, want, what in zip(_chain(c, r16)[1:], c["grads"][1:], ("dW", "dgain", "dbias")):
        _close(got, want, f"{name} {fmt} {what} from the stored output")


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_fp32_arithmetic_stays_inside_the_bounds(name, fmt):
    """fp32 convolutions and sums on the 16-bit operands against the fp64 reference of the same operands, with the GPU test's bounds."""
    c = _layer(name, fmt)
    frames, h, w, cin, cout = c["frames"], c["h"], c["w"], c["cin"], c["cout"]
    _, sa32, sg32 = packing.pack_conv3x3(c["W"].float(), c["gain"].float(), c["bias"].float(), dtype=R.DT[fmt])
    sa, sg = sa32.double(), sg32.double()
    r = R.prepare_ref(c["dY"], c["y16"], c["res"], c["st"], sa, sg, cin, fp32_stats=True)
    b = R.bounds_tables(r, frames, cout * h * w)
    # prepare in fp32
    mu32, rstd32 = r.mu.float(), torch.rsqrt((r.rstd ** -2).float())                 # (var + eps) rounded to fp32, then the reciprocal square root
    dz32 = r.dz.float()
    dacc16 = (rstd32.view(-1, 1, 1, 1) * dz32).to(R.DT[fmt])
    assert torch.equal(dacc16 == 0, r.dacc == 0)
    R.check(f"fp32 dacc {name} {fmt}", dacc16, r.dacc, R.bound_dacc(r, fmt), "nchw")
    s32 = _class_sums(dz32)
    R.check(f"fp32 d_sa {name} {fmt}", s32.sum(0), r.d_sa, b.d_sa, "table")
    R.check(f"fp32 d_sg {name} {fmt}", ((-rstd32 * mu32).view(-1, 1, 1) * s32).sum(0), r.d_sg, b.d_sg, "table")
    t1 = (dz32 * r.v.float()).sum((1, 2, 3)) - (sa32[:, :cout] * s32).sum((1, 2))
    t2 = (sg32[:, :cout] * s32).sum((1, 2))
    R.check(f"fp32 T1 {name} {fmt}", t1, r.T1, b.T1)
    R.check(f"fp32 T2 {name} {fmt}", t2, r.T2, b.T2)
    coef32 = R.dgrad_coef(r.mu, rstd32.double(), t1.double(), t2.double(), r.n_in).float()
    R.check(f"fp32 coef {name} {fmt}", coef32, r.coef, b.coef)
    # dgrad and wgrad in fp32 on the stored operand
    d64 = dacc16.double()
    skip =R.op16(torch.randn(frames, cin, h, w, generator=torch.Generator().manual_seed(3), dtype=torch.float64), fmt)
    for sk in (None, skip):
        dx64, conv_abs = R.dgrad_ref(d64, c["w16"], sk, c["x"], coef32)
        dx32 = F.conv_transpose2d(dacc16.float(), c["w16"].float(), padding=1) + (coef32[:, 1].view(-1, 1, 1, 1) * c["x"].float() + coef32[:, 0].view(-1, 1, 1, 1))
        if sk is not None:
            dx32 = dx32 + sk.float()
        R.check(f"fp32 dx {name} {fmt} skip={sk is not None}", dx32.to(R.DT[fmt]), dx64, R.bound_dx(dx64, fmt, cout, conv_abs, sk, coef32, c["x"]), "nchw")
    dw64, dw_abs = R.wgrad_ref(d64, c["x"])
    xp = F.pad(c["x"].float(), (1, 1, 1, 1))
    dw32 = torch.stack([torch.einsum("foyx,fcyx->oc", dacc16.float(), xp[:, :, t // 3:t // 3 + h, t % 3:t % 3 + w]) for t in range(9)], 1)
    R.check(f"fp32 dw_raw {name} {fmt}", dw32, dw64, R.bound_dw(frames * h * w, 1, dw_abs), "dw")


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_block_through_the_gated_dgrad(fmt):
    """x + conv1(conv0(x)) (lib/impala_cnn.py:50-52) backward as training.py chains it: prepare(conv1) -> gated dgrad (conv0's operand and
    gate_u) -> reduce(conv0) -> dgrad with the skip connection, against fp64 autograd; then the gated output and gate_u in fp32 inside the bounds."""
    frames, h, w, ch = 2, 16, 16, 64
    g = torch.Generator().manual_seed(77)
    W0, g0, b0 = _params(g, ch, ch)
    W1, g1, b1 = _params(g, ch, ch)
    x = R.op16(torch.relu(torch.randn(frames, ch, h, w, generator=g, dtype=torch.float64)) + 0.2 * torch.randn(frames, ch, h, w, generator=g, dtype=torch.float64), fmt)
    x.requires_grad_(True)
    dout = _acts(g, fmt, frames, ch, h, w, scale=1e-2 if fmt == "fp16" else 1.0)
    y0 = torch.relu(_pre_activation(x, W0, g0, b0, fmt))
    out = torch.relu(_pre_activation(y0, W1, g1, b1, fmt)) + x
    grads = torch.autograd.grad((out * dout).sum(), [x, W0, g0, b0, W1, g1, b1])
    x, y0, out = x.detach(), y0.detach(), out.detach()
    W0, g0, b0, W1, g1, b1 = (t.detach() for t in (W0, g0, b0, W1, g1, b1))
    (sa0, sg0), (sa1, sg1) = _tables(W0, g0, b0, fmt), _tables(W1, g1, b1, fmt)
    w0, w1 = R.op16(W0 * g0.view(1, -1, 1, 1), fmt), R.op16(W1 * g1.view(1, -1, 1, 1), fmt)
    st_x, st_y = R.stats_of(x), R.stats_of(y0)
    r1 = R.prepare_ref(dout, out, x, st_y, sa1, sg1, ch)
    dacc0, gate_u, conv_abs, rstd0, _ = R.dgrad_gated_ref(r1.dacc, w1, y0, r1.coef, st_x, ch)
    r0 = R.reduce_ref(dacc0, gate_u, st_x, sa0, sg0, ch)
    dx, _ = R.dgrad_ref(dacc0, w0, dout, x, r0.coef)
    got = (dx,) + conv_param_grads(R.wgrad_ref(dacc0, x)[0].contiguous(), r0.d_sa, r0.d_sg, W0, g0, b0) \
        + conv_param_grads(R.wgrad_ref(r1.dacc, y0)[0].contiguous(), r1.d_sa, r1.d_sg, W1, g1, b1)
    for a, b_, what in zip(got, grads, ("dx", "dW0", "dgain0", "dbias0", "dW1", "dgain1", "dbias1")):
        _close(a, b_, f"block {fmt} {what}")
    # fp32 evaluation of the gated epilogue on 16-bit operands
    y16, d1 = R.op16(y0, fmt), R.op16(r1.dacc, fmt)
    coef32 = r1.coef.float()
    want, want_u, conv_abs, rstd0, abs_u = R.dgrad_gated_ref(d1, w1, y16, coef32, st_x, ch, fp32_stats=True)
    r32 = rstd0.float().view(-1, 1, 1, 1)
    u32 = r32 * F.conv_transpose2d(d1.float(), w1.float(), padding=1) + ((r32 * coef32[:, 1].view(-1, 1, 1, 1)) * y16.float() + r32 * coef32[:, 0].view(-1, 1, 1, 1))
    got16 = torch.where(y16 > 0, u32, torch.zeros_like(u32)).to(R.DT[fmt])
    assert torch.equal((got16 == 0) | (want.abs() < R.tiny16(fmt)), (want == 0) | (want.abs() < R.tiny16(fmt)))
    R.check(f"fp32 gated dgrad {fmt}", got16, want, R.bound_dx(want, fmt, ch, conv_abs, None, coef32, y16, scale=rstd0), "nchw")
    R.check(f"fp32 gate_u {fmt}", (u32 * y16.float()).sum((1, 2, 3)), want_u, R.bound_sum(ch * h * w, abs_u, want_u))


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_pooled_entry_routes_like_max_pool2d(fmt):
    """conv -> ReLU -> stored 16-bit tensor -> max_pool2d(3, 2, 1): prepare_ref(dy=None, dpooled=) must gate and route exactly as autograd of
    the pool on the stored values does, with a plateau of equal positive values for the first-maximum rule, and give the layer's parameter gradients."""
    frames, h, w, cin, cout = 2, 16, 16, 32, 64
    g = torch.Generator().manual_seed(99)
    W, gain, bias = _params(g, cin, cout)
    x = R.op16(torch.relu(torch.randn(frames, cin, h, w, generator=g, dtype=torch.float64)), fmt)
    x[0, :, 3:12, 3:12] = 0.75                      # a constant patch: the convolution is constant on its interior, the stored values tie there
    pre = _pre_activation(x, W, gain, bias, fmt)
    y = torch.relu(pre)
    y16 = R.op16(y.detach(), fmt)
    y_st = y + (y16 - y.detach())                   # straight-through: the pool sees the stored values
    dp = _acts(g, fmt, frames, cout, h // 2, w // 2, scale=1e-2 if fmt == "fp16" else 1.0)
    g_pre, gW, gg, gb = torch.autograd.grad((F.max_pool2d(y_st, 3, 2, 1) * dp).sum(), [pre, W, gain, bias])
    win = F.unfold(F.pad(y16, (1, 1, 1, 1), value=-1.0), 3, stride=2).view(frames, cout, 9, -1)
    ties = ((win == win.max(2, keepdim=True).values).sum(2) > 1) & (win.max(2).values > 0)
    assert int(ties.sum()) > 100, "the plateau must produce windows whose positive maximum occurs more than once"
    W, gain, bias = W.detach(), gain.detach(), bias.detach()
    sa, sg = _tables(W, gain, bias, fmt)
    r = R.prepare_ref(None, y16, None, R.stats_of(x), sa, sg, cin, dpooled=dp)
    _close(r.dz, g_pre, f"pooled {fmt} dz")
    assert torch.equal(r.dz != 0, g_pre != 0)
    dW, dgain, dbias = conv_param_grads(R.wgrad_ref(r.dacc, x)[0].contiguous(), r.d_sa, r.d_sg, W, gain, bias)
    for a, b_, what in ((dW, gW, "dW"), (dgain, gg, "dgain"), (dbias, gb, "dbias")):
        _close(a, b_, f"pooled {fmt} {what}")
    # fp32: the routed sum of up to four window gradients, then rstd, one 16-bit rounding
    r = R.prepare_ref(None, y16, None, R.stats_of(x), sa, sg, cin, dpooled=dp, fp32_stats=True)
    routed32 = R.maxpool_backward_ref(dp.float(), y16.float())
    dacc16 = (torch.rsqrt((r.rstd ** -2).float()).view(-1, 1, 1, 1) * torch.where(y16 > 0, routed32, torch.zeros_like(routed32))).to(R.DT[fmt])
    R.check(f"fp32 pooled dacc {fmt}", dacc16, r.dacc, R.bound_dacc(r, fmt), "nchw")
