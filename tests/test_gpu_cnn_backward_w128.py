"""The stack-0 `firstconv` of the inverse dynamics model is a normed 3x3 conv on 128 x 128 pixels: the pool-fused forward with arg-max masks, the
pooled prepare (with and without the GroupNorm `n` fold), the weight gradient and the dgrad at W = 128, held to the fp64 reference and the bounds of
tests/cnn_backward_ref.py (imported, not copied) in both operand formats.  Needs an MI355X.

W = 128 is the width at which vpt_conv_bwd_prep_pooled_kernel runs ONE pooled row per pass (every "row below" comes from the other LDS buffer) and
vpt_conv_wgrad_kernel<128> runs with one LDS buffer instead of two.  H = 16 keeps the cases small: 8 passes / 16 steps per frame, the first and the
last with a halo row outside the image.

The `nfold` entry forms d(pooled) = r_P (G gain - ab0/n - xhat ab1/n) in fp32 and rounds it to 16 bits before routing it.  Its reference is the same
expression in fp64 on the same stored tensors (and on the kernel's own inputs ab, which come from the GPU's pass 1), rounded to 16 bits; the kernel's
value may differ from it by
    slack(dP) = ulp16(dP) + u r_P (8 |G gain| + 8 |ab0/n| + 14 |xhat ab1/n|)
-- one 16-bit ulp when the fp32 error carries the value across a rounding boundary, and the fp32 error itself: per term the operations it passes
through (x gain, two subtractions, x r_P with r_P's own 4u: 8u; the xhat term additionally (P - mu) r_P ab1: 14u).  The slack is routed like the
gradient (the routing reads P and the masks only, so it is the same on both sides) and added to every bound in the way the quantity depends on dz:
dacc + rstd slack (+ its ulp16: the rounding happens at the kernel's value), d_sa + sum slack, d_sg + |rstd mu| sum slack, T1 + sum slack |v| +
<|SA|, S_slack>, T2 + <|SG|, S_slack>, and (c0, c1) through their definitions."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import _native, ops, packing  # noqa: E402
from tests import cnn_backward_ref as R  # noqa: E402
from tests import test_gpu_cnn_backward_fp64 as T  # noqa: E402  (its operand helpers and checks: _nchw, _blocked, _layer_params, _act, _check_prepare, ...)

DEV = "cuda"
#        name  frames h   w    cin  cout
CASES = {"32_32": (2, 16, 128, 32, 32),
         "128_64": (3, 16, 128, 128, 64),
         "128_32": (2, 16, 128, 128, 32),
         "32_64": (3, 16, 128, 32, 64)}


@functools.lru_cache(maxsize=None)
def _case(name, fmt):
    """Operands on the device, the GPU forward's stored pre-pool output and the fp64 copies (computed once, never modified)."""
    frames, h, w, cin, cout = CASES[name]
    dt = R.DT[fmt]
    g = torch.Generator().manual_seed(128 + sum(map(ord, name)))
    W, gain, bias = T._layer_params(g, cin, cout)
    x = (torch.relu(torch.randn(frames, cin, h, w, generator=g)) + 0.2 * torch.randn(frames, cin, h, w, generator=g)).to(dt)
    gs = 1e-2 if fmt == "fp16" else 1.0
    dp, G, skip = T._act(g, dt, frames, cout, h // 2, w // 2, scale=gs), T._act(g, dt, frames, cout, h // 2, w // 2, scale=gs), T._act(g, dt, frames, cin, h, w, scale=gs)
    ng = 1 + 0.3 * torch.randn(cout, generator=g)
    wpk, sa, sg = ops.pack_conv3x3(W.to(DEV), gain.to(DEV), bias.to(DEV), dtype=dt)
    st = R.stats_of(x)
    c = dict(frames=frames, h=h, w=w, cin=cin, cout=cout, dt=dt, wpk=wpk, sa=sa, sg=sg, sa64=sa.cpu().double(), sg64=sg.cpu().double(),
             wt=packing.pack_conv3x3_dgrad(W.to(DEV), gain.to(DEV), dtype=dt), w16=(W * gain.view(1, -1, 1, 1)).to(dt).double(),
             st=st, st_dev=st.to(DEV), x64=x.double(), dp64=dp.double(), G64=G.double(), skip64=skip.double(), ng=ng,
             xb=T._blocked(x, dt), dpb=T._blocked(dp, dt), Gb=T._blocked(G, dt), skipb=T._blocked(skip, dt))
    c["pre"] = ops.conv3x3(c["xb"], wpk, sa, sg, c["st_dev"], cout)
    c["pooled"], c["mask"] = ops.conv3x3_pool_argmax(c["xb"], wpk, sa, sg, c["st_dev"], cout)
    torch.cuda.synchronize()
    c["pre64"] = T._nchw(c["pre"], cout, h, w)
    return c


@functools.lru_cache(maxsize=None)
def _pooled_reference(name, fmt):
    c = _case(name, fmt)
    return R.prepare_ref(None, c["pre64"], None, c["st"], c["sa64"], c["sg64"], c["cin"], dpooled=c["dp64"], fp32_stats=True)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_pool_argmax_forward_w128(name, fmt):
    """ops.conv3x3_pool_argmax against ops.conv3x3 + ops.maxpool(want_argmax): the pooled tensor bit for bit, and the masks decoded with torch's rule
    (first maximum in scan order = highest zero bit) equal to the arg-max bytes wherever a gradient can flow."""
    c = _case(name, fmt)
    want, am = ops.maxpool(c["pre"], want_argmax=True)
    torch.cuda.synchronize()
    assert torch.equal(c["pooled"].view(torch.int16), want.view(torch.int16))
    m = c["mask"].to(torch.int32) & 0xffff
    assert int(m.max()) <= 0x1ff
    inv = (~m) & 0x1ff
    assert bool((inv != 0).all())
    code = 8 - torch.floor(torch.log2(inv.float())).to(torch.int32)
    live = want.float() > 0
    assert float(live.float().mean()) > 0.2, float(live.float().mean())
    assert torch.equal(code[live], am.to(torch.int32)[live]), f"{int((code[live] != am.to(torch.int32)[live]).sum())} arg-max positions differ"
    assert bool((am[~live] == 15).all())


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_prepare_pooled_w128(name, fmt):
    """vpt_conv_bwd_prep_pooled_kernel<false> at one pooled row per pass + the finish and sum kernels; two calls give the same bits."""
    c = _case(name, fmt)
    r = _pooled_reference(name, fmt)
    outs = ops.conv_backward_prepare_pooled(c["dpb"], c["pooled"], c["mask"], c["st_dev"], c["sa"], c["sg"], c["cin"], want_t12=True)
    again = ops.conv_backward_prepare_pooled(c["dpb"], c["pooled"], c["mask"], c["st_dev"], c["sa"], c["sg"], c["cin"], want_t12=True)
    torch.cuda.synchronize()
    T._check_prepare(f"prepare pooled W=128 {name} {fmt}", c, fmt, r, outs)
    for a, b in zip(outs, again):
        assert torch.equal(a, b)


def _add_slack(c, fmt, r, b_dacc, b, slack_dp):
    """The bounds of a pooled prepare whose d(pooled) may differ from the reference's by slack_dp per element (module docstring)."""
    f, cout, h, w = r.dz.shape
    slack_dz = R.maxpool_backward_ref(slack_dp, c["pre64"]) * (r.v > 0)
    onehot = R.class_onehot(h, w)
    s_slack = torch.einsum("fop,ep->feo", slack_dz.reshape(f, cout, h * w), onehot)
    rs = r.rstd.view(f, 1, 1, 1) * slack_dz
    b_dacc = b_dacc + rs + R.ulp16(rs, fmt) * (rs > 0)
    sa, sg = c["sa64"][:, :cout].abs(), c["sg64"][:, :cout].abs()
    e_t1 = (slack_dz * r.v.abs()).sum((1, 2, 3)) + (sa * s_slack).sum((1, 2))
    e_t2 = (sg * s_slack).sum((1, 2))
    b.d_sa = b.d_sa + s_slack.sum(0)
    b.d_sg = b.d_sg + ((r.rstd * r.mu).abs().view(f, 1, 1) * s_slack).sum(0)
    b.T1, b.T2 = b.T1 + e_t1, b.T2 + e_t2
    e1 = r.rstd ** 2 / r.n_in * e_t1
    b.coef = b.coef + torch.stack([r.rstd / r.n_in * e_t2 + r.mu.abs() * e1, e1], 1)
    return b_dacc, b


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_prepare_pooled_nfold_w128(name, fmt):
    """vpt_conv_bwd_prep_pooled_kernel<true>: the GroupNorm `n` backward applied on the fly to G = d loss / d n(pooled)."""
    c = _case(name, fmt)
    frames, cout, h, w = c["frames"], c["cout"], c["h"], c["w"]
    ph, pw = h // 2, w // 2
    p64 = T._nchw(c["pooled"], cout, ph, pw)
    s_pool = R.stats_of(p64)
    ng_dev, s_pool_dev = c["ng"].to(DEV), s_pool.to(DEV)
    dg, db = torch.zeros(cout, device=DEV), torch.zeros(cout, device=DEV)
    ab = ops.frame_affine_backward_reduce(c["pooled"], c["Gb"], ng_dev, s_pool_dev, dg, db)
    outs = ops.conv_backward_prepare_pooled(c["Gb"], c["pooled"], c["mask"], c["st_dev"], c["sa"], c["sg"], c["cin"], want_t12=True, nfold=(ng_dev, s_pool_dev, ab))
    again = ops.conv_backward_prepare_pooled(c["Gb"], c["pooled"], c["mask"], c["st_dev"], c["sa"], c["sg"], c["cin"], want_t12=True, nfold=(ng_dev, s_pool_dev, ab))
    torch.cuda.synchronize()
    for a, b_ in zip(outs, again):
        assert torch.equal(a, b_)
    # d(pooled) in fp64 from the stored tensors and the kernel's own (ab0, ab1) / n as fp32 values (`nA`, `nB` in the kernel)
    n_pool = cout * ph * pw
    mp, rp = R.frame_mean_rstd(s_pool, n_pool, fp32_stats=True)
    nab = (ab.cpu().double() / n_pool).float().double()
    mp, rp, nA, nB = (t.view(frames, 1, 1, 1) for t in (mp, rp, nab[:, 0], nab[:, 1]))
    gg = c["G64"] * c["ng"].double().view(1, cout, 1, 1)
    xh = (p64 - mp) * rp
    dp64 = rp * (gg - nA - xh * nB)
    slack_dp = R.ulp16(dp64, fmt) + R.U * rp * (8 * gg.abs() + 8 * nA.abs() + 14 * (xh * nB).abs())
    r = R.prepare_ref(None, c["pre64"], None, c["st"], c["sa64"], c["sg64"], c["cin"], dpooled=R.op16(dp64, fmt), fp32_stats=True)
    b_dacc, b = _add_slack(c, fmt, r, R.bound_dacc(r, fmt), R.bounds_tables(r, frames, cout * h * w), slack_dp)
    what = f"prepare pooled nfold W=128 {name} {fmt}"
    got = T._nchw(outs[0], cout, h, w)
    closed = ~(R.maxpool_backward_ref(torch.ones_like(dp64), c["pre64"]) * (r.v > 0)).bool()
    assert not bool(got[closed].any()), f"{what}: dacc must be exactly zero where no window routes to an open gate"
    R.check(f"{what} dacc", got, r.dacc, b_dacc, "nchw")
    coef, d_sa, d_sg, t12 = (t.cpu().double() for t in outs[1:])
    R.check(f"{what} d_sa", d_sa[:, :cout], r.d_sa, b.d_sa, "table")
    R.check(f"{what} d_sg", d_sg[:, :cout], r.d_sg, b.d_sg, "table")
    assert not bool(d_sa[:, cout:].any()) and not bool(d_sg[:, cout:].any())
    R.check(f"{what} T1", t12[:, 0], r.T1, b.T1)
    R.check(f"{what} T2", t12[:, 1], r.T2, b.T2)
    R.check(f"{what} coef", coef, r.coef, b.coef)


@pytest.mark.parametrize("prefill", [False, True])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_wgrad_w128(name, fmt, prefill):
    """vpt_conv_wgrad_kernel<128> + the reduce kernel on the reference's operand rounded to 16 bits; with out= given and pre-filled the kernel adds."""
    c = _case(name, fmt)
    frames, h, w, cin, cout = CASES[name]
    dacc16 = _pooled_reference(name, fmt).dacc.to(c["dt"])
    dw64, dw_abs = R.wgrad_ref(dacc16.double(), c["x64"])
    groups = _native.load(fmt).vpt_conv3x3_wgrad_scratch_floats(frames, cin, cout) // (cout * 9 * cin)
    bound = R.bound_dw(frames * h * w, groups, dw_abs)
    out = None
    if prefill:
        out0 = torch.randn(cout, 9, cin, generator=torch.Generator().manual_seed(5))
        dw64 = dw64 + out0.double()
        bound = bound + R.U * dw64.abs()       # vpt_conv_wgrad_reduce_kernel: `*d = *d + s`, one more fp32 addition
    dacc_b = T._blocked(dacc16, c["dt"])
    outs = []
    for _ in range(2):
        out = out0.to(DEV) if prefill else None
        outs.append(ops.conv3x3_wgrad(dacc_b, c["xb"], out=out))
        assert out is None or outs[-1].data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    R.check(f"wgrad W=128 {name} {fmt} groups={groups} out={prefill}", outs[0].cpu(), dw64, bound, "dw")


@pytest.mark.parametrize("use_skip", [False, True])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_dgrad_w128(name, fmt, use_skip):
    """vpt_conv3x3_dgrad_kernel modes 2 / 3 at W = 128 (the IDM's dx0, the gradient the temporal conv's backward reads)."""
    c = _case(name, fmt)
    r = _pooled_reference(name, fmt)
    dacc16, coef = r.dacc.to(c["dt"]), r.coef.float()
    dx0, conv_abs = R.dgrad_ref(dacc16.double(), c["w16"], None, c["x64"], coef)
    dacc_b = T._blocked(dacc16, c["dt"])
    dx = ops.conv3x3_dgrad(dacc_b, c["wt"], c["cin"], skip=c["skipb"] if use_skip else None, xin=c["xb"], coef=coef.to(DEV))
    dx2 = ops.conv3x3_dgrad(dacc_b, c["wt"], c["cin"], skip=c["skipb"] if use_skip else None, xin=c["xb"], coef=coef.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(dx, dx2)
    skip = c["skip64"] if use_skip else None
    dx64 = dx0 if skip is None else dx0 + skip
    R.check(f"dgrad W=128 {name} {fmt} skip={use_skip}", T._nchw(dx, c["cin"], c["h"], c["w"]), dx64, R.bound_dx(dx64, fmt, c["cout"], conv_abs, skip, coef, c["x64"]), "nchw")
