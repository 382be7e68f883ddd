"""fp64 reference of the temporal conv's weight / bias gradient (ops.conv3d_t5_backward, vpt_conv3d_t5_bwd_kernel) with the ReLU gate PINNED to
the stored forward output, and the per-element bound the kernel is held to.  A plain helper (no test, no fixture): torch on the CPU only, nothing
of vpt_amd.

Layer (vpt_conv3d.hip, lib/policy.py:394-403):  y[f,p,o] = relu(sum_{dt,c} W[o,c,dt] img[f + dt - 2, p, c] / 255 + b[o]), a tap outside frame f's own
window [f - f % t, f - f % t + t) reads zero.  With g = dy [y > 0], y the STORED 16-bit tensor:
    dW[o,c,dt] = (1/255) sum_{f,p} g[f,p,o] img[f + dt - 2, p, c],      db[o] = sum_{f,p} g[f,p,o].

Bound, u = 2^-24, n = M H W terms per element:
    dW   (n + 2) u sum|g| byte / 255 + u |dW|          db   (n + 2) u sum|g| + u |db|
Every product g * byte is exact in fp32 (an 8-bit by an at most 11-bit significand), so what rounds is the fp32 summation of n terms in whatever
order -- (n - 1) u sum|terms| to first order -- one scaling by the fp32 constant 1/255 (2u: the constant and the multiply) and the value stored as
one fp32 number.  Nothing is fitted.  tests/test_conv3d_backward_ref_cpu.py shows that these functions are the true gradient (fp64 autograd of
oracle.vpt_oracle.conv3d_temporal, 1e-9) and that plain fp32 arithmetic stays inside the bound."""
import torch

U = 2.0 ** -24
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def blocked_to_nchw(x_blocked, c, h, w):
    """16-bit [F][c/32][h][w][32] -> fp64 [F][c][h][w] holding exactly the stored numbers."""
    f = x_blocked.shape[0]
    return x_blocked.cpu().view(f, c // 32, h, w, 32).permute(0, 1, 4, 2, 3).reshape(f, c, h, w).double()


def nchw_to_blocked(x, dtype):
    f, c, h, w = x.shape
    return x.view(f, c // 32, 32, h, w).permute(0, 1, 3, 4, 2).contiguous().to(dtype)


def tap_frames(m, t, dt, cross_window=False, shift=0):
    """(source frame of tap dt for every frame [m], whether the tap reads it [m]).  cross_window / shift are the two MUTATIONS the tests use to show
    that the bound separates a wrong kernel from a right one: taps allowed across the window edge (only the ends of the whole clip are padding), and
    every tap reading one frame later."""
    f = torch.arange(m)
    src = f + dt - 2 + shift
    lo = f - f % t
    valid = ((src >= 0) & (src < m)) if cross_window else ((src >= lo) & (src < lo + t))
    return src.clamp(0, m - 1), valid


def backward_ref(img_u8, y, dy, t, cross_window=False, shift=0):
    """img_u8 uint8 [M,H,W,3]; y, dy fp64 [M,O,H,W] holding the stored 16-bit values -> (dW [O,3,5], db [O], sum|g| byte/255 [O,3,5], sum|g| [O])."""
    m = img_u8.shape[0]
    x = img_u8.double()
    g = dy * (y > 0)
    ga = g.abs()
    dw = torch.zeros(y.shape[1], 3, 5, dtype=torch.float64)
    dw_abs = torch.zeros_like(dw)
    for dt in range(5):
        src, valid = tap_frames(m, t, dt, cross_window, shift)
        xs = x[src] * valid.view(m, 1, 1, 1)
        dw[:, :, dt] = torch.einsum("fohw,fhwc->oc", g, xs) / 255.0
        dw_abs[:, :, dt] = torch.einsum("fohw,fhwc->oc", ga, xs) / 255.0
    return dw, g.sum((0, 2, 3)), dw_abs, ga.sum((0, 2, 3))


def bounds(n, dw, db, dw_abs, db_abs):
    return (n + 2) * U * dw_abs + U * dw.abs(), (n + 2) * U * db_abs + U * db.abs()


def worst_ratio(got, ref, bound):
    """max err / bound (0 where both are exactly equal; inf where the bound is 0 and the error is not)."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.full_like(err, float("inf"))))
    return ratio


def check(what, got, ref, bound):
    """Print `max err / bound` (the measurement) and assert it is <= 1, naming the worst element."""
    ratio = worst_ratio(got, ref, bound)
    flat = int(ratio.reshape(-1).argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
    r = float(ratio.reshape(-1)[flat])
    print(f"{what}: max err / bound = {r:.3f}")
    assert r <= 1.0, (f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements beyond the bound, worst ratio {r:.3f} at (channel, image channel, tap) "
                      f"{idx}: got {float(got.double().reshape(-1)[flat]):.9g} want {float(ref.reshape(-1)[flat]):.9g} bound {float(bound.reshape(-1)[flat]):.3g}")
    return r
