"""ops.conv3d_t5_backward (vpt_conv3d_t5_bwd_kernel + vpt_slab_sum) held per element to the fp64 reference of tests/conv3d_backward_ref.py on
the SAME stored 16-bit tensors and bytes, in both operand formats.  Needs an MI355X.

The forward runs once per case on the GPU (ops.conv3d_t5) so that the stored output has realistic gates; kernel and reference then read the same
y0, dy0 and image, so both open exactly the same ReLU gates and only the kernel's arithmetic is judged.  Bound (derived in the helper's docstring,
u = 2^-24, n = M H W; tests/test_conv3d_backward_ref_cpu.py shows plain fp32 arithmetic meets it):
    dW   (n + 2) u sum|g| byte / 255 + u |dW|          db   (n + 2) u sum|g| + u |db|
Each check prints `max err / bound` and asserts <= 1.  In fp16 dy0 is scaled by 1e-2 (the loss scale's job in training).

Shapes (B, t, H, W): the first two make the taps clip at both edges of a window with a second window next to it (nothing may leak across); t = 1
leaves only the centre tap; (3, 5) has a window exactly as long as the kernel; (3, 3, 128, 128) is the model's own frame size and the smallest
batch at which a workgroup sweeps more than one (frame, chunk) item and the slab has more rows than one slice of the fixed-order sum.  Two mutations of the REFERENCE (taps allowed across the window
edge; every tap one frame late) must leave the bound at the taps concerned: the bound separates a wrong kernel from a right one."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from tests import conv3d_backward_ref as R  # noqa: E402

DEV = "cuda"
COUT = 128
#          B  t  H   W
SHAPES = [(2, 3, 16, 16), (2, 7, 16, 32), (1, 1, 16, 16), (3, 5, 16, 16),
          (3, 3, 128, 128)]     # 576 (frame, chunk) items: two per workgroup (the double-buffered byte slabs), 288 slab rows (the two-level sum)


@functools.lru_cache(maxsize=None)
def _case(i, fmt):
    """Operands on the device, the GPU forward's stored output, the fp64 reference and its bounds (computed once, never modified)."""
    b, t, h, w = SHAPES[i]
    dt = R.DT[fmt]
    g = torch.Generator().manual_seed(700 + i)
    img = torch.randint(0, 256, (b * t, h, w, 3), generator=g, dtype=torch.uint8)
    weight = torch.randn(COUT, 3, 5, 1, 1, generator=g) * 0.4
    bias = torch.randn(COUT, generator=g) * 0.2
    dy = (torch.randn(b * t, COUT, h, w, generator=g) * (1e-2 if fmt == "fp16" else 1.0)).to(dt)
    wfrag, bias_pad = ops.pack_conv3d_t5(weight.to(DEV), bias.to(DEV), dtype=dt)
    img_d = img.to(DEV)
    y0 = ops.conv3d_t5(img_d, wfrag, bias_pad, COUT, t)
    torch.cuda.synchronize()
    y64, dy64 = R.blocked_to_nchw(y0, COUT, h, w), dy.double()
    gate = float((y64 > 0).double().mean())
    assert 0.2 < gate < 0.8, gate                       # both gate states are well represented
    dw, db, dw_abs, db_abs = R.backward_ref(img, y64, dy64, t)
    b_dw, b_db = R.bounds(b * t * h * w, dw, db, dw_abs, db_abs)
    return dict(t=t, img=img, img_d=img_d, y0=y0, dy0=R.nchw_to_blocked(dy, dt).to(DEV), y64=y64, dy64=dy64, dw=dw, db=db, b_dw=b_dw, b_db=b_db)


def _run(c):
    dw, db = ops.conv3d_t5_backward(c["img_d"], c["y0"], c["dy0"], c["t"])
    torch.cuda.synchronize()
    assert dw.shape == (COUT, 3, 5, 1, 1) and db.shape == (COUT,)
    return dw.cpu().view(COUT, 3, 5), db.cpu()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_conv3d_backward_fp64(i, fmt):
    c = _case(i, fmt)
    dw, db = _run(c)
    R.check(f"conv3d backward {SHAPES[i]} {fmt} dW", dw, c["dw"], c["b_dw"])
    R.check(f"conv3d backward {SHAPES[i]} {fmt} db", db, c["db"], c["b_db"])
    if c["t"] == 1:
        assert not bool(dw[:, :, [0, 1, 3, 4]].any()), "t = 1: every tap but the centre reads padding only and must be exactly zero"
    dw2, db2 = _run(c)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "the same inputs must give the same bits"


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_conv3d_backward_accumulates_into_out(fmt):
    c = _case(0, fmt)
    g = torch.Generator().manual_seed(3)
    dw0, db0 = torch.randn(COUT, 3, 5, 1, 1, generator=g), torch.randn(COUT, generator=g)
    out = (dw0.to(DEV), db0.to(DEV))
    got = ops.conv3d_t5_backward(c["img_d"], c["y0"], c["dy0"], c["t"], out=out)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
    want_dw, want_db = c["dw"] + dw0.double().view(COUT, 3, 5), c["db"] + db0.double()
    # vpt_slab_sum_kernel: `*dst + tot`, one more fp32 addition
    R.check(f"conv3d backward out= {fmt} dW", got[0].cpu().view(COUT, 3, 5), want_dw, c["b_dw"] + R.U * want_dw.abs())
    R.check(f"conv3d backward out= {fmt} db", got[1].cpu(), want_db, c["b_db"] + R.U * want_db.abs())


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("i", [0, 1])
def test_mutated_reference_leaves_the_bound(i, fmt):
    c = _case(i, fmt)
    dw, _ = _run(c)
    cross = R.backward_ref(c["img"], c["y64"], c["dy64"], c["t"], cross_window=True)[0]
    shifted = R.backward_ref(c["img"], c["y64"], c["dy64"], c["t"], shift=1)[0]
    for dt in range(5):
        r_cross = float(R.worst_ratio(dw[:, :, dt], cross[:, :, dt], c["b_dw"][:, :, dt]).max())
        r_shift = float(R.worst_ratio(dw[:, :, dt], shifted[:, :, dt], c["b_dw"][:, :, dt]).max())
        print(f"{SHAPES[i]} {fmt} tap {dt}: err / bound against the cross-window reference {r_cross:.3g}, against the shifted one {r_shift:.3g}")
        if dt != 2:
            assert r_cross > 1, f"tap {dt}: the kernel agrees with a reference whose taps cross the window edge"
        assert r_shift > 1, f"tap {dt}: the kernel agrees with a reference whose taps are one frame late"
