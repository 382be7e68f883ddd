"""tests/conv3d_backward_ref.py is the true gradient of the temporal conv, and its bound admits plain fp32 arithmetic -- shown on the CPU, before
a GPU sees either.

1. backward_ref fed the layer's output rounded to 16 bits (the tensor the kernel reads its gate from) equals fp64 autograd of
   oracle.vpt_oracle.conv3d_temporal w.r.t. weight and bias to 1e-9 of the gradient's largest magnitude.  Rounding a positive number to 16 bits
   never reaches zero above the format's underflow, so the pinned gates are autograd's; asserted.
2. The same sums in fp32 -- exact products, torch's fp32 sum, and a strictly sequential fp32 sum as a second order, one scaling by 1/255 -- lie inside
   the bound the GPU test uses.
3. The two mutations of the GPU test (taps across the window edge, taps shifted by one frame) leave the bound by a wide margin at the taps concerned,
   and t = 1 gives exact zeros in every tap but the centre."""
import functools

import pytest
import torch

from oracle import vpt_oracle
from tests import conv3d_backward_ref as R

#          B  t  H   W
SHAPES = [(2, 3, 16, 16), (2, 7, 16, 32), (1, 1, 16, 16), (3, 5, 16, 16)]
COUT = 128


@functools.lru_cache(maxsize=None)
def _case(i, fmt):
    b, t, h, w = SHAPES[i]
    g = torch.Generator().manual_seed(900 + i)
    img = torch.randint(0, 256, (b * t, h, w, 3), generator=g, dtype=torch.uint8)
    sd = {"net.conv3d_layer.layer.weight": (torch.randn(COUT, 3, 5, 1, 1, generator=g, dtype=torch.float64) * 0.4).requires_grad_(),
          "net.conv3d_layer.layer.bias": (torch.randn(COUT, generator=g, dtype=torch.float64) * 0.2).requires_grad_()}
    dy = (torch.randn(b * t, COUT, h, w, generator=g) * (1e-2 if fmt == "fp16" else 1.0)).to(R.DT[fmt]).double()
    with torch.enable_grad():
        y = vpt_oracle.conv3d_temporal(sd, img.double().view(b, t, h, w, 3) / 255.0)            # [B,T,H,W,O]
        y_nchw = y.reshape(b * t, h, w, COUT).permute(0, 3, 1, 2)
        gw, gb = torch.autograd.grad((y_nchw * dy).sum(), [sd["net.conv3d_layer.layer.weight"], sd["net.conv3d_layer.layer.bias"]])
    y16 = y_nchw.detach().to(R.DT[fmt]).double()
    return dict(img=img, t=t, n=b * t * h * w, y=y_nchw.detach(), y16=y16, dy=dy, gw=gw.view(COUT, 3, 5), gb=gb)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_reference_is_the_gradient(i, fmt):
    c = _case(i, fmt)
    assert torch.equal(c["y16"] > 0, c["y"] > 0), "the stored tensor must open autograd's gates"
    dw, db, _, _ = R.backward_ref(c["img"], c["y16"], c["dy"], c["t"])
    assert float((dw - c["gw"]).abs().max()) <= 1e-9 * float(c["gw"].abs().max())
    assert float((db - c["gb"]).abs().max()) <= 1e-9 * float(c["gb"].abs().max())
    if c["t"] == 1:
        assert not bool(dw[:, :, [0, 1, 3, 4]].any())


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_fp32_arithmetic_meets_the_bound(i, fmt):
    c = _case(i, fmt)
    m = c["img"].shape[0]
    dw, db, dw_abs, db_abs = R.backward_ref(c["img"], c["y16"], c["dy"], c["t"])
    b_dw, b_db = R.bounds(c["n"], dw, db, dw_abs, db_abs)
    g32 = (c["dy"] * (c["y16"] > 0)).float()
    x32 = c["img"].float()
    inv = torch.tensor(1.0 / 255.0, dtype=torch.float32)
    for order in ("torch", "sequential"):
        got = torch.zeros(COUT, 3, 5, dtype=torch.float32)
        for dt in range(5):
            src, valid = R.tap_frames(m, c["t"], dt)
            prod = g32.permute(1, 0, 2, 3).reshape(COUT, 1, -1) * (x32[src] * valid.view(m, 1, 1, 1).float()).permute(3, 0, 1, 2).reshape(1, 3, -1)
            assert torch.equal(prod.double(), g32.double().permute(1, 0, 2, 3).reshape(COUT, 1, -1)
                               * (x32[src] * valid.view(m, 1, 1, 1).float()).double().permute(3, 0, 1, 2).reshape(1, 3, -1)), "the products are exact in fp32"
            got[:, :, dt] = (prod.sum(-1) if order == "torch" else prod.cumsum(-1)[..., -1]) * inv
        gb = g32.permute(1, 0, 2, 3).reshape(COUT, -1)
        gb = gb.sum(-1) if order == "torch" else gb.cumsum(-1)[:, -1]
        R.check(f"fp32 {order} dW {SHAPES[i]} {fmt}", got, dw, b_dw)
        R.check(f"fp32 {order} db {SHAPES[i]} {fmt}", gb, db, b_db)


@pytest.mark.parametrize("i", [0, 1])
def test_mutations_leave_the_bound(i):
    c = _case(i, "bf16")
    dw, db, dw_abs, db_abs = R.backward_ref(c["img"], c["y16"], c["dy"], c["t"])
    b_dw, _ = R.bounds(c["n"], dw, db, dw_abs, db_abs)
    cross = R.backward_ref(c["img"], c["y16"], c["dy"], c["t"], cross_window=True)[0]
    assert torch.equal(cross[:, :, 2], dw[:, :, 2])                       # the centre tap never leaves its window
    for dt in (0, 1, 3, 4):
        assert float(R.worst_ratio(cross[:, :, dt], dw[:, :, dt], b_dw[:, :, dt]).max()) > 100
    shifted = R.backward_ref(c["img"], c["y16"], c["dy"], c["t"], shift=1)[0]
    for dt in range(5):
        assert float(R.worst_ratio(shifted[:, :, dt], dw[:, :, dt], b_dw[:, :, dt]).max()) > 100
