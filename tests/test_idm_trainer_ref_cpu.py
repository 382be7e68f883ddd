"""The fp64 reference of the IDM trainer (tests/idm_trainer_ref.py) and the host twin of the IDM loss (packing.idm_loss_metrics), without a GPU:
the reference reproduces the oracle's forward, its loss passes torch's gradcheck, and the twin equals a direct torch expression."""
import torch

import vpt_amd  # noqa: F401
from vpt_amd import packing
from oracle import vpt_oracle as O
from tests import idm_trainer_ref as IR
from tests import labeler_ref as R
from tests import parity as P


def test_reference_reproduces_the_oracle_forward():
    """Unrounded, on the oracle's own CNN output: fp32 (the oracle) against fp64 of the same arithmetic -> 1e-5 max-abs on the log-probs."""
    _, cfg, sd = R.tiny_idm()
    b, t = 2, 6
    img = P.structured_frames(b, t, torch.Generator().manual_seed(3))
    ref = O.idm_forward(sd, cfg, img)
    with torch.no_grad():
        x = O.conv3d_temporal(sd, img.to(torch.float32) / 255.0)
        d = O.impala_cnn(sd, "net.img_process.cnn.", x.reshape(b * t, *x.shape[2:]))       # relu(dense): the reference applies the ReLU again, a no-op
        sd64 = {k: v.double() for k, v in sd.items() if v.dtype.is_floating_point}
        lp_b, lp_c = IR.forward(sd64, cfg, d.double(), b, t)
    err_b = float((lp_b.reshape(b, t, 20, 2) - ref["buttons"].double()).abs().max())
    err_c = float((lp_c.reshape(b, t, 2, -1) - ref["camera"].double()).abs().max())
    print(f"IDM trainer reference vs oracle.idm_forward: max-abs log-prob error buttons {err_b:.2e}, camera {err_c:.2e}")
    assert err_b < 1e-5 and err_c < 1e-5


def test_rounded_reference_stays_close_and_trainable_set():
    _, cfg, sd = R.tiny_idm()
    names = IR.trainable_names(sd, cfg)
    assert not any(n.startswith(("net.conv3d_layer.", "net.img_process.cnn.", "net.lastlayer.")) or n.endswith("b_nd") for n in names)
    assert "net.img_process.linear.layer.weight" in names and "pi_head.camera.linear_layer.bias" in names and "net.final_ln.weight" in names
    b, t = 1, 5
    g = torch.Generator().manual_seed(4)
    d = torch.randn(b * t, 256, generator=g).double()
    sd64 = {k: v.double() for k, v in sd.items() if v.dtype.is_floating_point}
    with torch.no_grad():
        exact = IR.forward(sd64, cfg, d, b, t)
        err = {}
        for mode in ("fp16", "bf16"):
            rounded = IR.forward(sd64, cfg, d, b, t, rnd=mode)
            err[mode] = max(float((a - e).abs().max()) for a, e in zip(rounded, exact))
    # the switch rounds (error > 0), the coarser format errs more, and O(1) logits behind a dozen GEMMs whose operands carry a relative 2^-8
    # stay far from an O(1) error
    assert 0.0 < err["fp16"] < err["bf16"] < 0.5, err


def test_loss_gradcheck_on_a_two_group_toy():
    """torch.autograd.gradcheck of the weighted grouped NLL (2 button groups of 2, 2 camera groups of 3) w.r.t. the logits."""
    g = torch.Generator().manual_seed(5)
    m = 4
    zb = torch.randn(m, 2, 2, generator=g, dtype=torch.float64, requires_grad=True)
    zc = torch.randn(m, 2, 3, generator=g, dtype=torch.float64, requires_grad=True)
    ab = torch.randint(0, 2, (m, 2), generator=g)
    ac = torch.randint(0, 3, (m, 2), generator=g)
    w = torch.tensor([1.0, 0.0, 0.5, 2.0], dtype=torch.float64)
    fn = lambda a, c: IR.loss_from_logprobs(torch.log_softmax(a / 2.0, -1), torch.log_softmax(c / 2.0, -1), ab, ac, w)
    assert torch.autograd.gradcheck(fn, (zb, zc), eps=1e-6, atol=1e-7)
    # ... and the twin of the kernel's gradient is that gradient (d/dz of log_softmax(z / T): (softmax - onehot) / T, scale = 1 / (sum w x T))
    gb, gc = torch.autograd.grad(fn(zb, zc), [zb, zc])
    lp_b, lp_c = torch.log_softmax(zb.detach() / 2.0, -1), torch.log_softmax(zc.detach() / 2.0, -1)
    twin = packing.idm_loss_grad(lp_b, lp_c, ab, ac, 1.0 / (float(w.sum()) * 2.0), w)
    assert torch.allclose(twin, torch.cat([gb.reshape(m, -1), gc.reshape(m, -1)], 1), atol=1e-12, rtol=0)
    assert float(twin[1].abs().max()) == 0.0


def test_idm_loss_metrics_against_a_direct_expression():
    g = torch.Generator().manual_seed(6)
    m = 7
    lp_b = torch.log_softmax(torch.randn(m, 20, 2, generator=g, dtype=torch.float64), -1)
    lp_c = torch.log_softmax(torch.randn(m, 2, 11, generator=g, dtype=torch.float64), -1)
    ab = torch.randint(0, 2, (m, 20), generator=g)
    ac = torch.randint(0, 11, (m, 2), generator=g)
    w = torch.rand(m, generator=g, dtype=torch.float64)
    w[2] = 0.0
    w[5] = 0.0
    lp_b[2] = float("nan")            # a row left out of the loss adds exact zeros whatever it holds
    fo, tot = packing.idm_loss_metrics(lp_b, lp_c, ab, ac, w)
    live = [r for r in range(m) if float(w[r]) != 0.0]
    exp = torch.zeros(8, dtype=torch.float64)
    for r in range(m):
        nll_b = -sum(lp_b[r, k, ab[r, k]] for k in range(20))
        nll_c = -sum(lp_c[r, k, ac[r, k]] for k in range(2))
        ent_b = -(lp_b[r].exp() * lp_b[r]).sum()
        ent_c = -(lp_c[r].exp() * lp_c[r]).sum()
        hit_b = sum(float(lp_b[r, k].argmax() == ab[r, k]) for k in range(20)) / 20.0
        hit_c = sum(float(lp_c[r, k].argmax() == ac[r, k]) for k in range(2)) / 2.0
        row = torch.stack([torch.as_tensor(v, dtype=torch.float64) for v in (nll_b, nll_c, ent_b, ent_c, hit_b, hit_c)])
        if r in live:
            assert torch.allclose(fo[r, :6], row, atol=1e-12, rtol=0)
            exp[:6] += w[r] * row
            exp[6] += w[r]
            exp[7] += 1
        assert float(fo[r, 6]) == float(w[r]) and float(fo[r, 7]) == 0.0
    assert torch.allclose(tot, exp, atol=1e-12, rtol=0) and not torch.isnan(tot).any()
    # all ones when no weights are given; the loss of the reference is the totals' (nll_b + nll_c) / sum w
    lp_b[2] = torch.log_softmax(torch.randn(20, 2, generator=g, dtype=torch.float64), -1)
    fo1, tot1 = packing.idm_loss_metrics(lp_b, lp_c, ab, ac)
    assert float(tot1[6]) == m and float(tot1[7]) == m
    assert abs(float((tot1[0] + tot1[1]) / tot1[6]) - float(IR.loss_from_logprobs(lp_b, lp_c, ab, ac))) < 1e-12
