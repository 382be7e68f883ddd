"""ops.full_attention_backward (vpt_full_attn_bwd_kernel: the backward of the IDM's mask-"none" attention) against fp64 autograd of
softmax(Q K^T / 128) V.  Needs an MI355X.  The bound is the project's for its fp32 attention backward (tests/test_gpu_training.py): rel-L2 < 1e-3
on each of dQ, dK, dV; on top of it the properties the trainer relies on -- zero padding columns, the same bits from call to call, a window
that does not depend on its neighbours, and the length check in front of any launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402

DEV = "cuda"
DH = 128


def _l2(a, ref):
    return float((a - ref).norm() / ref.norm().clamp(min=1e-30))


def _inputs(bsz, t, heads, pad=0, seed=4):
    g = torch.Generator().manual_seed(seed)
    hid = heads * DH
    qkv = torch.randn(bsz * t, 3 * hid + pad, generator=g)
    qkv[:, :hid] *= 2.0
    dout = torch.randn(bsz * t, hid, generator=g)
    return qkv, dout, hid


def _reference(qkv, dout, bsz, t, heads, hid):
    """fp64 autograd of the forward ops.full_attention computes -> d/d(qkv[:, :3 hid])."""
    x = qkv[:, :3 * hid].double().requires_grad_(True)
    sp = lambda z: z.reshape(bsz, t, heads, DH).permute(0, 2, 1, 3)
    q, k, v = sp(x[:, :hid]), sp(x[:, hid:2 * hid]), sp(x[:, 2 * hid:])
    out = (torch.softmax(q @ k.transpose(-1, -2) / DH, -1) @ v).permute(0, 2, 1, 3).reshape(bsz * t, hid)
    return torch.autograd.grad((out * dout.double()).sum(), x)[0]


def _run(qkv, dout, bsz, t, heads, hid):
    d = ops.full_attention_backward(qkv.to(DEV), dout.to(DEV), bsz, t, heads, hid)
    torch.cuda.synchronize()
    return d.cpu()


# all five key tiles full; one partial tile; one row past a tile edge; a single row
@pytest.mark.parametrize("bsz,t,heads", [(1, 160, 2), (2, 12, 2), (3, 33, 1), (1, 1, 1)])
def test_against_fp64_autograd(bsz, t, heads):
    qkv, dout, hid = _inputs(bsz, t, heads)
    ref = _reference(qkv, dout, bsz, t, heads, hid)
    d = _run(qkv, dout, bsz, t, heads, hid)
    assert d.shape == qkv.shape and d.dtype == torch.float32
    if t == 1:        # one key: P = 1, dS = 0 exactly
        assert float(d[:, :2 * hid].abs().max()) == 0.0
        assert torch.equal(d[:, 2 * hid:], dout)
        return
    for name, sl in (("dQ", slice(0, hid)), ("dK", slice(hid, 2 * hid)), ("dV", slice(2 * hid, 3 * hid))):
        err = _l2(d[:, sl].double(), ref[:, sl])
        print(f"full attention backward B={bsz} t={t} heads={heads}: {name} rel-L2 {err:.2e}")
        assert err < 1e-3, f"{name} rel L2 {err}"


def test_padding_columns_are_written_as_zeros():
    bsz, t, heads = 2, 12, 2
    qkv, dout, hid = _inputs(bsz, t, heads, pad=64, seed=5)       # ld = 3 hid + 64, non-zero values in the padding
    assert float(qkv[:, 3 * hid:].abs().min()) > 0.0
    ref = _reference(qkv, dout, bsz, t, heads, hid)
    d = _run(qkv, dout, bsz, t, heads, hid)
    assert float(d[:, 3 * hid:].abs().max()) == 0.0
    assert _l2(d[:, :3 * hid].double(), ref) < 1e-3


def test_two_calls_give_the_same_bits():
    bsz, t, heads = 3, 33, 2
    qkv, dout, hid = _inputs(bsz, t, heads, seed=6)
    assert torch.equal(_run(qkv, dout, bsz, t, heads, hid), _run(qkv, dout, bsz, t, heads, hid))


def test_a_window_does_not_depend_on_its_neighbour():
    t, heads = 40, 2
    qkv, dout, hid = _inputs(2, t, heads, seed=7)
    both = _run(qkv, dout, 2, t, heads, hid)
    alone = _run(qkv[:t].contiguous(), dout[:t].contiguous(), 1, t, heads, hid)
    assert torch.equal(both[:t], alone)


def test_too_long_a_window_raises_before_any_launch():
    heads = 1
    qkv, dout, hid = _inputs(1, 161, heads)
    with pytest.raises(NotImplementedError):
        ops.full_attention_backward(qkv.to(DEV), dout.to(DEV), 1, 161, heads, hid)
    # ... and the C entry point refuses the shapes the kernel cannot take (no launch: the arguments are checked first)
    q, d = qkv[:160].contiguous().to(DEV), dout[:160].contiguous().to(DEV)
    with pytest.raises(RuntimeError, match="vpt_full_attention_backward"):
        ops.full_attention_backward(q, d, 1, 160, 2, hid)            # hid != heads * 128
