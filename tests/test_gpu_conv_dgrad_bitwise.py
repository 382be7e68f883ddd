"""The dgrad modes of the 3x3 convolution (vpt_conv3x3_dgrad_kernel modes 2, 3, 6), held BIT FOR BIT to recorded results: sha256 of
ops.conv3x3_dgrad without and with `skip` (modes 2, 3) and of ops.conv3x3_dgrad_gated's operand and gate_u (mode 6), on CPU-seeded inputs, in
both operand formats.  Needs an MI355X.  The twin of tests/test_gpu_conv_fwd_bitwise.py.

The expected hashes (tests/golden/conv3x3_dgrad_hashes.json) were recorded by tools/conv_hash_record.py from the libraries of the commit BEFORE
the convolution's source was split by kernel family.  tests/test_gpu_cnn_backward_fp64.py holds the same modes to fp64 bounds, which a change that
reorders an addition would pass; moving code must not move one bit -- the K order of every output element stays (cout block, kernel row, kernel
column, 16-channel half) and the rounding points stay.

Shapes: the four CASES of tests/test_gpu_cnn_backward_fp64.py (one / two / three-plus channel blocks of the loop, a partial channel tile, all
nine edge classes, interior tiles, two frames); mode 6 on its BLOCK_CASES with cin = cout = the case's cin, as there.

gate_u is an fp64 atomic sum of per-tile fp32 partial sums: every addend has a 24-bit significand, so the fp64 sum of a frame's few tiles is
exact and does not depend on the order in which the tiles finish (the argument tests/test_gpu_conv_fwd_bitwise.py makes for the frame statistics)."""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops, packing  # noqa: E402
from tests.test_gpu_cnn_backward_fp64 import BLOCK_CASES, CASES  # noqa: E402

DEV = "cuda"
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv3x3_dgrad_hashes.json")


def _h(*ts):
    m = hashlib.sha256()
    for t in ts:
        m.update(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return m.hexdigest()


def case_hashes(name, fmt):
    """{"mode2" | "mode3": sha256 of dx, "mode6": sha256 of (operand, gate_u)} of one case in one operand format."""
    frames, h, w, cin, cout = CASES[name]
    dt = DT[fmt]
    gs = 1e-2 if fmt == "fp16" else 1.0          # the loss scale's job in training: the gradients must stay inside the format
    g = torch.Generator().manual_seed(2000 + sum(map(ord, name)))

    def blocked(t):
        return packing.nchw_to_blocked(t.float(), dtype=dt).to(DEV)

    def layer(ci, co):
        return torch.randn(co, ci, 3, 3, generator=g) * (1.6 / (ci * 9) ** 0.5), 1 + 0.2 * torch.randn(ci, generator=g)

    def act(c):                                  # a stored ReLU output: about half of its entries are exact zeros (the gates of mode 6)
        return torch.relu(torch.randn(frames, c, h, w, generator=g)).to(dt)

    def stats(t):
        flat = t.double().reshape(frames, -1)
        return torch.stack([flat.sum(1), (flat * flat).sum(1)], 1).contiguous().to(DEV)

    W, gain = layer(cin, cout)
    dacc = (gs * torch.randn(frames, cout, h, w, generator=g)).to(dt)
    skip = (gs * torch.randn(frames, cin, h, w, generator=g)).to(dt)
    xin = act(cin)
    coef = (gs * 0.1 * torch.randn(frames, 2, generator=g)).to(DEV)
    wt = packing.pack_conv3x3_dgrad(W.to(DEV), gain.to(DEV), dtype=dt)
    daccb, xinb = blocked(dacc), blocked(xin)
    dx2 = ops.conv3x3_dgrad(daccb, wt, cin, xin=xinb, coef=coef)
    dx3 = ops.conv3x3_dgrad(daccb, wt, cin, skip=blocked(skip), xin=xinb, coef=coef)
    torch.cuda.synchronize()
    out = {"mode2": _h(dx2), "mode3": _h(dx3)}
    if name in BLOCK_CASES:                      # a block's conv1 -> conv0: cin = cout = the case's cin
        W1, g1 = layer(cin, cin)
        dacc1 = (gs * torch.randn(frames, cin, h, w, generator=g)).to(dt)
        x0 = act(cin) + (0.2 * torch.randn(frames, cin, h, w, generator=g)).to(dt)      # conv0's input: only its statistics enter
        wt1 = packing.pack_conv3x3_dgrad(W1.to(DEV), g1.to(DEV), dtype=dt)
        dacc0, gate_u = ops.conv3x3_dgrad_gated(blocked(dacc1), wt1, cin, xinb, coef, stats(x0), cin)
        torch.cuda.synchronize()
        out["mode6"] = _h(dacc0, gate_u)
    return out


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_conv3x3_dgrad_bitwise(name, fmt):
    with open(GOLDEN) as f:
        golden = json.load(f)[fmt][name]
    got = case_hashes(name, fmt)
    assert sorted(got) == sorted(golden), (sorted(got), sorted(golden))
    for k in sorted(got):
        print(f"{name} {fmt} {k}: {got[k][:16]} (recorded {golden[k][:16]})")
    bad = [k for k in sorted(got) if got[k] != golden[k]]
    assert not bad, f"{name} {fmt}: outputs differ from the recorded ones in {bad}"
