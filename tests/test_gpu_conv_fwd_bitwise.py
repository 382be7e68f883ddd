"""The forward modes of vpt_conv3x3_kernel (0, 1, 4, 5, 7), held BIT FOR BIT to recorded results: sha256 of every output tensor and of the
frame statistics each launch accumulates, on CPU-seeded inputs, in both operand formats.  Needs an MI355X.

The expected hashes (tests/golden/conv3x3_fwd_hashes.json) were recorded by tools/conv_hash_record.py from the libraries of the commit BEFORE
the forward main loop was re-scheduled (first tap with C = 0 instead of zeroed accumulators, earlier fragment requests): a schedule change
must not move one bit -- the K order of every output element stays (channel block, kernel row, kernel column) and the rounding points stay.

Shapes: the four CASES of test_gpu_conv_mfma16.py (one, two and three channel blocks = prologue only / prologue + tail / loop body once; partial
channel tiles; all nine edge classes; interior tiles) plus `pool32` = 32 x 32, cin 64, cout 160 (seams both ways, second channel tile partial).
The 32-row / eight-wave tiles run on the cases whose height is a multiple of 32 (`pool32`: one frame of 32 x 32; `interior`: 64 x 64).

The frame statistics are fp64 atomic sums of per-tile fp32 partial sums: every addend has a 24-bit significand, so the fp64 sum of a frame's
few tiles is exact and does not depend on the order in which the tiles finish."""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops, packing  # noqa: E402
from tests.test_gpu_conv_mfma16 import CASES as _MFMA16_CASES  # noqa: E402

DEV = "cuda"
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv3x3_fwd_hashes.json")

#        name      frames h   w   cin cout
CASES = dict(_MFMA16_CASES, pool32=(1, 32, 32, 64, 160))


def _h(*ts):
    m = hashlib.sha256()
    for t in ts:
        m.update(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return m.hexdigest()


def case_hashes(name, fmt):
    """{"<mode tag>": sha256 of (output[, masks], stats_out)} of one case in one operand format."""
    frames, h, w, cin, cout = CASES[name]
    dt = DT[fmt]
    g = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    W = torch.randn(cout, cin, 3, 3, generator=g) * (1.6 / (cin * 9) ** 0.5)
    gain = 1 + 0.2 * torch.randn(cin, generator=g)
    bias = 0.1 * torch.randn(cin, generator=g)
    x = (torch.relu(torch.randn(frames, cin, h, w, generator=g)) + 0.2 * torch.randn(frames, cin, h, w, generator=g)).to(dt)
    res = torch.randn(frames, cout, h, w, generator=g).to(dt)
    wpk, sa, sg = ops.pack_conv3x3(W.to(DEV), gain.to(DEV), bias.to(DEV), dtype=dt)
    kk = (0.3 * torch.randn(frames, 9, sa.shape[1], generator=g)).to(DEV)
    rs = (0.5 + torch.rand(frames, generator=g)).to(DEV)
    rsc = (0.5 + torch.rand(frames, generator=g)).to(DEV)
    rb = (0.3 * torch.randn(frames, cout, generator=g)).to(DEV)
    flat = x.double().reshape(frames, -1)
    st_in = torch.stack([flat.sum(1), (flat * flat).sum(1)], 1).contiguous().to(DEV)
    xb = packing.nchw_to_blocked(x.float(), dtype=dt).to(DEV)
    resb = packing.nchw_to_blocked(res.float(), dtype=dt).to(DEV)

    def stats():
        return torch.zeros(frames, 2, dtype=torch.float64, device=DEV)

    out = {}
    tilings = ["throughput"] + (["throughput32"] if h % 32 == 0 else [])
    for tiling in tilings:
        tag = "" if tiling == "throughput" else "/rows32"
        s0, s1 = stats(), stats()
        y0 = ops.conv3x3(xb, wpk, sa, sg, st_in, cout, stats_out=s0, tiling=tiling)
        y1 = ops.conv3x3(xb, wpk, sa, sg, st_in, cout, res=resb, stats_out=s1, tiling=tiling)
        torch.cuda.synchronize()
        out["mode0" + tag] = _h(y0, s0)
        out["mode1" + tag] = _h(y1, s1)
    s5, s4, s7 = stats(), stats(), stats()
    y5 = ops.conv3x3_folded(xb, wpk, sa, sg, st_in, cout, kk_frame=kk, rs_frame=rs, res=resb, res_scale=rsc, res_bias=rb, stats_out=s5)
    y4 = ops.conv3x3_pool(xb, wpk, sa, sg, st_in, cout, stats_out=s4)
    y7, m7 = ops.conv3x3_pool_argmax(xb, wpk, sa, sg, st_in, cout, stats_out=s7)
    torch.cuda.synchronize()
    out["mode5"] = _h(y5, s5)
    out["mode4"] = _h(y4, s4)
    out["mode7"] = _h(y7, m7 & 0x1ff, s7)
    return out


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_conv3x3_forward_bitwise(name, fmt):
    with open(GOLDEN) as f:
        golden = json.load(f)[fmt][name]
    got = case_hashes(name, fmt)
    assert sorted(got) == sorted(golden), (sorted(got), sorted(golden))
    for k in sorted(got):
        print(f"{name} {fmt} {k}: {got[k][:16]} (recorded {golden[k][:16]})")
    bad = [k for k in sorted(got) if got[k] != golden[k]]
    assert not bad, f"{name} {fmt}: outputs / statistics differ from the recorded ones in {bad}"
