"""The attention kernels (vpt_attn_kernel banded and mask "none", vpt_attn_bwd_kernel, vpt_full_attn_bwd_kernel and the two finish kernels), held
BIT FOR BIT to recorded results: sha256 of ops.masked_attention / ops.full_attention in both operand formats, of ops.masked_attention_backward's
dqkvr and db_nd and of ops.full_attention_backward's dqkv, on CPU-seeded inputs.  Needs an MI355X.  The twin of tests/test_gpu_conv_dgrad_bitwise.py.

The expected hashes (tests/golden/attention_hashes.json) were recorded by tools/conv_hash_record.py from the libraries of the commit BEFORE the
tile helpers of csrc/vpt_attn_tile.h and the source csrc/vpt_attn_bwd.hip existed.  tests/test_gpu_attention_fp64.py holds the same kernels to exact
values and to fp64 bounds, which a change that reorders an addition or contracts a multiply-add differently would pass; moving code must not move
one bit -- every summation order, parenthesisation, sentinel and rounding point stays.

Cases: the seven attention_ref.SHAPES, each plain and with its episode starts (t = 1; one full tile; maxlen = 129 with all 160 key slots; starts around
a tile edge; t = 200 with the fifth key tile and five slabs per key; maxlen below the tile; an odd head count with padding columns), and the four
attention_ref.NONE_TS windows of mask "none" (B = 2, two heads) -- attention_ref.real_case inputs, seed = the banded case's position in that list of
fourteen, resp. the window length t.  The gradients are
fp32 and do not depend on the operand format: they are computed once per case and recorded with its "bf16" entry.

Why the gradients have ONE bit pattern, whatever order the workgroups run in.  dQ and dR: each element is written by exactly one workgroup (its query
tile).  dK / dV: a key is reached by several query tiles; each tile stores its piece to a slab slot of its own (banded: slot = query tile - key
tile, 0..4; mask "none": slot = query tile) and the finish kernel adds a key's slots in slot order, one thread per element.  db_nd: every workgroup
stores its [10][maxlen] piece to its own slab row (row = blockIdx) and vpt_slab_sum adds the rows in a fixed order that is a function of the row
count alone.  No atomics anywhere, and the grid is a function of (B, t, heads): the sums are the same expression on every run."""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from tests import attention_ref as A  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_hashes.json")
# name -> real_case arguments (B, t, maxlen, heads, episode starts, seed, causal)
CASES = {}
for _i, (_b, _t, _ml, _h, _w) in enumerate((b, t, ml, h, w) for b, t, ml, h, where in A.SHAPES for w in (None, where)):
    CASES[f"B{_b}-t{_t}-maxlen{_ml}-heads{_h}-{'qlo' if _w else 'plain'}"] = (_b, _t, _ml, _h, _w, _i, True)
for _t in A.NONE_TS:
    CASES[f"none-t{_t}"] = (2, _t, 0, 2, None, _t, False)


def _h(*ts):
    m = hashlib.sha256()
    for t in ts:
        m.update(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return m.hexdigest()


def case_hashes(name, fmt):
    """{"out": sha256 of the forward output in `fmt`} and, for fmt = "bf16", the fp32 gradients: "dqkvr" and "db_nd" (banded) or "dqkv" (mask "none")."""
    b, t, ml, heads, where, seed, causal = CASES[name]
    c = A.real_case(b, t, ml, heads, where, seed=seed, causal=causal)
    qkvr, dout = c.qkvr.to(DEV), c.dout.to(DEV)
    if causal:
        kmem, vmem, memvalid, b_nd = c.kmem.to(DEV), c.vmem.to(DEV), c.memvalid.to(DEV), c.b_nd.to(DEV)
        qlo = c.qlo.to(DEV) if c.qlo is not None else None
        out = {"out": _h(ops.masked_attention(qkvr, kmem, vmem, memvalid, b_nd, b, t, heads, c.hid, dtype=A.DT[fmt], qlo=qlo))}
        if fmt == "bf16":
            db = torch.zeros(10, ml, device=DEV)
            dqkvr = ops.masked_attention_backward(qkvr, kmem, vmem, memvalid, b_nd, dout, db, b, t, heads, c.hid, qlo=qlo)
            out["dqkvr"], out["db_nd"] = _h(dqkvr), _h(db)
    else:
        out = {"out": _h(ops.full_attention(qkvr, b, t, heads, c.hid, dtype=A.DT[fmt]))}
        if fmt == "bf16":
            out["dqkv"] = _h(ops.full_attention_backward(qkvr, dout, b, t, heads, c.hid))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_attention_bitwise(name, fmt):
    with open(GOLDEN) as f:
        golden = json.load(f)[fmt][name]
    got = case_hashes(name, fmt)
    assert sorted(got) == sorted(golden), (sorted(got), sorted(golden))
    for k in sorted(got):
        print(f"{name} {fmt} {k}: {got[k][:16]} (recorded {golden[k][:16]})")
    bad = [k for k in sorted(got) if got[k] != golden[k]]
    assert not bad, f"{name} {fmt}: outputs differ from the recorded ones in {bad}"
