"""The attention kernels -- vpt_attn_kernel (banded and mask "none"), vpt_attn_step_kernel, vpt_attn_bwd_kernel, vpt_full_attn_bwd_kernel and their finish
kernels -- held to the two instruments of tests/attention_ref.py: exact values on inputs whose softmax is exactly one-hot or (1/2, 1/2), element for
element, and an fp64 reference under a derived per-element bound on real-valued inputs.  Needs an MI355X.  Every check prints `max err / bound`.

Shapes (attention_ref.SHAPES): t = 1 with maxlen = 1; one full tile; maxlen = 129 (all 160 staged key slots, all 10 * 129 bias floats) with a second
tile of one query; episode starts around a tile edge; t = 200 (fifth key tile, five slabs per key); maxlen below the tile; an odd head count, whose
row length is padded to a multiple of 4 with nonzero values (heads = 1 likewise) -- the gradient of the padding must be exact zeros."""
import functools
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from tests import attention_ref as A  # noqa: E402

DEV = "cuda"
BANDED = [(b, t, ml, h, w) for b, t, ml, h, where in A.SHAPES for w in (None, where)]
IDS = [f"B{b}-t{t}-maxlen{ml}-heads{h}-{'qlo' if w else 'plain'}" for b, t, ml, h, w in BANDED]
RATIOS = {}


def _note(op, res):
    for k, v in res.items():
        RATIOS[(op, k)] = max(RATIOS.get((op, k), 0.0), v)


def _dev(c):
    d = SimpleNamespace(qkvr=c.qkvr.to(DEV), dout=c.dout.to(DEV))
    if c.causal:
        d.kmem, d.vmem, d.memvalid, d.b_nd = c.kmem.to(DEV), c.vmem.to(DEV), c.memvalid.to(DEV), c.b_nd.to(DEV)
        d.qlo = c.qlo.to(DEV) if c.qlo is not None else None
    return d


def _forward(c, d, fmt):
    if c.causal:
        out = ops.masked_attention(d.qkvr, d.kmem, d.vmem, d.memvalid, d.b_nd, c.B, c.t, c.heads, c.hid, dtype=A.DT[fmt], qlo=d.qlo)
    else:
        out = ops.full_attention(d.qkvr, c.B, c.t, c.heads, c.hid, dtype=A.DT[fmt])
    assert out.dtype == A.DT[fmt]
    return out


def _backward(c, d):
    if not c.causal:
        return ops.full_attention_backward(d.qkvr, d.dout, c.B, c.t, c.heads, c.hid), None
    db = torch.zeros(10, c.maxlen, device=DEV)
    dq = ops.masked_attention_backward(d.qkvr, d.kmem, d.vmem, d.memvalid, d.b_nd, d.dout, db, c.B, c.t, c.heads, c.hid, qlo=d.qlo)
    return dq, db


def _run_real(c, o, op, name):
    d = _dev(c)
    outs = {fmt: _forward(c, d, fmt) for fmt in ("bf16", "fp16")}
    dq, db = _backward(c, d)
    torch.cuda.synchronize()
    res, msgs = A.ratios(c, o, outs["bf16"].cpu(), dq.cpu(), db.cpu() if db is not None else None, "bf16")
    r16, m16 = A.ratios(c, o, outs["fp16"].cpu(), None, None, "fp16")
    res["out fp16"] = r16["out"]
    print(f"{op} {name}: max err / bound: " + "  ".join(f"{k} {v:.4f}" for k, v in res.items()))
    _note(op, res)
    assert not (msgs + m16), "\n".join(msgs + m16)


def _run_exact(c, name):
    o = A.compute(c, flush=True)
    d = _dev(c)
    outs = {fmt: _forward(c, d, fmt) for fmt in ("bf16", "fp16")}
    dq, db = _backward(c, d)
    torch.cuda.synchronize()
    msgs = []
    for fmt in ("bf16", "fp16"):
        msgs += A.exact_failures(c, o, outs[fmt].cpu(), dq.cpu() if fmt == "bf16" else None, db.cpu() if db is not None and fmt == "bf16" else None)
    return [f"{name}: {m}" for m in msgs]


@functools.lru_cache(maxsize=None)
def _real(i):
    c = A.real_case(*BANDED[i], seed=i)
    return c, A.compute(c)


@pytest.mark.parametrize("i", range(len(BANDED)), ids=IDS)
def test_banded_attention_real_values(i):
    c, o = _real(i)
    _run_real(c, o, "masked_attention" + (" qlo" if c.qlo is not None else ""), IDS[i])


@pytest.mark.parametrize("i", range(len(BANDED)), ids=IDS)
def test_banded_attention_exact_values(i):
    fails = []
    for fam, rule in A.EXACT_RUNS:
        fails += _run_exact(A.exact_case(*BANDED[i], family=fam, rule=rule, seed=i), f"{IDS[i]} {fam} {rule}")
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("t", A.NONE_TS)
def test_full_attention_real_values(t):
    c = A.real_case(2, t, 0, 2, seed=t, causal=False)
    _run_real(c, A.compute(c), "full_attention", f"t = {t}")


@pytest.mark.parametrize("t", A.NONE_TS)
def test_full_attention_exact_values(t):
    fails = []
    for fam, rule in A.EXACT_RUNS[:-1]:                  # (no bias family: mask "none" has no relative-position bias)
        fails += _run_exact(A.exact_case(2, t, 0, 2, family=fam, rule=rule, seed=t, causal=False), f"t = {t} {fam} {rule}")
    assert not fails, "\n".join(fails[:20])


# ---- the acting step ----------------------------------------------------------------------------------------------------------------------------------------
def _step(c, first, mode, fmt):
    """-> (out, next kmem, next vmem, next mask) on the CPU.  mode: "copy", "inplace" (memory in place, mask copied), "done" (everything in place)."""
    d = _dev(c)
    f8 = first.to(torch.uint8).to(DEV)
    km, vm, mk = d.kmem.clone(), d.vmem.clone(), d.memvalid.clone()
    if mode == "done":
        done = torch.zeros(c.B, dtype=torch.int32, device=DEV)
        out, ko, vo, mo = ops.masked_attention_step(d.qkvr, km, vm, mk, f8, d.b_nd, c.B, c.heads, c.hid, dtype=A.DT[fmt], inplace=True, done=done)
        assert ko is km and vo is vm and mo is mk and not bool(done.any()), "the in-place step must hand back its arguments and leave the counter zero"
    else:
        out, ko, vo, mo = ops.masked_attention_step(d.qkvr, km, vm, mk, f8, d.b_nd, c.B, c.heads, c.hid, dtype=A.DT[fmt], inplace=mode == "inplace")
        assert (ko is km and vo is vm) == (mode == "inplace") and torch.equal(mk, d.memvalid)
        if mode == "copy":
            assert torch.equal(km, d.kmem) and torch.equal(vm, d.vmem), "the copying step changed its input memory"
    torch.cuda.synchronize()
    return out.cpu(), ko.cpu(), vo.cpu(), mo.cpu()


@pytest.mark.parametrize("maxlen", A.STEP_MAXLENS)
def test_attention_step(maxlen):
    """Output under the bound (real values) and exact (one-hot and tie inputs); the shifted memory and the next mask bit for bit.  Sequence 0 starts an
    episode in the second pass, sequence 1 in neither."""
    fails = []
    modes = [("copy", "bf16"), ("inplace", "fp16"), ("done", "bf16")]
    for first in (torch.tensor([False, False]), torch.tensor([True, False])):
        c = A.real_case(2, 1, maxlen, 2, seed=maxlen)
        o, kout, vout, mout = A.step_ref(c, first)
        for mode, fmt in modes:
            out, ko, vo, mo = _step(c, first, mode, fmt)
            w, m = A.check(c, f"step out maxlen {maxlen} first {first.tolist()} {mode} {fmt}", "out", out, o.out, A.out_bound(o, fmt))
            print(f"masked_attention_step maxlen {maxlen} first {first.tolist()} {mode} {fmt}: max err / bound = {w:.4f}")
            _note("masked_attention_step", {f"out {fmt}": w})
            fails += [m] if m else []
            if not (torch.equal(ko, kout) and torch.equal(vo, vout) and torch.equal(mo, mout)):
                fails.append(f"maxlen {maxlen} first {first.tolist()} {mode}: shifted memory or next mask differ from the reference's")
        for fam, rule in [("onehot", 0), ("onehot", 1), ("onehot", 2), ("onehot", 7), ("tie", 0), ("tie", 4), ("bias", 0)]:
            c = A.exact_case(2, 1, maxlen, 2, family=fam, rule=rule, seed=maxlen)
            o, kout, vout, mout = A.step_ref(c, first)
            o = A.compute(SimpleNamespace(**{**vars(c), "memvalid": (c.memvalid.bool() & ~first.view(-1, 1)).to(torch.uint8)}), flush=True, backward=False)
            for mode, fmt in modes:
                out, ko, vo, mo = _step(c, first, mode, fmt)
                m = A.check_exact(c, f"step maxlen {maxlen} first {first.tolist()} {fam} {rule} {mode} {fmt}", "out", out, o.out)
                fails += [m] if m else []
                if not (torch.equal(ko, kout) and torch.equal(vo, vout) and torch.equal(mo, mout)):
                    fails.append(f"maxlen {maxlen} first {first.tolist()} {fam} {rule} {mode}: shifted memory or next mask differ from the reference's")
    assert not fails, "\n".join(fails[:20])


def test_print_worst_ratios():
    """Not a check: the table profiles/attention_fp64_ratios.md quotes (run the module with -s)."""
    for key in sorted(RATIOS):
        print("worst err / bound:", *key, f"{RATIOS[key]:.4f}")
