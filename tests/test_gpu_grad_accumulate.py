"""vpt_grad_accumulate_multi on the GPU, both libraries, against torch's `acc + g`.  The tensor set of tests/test_gpu_grad_norm.py: views of ONE
flat buffer at odd element offsets (unaligned 16-byte accesses) with sentinel elements between them, the sizes around the 4-element group and the
1024-element block, one tensor of 257 blocks, 300 tensors of 1..7 elements; magnitudes 1e-30 .. 1e30 with both signs, signed zeros in both operands.
One fp32 add per element has one correctly rounded result, so every check is bit for bit.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import _native, ops  # noqa: E402
from vpt_amd._native import ptr  # noqa: E402

DEV = "cuda"
SIZES = [1, 3, 4, 1023, 1024, 1025, 4097, 262149]
SENTINEL = -7.0
_DATA = {}


def _carve(flat, sizes):
    """Views of `flat` at odd element offsets, in order; one or two elements of `flat` stay between neighbours."""
    views, off = [], 1
    for n in sizes:
        views.append(flat[off:off + n])
        off += n + (2 if (off + n) % 2 else 1)
        assert off % 2 == 1
    assert off <= flat.numel()
    return views


def _values(rng, n):
    """n fp32 values of magnitude 1e-30 .. 1e30 with both signs; every seventh element a signed zero."""
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 30, n)).astype(np.float32)
    x[0::7] = np.where(rng.integers(0, 2, len(x[0::7])) == 1, np.float32(-0.0), np.float32(0.0))
    return x


def _data():
    """-> dict(sizes, acc: host arrays, g: three sets of host addends), made once and never written."""
    if not _DATA:
        rng = np.random.default_rng(23)
        sizes = SIZES + [int(x) for x in rng.integers(1, 8, 300)]
        acc = [_values(rng, n) for n in sizes]
        gs = [[_values(rng, n) for n in sizes] for _ in range(3)]
        for a, g in zip(acc, gs[0]):          # the four sign combinations of zero + zero, and x + (-x), in the first elements that exist
            pairs = [(0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0), (1.5, -1.5)]
            for i, (u, v) in enumerate(pairs[:len(a)]):
                a[i], g[i] = np.float32(u), np.float32(v)
        _DATA.update(sizes=sizes, acc=acc, g=gs)
    return _DATA


def _on_device(host, sizes):
    """A sentinel-filled flat buffer with `host` copied into its carved views -> (flat, views)."""
    flat = torch.full((sum(sizes) + 2 * len(sizes) + 8,), SENTINEL, dtype=torch.float32, device=DEV)
    views = _carve(flat, sizes)
    for v, h in zip(views, host):
        v.copy_(torch.from_numpy(h))
    assert all(v.data_ptr() % 8 == 4 for v in views)
    return flat, views


def _gap_mask(flat, views):
    """True where `flat` belongs to no view."""
    mask = torch.ones(flat.numel(), dtype=torch.bool, device=flat.device)
    for v in views:
        off = (v.data_ptr() - flat.data_ptr()) // 4
        mask[off:off + v.numel()] = False
    return mask


def _accumulate(fmt, accs, grads):
    """The raw entry point of library `fmt` over ops' table (ops.grad_accumulate_ binds the bf16 library's)."""
    table, blk, _ = ops._adam_table(grads, accs, grads, grads)
    _native.call("vpt_grad_accumulate_multi", ptr(table), len(accs), blk, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), fmt=fmt)
    torch.cuda.synchronize()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_sum_equals_torch_and_nothing_else_is_written(fmt):
    """(a) every accumulator torch.equal to acc + g of torch, and equal in its int32 bit pattern; (b) every sentinel of both flat buffers and every
    addend bit-unchanged."""
    d = _data()
    aflat, accs = _on_device(d["acc"], d["sizes"])
    gflat, grads = _on_device(d["g"][0], d["sizes"])
    want = [a + g for a, g in zip(accs, grads)]              # torch, before the launch
    assert all(bool(torch.isfinite(w).all()) for w in want)
    a_before, g_before = aflat.clone(), gflat.clone()
    if fmt == "bf16":
        assert ops.grad_accumulate_(accs, grads) is not None
        torch.cuda.synchronize()
    else:
        _accumulate(fmt, accs, grads)
    for i, (a, w) in enumerate(zip(accs, want)):
        assert torch.equal(a, w), (i, a.numel())
        assert torch.equal(_bits(a), _bits(w)), (i, a.numel())        # (signed zeros: -0 + -0 = -0, x + (-x) = +0)
    gaps = _gap_mask(aflat, accs)
    assert int(gaps.sum()) >= len(accs) and bool((aflat[gaps] == SENTINEL).all())
    assert torch.equal(_bits(aflat[gaps]), _bits(a_before[gaps]))
    assert torch.equal(_bits(gflat), _bits(g_before))
    assert not torch.equal(_bits(aflat), _bits(a_before))
    # the zero cases really are in the data: the big tensor's first five sums
    big = accs[SIZES.index(262149)][:5].cpu()
    assert big.tolist() == [0.0, 0.0, 0.0, 0.0, 0.0] and _bits(big).tolist() == [0, 0, 0, -2 ** 31, 0]


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_inf_and_nan_land_in_their_own_elements_only(fmt):
    """(c) an inf in the tail element of the 1025-element tensor's addend (the second block's only element: a partial group) and a nan in the first
    element of the 4097-element tensor's accumulator: exactly those two elements of the sum are non-finite, every other element is torch's."""
    d = _data()
    aflat, accs = _on_device(d["acc"], d["sizes"])
    gflat, grads = _on_device(d["g"][1], d["sizes"])
    i_inf, i_nan = SIZES.index(1025), SIZES.index(4097)
    grads[i_inf][-1] = float("inf")
    accs[i_nan][0] = float("nan")
    want = [a + g for a, g in zip(accs, grads)]
    a_before = aflat.clone()
    _accumulate(fmt, accs, grads)
    assert float(accs[i_inf][-1]) == float("inf") and bool(torch.isnan(accs[i_nan][0]))
    bad = [(i, int(j)) for i, a in enumerate(accs) for j in (~torch.isfinite(a)).nonzero().flatten().tolist()]
    assert bad == [(i_inf, 1024), (i_nan, 0)]
    for i, (a, w) in enumerate(zip(accs, want)):
        assert torch.equal(_bits(a), _bits(w)) or i == i_nan
    assert torch.equal(_bits(accs[i_nan][1:]), _bits(want[i_nan][1:]))
    gaps = _gap_mask(aflat, accs)
    assert torch.equal(_bits(aflat[gaps]), _bits(a_before[gaps]))


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_three_accumulations_in_order(fmt):
    """(d) ((a + g1) + g2) + g3 of torch, and the same inputs give the same bits a second time."""
    d = _data()
    runs = []
    for _ in range(2):
        _, accs = _on_device(d["acc"], d["sizes"])
        sets = [_on_device(g, d["sizes"])[1] for g in d["g"]]
        want = [((a + g1) + g2) + g3 for a, g1, g2, g3 in zip(accs, *sets)]
        for grads in sets:
            _accumulate(fmt, accs, grads)
        assert all(torch.equal(_bits(a), _bits(w)) for a, w in zip(accs, want))
        runs.append(torch.cat([a.clone() for a in accs]))
    assert torch.equal(_bits(runs[0]), _bits(runs[1]))
    _, fresh = _on_device(d["acc"], d["sizes"])
    other = [(a + (g1 + g2)) + g3 for a, g1, g2, g3 in zip(fresh, *sets)]
    assert not torch.equal(_bits(torch.cat(other)), _bits(runs[0])), "the data cannot tell the order of the additions"


def test_front_end_refuses_mismatches_and_aliases():
    """(e) ValueError on mismatched lengths, mismatched sizes and an accumulator that shares storage with its addend; nothing is launched."""
    a = [torch.ones(5, device=DEV), torch.ones(1030, device=DEV)]
    g = [torch.ones(5, device=DEV), torch.ones(1030, device=DEV)]
    with pytest.raises(ValueError, match="accumulators"):
        ops.grad_accumulate_(a, g[:1])
    with pytest.raises(ValueError, match="elements"):
        ops.grad_accumulate_(a, [g[0], torch.ones(1029, device=DEV)])
    with pytest.raises(ValueError, match="shares storage"):
        ops.grad_accumulate_(a, [g[0], a[1]])
    with pytest.raises(ValueError, match="shares storage"):
        ops.grad_accumulate_([a[1][:100]], [a[1][50:150]])
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.grad_accumulate_([a[0]], [g[0].double()])
    torch.cuda.synchronize()
    assert all(bool((t == 1).all()) for t in a + g)
    assert ops.grad_accumulate_([], []) is None
    # two views of ONE buffer that do not overlap are fine (the arena's views next to a gradient cut from the same allocation)
    ops.grad_accumulate_([a[1][:100]], [a[1][100:200]])
    torch.cuda.synchronize()
    assert bool((a[1][:100] == 2).all()) and bool((a[1][100:] == 1).all())
