"""vpt_grad_norm_multi and vpt_adam_step_multi_clip on the GPU, both libraries, against the host twin (tests/grad_norm_ref.py) and its fp64 reference.
Tensors are views of ONE flat buffer at odd element offsets (unaligned 16-byte loads): the sizes around the 4-element group and the 1024-element
block, one tensor of 257 blocks (stage one's strided pass), 300 tensors of 1..7 elements (more than 256: stage two's).  About 1.3 MB.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import _native, ops  # noqa: E402
from vpt_amd._native import ptr  # noqa: E402
from tests import grad_norm_ref as R  # noqa: E402

DEV = "cuda"
SIZES = [1, 3, 4, 1023, 1024, 1025, 4097, 262149]
SCALES = [1.0, 1.0 / 2560, 1.0 / 3, 7e-5]
_DATA, _TWIN = {}, {}


def _carve(flat, sizes):
    """Views of `flat` at odd element offsets, in order."""
    views, off = [], 1
    for n in sizes:
        views.append(flat[off:off + n])
        off += n + (2 if (off + n) % 2 else 1)        # the next offset is odd again
        assert off % 2 == 1
    assert off <= flat.numel()
    return views


def _data():
    """-> (host arrays, device views): the fixed sizes, one random size < 50 000, 300 tiny tensors; a magnitude per tensor in 1e-6 .. 1e3."""
    if not _DATA:
        rng = np.random.default_rng(11)
        sizes = SIZES + [int(rng.integers(1, 50000))] + [int(x) for x in rng.integers(1, 8, 300)]
        host = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3)).astype(np.float32) for n in sizes]
        flat = torch.zeros(sum(sizes) + 2 * len(sizes) + 8, dtype=torch.float32, device=DEV)
        views = _carve(flat, sizes)
        for v, h in zip(views, host):
            v.copy_(torch.from_numpy(h))
        assert all(v.data_ptr() % 8 == 4 for v in views)
        _DATA.update(host=host, views=views, flat=flat, sizes=sizes)
    return _DATA["host"], _DATA["views"]


def _twin(scale, max_norm):
    key = (scale, max_norm)
    if key not in _TWIN:
        _TWIN[key] = R.restate_f32(_data()[0], scale, max_norm)
    return _TWIN[key]


def _raw_norm(fmt, grads, scale, max_norm, flag=None):
    """vpt_grad_norm_multi of library `fmt` with a workspace of the test's own -> (norm_out [4], per_tensor, tensor sums fp64, block partials)."""
    table, blk, _ = ops._adam_table(grads)
    n_t = len(grads)
    nbytes = int(_native.load(fmt).vpt_grad_norm_workspace_bytes(n_t, blk))
    assert nbytes == 8 * n_t + 4 * blk
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.full((4,), float("nan"), dtype=torch.float32, device=DEV)
    per = torch.full((n_t,), float("nan"), dtype=torch.float32, device=DEV)
    _native.call("vpt_grad_norm_multi", ptr(table), n_t, blk, ctypes.c_float(scale), ctypes.c_float(max_norm), ptr(ws), ptr(out), ptr(per), ptr(flag),
                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), fmt=fmt)
    torch.cuda.synchronize()
    return out, per, ws[:2 * n_t].view(torch.float64).clone(), ws[2 * n_t:].clone()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("scale", SCALES)
def test_kernels_equal_the_twin_and_sit_inside_the_bound(fmt, scale):
    """(a) block partials, per-tensor fp64 sums and the coefficient torch.equal to the twin, the norm equal or 1 ulp away; (b) the norm within the
    derived bound of the fp64 reference."""
    host, views = _data()
    probe = _twin(scale, 0.0)
    max_norm = float(probe["norm"]) * 0.37                   # well below the norm: a coefficient that is not 1
    tw = _twin(scale, max_norm)
    out, per, tsum, partials = _raw_norm(fmt, views, scale, max_norm)
    assert torch.equal(partials.cpu(), torch.from_numpy(np.concatenate(tw["partials"])))
    assert torch.equal(tsum.cpu(), torch.from_numpy(tw["tensor_sums"]))
    got, want = out.cpu().numpy(), tw["out"]
    ulp = abs(int(got[:1].view(np.int32)[0]) - int(want[:1].view(np.int32)[0]))
    print(f"[{fmt}] scale {scale:g}: norm {got[0]!r} twin {want[0]!r} ({ulp} ulp), coef {got[1]!r} twin {want[1]!r}")
    assert ulp <= 1
    assert got[1] == want[1] and 0.0 < got[1] < 1.0 and got[2] == 0.0 and got[3] == 0.0
    assert got[1] == R.coef_f32(got[0], max_norm)
    assert torch.equal(per.cpu(), torch.from_numpy(tw["per_tensor"])) or float((per.cpu().view(torch.int32) - torch.from_numpy(tw["per_tensor"]).view(torch.int32)).abs().max()) <= 1
    ref = R.norm_f64(host, scale)
    err = abs(float(got[0]) - ref) / ref
    print(f"[{fmt}] scale {scale:g}: norm vs fp64: max err / bound = {err / R.BOUND:.3f}")
    assert err <= R.BOUND
    # one tensor of magnitude 1e3 can carry the whole norm: each tensor's own norm is held to the same bound
    refs = np.array([R.norm_f64([h], scale) for h in host])
    errs = np.abs(per.cpu().numpy().astype(np.float64) - refs) / refs
    print(f"[{fmt}] scale {scale:g}: per-tensor norms vs fp64: max err / bound = {errs.max() / R.BOUND:.3f}")
    assert errs.max() <= R.BOUND
    # ops.grad_norm (bf16 library) is the same launch
    if fmt == "bf16":
        o2, p2 = ops.grad_norm(views, scale=scale, max_norm=max_norm, per_tensor=True)
        assert torch.equal(o2, out) and torch.equal(p2, per)
        assert float(ops.grad_norm(views, scale=scale)[1]) == 1.0 and float(ops.grad_norm(views, scale=scale, max_norm=float("inf"))[1]) == 1.0


def test_mutated_twins_land_far_outside_the_bound():
    """(b) what the bound can see on THIS data: a twin that drops each tensor's partial tail group, ignores the scale or skips the cross-wave stage
    misses the fp64 reference by far more than the bound the device result is held to."""
    host, _ = _data()
    scale = 1.0 / 3
    ref = R.norm_f64(host, scale)
    # the tiny tensors alone as well: there the tail groups are most of the norm
    tiny = host[len(SIZES) + 1:]
    ref_tiny = R.norm_f64(tiny, scale)
    # ... and the 257-block tensor alone: every wave of every block carries a quarter of it (on the whole set one 1e3-magnitude tiny tensor, all wave 0, dominates)
    large = [host[SIZES.index(262149)]]
    for mut, data, r in ((dict(drop_tail=True), tiny, ref_tiny), (dict(use_scale=False), host, ref), (dict(cross_wave=False), large, R.norm_f64(large, scale))):
        err = abs(float(R.restate_f32(data, scale, **mut)["norm"]) - r) / r
        print(f"mutation {mut}: err / bound = {err / R.BOUND:.3e}")
        assert err > 1000 * R.BOUND, (mut, err)
    flat = torch.zeros(4096, device=DEV)        # ... and the device on the tiny tensors alone is inside it
    views = _carve(flat, [len(t) for t in tiny])
    for v, h in zip(views, tiny):
        v.copy_(torch.from_numpy(h))
    out, _, _, _ = _raw_norm("bf16", views, scale, 0.0)
    assert abs(float(out[0]) - ref_tiny) <= R.BOUND * ref_tiny


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_planted_value_in_the_last_tail_element(fmt):
    """(c) 1e4 in the last element of the last tensor, everything else zero: exactly 1e4."""
    flat = torch.zeros(8192, dtype=torch.float32, device=DEV)
    views = _carve(flat, [1023, 4097, 3, 1030])              # the last tensor: a second block of 6 elements, one whole group and a partial one
    views[-1][-1] = 1e4
    out, per, _, _ = _raw_norm(fmt, views, 1.0, 5.0)
    assert float(out[0]) == 1e4 and float(per[-1]) == 1e4 and float(per[:-1].abs().max()) == 0.0
    assert float(out[1]) == float(R.coef_f32(np.float32(1e4), 5.0)) and float(out[2]) == 0.0


def _adam_state(views, seed):
    g = torch.Generator().manual_seed(seed)
    sizes = [v.numel() for v in views]
    bufs = [torch.zeros(_DATA["flat"].numel(), device=DEV) for _ in range(3)]
    p, m, v = (_carve(b, sizes) for b in bufs)
    for i in range(len(sizes)):
        p[i].copy_(torch.randn(sizes[i], generator=g))
        m[i].copy_(torch.randn(sizes[i], generator=g) * 1e-2)
        v[i].copy_(torch.rand(sizes[i], generator=g) * 1e-3)
    return bufs, p, m, v


HYPER = (3, ctypes.c_float(1e-2), ctypes.c_float(0.9), ctypes.c_float(0.999), ctypes.c_float(1e-8), ctypes.c_float(0.039428))


def _adam(fmt, name, grads, state, grad_scale, flag=None, coef=None):
    bufs, p, m, v = state
    table, blk, _ = ops._adam_table(grads, p, m, v)
    args = [ptr(table), len(grads), blk, *HYPER, ctypes.c_float(grad_scale), ptr(flag)]
    if name == "vpt_adam_step_multi_clip":
        args.append(ptr(coef))
    _native.call(name, *args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), fmt=fmt)
    torch.cuda.synchronize()
    return [b.clone() for b in bufs]


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_clipped_adam_equals_adam_on_premultiplied_gradients(fmt):
    """(d) vpt_adam_step_multi_clip with the kernel's coefficient == the unchanged vpt_adam_step_multi on (g * grad_scale) * coef formed in torch
    (grad_scale = 1 passed); with the threshold above the norm (coefficient exactly 1) == the unclipped entry.  p, m and v, bit for bit."""
    _, views = _data()
    gs = 1.0 / 3
    out, _, _, _ = _raw_norm(fmt, views, gs, 0.0)
    max_norm = float(out[0]) * 0.37
    out, _, _, _ = _raw_norm(fmt, views, gs, max_norm)
    assert 0.0 < float(out[1]) < 1.0
    clipped = _adam(fmt, "vpt_adam_step_multi_clip", views, _adam_state(views, 5), gs, coef=out[1:])
    pre_flat = (_DATA["flat"] * torch.tensor(gs, dtype=torch.float32, device=DEV)) * out[1]
    pre = _carve(pre_flat, _DATA["sizes"])
    anchor = _adam(fmt, "vpt_adam_step_multi", pre, _adam_state(views, 5), 1.0)
    before = [b.clone() for b in _adam_state(views, 5)[0]]
    for a, b, c in zip(clipped, anchor, before):
        assert torch.equal(a, b) and not torch.equal(a, c)
    out1, _, _, _ = _raw_norm(fmt, views, gs, float(out[0]) * 2.0)
    assert float(out1[1]) == 1.0
    same = _adam(fmt, "vpt_adam_step_multi_clip", views, _adam_state(views, 5), gs, coef=out1[1:])
    plain = _adam(fmt, "vpt_adam_step_multi", views, _adam_state(views, 5), gs)
    for a, b, c in zip(same, plain, clipped):
        assert torch.equal(a, b) and not torch.equal(a, c)
    # ops.adam_step_multi_ issues exactly these launches
    if fmt == "bf16":
        bufs, p, m, v = _adam_state(views, 5)
        flag = torch.ones(1, dtype=torch.int32, device=DEV)
        per = torch.empty(len(views), device=DEV)
        no = torch.empty(4, device=DEV)
        ops.adam_step_multi_(p, views, m, v, HYPER[0], lr=1e-2, weight_decay=0.039428, grad_scale=gs, found_inf=flag, max_grad_norm=max_norm, norm_out=no, per_tensor_norms=per)
        torch.cuda.synchronize()
        assert torch.equal(no, out) and int(flag) == 0 and all(torch.equal(a, b) for a, b in zip(bufs, clipped))


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_gradient_sets_the_flag_and_the_step_is_left_out(fmt, bad):
    """(e) one inf / nan in a tail element: flag set, norm_out[2] == 1, coefficient 0, the clipped Adam launch leaves p, m, v bit-unchanged; a later
    clean call does not clear the flag."""
    _, views = _data()
    flat = _DATA["flat"].clone()
    mine = _carve(flat, _DATA["sizes"])
    mine[5][-1] = bad                                        # 1025 elements: the second block's only element, a partial group
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, per, _, _ = _raw_norm(fmt, mine, 1.0, 5.0, flag=flag)
    assert int(flag) == 1 and float(out[2]) == 1.0 and float(out[1]) == 0.0 and not bool(torch.isfinite(out[0]))
    assert not bool(torch.isfinite(per[5])) and bool(torch.isfinite(per[4])) and bool(torch.isfinite(per[6]))
    state = _adam_state(views, 7)
    before = [b.clone() for b in state[0]]
    after = _adam(fmt, "vpt_adam_step_multi_clip", mine, state, 1.0, flag=flag, coef=out[1:])
    assert all(torch.equal(a, b) for a, b in zip(after, before))
    out2, _, _, _ = _raw_norm(fmt, views, 1.0, 5.0, flag=flag)
    assert int(flag) == 1 and float(out2[2]) == 0.0 and float(out2[1]) > 0.0
    # a finite gradient whose square overflows fp32: the sum is not finite either
    big = torch.zeros(9, device=DEV)
    big[1:] = 3e38
    flag.zero_()
    out3, _, _, _ = _raw_norm(fmt, [big[1:]], 1.0, 5.0, flag=flag)
    assert int(flag) == 1 and float(out3[2]) == 1.0 and float(out3[1]) == 0.0


def test_ten_identical_calls_are_bit_equal():
    """(f)"""
    _, views = _data()
    runs = [ops.grad_norm(views, scale=1.0 / 3, max_norm=1.0, per_tensor=True) for _ in range(10)]
    torch.cuda.synchronize()
    assert all(torch.equal(o, runs[0][0]) and torch.equal(p, runs[0][1]) for o, p in runs[1:])


@pytest.mark.parametrize("blocks,tensors", [(127, 1), (1, 64), (3, 1), (242707, 129)])
def test_workspace_holds_an_odd_number_of_partials(blocks, tensors):
    """The workspace is [tensors] fp64 + [blocks] fp32: with an odd block count its byte size is no multiple of 8, and ops' buffer must still hold the
    last partial (the cases: 8 x tensors + 4 x (blocks - 1) a multiple of the allocator's 512 bytes, twice; the smallest odd count; the 2x policy's)."""
    nbytes = int(_native.load("bf16").vpt_grad_norm_workspace_bytes(tensors, blocks))
    assert nbytes == 8 * tensors + 4 * blocks and nbytes % 8 == 4
    ws = ops._grad_norm_workspace(tensors, blocks, DEV)
    assert ws.numel() * ws.element_size() >= nbytes and ws.data_ptr() % 8 == 0


def test_grad_norm_writes_nothing_outside_its_buffers():
    """One tensor of 127 blocks: 8 + 4 x 126 = 512 bytes, so the last partial is the first byte past a 512-byte allocation.  The caching allocator is led to
    place ops.grad_norm's buffers BETWEEN live sentinel tensors: 512-byte sentinels are laid out back to back, every other one is freed, and the freed
    512-byte holes are what the allocator's best fit hands out next; a store past a buffer's end lands in the sentinel behind it.  The norm must also
    be the twin's (the finish reads that partial back)."""
    rng = np.random.default_rng(3)
    host = rng.standard_normal(127 * 1024 - 5).astype(np.float32)
    g = torch.from_numpy(host).to(DEV)
    torch.cuda.synchronize()
    fence = [torch.full((128,), -7.0, dtype=torch.float32, device=DEV) for _ in range(256)]
    keep = fence[0::2]
    holes = sorted(t.data_ptr() for t in fence[1::2])
    del fence
    norm_out, per = ops.grad_norm([g], scale=1.0, max_norm=1.0, per_tensor=True)
    torch.cuda.synchronize()
    assert {norm_out.data_ptr(), per.data_ptr()} & set(holes), "the allocator did not reuse the holes between the sentinels: the layout this test relies on"
    assert all(bool((t == -7.0).all()) for t in keep)
    tw = R.restate_f32([host], 1.0, 1.0)
    assert torch.equal(norm_out.cpu(), torch.from_numpy(tw["out"])) and float(per[0]) == float(tw["per_tensor"][0])
