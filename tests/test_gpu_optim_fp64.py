"""The optimiser kernels of vpt_optim.hip on the GPU, both libraries, against the fp64 reference of tests/optim_ref.py with its derived bounds:
vpt_adam_step, vpt_adam_step_multi, vpt_adam_step_multi_clip and vpt_adam_step_groups (coupled, decoupled, with and without the clip coefficient) -- p', m'
AND v' of every element over three consecutive steps, each step's reference starting from the device's own previous outputs; everything outside the tensors
bit-unchanged; the mutated references far from the device's outputs; and vpt_grads_nonfinite_multi on its own.  The bf16 library goes through the ops.*
wrappers the trainers call, the fp16 library through the same C entry points by name.  The tests that prove groups == multi (tests/test_gpu_adam_groups.py)
and clip == multi on pre-multiplied gradients (tests/test_gpu_grad_norm.py) hang from this anchor.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import _native, ops  # noqa: E402
from vpt_amd._native import ptr  # noqa: E402
from tests import optim_ref as R  # noqa: E402

DEV = "cuda"
STEPS = 3
GUARD = -7.0                # what the gaps between the views and the words around the flat buffers hold
_RUNS = {}
cf = ctypes.c_float


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _offsets(sizes, layout, first=None):
    """Element offsets of the views in one flat buffer: 'odd' = every view starts at an odd element (no 8-byte alignment: tests/test_gpu_grad_norm.py's
    carving), 'aligned' = at a multiple of four (16 bytes), at least one guard word in front of each.  -> (offsets, total with 8 trailing guard words)."""
    offs, off = [], (first if first is not None else (1 if layout == "odd" else 4))
    for n in sizes:
        offs.append(off)
        off += n + 1
        if layout == "odd":
            off += 1 - off % 2
        else:
            off += -off % 4
    return offs, off + 8


def _upload(c, layout):
    """The case's four lists as views of four flat device buffers -> (host flats, device flats, views per quantity, mask of the elements inside tensors)."""
    sizes = [x.size for x in c.p]
    offs, total = _offsets(sizes, layout, c.offset)
    inside = np.zeros(total, bool)
    host, flats, views = {}, {}, {}
    for q in "pgmv":
        h = np.full(total, GUARD, np.float32)
        for x, o in zip(getattr(c, q), offs):
            h[o:o + x.size] = x
            inside[o:o + x.size] = True
        host[q] = h
        flats[q] = torch.tensor(h, device=DEV)
        views[q] = [flats[q][o:o + n] for o, n in zip(offs, sizes)]
    live = [v for v in views["p"] if v.numel()]
    assert all(v.data_ptr() % 8 == 4 for v in live) if layout == "odd" else all(v.data_ptr() % 16 == 0 for v in live)
    return host, flats, views, inside


def _launch(fmt, c, views, step, max_norm):
    """One step of the case's entry point -> the device's clip coefficient (None when unclipped)."""
    h, p, g, m, v = c.hyper, views["p"], views["g"], views["m"], views["v"]
    norm_out = torch.full((4,), float("nan"), dtype=torch.float32, device=DEV) if c.clip else None
    if c.entry == "single":
        if fmt == "bf16":
            ops.adam_step_(p[0], g[0], m[0], v[0], step, h.lr, h.beta1, h.beta2, h.eps, h.wd, h.grad_scale)
        else:
            _native.call("vpt_adam_step", ptr(p[0]), ptr(g[0]), ptr(m[0]), ptr(v[0]), ctypes.c_uint64(p[0].numel()), step, cf(h.lr), cf(h.beta1), cf(h.beta2),
                         cf(h.eps), cf(h.wd), cf(h.grad_scale), _stream(), fmt=fmt)
    elif fmt == "bf16" and c.entry == "multi":
        ops.adam_step_multi_(p, g, m, v, step, h.lr, h.beta1, h.beta2, h.eps, h.wd, h.grad_scale, max_grad_norm=max_norm, norm_out=norm_out)
    elif fmt == "bf16":
        ops.adam_step_groups_(p, g, m, v, step, [x[0] for x in c.lr_wd], [x[1] for x in c.lr_wd], h.beta1, h.beta2, h.eps, h.grad_scale, decoupled=c.decoupled,
                              max_grad_norm=max_norm, norm_out=norm_out)
    else:
        table, blk, _ = ops._adam_table(g, p, m, v)
        n_t = len(p)
        keep = [table]
        if c.clip:
            ws = torch.empty(int(_native.load(fmt).vpt_grad_norm_workspace_bytes(n_t, blk)) // 8 + 1, dtype=torch.float64, device=DEV)
            _native.call("vpt_grad_norm_multi", ptr(table), n_t, blk, cf(h.grad_scale), cf(max_norm), ptr(ws), ptr(norm_out), None, None, _stream(), fmt=fmt)
            keep.append(ws)
        coef = ptr(norm_out[1:]) if c.clip else None
        if c.entry == "multi":
            args = [ptr(table), n_t, blk, step, cf(h.lr), cf(h.beta1), cf(h.beta2), cf(h.eps), cf(h.wd), cf(h.grad_scale), None]
            _native.call("vpt_adam_step_multi_clip" if c.clip else "vpt_adam_step_multi", *(args + ([coef] if c.clip else [])), _stream(), fmt=fmt)
        else:
            rec = np.zeros(n_t, dtype=[("lr", "<f4"), ("wd", "<f4")])
            rec["lr"], rec["wd"] = [x[0] for x in c.lr_wd], [x[1] for x in c.lr_wd]
            groups = torch.from_numpy(rec.view(np.uint8)).to(DEV)
            keep.append(groups)
            _native.call("vpt_adam_step_groups", ptr(table), ptr(groups), n_t, blk, step, cf(h.beta1), cf(h.beta2), cf(h.eps), cf(h.grad_scale),
                         1 if c.decoupled else 0, None, coef, _stream(), fmt=fmt)
    torch.cuda.synchronize()
    if not c.clip:
        return None
    no = norm_out.cpu().numpy()
    assert 0.0 < no[1] < 1.0 and no[2] == 0.0, no
    return float(no[1])


def _run(fmt, name, layout, steps=STEPS):
    """The case's `steps` consecutive steps on the device -> per step (inputs p, m, v as lists of host arrays, outputs likewise, coefficient); the checks
    on everything outside the tensors are made here, after every step.  Cached: the mutation test reads the first step of runs the main test made."""
    key = (fmt, name, layout)
    if key in _RUNS and len(_RUNS[key]) >= steps:
        return _RUNS[key]
    c = R.case(name)
    host, flats, views, inside = _upload(c, layout)
    max_norm = R.clip_inputs(c)[0] if c.clip else None
    sizes = [x.size for x in c.p]
    offs, _ = _offsets(sizes, layout, c.offset)
    carve = lambda flat: [flat[o:o + n] for o, n in zip(offs, sizes)]
    out, before = [], {q: host[q] for q in "pmv"}
    for k in range(steps):
        coef = _launch(fmt, c, views, c.step + k, max_norm)
        after = {q: flats[q].cpu().numpy().copy() for q in "pmv"}
        for q in "pmv":        # the gaps between the views and the guard words around the buffer: bit-unchanged
            assert np.array_equal(after[q][~inside].view(np.int32), host[q][~inside].view(np.int32)), (name, fmt, layout, k, q)
        assert np.array_equal(flats["g"].cpu().numpy().view(np.int32), host["g"].view(np.int32)), (name, fmt, layout, k, "g")
        out.append(({q: carve(before[q]) for q in "pmv"}, {q: carve(after[q]) for q in "pmv"}, coef))
        before = after
    if c.entry != "single":      # (the mutations are designated on table cases; the large single case is not worth keeping)
        _RUNS[key] = out
    return out


def _check(fmt, name, layout, top):
    """Every step of one run against the reference of that step's own inputs; `top` collects max err / bound per quantity."""
    c = R.case(name)
    for k, (src, got, coef) in enumerate(_run(fmt, name, layout)):
        ref = R.reference(src["p"], c.g, src["m"], src["v"], c.step + k, c.hyper, coef=coef, decoupled=c.decoupled, lr_wd_per_tensor=c.lr_wd)
        assert R.regime_ok(ref, c.hyper), (name, k)
        for i, r in enumerate(ref):
            rs = R.ratios(got["p"][i], got["m"][i], got["v"][i], r)
            for j in range(3):
                top[j] = max(top[j], rs[j])
            assert max(rs) <= 1.0, (name, fmt, layout, k, i, rs)
        if "zero" in c.roles:      # m = v = g = 0: without decay m and v stay 0 and p keeps its bits; with it the decay alone moves p
            i = c.roles["zero"]
            wd = c.lr_wd[i][1] if c.lr_wd is not None else c.hyper.wd
            if wd == 0.0:
                assert not got["m"][i].any() and not got["v"][i].any()
                assert np.array_equal(got["p"][i].view(np.int32), c.p[i].view(np.int32)), (name, fmt, layout, k)
            else:
                assert not np.array_equal(got["p"][i], src["p"][i])


ENTRIES = ["vpt_adam_step", "vpt_adam_step_multi", "vpt_adam_step_multi_clip", "vpt_adam_step_groups[coupled]", "vpt_adam_step_groups[decoupled]",
           "vpt_adam_step_groups[coupled, clip]", "vpt_adam_step_groups[decoupled, clip]"]


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_point_inside_the_bounds_of_the_fp64_reference(entry, fmt):
    """Every case of the entry point (tests/optim_ref.py: cases()), the table launches in both layouts (views at odd elements, and 16-byte aligned)."""
    names = [c.name for c in R.cases() if R.entry_point(c) == entry]
    assert names
    top = [0.0, 0.0, 0.0]
    for name in names:
        c = R.case(name)
        for layout in (("odd", "aligned") if c.entry != "single" else (("odd",) if c.offset else ("aligned",))):
            _check(fmt, name, layout, top)
    print(f"[{fmt}] {entry}: {len(names)} cases, max err / bound  p' {top[0]:.3f}  m' {top[1]:.3f}  v' {top[2]:.3f}")


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_mutated_reference_misses_the_device(mut, fmt):
    """What the bounds can see: the reference with one of the listed mistakes built in lies outside the bound of the device's outputs on the tensor
    designated for it (tests/test_optim_ref_cpu.py shows the same inputs put the mutated emulation at least 10 bounds away)."""
    name, role = R.DESIGNATED[mut]
    c = R.case(name)
    i = c.roles[role]
    src, got, coef = _run(fmt, name, "odd", steps=1)[0]
    kw = dict(coef=coef, decoupled=c.decoupled, lr_wd_per_tensor=c.lr_wd)
    ref = R.reference(src["p"], c.g, src["m"], src["v"], c.step, c.hyper, **kw)[i]
    bad = R.reference(src["p"], c.g, src["m"], src["v"], c.step, c.hyper, mutate=mut, **kw)[i]
    bad.b_p, bad.b_m, bad.b_v = ref.b_p, ref.b_m, ref.b_v
    rs = R.ratios(got["p"][i], got["m"][i], got["v"][i], bad)
    print(f"[{fmt}] mutation {mut} on {name} [{role}]: device vs mutated reference, err / bound  p' {rs[0]:.3e}  m' {rs[1]:.3e}  v' {rs[2]:.3e}")
    assert max(R.ratios(got["p"][i], got["m"][i], got["v"][i], ref)) <= 1.0
    assert max(rs) > 1.0


def test_zero_length_single_tensor_is_left_alone():
    """n = 0: no launch, nothing written (vpt_adam_launch returns before the grid is formed)."""
    flat = torch.full((4, 8), GUARD, device=DEV)
    for fmt in ("bf16", "fp16"):
        _native.call("vpt_adam_step", ptr(flat[0][4:]), ptr(flat[1][4:]), ptr(flat[2][4:]), ptr(flat[3][4:]), ctypes.c_uint64(0), 1, cf(1e-2), cf(0.9), cf(0.999),
                     cf(1e-8), cf(0.1), cf(1.0), _stream(), fmt=fmt)
    empty = [flat[k][4:4] for k in range(4)]
    ops.adam_step_(*empty, 1, 1e-2, weight_decay=0.1)
    torch.cuda.synchronize()
    assert bool((flat == GUARD).all())


# ---- vpt_grads_nonfinite_multi on its own ---------------------------------------------------------------------------------------------------------------------
def _nonfinite(fmt, grads, flag):
    table, blk, _ = ops._adam_table(grads)
    _native.call("vpt_grads_nonfinite_multi", ptr(table), len(grads), blk, ptr(flag), _stream(), fmt=fmt)
    torch.cuda.synchronize()
    return int(flag)


def _gradient_views():
    c = R.case("multi/A/s0/t1")
    sizes = [x.size for x in c.g]
    offs, total = _offsets(sizes, "odd")
    h = np.full(total, GUARD, np.float32)
    for x, o in zip(c.g, offs):
        h[o:o + x.size] = x
    return sizes, offs, h


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_grads_nonfinite_finds_one_planted_value_anywhere(fmt):
    """One +inf, -inf or NaN per launch in the table list of the Adam cases (views at odd elements, the two zero-length tensors in it): the flag reads 1 and
    the gradients keep their bits.  The places: the first element of the first tensor; the four positions of a full group; every position of a 1-, 2- and
    3-element tail; an element only the last wave of a block owns (threads 192..255 hold elements 768..1023); the last element of the last non-empty
    tensor; a 1-element tensor among the 300."""
    sizes, offs, h = _gradient_views()
    idx = {n: sizes.index(n) for n in (2, 5, 1023, 1024, 1025)}
    last = max(i for i, n in enumerate(sizes) if n)
    one = next(i for i in range(len(R.TABLE_SIZES), len(sizes)) if sizes[i] == 1)
    places = [(0, 0)] + [(idx[1024], 512 + k) for k in range(4)] + [(idx[1025], 1024), (idx[5], 4), (idx[2], 0), (idx[2], 1)] + \
             [(idx[1023], 1020 + k) for k in range(3)] + [(idx[1024], 1001), (last, sizes[last] - 1), (one, 0)]
    flat = torch.from_numpy(h).to(DEV)
    views = [flat[o:o + n] for o, n in zip(offs, sizes)]
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert _nonfinite(fmt, views, flag) == 0
    for t, j in places:
        for bad in (float("inf"), float("-inf"), float("nan")):
            mine = h.copy()
            mine[offs[t] + j] = bad
            flat.copy_(torch.from_numpy(mine))
            flag.zero_()
            assert _nonfinite(fmt, views, flag) == 1, (t, j, bad)
            assert np.array_equal(flat.cpu().numpy().view(np.int32), mine.view(np.int32))
            if fmt == "bf16":      # the wrapper the fp16 trainers call when clipping is off (it drops the zero-length tensors)
                assert int(ops.grads_nonfinite(views)) == 1, (t, j, bad)
    flat.copy_(torch.from_numpy(h))
    assert int(ops.grads_nonfinite(views)) == 0


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_grads_nonfinite_passes_the_largest_and_smallest_finite_values_and_only_sets(fmt):
    """FLT_MAX, -FLT_MAX, the smallest subnormal and -0.0 in every element (x - x is 0 for each): the flag stays 0.  A flag that is already 1 stays 1 on
    clean input (the kernel only ever sets).  The gradients and the guard words keep their bits."""
    sizes, offs, h = _gradient_views()
    fmax = np.finfo(np.float32).max
    vals = np.array([fmax, -fmax, np.float32(2.0 ** -149), -0.0], np.float32)
    for shift in range(4):
        mine = h.copy()
        for o, n in zip(offs, sizes):
            mine[o:o + n] = vals[(np.arange(n) + shift) % 4]
        flat = torch.from_numpy(mine).to(DEV)
        views = [flat[o:o + n] for o, n in zip(offs, sizes)]
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        assert _nonfinite(fmt, views, flag) == 0, shift
        assert np.array_equal(flat.cpu().numpy().view(np.int32), mine.view(np.int32))
    flag.fill_(1)
    assert _nonfinite(fmt, views, flag) == 1
    flag.fill_(5)
    assert _nonfinite(fmt, views, flag) == 5
