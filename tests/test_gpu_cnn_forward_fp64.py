"""The parts of the CNN forward that only tests/test_gpu_kernels.py judged -- vpt_conv3x3_small_kernel (the latency tiling), the frame statistics of every conv3x3
forward mode, vpt_pool_kernel<ARGMAX>, vpt_channel_stats_kernel and vpt_nfold_coef_kernel -- held per element / per sum to the fp64 references and derived bounds of
tests/cnn_forward_ref.py (its docstring has the derivations and the counted chain lengths; tests/test_cnn_forward_ref_cpu.py pins them on the CPU).  Both operand
formats.  Every call runs twice and the two results are compared on bits (the statistics are fp64 atomic sums of a frame's few fp32 partial sums: exact, so they do
not depend on the order the workgroups finish in -- tests/test_gpu_conv_fwd_bitwise.py).  Needs an MI355X.  Measured ratios: profiles/cnn_forward_fp64_ratios.md."""
import contextlib
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import _native, ops, packing  # noqa: E402
from tests import cnn_forward_ref as R  # noqa: E402

DEV = "cuda"
D = torch.float64


def _bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _blocked(x, fmt):
    return packing.nchw_to_blocked(x.float(), dtype=R.DT[fmt]).to(DEV)


def _twice(fn, what):
    """fn() -> tuple of tensors (None allowed); run twice, every output equal bit for bit -> the first result."""
    a = fn()
    b = fn()
    torch.cuda.synchronize()
    for i, (u, v) in enumerate(zip(a, b)):
        assert u is None or torch.equal(_bits(u), _bits(v)), f"{what}: output {i} differs between two identical calls"
    return a


def _check_sums(got, want, allowed, what):
    worst, msg = R.stats_failure(got, want, allowed, what)
    print(f"{what}: worst err / bound {worst:.4f}")
    assert msg is None, msg


@contextlib.contextmanager
def _halo_dma(fmt, on):
    """As tests/test_gpu_conv_halo_dma.py: -1 = the shipped selection, 0 = the register-staged path everywhere; always restored."""
    lib = _native.load(fmt)
    lib.vpt_conv3x3_set_halo_dma.argtypes, lib.vpt_conv3x3_set_halo_dma.restype = [ctypes.c_int], ctypes.c_int
    lib.vpt_conv3x3_set_halo_dma(-1 if on else 0)
    try:
        yield
    finally:
        lib.vpt_conv3x3_set_halo_dma(-1)


# ---- conv3x3, latency tiling ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_stats", [False, True])
@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("name", list(R.LATENCY_CASES))
def test_conv3x3_latency_fp64(name, fmt, use_res, with_stats):
    c = R.latency_case(name, fmt)
    what = f"conv3x3 latency {name} {fmt} res={use_res} stats={with_stats}"
    xb, resb = _blocked(c["x"], fmt), _blocked(c["res"], fmt) if use_res else None
    wpk, sa, sg, st_in = c["wpk"].to(DEV), c["sa"].to(DEV), c["sg"].to(DEV), c["stats_in"].to(DEV)

    def run():
        st = torch.zeros(c["frames"], 2, dtype=D, device=DEV) if with_stats else None
        return ops.conv3x3(xb, wpk, sa, sg, st_in, c["cout"], res=resb, stats_out=st, tiling="latency"), st
    y, st = _twice(run, what)
    y = packing.blocked_to_nchw(y.cpu(), c["cout"], c["h"], c["w"]).double()
    worst, msg = R.failure(y, c["y64"][use_res], c["bound"][use_res], what)
    print(f"{what}: worst err / bound {worst:.4f}")
    assert msg is None, msg
    if with_stats:
        _check_sums(st, *R.latency_stats_ref(c, use_res), f"{what} stats_out")


# ---- statistics of the throughput kernel's modes -------------------------------------------------------------------------------------------------------
def _throughput_runs(c, fmt):
    """-> [(tag, n_add, fn)]: fn() -> (stored tensor whose fp64 sums are the reference, stats_out): every mode and tiling the case takes."""
    frames, cout, h, w = c["frames"], c["cout"], c["h"], c["w"]
    dev = lambda t: t.to(DEV)
    xb, resb = _blocked(c["x"], fmt), _blocked(c["res"], fmt)
    wpk, sa, sg, st_in = dev(c["wpk"]), dev(c["sa"]), dev(c["sg"]), dev(c["stats_in"])
    kk, rs, rsc, rb, og = dev(c["kk"]), dev(c["rs"]), dev(c["rsc"]), dev(c["rb"]), dev(c["out_gain"])
    stats = lambda: torch.zeros(frames, 2, dtype=D, device=DEV)

    def conv(res, tiling):
        def fn():
            st = stats()
            return ops.conv3x3(xb, wpk, sa, sg, st_in, cout, res=res, stats_out=st, tiling=tiling), st
        return fn

    def folded(res):
        def fn():
            st = stats()
            return ops.conv3x3_folded(xb, wpk, sa, sg, st_in, cout, kk_frame=kk, rs_frame=rs, res=resb if res else None, res_scale=rsc if res else None,
                                      res_bias=rb if res else None, stats_out=st), st
        return fn

    def pool(gain):
        def fn():
            st = stats()
            y = ops.conv3x3_pool(xb, wpk, sa, sg, st_in, cout, stats_out=st, out_gain=og if gain else None)
            return (ops.conv3x3_pool(xb, wpk, sa, sg, st_in, cout) if gain else y), st      # with the gain: the statistics stay those of the ungained tensor
        return fn

    def pool_argmax():
        st = stats()
        return ops.conv3x3_pool_argmax(xb, wpk, sa, sg, st_in, cout, stats_out=st)[0], st
    runs = [("mode0", R.N_ADD_FWD16, conv(None, "throughput")), ("mode1", R.N_ADD_FWD16, conv(resb, "throughput")),
            ("mode0 folded", R.N_ADD_FWD16, folded(False)), ("mode5", R.N_ADD_FWD16, folded(True)),
            ("mode4", R.n_add_pool_fused(h, w), pool(False)), ("mode4 out_gain", R.n_add_pool_fused(h, w), pool(True)),
            ("mode7", R.n_add_pool_fused(h, w), pool_argmax)]
    if h % 32 == 0:
        runs += [("mode0 rows32", R.N_ADD_FWD32, conv(None, "throughput32")), ("mode1 rows32", R.N_ADD_FWD32, conv(resb, "throughput32"))]
    return runs


def test_throughput_cases_are_those_of_the_existing_files():
    from tests.test_gpu_conv_fwd_bitwise import CASES      # = the CASES of tests/test_gpu_conv_mfma16.py + pool32
    assert R.THROUGHPUT_CASES == dict(CASES)


@pytest.mark.parametrize("halo", [True, False])
@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("name", list(R.THROUGHPUT_CASES))
def test_conv3x3_throughput_stats_fp64(name, fmt, halo):
    """stats_out of modes 0, 1, 5, 4, 7 and of the 32-row tiles against the fp64 sums of the tensor each launch stored, with the halo-DMA selection on and off."""
    c = R.throughput_case(name, fmt)
    with _halo_dma(fmt, halo):
        for tag, n_add, fn in _throughput_runs(c, fmt):
            what = f"conv3x3 stats {name} {fmt} halo_dma={halo} {tag}"
            y, st = _twice(fn, what)
            _check_sums(st, *R.stored_stats_ref(y.cpu(), n_add), what)


# ---- max pool ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_argmax", [False, True])
@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("name", list(R.POOL_CASES))
def test_maxpool_exact(name, fmt, want_argmax):
    c = R.pool_case(name, fmt)
    what = f"maxpool {name} {fmt} argmax={want_argmax}"
    xb = _blocked(c["x"], fmt)

    def run():
        st = torch.zeros(c["f"], 2, dtype=D, device=DEV)
        out = ops.maxpool(xb, stats_out=st, want_argmax=want_argmax)
        return (out[0], out[1], st) if want_argmax else (out, None, st)
    y, am, st = _twice(run, what)
    ph, pw = c["h"] // 2, c["w"] // 2
    want = packing.nchw_to_blocked(c["pooled"].float(), dtype=R.DT[fmt])
    neq = _bits(y.cpu()) != _bits(want)
    print(f"{what}: {int(neq.sum())} of {neq.numel()} pooled values differ")
    assert not bool(neq.any()), f"{what}: {int(neq.sum())} of {neq.numel()} pooled values differ; first at {neq.nonzero()[0].tolist()}"
    if want_argmax:      # every element: 15 where the window's maximum is 0, nothing is skipped
        got = packing.blocked_to_nchw(am.cpu(), c["c"], ph, pw).to(torch.uint8)
        bad = got != c["argmax"]
        print(f"{what}: {int(bad.sum())} of {bad.numel()} arg-max bytes differ")
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} arg-max bytes differ; first at {bad.nonzero()[0].tolist()}: got {got[bad][0].item()}, want {c['argmax'][bad][0].item()}"
    _check_sums(st, c["sums"], c["allowed"], f"{what} stats_out")


# ---- channel_stats -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("name", list(R.CHANNEL_STATS_CASES))
def test_channel_stats_fp64(name, fmt):
    c = R.channel_stats_case(name, fmt)
    what = f"channel_stats {name} {fmt}"
    qb = _blocked(c["q"], fmt)
    chs, = _twice(lambda: (ops.channel_stats(qb),), what)
    _check_sums(chs, c["sums"], c["allowed"], what)


# ---- nfold_coef ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("name", list(R.NFOLD_CASES))
def test_nfold_coef_fp64(name, fmt):
    c = R.nfold_case(name, fmt)
    what = f"nfold_coef {name} {fmt}"
    dev = lambda t: t.to(DEV)
    args = [dev(c[k]) for k in ("tot", "chs", "gain", "bias", "sa", "sg", "tb", "tg")]
    kk, rs, rsc, rb = _twice(lambda: ops.nfold_coef(*args, c["hw"], c["c"]), what)
    for got, key in ((kk, "kk"), (rs, "rs"), (rsc, "res_scale"), (rb, "res_bias")):
        worst, msg = R.failure(got.cpu().double(), c[key], c["b_" + key], f"{what} {key}")
        print(f"{what} {key}: worst err / bound {worst:.4f}")
        assert msg is None, msg
