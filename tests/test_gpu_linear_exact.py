"""The linear-layer kernels -- vpt_gemm_kernel (ten compile-time epilogues + the generic one), vpt_gemm256_kernel, vpt_gemm_tn_kernel,
vpt_splitk_epilogue_kernel, vpt_dense_fold_epilogue_kernel, vpt_gemv_kernel<MR, ROWS, LN> -- held to the two instruments of tests/linear_ref.py:
THE integer result on integer operands (fp32 output bit-equal, 16-bit output its one RNE rounding), and an fp64 reference under a derived
per-element bound on real-valued operands at K <= 256.  Needs an MI355X.  Both operand formats.

Shapes are the smallest that reach each path: 1, 2, 3 and 4 k-steps of the MFMA main loop ("loop never runs", "loop once"), M = 1 and M = 257
(every staged row of a tile clamps to row M - 1 - m0), N that is no multiple of 4 (generic epilogue), a split-K whose last run is empty or
short, every ROWS of the weight-streaming kernel through the launch rule (never forced), its second round of prefetched loads, odd N, the fused
LayerNorm prologue at every row count class, and the TN kernel below one tile in every dimension."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import _native, ops  # noqa: E402
from vpt_amd._native import ptr  # noqa: E402
from vpt_amd.training import linear_backward  # noqa: E402
from tests import linear_ref as R  # noqa: E402

DEV = "cuda"
D = torch.float64
FMTS = ["bf16", "fp16"]

#        bias   relu   res    mask   f32    16-bit      (the rows of test_linear_epilogue_variants)
ROWS10 = [(True, False, False, False, True, False),     # qkvr / heads
          (True, False, True, False, True, False),      # proj / mlp1
          (False, True, False, False, False, True),     # mlp0
          (False, True, False, False, True, False),     # img linear / lastlayer (inference)
          (False, True, False, False, True, True),      # ... (training forward keeps both)
          (False, False, False, False, True, False),    # dgrad -> fp32
          (False, False, False, False, False, True),    # dense dgrad -> 16-bit
          (False, False, True, False, True, False),     # dgrad + skip
          (False, False, False, True, False, True),     # dgrad through a ReLU gate -> 16-bit
          (True, True, True, True, True, True)]         # all on: no dedicated instantiation, the generic epilogue
BIAS_F32, RELU_16 = ROWS10[0], ROWS10[2]


def _pack(w16):
    """[N, K] 16-bit (K % 32 == 0) -> the packed image [ceil(N/128)][K/32][128][32] on the device, in plain torch (not the library's packer)."""
    n, k = w16.shape
    nt = (n + 127) // 128
    wp = torch.zeros(nt * 128, k, dtype=w16.dtype)
    wp[:n] = w16
    return wp.view(nt, 128, k // 32, 32).permute(0, 2, 1, 3).contiguous().to(DEV)


@functools.lru_cache(maxsize=None)
def _case(kind, fmt, m, n, k):
    """Operands on both sides + the fp64 product, computed once per (kind, format, shape) and never modified."""
    g = torch.Generator().manual_seed(m + 3 * n + 7 * k + (0 if kind == "int" else 1))
    dt = R.DT[fmt]
    if kind == "int":
        a, w = R.ints(g, m, k).to(dt), R.ints(g, n, k).to(dt)
        bias, res, mask = R.ints(g, n), R.ints(g, m, n), R.ints(g, m, n).to(dt)
    else:
        a, w = R.reals(g, fmt, m, k), R.reals(g, fmt, n, k, scale=k ** -0.5)
        bias, res, mask = torch.randn(n, generator=g), torch.randn(m, n, generator=g), R.reals(g, fmt, m, n)
    a64, w64 = a.to(D), w.to(D)
    c = dict(m=m, n=n, k=k, fmt=fmt, dt=dt, a=a, w=w, bias=bias, res=res, mask=mask, pre=a64 @ w64.t(), mag=a64.abs() @ w64.abs().t(),
             A=a.to(DEV), wpk=_pack(w), bias_d=bias.to(DEV), res_d=res.to(DEV), mask_d=mask.to(DEV))
    return c


def _ref(c, bias, relu, res, mask, pre=None):
    """(y64, mag) of one epilogue row from the cached product (linear_ref's stages in linear_ref's order)."""
    y = c["pre"] if pre is None else pre
    mag = c["mag"]
    if bias:
        y, mag = y + c["bias"].to(D), mag + c["bias"].to(D).abs()
    if relu:
        y = torch.relu(y)
    if mask:
        y = torch.where(c["mask"].to(D) > 0, y, torch.zeros_like(y))
    if res:
        y, mag = y + c["res"].to(D), mag + c["res"].to(D).abs()
    return y, mag


def _linear(c, row, **kw):
    bias, relu, res, mask, f32, b16 = row
    o32, o16 = ops.linear(c["A"], c["wpk"], c["n"], bias=c["bias_d"] if bias else None, res=c["res_d"] if res else None, relu=relu,
                          mask=c["mask_d"] if mask else None, out_f32=f32, out_bf16=b16, **kw)
    torch.cuda.synchronize()
    return (o32.cpu() if o32 is not None else None), (o16.cpu() if o16 is not None else None)


def _check_int(c, row, o32, o16, what, fails):
    y = _ref(c, *row[:4])[0]
    assert (o32 is not None) == row[4] and (o16 is not None) == row[5]
    for o in (o32, o16):
        if o is not None:
            msg = R.exact_failure(o, y, f"{what} (M, N, K) = {(c['m'], c['n'], c['k'])} {c['fmt']} row {row}")
            if msg:
                fails.append(msg)


def test_the_first_row_check_is_the_reference():
    """_ref (from the cached product) is linear_ref."""
    c = _case("real", "bf16", 3, 5, 64)
    for row in ROWS10:
        y, mag = R.linear_ref(c["a"], c["w"], c["bias"] if row[0] else None, row[1], c["mask"] if row[3] else None, c["res"] if row[2] else None)
        y2, mag2 = _ref(c, *row[:4])
        assert torch.equal(y, y2) and torch.equal(mag, mag2)


# ---- vpt_gemm_kernel ------------------------------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(1, 4, 64), (129, 68, 128), (257, 132, 192), (256, 128, 64), (255, 124, 256),        # vector epilogues: 1 / 2 / 3 / 1 / 4 k-steps
               (3, 5, 64), (257, 131, 192)]                                                        # N % 4 != 0: the generic epilogue


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
def test_gemm_integer(m, n, k, fmt):
    c = _case("int", fmt, m, n, k)
    fails = []
    for row in ROWS10:
        o32, o16 = _linear(c, row, tiling="throughput")
        _check_int(c, row, o32, o16, "vpt_gemm_kernel", fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("m,n,k", [(257, 132, 192), (257, 131, 192)])
def test_gemm_padded_16bit_output(m, n, k, fmt):
    """out_bf16_ld = 64 * ceil(n / 64): the result in columns < n, exact zeros in the padding (it is the next GEMM's K padding)."""
    c = _case("int", fmt, m, n, k)
    ld = 64 * ((n + 63) // 64)
    for row in (RELU_16, ROWS10[9]):
        o32, o16 = _linear(c, row, tiling="throughput", out_bf16_ld=ld)
        assert tuple(o16.shape) == (m, ld)
        y = _ref(c, *row[:4])[0]
        msg = R.exact_failure(o16[:, :n].contiguous(), y, f"padded 16-bit output {(m, n, k)} {fmt} row {row}")
        assert msg is None, msg
        assert not bool(o16[:, n:].view(torch.int16).any()), "padding columns are not exactly zero"


RATIOS = {}


def _note(kernel, fmt, kind, ratio):
    key = (kernel, fmt, kind)
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)


def _check_real(c, row, o32, o16, kernel, fails, k=None, s=1):
    y, mag = _ref(c, *row[:4])
    k = c["k"] if k is None else k
    if o32 is not None:
        worst, msg = R.bound_ratio(o32, y, R.bound(mag, k, s))
        _note(kernel, c["fmt"], "fp32", worst)
        print(f"{kernel} {(c['m'], c['n'], c['k'])} {c['fmt']} row {row} fp32 out: worst err / bound = {worst:.4f}")
        if msg:
            fails.append(f"{kernel} {(c['m'], c['n'], c['k'])} {c['fmt']} row {row}: {msg}")
    if o16 is not None:
        worst, msg = R.bound_ratio(o16, y, R.bound16(y, mag, k, c["fmt"], s))
        _note(kernel, c["fmt"], "16-bit", worst)
        print(f"{kernel} {(c['m'], c['n'], c['k'])} {c['fmt']} row {row} 16-bit out: worst err / bound = {worst:.4f}")
        if msg:
            fails.append(f"{kernel} {(c['m'], c['n'], c['k'])} {c['fmt']} row {row}: {msg}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("m,n,k", [(257, 132, 192), (257, 131, 192)])
def test_gemm_real(m, n, k, fmt):
    c = _case("real", fmt, m, n, k)
    fails = []
    for row in ROWS10:
        o32, o16 = _linear(c, row, tiling="throughput")
        _check_real(c, row, o32, o16, "vpt_gemm_kernel", fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("kernel,tiling,m,n,k", [("vpt_gemm_kernel", "throughput", 129, 68, 128), ("vpt_gemv_kernel", "latency", 2, 7, 192)])
def test_fp16_subnormal_operands_are_kept(kernel, tiling, m, n, k):
    """A in fp16's subnormal range (nonzero multiples of 2^-24 below 2^-14), W scaled by 2^10 so that every result is a normal fp32: an MFMA or a packed
    dot product that flushed its fp16 input subnormals would return zeros here -- and lose the small gradients of the loss-scaled fp16 backward."""
    g = torch.Generator().manual_seed(77)
    a = (torch.randint(1, 1024, (m, k), generator=g) * (torch.randint(0, 2, (m, k), generator=g) * 2 - 1)).double() * 2.0 ** -24
    a16 = a.to(torch.float16)
    assert torch.equal(a16.double(), a) and float(a.abs().max()) < 2.0 ** -14
    w16 = (torch.randn(n, k, generator=g) * 1024).to(torch.float16)
    y, mag = R.linear_ref(a16, w16)
    assert float(y.abs().median()) > 2.0 ** -100
    o32, _ = ops.linear(a16.to(DEV), _pack(w16), n, out_f32=True, out_bf16=False, tiling=tiling)
    torch.cuda.synchronize()
    worst, msg = R.bound_ratio(o32.cpu(), y, R.bound(mag, k))
    print(f"{kernel} fp16 subnormal A {(m, n, k)}: worst err / bound = {worst:.4f}; |out| / |y64| = {float(o32.cpu().double().norm() / y.norm()):.6f}")
    _note(kernel, "fp16", "subnormal A", worst)
    assert msg is None, msg


# ---- many tiles: xcd_remap, interior tiles, the double buffer of vpt_gemm256_kernel -----------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("k", [64, 128, 192])
def test_many_tiles_integer_both_tilings(k, fmt):
    m, n = 4097, 3076                      # 17 x 25 tiles of 256 x 128; 17 x 13 = 221 >= 192 tiles of 256 x 256 with an odd number of 128-column halves
    c = _case("int", fmt, m, n, k)
    fails = []
    for row in (BIAS_F32, RELU_16):
        outs = {}
        for tiling in ("throughput", "throughput256"):
            o32, o16 = _linear(c, row, tiling=tiling)
            _check_int(c, row, o32, o16, f"tiling={tiling}", fails)
            outs[tiling] = o32 if o32 is not None else o16
        it = torch.int32 if outs["throughput"].dtype == torch.float32 else torch.int16
        if not torch.equal(outs["throughput"].view(it), outs["throughput256"].view(it)):
            fails.append(f"row {row}: the two tilings differ")
    assert not fails, "\n".join(fails)


# ---- explicit split-K -----------------------------------------------------------------------------------------------------------------------------------------
def _runs(k, s, unit):
    """The K ranges of the S slices: ceil(steps / S) steps of `unit` each (64: vpt_gemm_kernel, 32: vpt_gemv_kernel), the last ones short or empty."""
    steps = k // unit
    per = (steps + s - 1) // s
    return [(min(i * per, steps) * unit, min((i + 1) * per, steps) * unit) for i in range(s)]


def _check_split(c, s, bias, tiling, unit, empty, fails):
    """Raw slices: slice i = the exact product over its own K run (+ bias in slice 0 only), an empty run = exact zeros; summed: the exact layer."""
    m, n, k = c["m"], c["n"], c["k"]
    what = f"split-K (M, N, K, S) = {(m, n, k, s)} {c['fmt']} tiling={tiling} bias={bias}"
    runs = _runs(k, s, unit)
    assert [i for i, (b, e) in enumerate(runs) if b == e] == empty, runs
    a64, w64 = c["a"].to(D), c["w"].to(D)
    for raw in (True, False):
        poison = torch.full((s, m, n), float("nan"), device=DEV)       # a slice nobody writes must come from torch.zeros, not from this block
        del poison
        o32, _ = ops.linear(c["A"], c["wpk"], n, bias=c["bias_d"] if bias else None, out_f32=True, out_bf16=False, splitk=s, splitk_raw=raw, tiling=tiling)
        torch.cuda.synchronize()
        o32 = o32.cpu()
        if raw:
            assert tuple(o32.shape) == (s, m, n)
            for i, (b, e) in enumerate(runs):
                want = a64[:, b:e] @ w64[:, b:e].t() + (c["bias"].to(D) if bias and i == 0 else 0)
                msg = R.exact_failure(o32[i], want, f"{what} slice {i} (k {b}..{e})")
                if msg:
                    fails.append(msg)
        else:
            msg = R.exact_failure(o32, _ref(c, bias, False, False, False)[0], f"{what} summed")
            if msg:
                fails.append(msg)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("m,n,k,s,bias,empty", [(40, 132, 320, 4, False, [3]),       # 5 steps in runs of 2, 2, 1 and none
                                                (40, 132, 512, 4, False, []),
                                                (257, 131, 320, 2, True, []),        # generic epilogue: runs of 3 and 2
                                                (40, 132, 320, 4, True, [3])])       # vector epilogue with a bias
def test_gemm_explicit_splitk(m, n, k, s, bias, empty, fmt):
    c = _case("int", fmt, m, n, k)
    fails = []
    _check_split(c, s, bias, "throughput", 64, empty, fails)
    assert not fails, "\n".join(fails)


# ---- automatic / named split finished by vpt_splitk_epilogue_kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("m,n,k,kw", [(9, 132, 2048, dict(tiling="auto")), (512, 260, 2112, dict(tiling="auto")), (40, 132, 2048, dict(tiling="throughput", splitk="nk"))])
def test_split_with_epilogue_kernel_integer(m, n, k, kw, fmt):
    """8 < M <= 512, K >= 2048 and few tiles under "auto", or splitk="nk": four K slices (33 steps in runs of 9, 9, 9, 6 at K = 2112) summed by the
    epilogue kernel with bias, ReLU, gate, residual and both outputs."""
    tiles = ((m + 255) // 256) * ((n + 127) // 128)
    assert (ops.nk_splitk(n, k) if kw.get("splitk") == "nk" else min(16, k // 512, 256 // tiles)) == 4 and tiles < 128
    c = _case("int", fmt, m, n, k)
    fails = []
    for row in (ROWS10[9], ROWS10[1], RELU_16):
        o32, o16 = _linear(c, row, **kw)
        _check_int(c, row, o32, o16, f"split + epilogue kernel {kw}", fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("fmt", FMTS)
def test_splitk_epilogue_kernel_real(fmt):
    """vpt_linear_splitk_epilogue called directly on the four raw slices of a K = 256 product: S = 4 in the bound."""
    m, n, k, s = 40, 132, 256, 4
    c = _case("real", fmt, m, n, k)
    part, _ = ops.linear(c["A"], c["wpk"], n, out_f32=True, out_bf16=False, splitk=s, splitk_raw=True, tiling="throughput")
    fails = []
    for row in (ROWS10[9], ROWS10[1], RELU_16):
        bias, relu, res, mask, f32, b16 = row
        o32 = torch.empty(m, n, device=DEV) if f32 else None
        o16 = torch.empty(m, n, dtype=c["dt"], device=DEV) if b16 else None
        _native.call("vpt_linear_splitk_epilogue", ptr(part), s, ptr(c["bias_d"] if bias else None), ptr(c["res_d"] if res else None), ptr(o32), ptr(o16),
                     m, n, n, n, n, 1 if relu else 0, ptr(c["mask_d"] if mask else None), n if mask else 0, ops._stream(), fmt=fmt)
        torch.cuda.synchronize()
        _check_real(c, row, o32.cpu() if f32 else None, o16.cpu() if b16 else None, "vpt_splitk_epilogue_kernel", fails, s=s)
    assert not fails, "\n".join(fails)


def test_dense_fold_epilogue_fp64():
    """ops.dense_fold_epilogue against fp64 from the same partial slices and frame statistics, under the bound derived in linear_ref.py; frame 1 has
    |mean| * rstd ~ 1000 (the -rstd * mean * sg term dominates its outputs)."""
    g = torch.Generator().manual_seed(9)
    s, m, n, count = 5, 7, 260, 4096
    x = torch.randn(m, count, generator=g, dtype=D)
    x[1] = 50.0 + 0.05 * x[1]
    stats = torch.stack([x.sum(1), (x * x).sum(1)], 1).contiguous()
    part = torch.randn(s, m, n, generator=g) * 8
    sg, sb = torch.randn(n, generator=g) * 4, torch.randn(n, generator=g)
    out64, bnd = R.dense_fold_ref(part, stats, count, sg, sb)
    mean, var = stats[1, 0] / count, stats[1, 1] / count - (stats[1, 0] / count) ** 2
    assert float(mean.abs() / torch.sqrt(var + R.EPS)) > 500
    out = ops.dense_fold_epilogue(part.to(DEV), stats.to(DEV), count, sg.to(DEV), sb.to(DEV))
    torch.cuda.synchronize()
    worst, msg = R.bound_ratio(out.cpu(), out64, bnd)
    print(f"vpt_dense_fold_epilogue_kernel {(s, m, n)}: worst err / bound = {worst:.4f}")
    _note("vpt_dense_fold_epilogue_kernel", "-", "fp32", worst)
    assert msg is None, msg


# ---- vpt_gemv_kernel ------------------------------------------------------------------------------------------------------------------------------------------
def _gemv_rows(n, s=1):
    """vpt_gemv_launch's rule: the fewest output columns per workgroup with N * S <= 1280 * ROWS, at most 16."""
    rows = 2
    while rows < 16 and n * s > 1280 * rows:
        rows *= 2
    return rows


#              M  N      K     ROWS
GEMV_SHAPES = [(1, 6, 32, 2),               # one k block: one lane group of one wave works
               (2, 7, 1056, 2),             # odd N: the last workgroup has one valid column
               (1, 6, 8224, 2),             # 257 k blocks: the second round of 8 prefetched loads holds one block
               (3, 2564, 4128, 4),          # 129 blocks = one round of 128 + 1
               (5, 5124, 2080, 8),          # 65 = 64 + 1
               (8, 10244, 1056, 16)]        # 33 = 32 + 1; N * S > 10240: the only way to ROWS = 16


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("tiling", ["latency", "auto"])
@pytest.mark.parametrize("m,n,k,rows", GEMV_SHAPES)
def test_gemv_integer(m, n, k, rows, tiling, fmt):
    assert _gemv_rows(n) == rows and m <= 8
    c = _case("int", fmt, m, n, k)
    fails = []
    for row in ROWS10:
        o32, o16 = _linear(c, row, tiling=tiling)
        _check_int(c, row, o32, o16, f"vpt_gemv_kernel ROWS={rows} tiling={tiling}", fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("m,n,k,s,rows,empty", [(2, 6, 96, 4, 2, [3]),               # 3 k blocks in 4 runs: the last is empty
                                                (4, 130, 8192, 7, 2, []),            # 256 blocks in runs of 37 ... 34
                                                (1, 256, 65536, 16, 4, [])])         # the dense layer's shape at T = 1
def test_gemv_splitk(m, n, k, s, rows, empty, bias, fmt):
    assert _gemv_rows(n, s) == rows
    c = _case("int", fmt, m, n, k)
    fails = []
    _check_split(c, s, bias, "latency", 32, empty, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("tiling", ["latency", "auto"])
def test_gemv_real(tiling, fmt):
    c = _case("real", fmt, 2, 7, 192)
    fails = []
    for row in ROWS10:
        o32, o16 = _linear(c, row, tiling=tiling)
        _check_real(c, row, o32, o16, "vpt_gemv_kernel", fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("relu_in", [False, True])
@pytest.mark.parametrize("m,k,n", [(1, 32, 6), (2, 1056, 7), (3, 3072, 2564), (4, 1024, 130), (5, 32, 6), (8, 3072, 10244)])
def test_layernorm_linear_bit_equal(m, k, n, relu_in, fmt):
    """The fused LayerNorm prologue (MR = 1, 2, 4: shared by the workgroup; MR = 8: a wave per row; every ROWS) = vpt_layernorm_forward + the
    weight-streaming kernel, bit for bit, normalised rows included."""
    dt = R.DT[fmt]
    g = torch.Generator().manual_seed(m * 7 + k + n)
    x = (torch.randn(m, k, generator=g) * 1.3 + 0.2).to(DEV)
    gain, lb = (1 + 0.2 * torch.randn(k, generator=g)).to(DEV), (0.1 * torch.randn(k, generator=g)).to(DEV)
    wpk = _pack(R.reals(g, fmt, n, k, scale=k ** -0.5))
    bias, res = (0.1 * torch.randn(n, generator=g)).to(DEV), torch.randn(m, n, generator=g).to(DEV)
    ln32, ln16 = ops.layernorm(x, gain, lb, relu_in=relu_in, out_f32=True, dtype=dt)
    o32, o16 = ops.linear(ln16, wpk, n, bias=bias, res=res, relu=True, out_f32=True, out_bf16=True, tiling="latency")
    f_ln32, f32_, f16_ = ops.layernorm_linear(x, gain, lb, wpk, n, bias=bias, res=res, relu=True, relu_in=relu_in, ln_out_f32=True, out_f32=True, out_bf16=True, dtype=dt)
    torch.cuda.synchronize()
    assert f16_.dtype == dt and bool(torch.isfinite(f32_).all())
    assert torch.equal(f_ln32, ln32), "normalised rows differ"
    assert torch.equal(f32_, o32), f"fp32 output differs; first at {R.first_bad((f32_ != o32).cpu())}"
    assert torch.equal(f16_.view(torch.int16), o16.view(torch.int16))


# ---- vpt_gemm_tn_kernel ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tn_case(kind, fmt, m, n, k):
    g = torch.Generator().manual_seed(5 * m + n + 11 * k)
    np_ = n + 8                                           # dy is [M, Np] with Np > n: the padding columns (nonzero here) are not part of dW
    if kind == "int":
        dy, x, base = R.ints(g, m, np_).to(R.DT[fmt]), R.ints(g, m, k).to(R.DT[fmt]), R.ints(g, n, k)
    else:
        dy, x, base = R.reals(g, fmt, m, np_), R.reals(g, fmt, m, k), torch.randn(n, k, generator=g)
    return dict(dy=dy, x=x, base=base, dy_d=dy.to(DEV), x_d=x.to(DEV))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("m,n,k", [(1, 8, 8), (63, 264, 136), (64, 256, 128), (65, 8, 136), (129, 520, 264), (200, 1032, 520)])
def test_wgrad_tn_integer(m, n, k, accumulate, fmt):
    c = _tn_case("int", fmt, m, n, k)
    out = c["base"].to(DEV) if accumulate else None
    dw = ops.linear_wgrad(c["dy_d"], c["x_d"], n, out=out)
    torch.cuda.synchronize()
    want = R.wgrad_ref(c["dy"], c["x"], n, base=c["base"] if accumulate else None)[0]
    msg = R.exact_failure(dw.cpu(), want, f"vpt_gemm_tn_kernel (M, n, k) = {(m, n, k)} {fmt} accumulate={accumulate}")
    assert msg is None, msg


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("accumulate", [False, True])
def test_wgrad_tn_real(accumulate, fmt):
    m, n, k = 65, 264, 136
    c = _tn_case("real", fmt, m, n, k)
    dw = ops.linear_wgrad(c["dy_d"], c["x_d"], n, out=c["base"].to(DEV) if accumulate else None)
    torch.cuda.synchronize()
    want, mag = R.wgrad_ref(c["dy"], c["x"], n, base=c["base"] if accumulate else None)
    worst, msg = R.bound_ratio(dw.cpu(), want, R.bound(mag, m))          # the reduction length is M
    print(f"vpt_gemm_tn_kernel {(m, n, k)} {fmt} accumulate={accumulate}: worst err / bound = {worst:.4f}")
    _note("vpt_gemm_tn_kernel", fmt, "fp32", worst)
    assert msg is None, msg


# ---- training.linear_backward and its helpers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("m,n,k", [(40, 121, 256), (257, 300, 192)])
def test_linear_backward_integer(m, n, k, fmt):
    """dx = gate(dy W) + skip (fp32 and padded 16-bit) and dW = dy^T x, exact: pins pack_linear(transposed=True, k_pad=Np) and both GEMMs' index maps."""
    dt = R.DT[fmt]
    g = torch.Generator().manual_seed(m + n + k)
    np_, ld = 64 * ((n + 63) // 64), k + 64
    dy, x, W = R.ints(g, m, n), R.ints(g, m, k), R.ints(g, n, k)
    mask, skip = R.ints(g, m, k).to(dt), R.ints(g, m, k)
    dy16 = torch.zeros(m, np_, dtype=dt)
    dy16[:, :n] = dy.to(dt)
    dx32, dx16, dw = linear_backward(dy16.to(DEV), n, x.to(dt).to(DEV), W.to(DEV), res=skip.to(DEV), mask=mask.to(DEV), dx_f32=True, dx_bf16_ld=ld)
    torch.cuda.synchronize()
    want_dx = R.exact(dy, W.t(), mask=mask, res=skip)
    want_dw = R.wgrad_ref(dy, x, n)[0]
    for got, want, what in ((dx32.cpu(), want_dx, "dx fp32"), (dx16.cpu()[:, :k].contiguous(), want_dx, "dx 16-bit"), (dw.cpu().contiguous(), want_dw, "dW")):
        msg = R.exact_failure(got, want, f"linear_backward (M, n, K) = {(m, n, k)} {fmt} {what}")
        assert msg is None, msg
    assert tuple(dx16.shape) == (m, ld) and not bool(dx16.cpu()[:, k:].view(torch.int16).any())


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("m", [1, 300, 8192])
def test_gate_cast_and_column_sum_integer(m, fmt):
    dt = R.DT[fmt]
    n, ldo = 121, 128
    g = torch.Generator().manual_seed(m)
    x, mask = R.ints(g, m, n), R.ints(g, m, n + 7).to(dt)
    for mk in (None, mask):
        out = ops.gate_cast(x.to(DEV), ldo, mask=mk.to(DEV) if mk is not None else None, dtype=dt)
        torch.cuda.synchronize()
        want = x.to(D) if mk is None else torch.where(mk[:, :n].to(D) > 0, x.to(D), torch.zeros(m, n, dtype=D))
        assert out.dtype == dt and tuple(out.shape) == (m, ldo)
        msg = R.exact_failure(out.cpu()[:, :n].contiguous(), want, f"gate_cast M = {m} {fmt} mask={mk is not None}")
        assert msg is None, msg
        assert not bool(out.cpu()[:, n:].view(torch.int16).any())
    base = R.ints(g, n)
    acc = base.clone().to(DEV)
    ops.column_sum_(acc, out, n)                            # out[N] += column sums (8 * 8192 < 2^24: exact in any order)
    torch.cuda.synchronize()
    msg = R.exact_failure(acc.cpu().view(1, n), (want.sum(0) + base.to(D)).view(1, n), f"column_sum_ M = {m} {fmt}")
    assert msg is None, msg


def test_print_worst_ratios():
    """Not a check: the table of worst err / bound per kernel that DESIGN.md section 7 quotes (run the module with -s)."""
    for key in sorted(RATIOS):
        print("worst err / bound:", *key, f"{RATIOS[key]:.4f}")
