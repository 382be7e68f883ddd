"""tests/linear_ref.py is the true linear layer, plain fp32 arithmetic meets both of its instruments, and each instrument sees the defects it is there
for -- shown on the CPU, before a GPU sees either (tests/test_gpu_linear_exact.py is the GPU half).

1. linear_ref / wgrad_ref / dense_fold_ref equal fp64 torch (nn.functional.linear, autograd, layer_norm) on each epilogue.
2. fp32 arithmetic on the same operands -- accumulated in 64-wide k-chunks as the kernels do, and as one matmul -- gives THE integer result on integer
   operands (fp32 bit-equal, 16-bit output its one RNE rounding) and lies inside every bound on real-valued ones.  A check plain fp32 cannot meet
   would be wrong.
3. Six mutations of the reference (one dropped product, one k-block taken twice, rows M-1 and M-2 swapped, bias after the ReLU, gate after the residual,
   a truncating second rounding of the 16-bit output) each FAIL the instrument they are aimed at."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import linear_ref as R

D = torch.float64
FMTS = ["bf16", "fp16"]


def _fp32_linear(a, w, bias=None, relu=False, mask=None, res=None, chunk=64, splits=1):
    """The layer in fp32: chunk = 64 -> one partial product per 64-wide k-chunk added to a running fp32 sum (per K slice; slices summed in order, bias in
    slice 0), chunk = None -> one matmul."""
    a32, w32 = a.float(), w.float()
    k = a32.shape[1]
    if chunk is None:
        y = a32 @ w32.t()
    else:
        steps = (k + chunk - 1) // chunk
        per = (steps + splits - 1) // splits
        y = torch.zeros(a32.shape[0], w32.shape[0])
        for s in range(splits):
            acc = torch.zeros_like(y)
            for st in range(s * per, min((s + 1) * per, steps)):
                acc = acc + a32[:, st * chunk:(st + 1) * chunk] @ w32[:, st * chunk:(st + 1) * chunk].t()
            y = y + acc
    if bias is not None:
        y = y + bias
    if relu:
        y = torch.relu(y)
    if mask is not None:
        y = torch.where(mask.float() > 0, y, torch.zeros_like(y))
    if res is not None:
        y = y + res
    return y


@functools.lru_cache(maxsize=None)
def _operands(kind, fmt, m, n, k, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + m + 3 * n + 7 * k)
    if kind == "int":
        return dict(a=R.ints(g, m, k).to(R.DT[fmt]), w=R.ints(g, n, k).to(R.DT[fmt]), bias=R.ints(g, n), res=R.ints(g, m, n), mask=R.ints(g, m, n).to(R.DT[fmt]))
    return dict(a=R.reals(g, fmt, m, k), w=R.reals(g, fmt, n, k, scale=k ** -0.5), bias=torch.randn(n, generator=g), res=torch.randn(m, n, generator=g),
                mask=R.reals(g, fmt, m, n))


EPILOGUES = {"plain": dict(), "bias": dict(bias=True), "bias_res": dict(bias=True, res=True), "relu": dict(relu=True), "mask": dict(mask=True),
             "all": dict(bias=True, relu=True, mask=True, res=True)}


def _kw(o, flags):
    return dict(bias=o["bias"] if flags.get("bias") else None, relu=bool(flags.get("relu")), mask=o["mask"] if flags.get("mask") else None,
                res=o["res"] if flags.get("res") else None)


# ---- 1. the reference is the operation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", list(EPILOGUES))
def test_reference_equals_fp64_torch(epi):
    o = _operands("real", "bf16", 9, 13, 64)
    kw = _kw(o, EPILOGUES[epi])
    y, mag = R.linear_ref(o["a"], o["w"], **kw)
    want = F.linear(o["a"].to(D), o["w"].to(D), kw["bias"].to(D) if kw["bias"] is not None else None)
    if kw["relu"]:
        want = F.relu(want)
    if kw["mask"] is not None:
        want = want * (kw["mask"].to(D) > 0).to(D)
    if kw["res"] is not None:
        want = want + kw["res"].to(D)
    assert torch.allclose(y, want, rtol=0, atol=1e-12)
    assert bool((mag >= y.abs() - 1e-12).all())


def test_wgrad_reference_equals_autograd():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(11, 16, generator=g, dtype=D)
    w = torch.randn(8, 16, generator=g, dtype=D, requires_grad=True)
    dy = torch.randn(11, 24, generator=g, dtype=D)               # padded to Np = 24 > n = 8: the padding columns are not part of dW
    (x @ w.t()).backward(dy[:, :8])
    base = torch.randn(8, 16, generator=g, dtype=D)
    dw, mag = R.wgrad_ref(dy, x, 8)
    assert torch.allclose(dw, w.grad, rtol=0, atol=1e-12)
    assert torch.allclose(R.wgrad_ref(dy, x, 8, base=base)[0], w.grad + base, rtol=0, atol=1e-12)
    assert bool((mag >= dw.abs()).all())


def test_dense_fold_reference_equals_layer_norm_then_linear():
    """rstd * (x @ (W g)^T) - rstd * mean * sg + sb  ==  LayerNorm(x; g, b) @ W^T, from the frame statistics of x; one frame has |mean| * rstd ~ 1000."""
    g = torch.Generator().manual_seed(3)
    m, n, k, s = 4, 10, 256, 4
    x = torch.randn(m, k, generator=g, dtype=D)
    x[1] = 50.0 + 0.05 * x[1]
    W, gain, lb = torch.randn(n, k, generator=g, dtype=D) / 16, 1 + 0.2 * torch.randn(k, generator=g, dtype=D), 0.1 * torch.randn(k, generator=g, dtype=D)
    wg = W * gain
    part = torch.stack([x[:, i * 64:(i + 1) * 64] @ wg[:, i * 64:(i + 1) * 64].t() for i in range(s)])
    stats = torch.stack([x.sum(1), (x * x).sum(1)], 1)
    out, bnd = R.dense_fold_ref(part, stats, k, wg.sum(1), W @ lb)
    want = F.layer_norm(x, (k,), gain, lb, eps=R.EPS) @ W.t()
    assert float((stats[1, 0] / k).abs() * (1 / torch.sqrt(stats[1, 1] / k - (stats[1, 0] / k) ** 2 + R.EPS))) > 500
    assert torch.allclose(out, want, rtol=1e-9, atol=1e-9)
    # the kernel's arithmetic in fp32 lies inside the bound
    mean32 = (stats[:, 0] / k).float()
    var32 = (stats[:, 1] / k - (stats[:, 0] / k) ** 2).clamp(min=0).float()
    rstd32 = torch.rsqrt(var32 + torch.tensor(R.EPS))
    v = torch.zeros(m, n)
    for i in range(s):
        v = v + part[i].float()
    got = rstd32.view(-1, 1) * v + ((-rstd32 * mean32).view(-1, 1) * wg.sum(1).float().view(1, -1) + (W @ lb).float().view(1, -1))
    worst, msg = R.bound_ratio(got, *R.dense_fold_ref(part.float(), stats, k, wg.sum(1).float(), (W @ lb).float()))
    print(f"dense fold, fp32 arithmetic: worst err / bound = {worst:.3f}")
    assert msg is None, msg


# ---- 2. plain fp32 arithmetic meets both instruments -----------------------------------------------------------------------------------------------------
INT_SHAPES = [(3, 6, 8224), (5, 256, 65536), (257, 260, 192), (1, 4, 64), (40, 132, 320), (2, 7, 1056)]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("m,n,k", INT_SHAPES)
def test_fp32_arithmetic_gives_the_integer_result(m, n, k, fmt):
    o = _operands("int", fmt, m, n, k)
    biggest = 0.0
    for epi in ("bias_res", "relu", "all"):
        kw = _kw(o, EPILOGUES[epi])
        ex = R.exact(o["a"], o["w"], **kw)
        biggest = max(biggest, ex.abs().max().item())
        for chunk, splits in ((64, 1), (64, 4), (None, 1)):
            y32 = _fp32_linear(o["a"], o["w"], chunk=chunk, splits=splits, **kw)
            assert R.exact_failure(y32, ex) is None
            assert R.exact_failure(y32.to(R.DT[fmt]), ex) is None
    assert biggest < 65504 and biggest < 2 ** 24          # fp16 outputs stay finite, fp32 holds the integers


REAL_SHAPES = [(257, 132, 192, 1), (257, 131, 192, 1), (2, 7, 192, 1), (40, 132, 256, 4)]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("m,n,k,s", REAL_SHAPES)
def test_fp32_arithmetic_lies_inside_the_bound(m, n, k, s, fmt):
    o = _operands("real", fmt, m, n, k)
    for epi in EPILOGUES:
        kw = _kw(o, EPILOGUES[epi])
        y64, mag = R.linear_ref(o["a"], o["w"], **kw)
        for chunk in (64, None):
            y32 = _fp32_linear(o["a"], o["w"], chunk=chunk, splits=s if chunk else 1, **kw)
            w32, msg = R.bound_ratio(y32, y64, R.bound(mag, k, s))
            assert msg is None, msg
            w16, msg = R.bound_ratio(y32.to(R.DT[fmt]), y64, R.bound16(y64, mag, k, fmt, s))
            assert msg is None, msg
            assert w32 < 0.1 and w16 < 0.6, (w32, w16)        # (measured 0.023 / 0.497: the fp32 bound is a worst case, the 16-bit one is half an ulp)


@pytest.mark.parametrize("fmt", FMTS)
def test_fp32_weight_gradient_meets_both(fmt):
    g = torch.Generator().manual_seed(5)
    m, n, k, np_ = 65, 264, 136, 320
    dy = torch.zeros(m, np_)
    dy[:, :n] = R.ints(g, m, n)
    x, base = R.ints(g, m, k), R.ints(g, n, k)
    ex = R.wgrad_ref(dy, x, n, base=base)[0]
    assert R.exact_failure(dy[:, :n].t() @ x + base, ex) is None
    dyr, xr = R.reals(g, fmt, m, np_), R.reals(g, fmt, m, k)
    dw64, mag = R.wgrad_ref(dyr, xr, n)
    worst, msg = R.bound_ratio(dyr.float()[:, :n].t() @ xr.float(), dw64, R.bound(mag, m))
    assert msg is None and worst < 0.1, (worst, msg)


# ---- 3. the instruments see the defects they are there for -----------------------------------------------------------------------------------------------
def _mutated(kind, o, k):
    """The reference with one defect: -> (y64, mag) as linear_ref with bias, ReLU, gate and residual all on."""
    a, w, bias, mask, res = o["a"].to(D), o["w"].to(D), o["bias"].to(D), o["mask"].to(D), o["res"].to(D)
    m = a.shape[0]
    mag = a.abs() @ w.abs().t() + bias.abs() + res.abs()
    gate = lambda y: torch.where(mask > 0, y, torch.zeros_like(y))
    if kind == "dropped_product":
        a = a.clone()
        a[m // 2, k - 1] = 0
    pre = a @ w.t()
    if kind == "k_block_twice":
        pre = pre + a[:, k - 64:] @ w[:, k - 64:].t()
    if kind == "bias_after_relu":
        y = gate(torch.relu(pre) + bias) + res
    elif kind == "gate_after_residual":
        y = gate(torch.relu(pre + bias) + res)
    else:
        y = gate(torch.relu(pre + bias)) + res
    if kind == "rows_swapped":
        y = y.clone()
        y[[m - 1, m - 2]] = y[[m - 2, m - 1]]
    return y, mag


MUTATIONS = ["dropped_product", "k_block_twice", "rows_swapped", "bias_after_relu", "gate_after_residual"]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("kind", MUTATIONS)
@pytest.mark.parametrize("m,n,k", [(257, 132, 192), (3, 6, 8224)])
def test_integer_instrument_fails_each_mutation(m, n, k, kind, fmt):
    o = _operands("int", fmt, m, n, k)
    y32 = _fp32_linear(o["a"], o["w"], **_kw(o, EPILOGUES["all"]))
    assert R.exact_failure(y32, R.exact(o["a"], o["w"], **_kw(o, EPILOGUES["all"]))) is None
    mut = _mutated(kind, o, k)[0]
    assert R.exact_failure(y32, mut) is not None
    assert R.exact_failure(y32.to(R.DT[fmt]), mut) is not None
    if kind == "dropped_product":        # without the ReLU and the gate, EVERY element of the row that lost a product differs
        a2 = o["a"].clone()
        a2[m // 2, k - 1] = 0
        diff = _fp32_linear(o["a"], o["w"], bias=o["bias"]) != R.exact(a2, o["w"], bias=o["bias"]).float()
        assert bool(diff[m // 2].all()) and int(diff.sum()) == n


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("kind", MUTATIONS)
def test_bound_instrument_fails_each_mutation(kind, fmt):
    m, n, k = 257, 132, 192
    o = _operands("real", fmt, m, n, k)
    y32 = _fp32_linear(o["a"], o["w"], **_kw(o, EPILOGUES["all"]))
    y64, mag = _mutated(kind, o, k)
    assert R.bound_ratio(y32, y64, R.bound(mag, k))[1] is not None
    assert R.bound_ratio(y32.to(R.DT[fmt]), y64, R.bound16(y64, mag, k, fmt))[1] is not None


def test_one_lost_product_is_far_outside_the_bound_at_k_256():
    """The reason the O(K) bound is used at K <= 256 only: there a single a * w of typical size is ~100 x the bound."""
    o = _operands("real", "bf16", 40, 132, 256)
    y64, mag = R.linear_ref(o["a"], o["w"])
    typical = (o["a"].to(D).abs().mean() * o["w"].to(D).abs().mean()).item()
    assert typical / R.bound(mag, 256).median().item() > 50


def test_truncating_second_rounding_fails_the_integer_instrument():
    """fp32 -> bf16 by dropping the low 16 bits instead of rounding to nearest even."""
    o = _operands("int", "bf16", 257, 132, 192)
    ex = R.exact(o["a"], o["w"], bias=o["bias"])
    y32 = _fp32_linear(o["a"], o["w"], bias=o["bias"])
    assert R.exact_failure(y32.to(torch.bfloat16), ex) is None
    trunc = (y32.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    msg = R.exact_failure(trunc, ex)
    assert msg is not None and "first at (row, col)" in msg


def test_ulp16_is_the_spacing_of_the_format():
    for fmt, dt in R.DT.items():
        v = torch.tensor([1.0, 1.5, 2.0, 3.99, 1000.0, 2.0 ** R.EMIN[fmt], 2.0 ** (R.EMIN[fmt] - 3), 0.0], dtype=D)
        up = torch.nextafter(v.to(dt).float().to(dt), torch.tensor(float("inf"), dtype=dt))
        assert torch.equal(R.ulp16(v, fmt), (up.to(D) - v.to(dt).to(D)))
