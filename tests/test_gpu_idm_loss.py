"""ops.idm_loss (vpt_idm_loss_kernel: the IDM's 20 two-way button groups + 2 eleven-way camera groups in one sweep) against its host twin
packing.idm_loss_metrics / idm_loss_grad (fp64 torch).  Needs an MI355X.
Bounds: dz within one rounding of the 16-bit format of the twin's value (the kernel forms it in fp32 from expf: half an ulp of the format for the
cast plus fp32 noise, i.e. < 1 ulp); frame_out within 1e-5 absolute (fp32 sums of at most 40 log-probs of magnitude < 10); totals within 1e-5
relative (fp32 tree over M <= 300 records)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops, packing  # noqa: E402

DEV = "cuda"
GB, NB, GC, NC = 20, 2, 2, 11
EPS16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}       # one unit in the last place, relative
TINY16 = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -24}    # ... and the smallest spacing near zero


def _inputs(m, seed=0, weights=True):
    g = torch.Generator().manual_seed(seed)
    lp_b = torch.log_softmax(torch.randn(m, GB, NB, generator=g), -1)
    lp_c = torch.log_softmax(torch.randn(m, GC, NC, generator=g), -1)
    ab = torch.randint(0, NB, (m, GB), generator=g)
    ac = torch.randint(0, NC, (m, GC), generator=g)
    w = None
    if weights:
        w = torch.rand(m, generator=g) + 0.25
        w[::3] = 0.0                       # rows left out of the loss (row 0 among them)
        if m == 1:
            w[0] = 0.75
    return lp_b, lp_c, ab, ac, w


def _gpu(lp_b, lp_c, ab, ac, w, scale, dtype):
    dz, fo, tot = ops.idm_loss(lp_b.to(DEV), lp_c.to(DEV), ab.to(DEV), ac.to(DEV), scale, weight=None if w is None else w.to(DEV), dtype=dtype)
    torch.cuda.synchronize()
    return dz.cpu(), fo.cpu(), tot.cpu()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("m", [1, 5, 300])
def test_against_the_host_twin(m, dtype):
    lp_b, lp_c, ab, ac, w = _inputs(m, seed=m)
    scale = 0.37
    dz, fo, tot = _gpu(lp_b, lp_c, ab, ac, w, scale, dtype)
    fo_ref, tot_ref = packing.idm_loss_metrics(lp_b, lp_c, ab, ac, w)
    g_ref = packing.idm_loss_grad(lp_b, lp_c, ab, ac, scale, w)
    n = GB * NB + GC * NC
    assert dz.shape == (m, 64) and dz.dtype == dtype
    err = (dz[:, :n].double() - g_ref).abs()
    assert bool((err <= EPS16[dtype] * g_ref.abs() + TINY16[dtype]).all()), float((err / g_ref.abs().clamp(min=1e-30)).max())
    assert float(dz[:, n:].abs().max()) == 0.0                                   # padding columns
    assert float(dz[w == 0].abs().max() if bool((w == 0).any()) else 0.0) == 0.0   # rows left out
    assert float((fo.double() - fo_ref).abs().max()) < 1e-5
    assert float(((tot.double() - tot_ref).abs() / tot_ref.abs().clamp(min=1e-30)).max()) < 1e-5
    assert float(fo[:, 7].abs().max()) == 0.0 and torch.equal(fo[:, 6], w)


def test_zero_weight_rows_ignore_their_labels_and_unweighted_default():
    m = 5
    lp_b, lp_c, ab, ac, w = _inputs(m, seed=11)
    dz0, _, tot0 = _gpu(lp_b, lp_c, ab, ac, w, 1.0, torch.bfloat16)
    ab2, ac2 = ab.clone(), ac.clone()
    ab2[w == 0] = 1 - ab2[w == 0]                  # other labels, still in range, on the rows with w = 0
    ac2[w == 0] = (ac2[w == 0] + 5) % NC
    dz1, _, tot1 = _gpu(lp_b, lp_c, ab2, ac2, w, 1.0, torch.bfloat16)
    assert torch.equal(dz0, dz1) and torch.equal(tot0, tot1)
    assert float(dz0[w == 0].abs().max()) == 0.0
    # weight=None is weight = ones
    a = _gpu(lp_b, lp_c, ab, ac, None, 0.5, torch.bfloat16)
    b = _gpu(lp_b, lp_c, ab, ac, torch.ones(m), 0.5, torch.bfloat16)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_hits_count_groups_and_ties_take_the_lowest_index():
    m = 2
    lp_b = torch.full((m, GB, NB), -0.6931471805599453)      # every button group tied: arg-max = class 0
    lp_c = torch.log_softmax(torch.arange(NC).float().repeat(m, GC, 1), -1)       # arg-max = class 10
    ab = torch.zeros(m, GB, dtype=torch.int64)
    ab[1, :5] = 1                                             # 15 of 20 groups hit in row 1
    ac = torch.tensor([[10, 10], [10, 3]])
    _, fo, _ = _gpu(lp_b, lp_c, ab, ac, None, 1.0, torch.bfloat16)
    assert fo[:, 4].tolist() == [1.0, 0.75] and fo[:, 5].tolist() == [1.0, 0.5]


def test_totals_are_the_same_bits_from_call_to_call():
    lp_b, lp_c, ab, ac, w = _inputs(300, seed=3)
    a = _gpu(lp_b, lp_c, ab, ac, w, 0.01, torch.float16)
    b = _gpu(lp_b, lp_c, ab, ac, w, 0.01, torch.float16)
    assert torch.equal(a[2], b[2]) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
