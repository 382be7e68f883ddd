"""vpt_gae_kernel (ops.gae) against its float32 host twin tests/gae_ref.py: bit for bit.  Needs an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from tests import gae_ref as G  # noqa: E402

DEV = "cuda"


@pytest.mark.parametrize("b,t", G.CASES)
@pytest.mark.parametrize("gamma,lam", [(0.999, 0.95), (0.9, 1.0)])
def test_gae_equals_the_float32_twin_bit_for_bit(b, t, gamma, lam):
    """`first` at t = 0, mid-row and t = T - 1, next_first both ways (tests/gae_ref.make_case); B = 5 x T = 130 walks 130 steps per lane."""
    r, v, first, last, nf = G.make_case(b, t)
    adv_ref, ret_ref = G.gae_f32(r, v, first, last, nf, gamma, lam)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    adv, ret = ops.gae(dev(r), dev(v), dev(first), dev(last), dev(nf), gamma=gamma, lam=lam)
    torch.cuda.synchronize()
    assert adv.dtype == ret.dtype == torch.float32 and tuple(adv.shape) == tuple(ret.shape) == (b, t)
    assert torch.equal(adv.cpu(), torch.from_numpy(adv_ref)) and torch.equal(ret.cpu(), torch.from_numpy(ret_ref))
    adv8, ret8 = ops.gae(dev(r), dev(v), dev(first).to(torch.uint8), dev(last), dev(nf).to(torch.uint8), gamma=gamma, lam=lam)     # uint8 flags
    assert torch.equal(adv8, adv) and torch.equal(ret8, ret)


def test_gae_stops_at_an_episode_start_and_validates_shapes():
    r, v = torch.ones(1, 4, device=DEV), torch.zeros(1, 4, device=DEV)
    r[0, 2:], v[0, 2:] = float("nan"), float("nan")
    first = torch.tensor([[False, False, True, False]], device=DEV)
    adv, ret = ops.gae(r, v, first, torch.full((1,), float("nan"), device=DEV), torch.tensor([True], device=DEV), gamma=0.5, lam=1.0)
    torch.cuda.synchronize()
    assert adv[0, :2].tolist() == [1.5, 1.0] and bool(torch.isnan(adv[0, 2:]).all())
    with pytest.raises(ValueError, match="share one"):
        ops.gae(r, v[:, :3].contiguous(), first, torch.zeros(1, device=DEV), torch.tensor([True], device=DEV))
    with pytest.raises(ValueError, match="last_value"):
        ops.gae(r, v, first, torch.zeros(2, device=DEV), torch.tensor([True], device=DEV))
