"""tests/gae_ref.py on the CPU: the float32 twin of vpt_gae_kernel against the fp64 textbook recursion run per episode segment, within the
recurrence's propagated rounding (T 4u sum |terms|)."""
import numpy as np
import pytest

from tests import gae_ref as G

@pytest.mark.parametrize("b,t", G.CASES)
@pytest.mark.parametrize("gamma,lam", [(0.999, 0.95), (0.9, 1.0)])
def test_float32_twin_against_the_fp64_segments(b, t, gamma, lam):
    r, v, first, last, nf = G.make_case(b, t)
    adv, ret = G.gae_f32(r, v, first, last, nf, gamma, lam)
    adv64, ret64, bound = G.gae_f64_segments(r, v, first, last, nf, gamma, lam)
    assert adv.dtype == ret.dtype == np.float32
    ea, er = np.abs(adv - adv64), np.abs(ret - ret64)
    print(f"gae twin ({b}, {t}) gamma {gamma} lambda {lam}: max err / bound adv {float((ea / bound).max()):.3f}, ret {float((er / bound).max()):.3f}")
    assert (ea <= bound).all() and (er <= bound).all()


def test_an_episode_start_cuts_the_recursion():
    """Nothing of the next episode flows back over a `first` flag, NaN included; next_first cuts the bootstrap from last_value."""
    r, v = np.ones((1, 4), np.float32), np.zeros((1, 4), np.float32)
    first = np.array([[False, False, True, False]])
    r[0, 2:], v[0, 2:] = np.nan, np.nan
    adv, ret = G.gae_f32(r, v, first, np.array([np.nan], np.float32), np.array([True]), 0.5, 1.0)
    assert adv[0, :2].tolist() == [1.5, 1.0] and np.isnan(adv[0, 2:]).all()
    adv2, _ = G.gae_f32(np.ones((1, 2), np.float32), np.zeros((1, 2), np.float32), np.zeros((1, 2), bool), np.array([4.0], np.float32), np.array([False]), 0.5, 1.0)
    assert adv2[0].tolist() == [1.0 + 0.5 * (1.0 + 0.5 * 4.0), 1.0 + 0.5 * 4.0]
