"""The window plan and the feature-slot plan of the IDM video labeller (packing.label_windows / idm_feature_plan) against brute force."""
import pytest
import torch

import vpt_amd  # noqa: F401
from vpt_amd import packing

CASES = [(31, 12, 6), (30, 12, 6), (12, 12, 6), (7, 12, 6), (300, 128, 64), (13, 12, 12), (40, 12, 5)]


def _brute_windows(n, L, S):
    if n < L:
        return [0], n
    starts = []
    s = 0
    while s + L <= n:
        starts.append(s)
        s += S
    if starts[-1] != n - L:
        starts.append(n - L)
    return starts, L


@pytest.mark.parametrize("n,L,S", CASES)
def test_windows_and_owner_against_brute_force(n, L, S):
    starts, length, owner = packing.label_windows(n, L, S)
    want_starts, want_len = _brute_windows(n, L, S)
    assert starts.dtype == torch.int32 and owner.dtype == torch.int32
    assert starts.tolist() == want_starts and length == want_len
    assert owner.shape == (n,)                      # every frame is labelled exactly once ...
    for f in range(n):
        k = int(owner[f])
        assert want_starts[k] <= f < want_starts[k] + want_len      # ... by a window that holds it ...
        cost = [abs(2 * (f - s) - (want_len - 1)) if s <= f < s + want_len else None for s in want_starts]
        best = min(c for c in cost if c is not None)
        assert k == cost.index(best), (f, k, cost)                  # ... the most central one, the lower window on ties
    # the last frame of the video is covered (the tail window)
    assert want_starts[-1] + want_len == n


def test_interior_windows_serve_offsets_32_to_95():
    starts, length, owner = packing.label_windows(300, 128, 64)
    assert starts.tolist() == [0, 64, 128, 172] and length == 128
    for k in (1,):            # windows whose both neighbours sit a full stride away
        served = [f - int(starts[k]) for f in range(300) if int(owner[f]) == k]
        assert served == list(range(32, 96))
    assert [f for f in range(300) if int(owner[f]) == 0] == list(range(0, 96))      # the first window serves the video's head
    assert int(owner[299]) == 3 and int(owner[172 + 127]) == 3                       # the last one its tail
    # a video that is a whole number of strides: every interior window serves 32..95
    starts, _, owner = packing.label_windows(64 * 7, 128, 64)
    for k in range(1, starts.numel() - 1):
        assert [f - int(starts[k]) for f in range(64 * 7) if int(owner[f]) == k] == list(range(32, 96))


@pytest.mark.parametrize("n,L,S", CASES)
def test_feature_slots_reproduce_the_zero_padded_taps(n, L, S):
    plan = packing.idm_feature_plan(n, L, S)
    starts, length = plan.starts.tolist(), plan.length
    n_win = len(starts)
    n_slots = plan.src.numel()
    assert plan.win_rows.shape == (n_win * length,) and plan.sel_rows.shape == (n,)
    assert all(t.dtype == torch.int32 for t in (plan.src, plan.lo, plan.hi, plan.win_rows, plan.sel_rows))
    assert n_slots <= n + 4 * n_win
    keys = list(zip(plan.src.tolist(), plan.lo.tolist(), plan.hi.tolist()))
    assert keys == sorted(set(keys))                                    # distinct keys, sorted
    assert sorted(set(plan.win_rows.tolist())) == list(range(n_slots))  # every slot is used
    for k, s in enumerate(starts):
        padded = [None, None] + list(range(s, s + length)) + [None, None]       # the window with two zero frames on either side
        for o in range(length):
            want = padded[o:o + 5]                                               # the five taps Conv3d(5,1,1), padding 2, reads at offset o
            j = int(plan.win_rows[k * length + o])
            src, lo, hi = keys[j]
            got = [src + dt - 2 if lo <= src + dt - 2 < hi else None for dt in range(5)]
            assert got == want, (k, o, keys[j])
            assert (src, lo, hi) == (s + o, max(s, s + o - 2), min(s + length, s + o + 3))
            assert 0 <= lo < hi <= n
    for f in range(n):
        k, o = divmod(int(plan.sel_rows[f]), length)
        assert k == int(plan.owner[f]) and starts[k] + o == f


def test_feature_plan_shares_interior_frames():
    plan = packing.idm_feature_plan(1024, 128, 64)
    n_win = plan.starts.numel()
    assert n_win == 15 and plan.src.numel() == 1024 + 4 * (n_win - 1)           # 2 edge rows per inner window edge; the video's own ends are shared
    assert plan.src.numel() / (n_win * 128) < 0.57


@pytest.mark.parametrize("bad", [(10, 12, 0), (10, 12, 13), (10, 161, 80), (0, 12, 6)])
def test_bad_arguments_raise(bad):
    with pytest.raises(ValueError):
        packing.label_windows(*bad)
