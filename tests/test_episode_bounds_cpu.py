"""packing.episode_bounds (the host twin of vpt_episode_bounds_kernel): `first` honoured at every frame of a [B, t] chunk must give
exactly what stepping the oracle's band_visibility one frame at a time gives, with the state mask carried -- the reference's BC loop
(behavioural_cloning.py:95-112) -- and must reduce to band_visibility(t, ...) when no `first` lies beyond t = 0."""
import pytest
import torch

import vpt_amd  # noqa: F401
from vpt_amd import packing
from oracle import vpt_oracle as O

GRID = [(maxlen, t) for maxlen in (4, 16, 128) for t in (1, 3, 5, 40, 200)]


def implied_visibility(first, state_mask, maxlen):
    """bool [B, t, t + maxlen] from (qlo, state_mask): band, j >= qlo, memory rows additionally need state_mask."""
    bsz, t = first.shape
    qlo, nxt = packing.episode_bounds(first, state_mask, maxlen)
    assert qlo.dtype == torch.int32 and tuple(qlo.shape) == (bsz, t) and nxt.dtype == torch.bool and tuple(nxt.shape) == (bsz, maxlen)
    i = torch.arange(t).view(1, t, 1)
    j = torch.arange(t + maxlen).view(1, 1, t + maxlen)
    rows = torch.cat([state_mask.reshape(bsz, maxlen), torch.ones(bsz, t, dtype=torch.bool)], 1)
    return (j >= i + 1) & (j <= i + maxlen) & (j >= qlo.view(bsz, t, 1).long()) & rows.view(bsz, 1, -1), nxt


def stepped_visibility(first, state_mask, maxlen):
    """The same from the oracle at T = 1, frame by frame: at frame p the memory holds rows p .. p + maxlen - 1 of [memory ; chunk]."""
    bsz, t = first.shape
    vis = torch.zeros(bsz, t, t + maxlen, dtype=torch.bool)
    mask = state_mask.reshape(bsz, 1, maxlen)
    for p in range(t):
        v, mask = O.band_visibility(1, maxlen, first[:, p], mask)
        vis[:, p, p:p + maxlen + 1] = v[:, 0]
    return vis, mask.reshape(bsz, maxlen)


def cases(maxlen, t, seed):
    g = torch.Generator().manual_seed(seed)
    bsz = 6
    first = torch.rand(bsz, t, generator=g) < 0.15
    first[0] = False                       # no start at all
    first[1] = False; first[1, 0] = True
    first[2] = False; first[2, t - 1] = True
    first[3] = True                        # a start at every frame
    state_mask = torch.rand(bsz, maxlen, generator=g) < 0.6
    state_mask[4] = False
    return first, state_mask


@pytest.mark.parametrize("maxlen,t", GRID)
def test_per_frame_bounds_equal_stepping_the_oracle(maxlen, t):
    for seed in range(3):
        first, state_mask = cases(maxlen, t, 100 * maxlen + t + seed)
        got, got_mask = implied_visibility(first, state_mask, maxlen)
        want, want_mask = stepped_visibility(first, state_mask, maxlen)
        assert torch.equal(got, want)
        assert torch.equal(got_mask, want_mask)


@pytest.mark.parametrize("maxlen,t", GRID)
def test_reduces_to_the_chunk_rule_without_later_starts(maxlen, t):
    first, state_mask = cases(maxlen, t, 7 * maxlen + t)
    first[:, 1:] = False
    first[::2, 0] = True
    got, got_mask = implied_visibility(first, state_mask, maxlen)
    want, want_mask = O.band_visibility(t, maxlen, first[:, 0], state_mask.reshape(-1, 1, maxlen))
    assert torch.equal(got, want)
    assert torch.equal(got_mask, want_mask.reshape(-1, maxlen))


def test_shapes_accepted():
    first = torch.zeros(2, 5, dtype=torch.bool)
    first[1, 3] = True
    qlo, nxt = packing.episode_bounds(first, None, 4)
    assert qlo.tolist() == [[0] * 5, [0, 0, 0, 7, 7]]
    q2, n2 = packing.episode_bounds(first, torch.zeros(2, 1, 4, dtype=torch.bool), 4)
    assert torch.equal(q2, qlo) and torch.equal(n2, nxt)
    # t = 5 > maxlen = 4: every kept row is a chunk row (5 + r - 4 = frames 1..4); row 1 keeps frames >= 3 only
    assert nxt.tolist() == [[True] * 4, [False, False, True, True]]
