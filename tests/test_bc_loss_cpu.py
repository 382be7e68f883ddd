"""The host side of the weighted BC loss (no GPU): packing.bc_loss_metrics -- the twin the GPU tests hold vpt_bc_loss_kernel to -- against the
reference's formulas written out directly (lib/action_head.py:176-193, behavioural_cloning.py:107), and SequenceBatcher(pad_last=True) on the
synthetic recordings of tests/test_sequence_batcher_cpu.py."""
import gzip
import json
import os
import random
import warnings

import numpy as np
import pytest
import torch

import vpt_amd  # noqa: F401
from vpt_amd import clip_loader, packing
from vpt_amd.sequence_batcher import SequenceBatcher
from oracle import action_codec as A

GOLD = os.path.join(os.path.dirname(__file__), "golden")
with gzip.open(os.path.join(GOLD, "clip_actions_seed0.json.gz"), "rt") as fh:
    RECS = json.load(fh)
H, W = 36, 64


# ---------------------------------------------------------------------------------------------------------
# 3a. the twin against first principles
# ---------------------------------------------------------------------------------------------------------
def test_twin_matches_the_formulas_written_out():
    g = torch.Generator().manual_seed(5)
    m, nb, nc = 7, 50, 11
    lp_b = torch.log_softmax(torch.randn(m, nb, generator=g, dtype=torch.float64) * 2, -1)
    lp_c = torch.log_softmax(torch.randn(m, nc, generator=g, dtype=torch.float64) * 2, -1)
    ab, ac = torch.randint(0, nb, (m,), generator=g), torch.randint(0, nc, (m,), generator=g)
    ab[2], ac[2] = lp_b[2].argmax(), lp_c[2].argmax()            # both hit values occur
    ab[3], ac[3] = (lp_b[3].argmax() + 1) % nb, (lp_c[3].argmax() + 1) % nc
    w = torch.tensor([1.0, 0.0, 0.3, 1.0, 2.0, 0.0, 0.5], dtype=torch.float64)
    frame_out, totals = packing.bc_loss_metrics(lp_b, lp_c, ab, ac, w)
    assert frame_out.dtype == totals.dtype == torch.float64 and tuple(frame_out.shape) == (m, 8) and tuple(totals.shape) == (8,)
    want = torch.stack([-lp_b.gather(1, ab[:, None])[:, 0], -lp_c.gather(1, ac[:, None])[:, 0],
                        -(lp_b.exp() * lp_b).sum(-1), -(lp_c.exp() * lp_c).sum(-1),
                        (lp_b.argmax(-1) == ab).double(), (lp_c.argmax(-1) == ac).double(), w, torch.zeros(m, dtype=torch.float64)], 1)
    assert torch.equal(frame_out[:, [0, 1, 4, 5, 6, 7]], want[:, [0, 1, 4, 5, 6, 7]])
    assert torch.allclose(frame_out[:, 2:4], want[:, 2:4], rtol=1e-14, atol=0)
    assert set(frame_out[:, 4].tolist()) == {0.0, 1.0}
    want_tot = torch.cat([(w[:, None] * want[:, :6]).sum(0), w.sum().view(1), torch.tensor([5.0], dtype=torch.float64)])
    assert torch.allclose(totals, want_tot, rtol=1e-14, atol=0)
    # the loss of behavioural_cloning.py:107 generalised: sum w (nll_b + nll_c) / sum w
    loss = (w * (want[:, 0] + want[:, 1])).sum() / w.sum()
    assert abs(float((totals[0] + totals[1]) / totals[6]) - float(loss)) < 1e-14
    # weight=None is all ones
    f1, t1 = packing.bc_loss_metrics(lp_b, lp_c, ab, ac)
    f2, t2 = packing.bc_loss_metrics(lp_b, lp_c, ab, ac, torch.ones(m))
    assert torch.equal(f1, f2) and torch.equal(t1, t2) and float(t1[7]) == m


def test_twin_zero_weight_rows_add_exact_zeros_whatever_they_hold():
    g = torch.Generator().manual_seed(6)
    m, nb, nc = 4, 50, 11
    lp_b = torch.log_softmax(torch.randn(m, nb, generator=g) * 2, -1)
    lp_c = torch.log_softmax(torch.randn(m, nc, generator=g) * 2, -1)
    ab, ac = torch.randint(0, nb, (m,), generator=g), torch.randint(0, nc, (m,), generator=g)
    w = torch.tensor([1.0, 0.0, 0.3, 2.0])
    keep = torch.tensor([0, 2, 3])
    _, want = packing.bc_loss_metrics(lp_b[keep], lp_c[keep], ab[keep], ac[keep], w[keep])
    lp_b[1], lp_c[1], ab[1], ac[1] = float("nan"), float("nan"), -1, nc + 5       # a padded frame: garbage log-probs, labels out of range
    _, totals = packing.bc_loss_metrics(lp_b, lp_c, ab, ac, w)
    assert bool(torch.isfinite(totals).all()) and torch.equal(totals, want)
    # a log-prob of -inf (a masked action) counts 0 in the entropy
    lp = torch.tensor([[0.0, float("-inf")]])
    f, _ = packing.bc_loss_metrics(lp, lp, torch.tensor([0]), torch.tensor([0]))
    assert f[0, :6].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0, 1.0]


# ---------------------------------------------------------------------------------------------------------
# 3b. SequenceBatcher(pad_last=True)
# ---------------------------------------------------------------------------------------------------------
def _video(name, n):
    """Deterministic frames: pixel value encodes (recording, frame index)."""
    base = sum(map(ord, name)) % 200
    return [np.full((H, W, 3), (base + 7 * i) % 256, np.uint8) + np.arange(3, dtype=np.uint8) for i in range(n)]


def _tag_processor(frames, cursor_state):
    """128 x 128 frames that still tell the source frames apart (their first pixel's value), without the cost of the real resize."""
    out = torch.zeros(len(frames), 128, 128, 3, dtype=torch.uint8)
    for i, f in enumerate(frames):
        out[i] = torch.as_tensor(np.asarray(f))[0, 0].to(torch.uint8)
    return out


class CountingEncoder:
    """The numpy oracle's encoder (agent.py's ACTION_TRANSFORMER_KWARGS), recording every action dict it is handed."""

    def __init__(self):
        self.seen = []

    def __call__(self, actions):
        assert all(isinstance(a, dict) and "camera" in a for a in actions)       # a padded item would have no action
        self.seen.append(len(actions))
        camera = np.stack([np.asarray(a["camera"], dtype=np.float64) for a in actions])
        buttons = np.array([[int(a.get(k, 0)) for k in A.BUTTONS_ALL] for a in actions], dtype=np.int64)
        return A.from_factored(buttons, A.discretize(camera, maxval=10, binsize=2, mu=10.0, mu_law=True))


@pytest.fixture()
def dataset(tmp_path):
    lengths = {"a": 23, "b": 9, "c": 40, "d": 15, "e": 31}
    videos = {}
    for k, (name, n) in enumerate(lengths.items()):
        steps = RECS[k % len(RECS)]["steps"][:n]
        with open(tmp_path / f"{name}.jsonl", "w") as f:
            f.write("\n".join(json.dumps(s) for s in steps))
        (tmp_path / f"{name}.mp4").write_bytes(b"")                 # only the name is used: the decoder below is in-memory
        videos[str(tmp_path / f"{name}.mp4")] = _video(name, n if name != "d" else n - 4)
    return tmp_path, videos


def _loader(root, videos, n_workers, seed=3):
    random.seed(seed)
    return clip_loader.DataLoader(str(root), n_workers=n_workers, batch_size=n_workers, n_epochs=2, device="cpu",
                                  decoder=lambda p: iter(videos[p]), frame_processor=_tag_processor, chunk_frames=5)


def _run(root, videos, n_workers, seq_len, **kw):
    enc = CountingEncoder()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sb = SequenceBatcher(_loader(root, videos, n_workers), seq_len, action_encoder=enc, **kw)
        chunks = list(sb)
    return sb, chunks, enc


KEYS = {"img", "first", "act_buttons", "act_camera", "episode_id"}


@pytest.mark.parametrize("n_workers", [2, 3])
@pytest.mark.parametrize("seq_len", [4, 7])
def test_pad_last_keeps_the_tail_chunk(dataset, n_workers, seq_len):
    root, videos = dataset
    sb0, plain, enc0 = _run(root, videos, n_workers, seq_len)
    sb1, padded, enc1 = _run(root, videos, n_workers, seq_len, pad_last=True)
    assert all(set(c) == KEYS for c in plain)                                   # pad_last=False: today's dict, no weight
    assert sb1.dropped_frames == 0
    dropped = sb0.dropped_frames
    assert len(padded) == len(plain) + (1 if dropped else 0) and sb1.n_chunks == len(padded)
    for c0, c1 in zip(plain, padded):                                           # the chunks before the last: key for key, plus weight == 1
        assert set(c1) == KEYS | {"weight"}
        for k in KEYS:
            assert torch.equal(c0[k], c1[k]), k
        assert c1["weight"].dtype == torch.float32 and torch.equal(c1["weight"], torch.ones(n_workers, seq_len))
    with pytest.raises(StopIteration):
        next(sb1)
    if not dropped:
        return
    # the last chunk: exactly the items pad_last=False drops, in lane order, then padding.  What those items are comes from the lanes themselves:
    # the loader's own round-robin up to the first empty lane, minus what the full chunks delivered.
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dl = _loader(root, videos, n_workers)
        lanes, k = [[] for _ in range(n_workers)], 0
        while True:
            item = dl.next_lane_item(k % n_workers)
            if item is None:
                break
            lanes[k % n_workers].append(item)
            k += 1
    done = len(plain) * seq_len
    tail = [lane[done:] for lane in lanes]
    assert sum(len(r) for r in tail) == dropped > 0
    last = padded[-1]
    assert set(last) == KEYS | {"weight"}
    real_actions = []
    for b, r in enumerate(tail):
        n = len(r)
        assert last["weight"][b].tolist() == [1.0] * n + [0.0] * (seq_len - n)
        assert last["episode_id"][b].tolist() == [it[0] for it in r] + [-1] * (seq_len - n)
        if n:
            assert torch.equal(last["img"][b, :n], torch.stack([torch.as_tensor(it[1]) for it in r]))
        assert int(last["img"][b, n:].to(torch.int64).abs().sum()) == 0
        assert bool(last["first"][b, n:].all())
        assert last["act_buttons"][b, n:].tolist() == [0] * (seq_len - n) and last["act_camera"][b, n:].tolist() == [0] * (seq_len - n)
        prev = lanes[b][done - 1][0] if done else None
        for i, it in enumerate(r):                                              # `first` of the real items: a change of recording, as in every chunk
            assert bool(last["first"][b, i]) == (prev is None or it[0] != prev)
            prev = it[0]
        real_actions += [it[2] for it in r]
    wb, wc = CountingEncoder()(real_actions)
    real = last["weight"].reshape(-1) > 0
    assert last["act_buttons"].reshape(-1)[real].tolist() == wb.tolist() and last["act_camera"].reshape(-1)[real].tolist() == wc.tolist()
    # the encoder never saw a padded item: one call per chunk, the last with the real items only
    assert enc1.seen == [n_workers * seq_len] * len(plain) + [dropped]


def test_pad_last_makes_no_all_padding_chunk_when_the_stream_is_a_multiple_of_the_chunk(dataset):
    root, videos = dataset
    exact = 0
    for n_workers, seq_len in ((1, 1), (1, 2), (2, 1), (2, 2), (3, 1)):
        sb0, plain, _ = _run(root, videos, n_workers, seq_len)
        if sb0.dropped_frames:
            continue
        exact += 1                                       # the first empty lane is met at the very start of a chunk
        sb1, padded, _ = _run(root, videos, n_workers, seq_len, pad_last=True)
        assert len(padded) == len(plain) and all(bool((c["weight"] == 1).all()) for c in padded) and sb1.dropped_frames == 0
    assert exact >= 1
