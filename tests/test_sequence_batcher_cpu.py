"""vpt_amd.sequence_batcher.SequenceBatcher on the CPU: the synthetic recordings of tests/test_clip_loader_cpu.py, an in-memory decoder, the
oracle as frame processor and oracle/action_codec.py as action encoder.  Row b of the chunks is the loader's lane b; `first` marks every
change of recording, chunk edges and the very first item included; an incomplete last chunk is dropped and counted."""
import gzip
import json
import os
import random
import warnings

import numpy as np
import pytest
import torch

import vpt_amd  # noqa: F401
from vpt_amd import clip_loader
from vpt_amd.sequence_batcher import SequenceBatcher
from oracle import action_codec as A
from oracle import clip_oracle as C

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = dict(np.load(os.path.join(GOLD, "clip_seed0.npz")))
with gzip.open(os.path.join(GOLD, "clip_actions_seed0.json.gz"), "rt") as fh:
    RECS = json.load(fh)
H, W = 36, 64


def _video(name, n):
    """Deterministic frames: pixel value encodes (recording, frame index)."""
    base = sum(map(ord, name)) % 200
    return [np.full((H, W, 3), (base + 7 * i) % 256, np.uint8) + np.arange(3, dtype=np.uint8) for i in range(n)]


def _oracle_processor(frames, cursor_state):
    cur = G["cursor_bgra"]
    alpha, image = cur[:16, :16, 3:] / 255.0, cur[:16, :16, :3]
    out = [C.process_frame(f.numpy(), bool(s[0]), int(s[1]), int(s[2]), image, alpha) for f, s in zip(frames, cursor_state)]
    return torch.from_numpy(np.stack(out)) if out else torch.zeros(0, 128, 128, 3, dtype=torch.uint8)


def oracle_encoder(actions):
    """env actions -> joint indices with the numpy oracle (agent.py's ACTION_TRANSFORMER_KWARGS: maxval 10, binsize 2, mu-law mu 10)."""
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
        videos[str(tmp_path / f"{name}.mp4")] = _video(name, n if name != "d" else n - 4)   # "d": the video ends 4 frames early
    return tmp_path, lengths, videos


def _blank_processor(frames, cursor_state):
    """For the tests that look at ids and flags only."""
    return torch.zeros(len(frames), 128, 128, 3, dtype=torch.uint8)


def _loader(root, videos, n_workers, seed=3, processor=_oracle_processor):
    random.seed(seed)
    return clip_loader.DataLoader(str(root), n_workers=n_workers, batch_size=n_workers, n_epochs=2, device="cpu",
                                  decoder=lambda p: iter(videos[p]), frame_processor=processor, chunk_frames=5)


def _lane_streams(root, videos, n_workers, seed=3):
    """Lane b's item stream, from the loader's own round-robin iteration (batch_size = n_workers: item k of a batch is lane k's)."""
    lanes = [[] for _ in range(n_workers)]
    for frames, actions, ids in _loader(root, videos, n_workers, seed):
        for b in range(n_workers):
            lanes[b].append((ids[b], frames[b], actions[b]))
    return lanes


def _run(root, videos, n_workers, seq_len, seed=3, processor=_oracle_processor):
    sb = SequenceBatcher(_loader(root, videos, n_workers, seed, processor), seq_len, action_encoder=oracle_encoder)
    return sb, list(sb)


@pytest.mark.parametrize("n_workers", [2, 3])
@pytest.mark.parametrize("seq_len", [4, 7])
def test_rows_are_lanes_and_first_marks_every_change_of_recording(dataset, n_workers, seq_len):
    root, lengths, videos = dataset
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lanes = _lane_streams(root, videos, n_workers)
        sb, chunks = _run(root, videos, n_workers, seq_len)
    assert sb.n_rows == n_workers and len(chunks) == sb.n_chunks >= 2
    where = set()
    for c in chunks:
        assert c["img"].dtype == torch.uint8 and tuple(c["img"].shape) == (n_workers, seq_len, 128, 128, 3)
        assert c["first"].dtype == torch.bool and tuple(c["first"].shape) == (n_workers, seq_len)
        for k in ("act_buttons", "act_camera", "episode_id"):
            assert c[k].dtype == torch.int64 and tuple(c[k].shape) == (n_workers, seq_len), k
    for b in range(n_workers):
        ids = torch.cat([c["episode_id"][b] for c in chunks]).tolist()
        img = torch.cat([c["img"][b] for c in chunks])
        first = torch.cat([c["first"][b] for c in chunks]).tolist()
        n = len(ids)
        want = lanes[b][:n]
        assert len(want) == n                                      # the batcher never runs ahead of the loader's own stop
        assert ids == [w[0] for w in want]
        assert torch.equal(img, torch.stack([torch.as_tensor(w[1]) for w in want]))
        wb, wc = oracle_encoder([w[2] for w in want])
        assert torch.cat([c["act_buttons"][b] for c in chunks]).tolist() == wb.tolist()
        assert torch.cat([c["act_camera"][b] for c in chunks]).tolist() == wc.tolist()
        assert first == [k == 0 or ids[k] != ids[k - 1] for k in range(n)]
        where |= {"start" if k % seq_len == 0 else ("end" if k % seq_len == seq_len - 1 else "mid") for k in range(1, n) if first[k]}
    assert "mid" in where                                          # recordings change inside chunks, not only at their edges


def test_boundaries_fall_on_chunk_starts_chunk_ends_and_mid_chunk(dataset):
    root, lengths, videos = dataset
    where = set()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for n_workers in (2, 3):
            for seq_len in (4, 7):
                for seed in (3, 4, 5):
                    _, chunks = _run(root, videos, n_workers, seq_len, seed, processor=_blank_processor)
                    for ci, c in enumerate(chunks):
                        f = c["first"]
                        assert bool(f[:, 0].all()) if ci == 0 else True
                        if ci > 0 and bool(f[:, 0].any()):
                            where.add("start")
                        if bool(f[:, -1].any()):
                            where.add("end")
                        if bool(f[:, 1:-1].any()):
                            where.add("mid")
    assert where == {"start", "end", "mid"}


@pytest.mark.parametrize("n_workers,seq_len", [(2, 4), (3, 7)])
def test_stop_rule_and_dropped_frames(dataset, n_workers, seq_len):
    """Iteration ends when a lane cannot supply its item; what the incomplete chunk had collected is dropped and counted, so
    delivered + dropped = what the loader's own lanes handed out before the first empty one."""
    root, lengths, videos = dataset
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dl = _loader(root, videos, n_workers, processor=_blank_processor)
        total = 0
        while True:                                               # the lanes' items, round-robin, up to the first empty lane
            if dl.next_lane_item(total % n_workers) is None:
                break
            total += 1
        sb, chunks = _run(root, videos, n_workers, seq_len, processor=_blank_processor)
    delivered = len(chunks) * n_workers * seq_len
    assert delivered + sb.dropped_frames == total
    assert 0 <= sb.dropped_frames < n_workers * seq_len
    with pytest.raises(StopIteration):
        next(sb)
    assert delivered + sb.dropped_frames == total                  # a second StopIteration drops nothing more


def test_deterministic_under_random_seed(dataset):
    root, lengths, videos = dataset
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, a = _run(root, videos, 3, 4, seed=11)
        _, b = _run(root, videos, 3, 4, seed=11)
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert set(x) == set(y) == {"img", "first", "act_buttons", "act_camera", "episode_id"}
        for k in x:
            assert torch.equal(x[k], y[k]), k


def test_argument_checks(dataset):
    root, lengths, videos = dataset
    with pytest.raises(ValueError):
        SequenceBatcher(_loader(root, videos, 2), 0, action_encoder=oracle_encoder)
