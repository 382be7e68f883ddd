"""labeler.labelled_chunks on CPU tensors: the [B, T] chunks BCTrainer.step trains on, from labelled videos (pure tensor logic)."""
import pytest
import torch

import vpt_amd  # noqa: F401
from vpt_amd.labeler import VideoLabels, labelled_chunks


def _video(n, seed, null_at=()):
    """n frames whose every pixel is the frame's number (+ 100 * seed), and labels that say which frame they belong to."""
    base = 100 * seed
    frames = (torch.arange(n, dtype=torch.int64).view(n, 1, 1, 1) + base).expand(n, 128, 128, 3).to(torch.uint8).contiguous()
    null = torch.zeros(n, dtype=torch.uint8)
    null[list(null_at)] = 1
    lab = VideoLabels(buttons=torch.zeros(n, 20, dtype=torch.int64), camera=torch.full((n, 2), 5, dtype=torch.int64),
                      log_prob=torch.zeros(n), joint_buttons=torch.arange(n) + 1000 * seed + 1, joint_camera=torch.arange(n) + 2000 * seed + 1,
                      camera_deg=torch.zeros(n, 2, dtype=torch.float64), null=null, pd={}, plan=None)
    return frames, lab


def _real_items(chunks, row):
    """The real items of one row over all chunks, concatenated."""
    keep = [c["weight"][row] > 0 for c in chunks]
    cat = lambda key: torch.cat([c[key][row][k] for c, k in zip(chunks, keep)])
    return {key: cat(key) for key in ("img", "first", "act_buttons", "act_camera", "episode_id")}


def _check_padding(chunks):
    for c in chunks:
        pad = c["weight"] == 0
        assert set(c["weight"].unique().tolist()) <= {0.0, 1.0}
        assert not c["img"][pad].any()                       # zero image
        assert c["first"][pad].all()                         # first = True
        assert (c["episode_id"][pad] == -1).all() and (c["episode_id"][~pad] >= 0).all()
        assert (c["act_buttons"][pad] == 0).all() and (c["act_camera"][pad] == 0).all()
        # padding only ever follows the real items of a row
        w = c["weight"]
        assert (w[:, 1:] <= w[:, :-1]).all()


def test_shapes_dtypes_and_keys():
    chunks = list(labelled_chunks([_video(5, 0)], n_rows=2, seq_len=4, drop_null=False))
    assert len(chunks) == 2
    c = chunks[0]
    assert set(c) == {"img", "first", "act_buttons", "act_camera", "episode_id", "weight"}
    assert c["img"].shape == (2, 4, 128, 128, 3) and c["img"].dtype == torch.uint8
    assert c["first"].shape == (2, 4) and c["first"].dtype == torch.bool
    assert c["act_buttons"].dtype == torch.int64 and c["act_camera"].dtype == torch.int64 and c["act_buttons"].shape == (2, 4)
    assert c["episode_id"].dtype == torch.int64 and c["weight"].dtype == torch.float32
    assert c["weight"][1].sum() == 0                         # a row without a video is padding throughout
    _check_padding(chunks)


def test_first_and_episode_id_across_chunk_edges():
    # row 0 plays videos 0 and 2 (5 + 6 frames), row 1 plays video 1 (9 frames); chunks of 4: video 2 starts inside chunk 1 at t = 1
    vids = [_video(5, 0), _video(9, 1), _video(6, 2)]
    chunks = list(labelled_chunks(vids, n_rows=2, seq_len=4, drop_null=False))
    assert len(chunks) == 3
    _check_padding(chunks)
    r0, r1 = _real_items(chunks, 0), _real_items(chunks, 1)
    assert r0["episode_id"].tolist() == [0] * 5 + [2] * 6 and r1["episode_id"].tolist() == [1] * 9
    assert r0["first"].tolist() == [True] + [False] * 4 + [True] + [False] * 5         # the row's first item, and where its video changes
    assert r1["first"].tolist() == [True] + [False] * 8                                # not at a chunk edge inside one video
    assert chunks[1]["first"][0].tolist() == [False, True, False, False] and chunks[1]["first"][1].tolist() == [False] * 4
    assert chunks[2]["weight"].tolist() == [[1, 1, 1, 0], [1, 0, 0, 0]]
    # the concatenation of the real items reproduces each video's frames and labels, in order
    for row, order in ((r0, (0, 2)), (r1, (1,))):
        assert torch.equal(row["img"], torch.cat([vids[i][0] for i in order]))
        assert torch.equal(row["act_buttons"], torch.cat([vids[i][1].joint_buttons for i in order]))
        assert torch.equal(row["act_camera"], torch.cat([vids[i][1].joint_camera for i in order]))


def test_null_frames_are_dropped_or_kept():
    vids = [_video(7, 0, null_at=(0, 3, 6)), _video(4, 1, null_at=(0, 1, 2, 3))]
    kept = list(labelled_chunks(vids, n_rows=2, seq_len=3, drop_null=False))
    assert sum(int(c["weight"].sum()) for c in kept) == 11
    assert _real_items(kept, 0)["act_buttons"].tolist() == vids[0][1].joint_buttons.tolist()     # null frames kept, weight 1
    dropped = list(labelled_chunks(vids, n_rows=2, seq_len=3, drop_null=True))
    assert len(dropped) == 2
    _check_padding(dropped)
    r0 = _real_items(dropped, 0)
    want = [1, 2, 4, 5]
    assert r0["act_buttons"].tolist() == [vids[0][1].joint_buttons[i].item() for i in want]
    assert torch.equal(r0["img"], vids[0][0][want])
    assert r0["first"].tolist() == [True, False, False, False]
    assert sum(int(c["weight"][1].sum()) for c in dropped) == 0                                  # a video of null frames only leaves nothing
    assert list(labelled_chunks([vids[1]], n_rows=1, seq_len=3)) == []                           # ... and alone, no chunk at all


def test_exact_multiple_has_no_padding_and_bad_arguments_raise():
    chunks = list(labelled_chunks([_video(8, 0), _video(8, 1)], n_rows=2, seq_len=4, drop_null=False))
    assert len(chunks) == 2 and all(bool((c["weight"] == 1).all()) for c in chunks)
    with pytest.raises(ValueError):
        labelled_chunks([_video(8, 0)], n_rows=0, seq_len=4)
    with pytest.raises(ValueError):
        labelled_chunks([(torch.zeros(8, 64, 64, 3, dtype=torch.uint8), _video(8, 0)[1])], n_rows=1, seq_len=4)
