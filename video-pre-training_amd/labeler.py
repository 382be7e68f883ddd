"""Pseudo-labelling with the inverse dynamics model, and training chunks from the labels  (`from vpt_amd.labeler import ...`).

The link of the VPT method between the IDM and the BC trainer: `InverseActionPolicy.label_video(frames)` labels a whole recording on the
device (IDMEngine.forward_windows: overlapping windows, every frame labelled by the window in which it is most central) and returns a
`VideoLabels`; `labelled_chunks` turns labelled recordings into the [B, T] chunks `training.BCTrainer.step` trains on -- the dict
`SequenceBatcher(pad_last=True)` yields.  Nothing here goes to the host: the reference pulls every prediction through `.cpu().numpy()`
(inverse_dynamics_model.py:61-72) and the contractor loader re-reads actions from json (data_loader.py:48-128)."""
from dataclasses import dataclass
from typing import Any, Dict, Iterator, Sequence, Tuple

import torch


@dataclass
class VideoLabels:
    """The labels of one video of N frames (all tensors on the model's device).
      buttons        int64 [N, 20]  the IDM's factored buttons in Buttons.ALL order (arg-max per button, lowest index on ties)
      camera         int64 [N, 2]   camera bins
      log_prob       fp32  [N]      log-probability of the chosen action: a confidence a caller may threshold
      joint_buttons, joint_camera   int64 [N]  the policy's joint action indices (CameraHierarchicalMapping.from_factored): BC targets
      camera_deg     fp64  [N, 2]   the camera bins as angles (CameraQuantizer.undiscretize, mu-law)
      null           uint8 [N]      1 where nothing is pressed and the camera rests: the frames the reference's loader drops
      pd             {"buttons": fp32 [N, 20, 2], "camera": fp32 [N, 2, n_bins]}  the stitched log-probs the labels were read from
      plan           packing.IDMFeaturePlan: windows, the window that labelled each frame (owner), the feature slots"""
    buttons: torch.Tensor
    camera: torch.Tensor
    log_prob: torch.Tensor
    joint_buttons: torch.Tensor
    joint_camera: torch.Tensor
    camera_deg: torch.Tensor
    null: torch.Tensor
    pd: Dict[str, torch.Tensor]
    plan: Any

    def __len__(self):
        return self.buttons.shape[0]


def labelled_chunks(videos: Sequence[Tuple[torch.Tensor, VideoLabels]], n_rows: int, seq_len: int, drop_null: bool = True, *, augment=None) -> Iterator[dict]:
    """[B = n_rows, T = seq_len] training chunks from labelled videos: a list of (frames uint8 [N,128,128,3], VideoLabels).

    Video i goes to row i % n_rows; a row plays its videos one after the other.  drop_null=True removes the null-labelled frames first, as the
    reference's loader drops null actions (data_loader.py:48-128); False keeps them, with weight 1 like every real frame.  Each chunk is the dict
    `SequenceBatcher(pad_last=True)` yields:
      img          uint8 [B, T, 128, 128, 3]
      first        bool  [B, T]   true at a row's very first item and wherever its video changes (across chunk edges too)
      act_buttons, act_camera     int64 [B, T]  the labels' joint indices
      episode_id   int64 [B, T]   the video's position in `videos`
      weight       fp32  [B, T]   1 for a frame, 0 for padding (BCTrainer.step's `frame_weight`)
    A row that has run out of frames is padded as SequenceBatcher._padded_chunk pads: zero image, first = True, action indices 0,
    episode_id = -1, weight = 0.  Unlike the loader's protocol, which stops at the first empty lane, iteration goes on until EVERY row is
    empty, so each kept frame of each video appears exactly once, in order.  Pure tensor logic: runs on whatever device the inputs are on.
    augment: optional callable chunk dict -> chunk dict applied to every chunk (augment.FrameAugmenter: one image transform per video, keyed by
    episode_id; padding frames stay as they are).  None: the chunks are what they were."""
    n_rows, seq_len = int(n_rows), int(seq_len)
    if n_rows < 1 or seq_len < 1:
        raise ValueError("labelled_chunks: n_rows and seq_len must be at least 1")
    videos = list(videos)
    for i, (frames, lab) in enumerate(videos):
        if frames.dtype != torch.uint8 or frames.dim() != 4 or tuple(frames.shape[1:]) != (128, 128, 3) or frames.shape[0] != len(lab):
            raise ValueError(f"labelled_chunks: video {i}: frames must be uint8 [{len(lab)},128,128,3], got {frames.dtype} {tuple(frames.shape)}")
    chunks = _chunks(videos, n_rows, seq_len, bool(drop_null))
    return chunks if augment is None else (augment(c) for c in chunks)


def _chunks(videos, n_rows, seq_len, drop_null):
    if not videos:
        return
    dev = videos[0][0].device
    rows = [dict(img=[], jb=[], jc=[], id=[]) for _ in range(n_rows)]
    for i, (frames, lab) in enumerate(videos):
        keep = (lab.null == 0) if drop_null else torch.ones_like(lab.null, dtype=torch.bool)
        r = rows[i % n_rows]
        r["img"].append(frames[keep])
        r["jb"].append(lab.joint_buttons[keep])
        r["jc"].append(lab.joint_camera[keep])
        r["id"].append(torch.full((int(keep.sum()),), i, dtype=torch.int64, device=dev))
    streams = []
    for r in rows:
        if r["id"]:
            ids = torch.cat(r["id"])
            prev = torch.cat([torch.full((1,), -1, dtype=torch.int64, device=dev), ids[:-1]])
            streams.append(dict(img=torch.cat(r["img"]), jb=torch.cat(r["jb"]), jc=torch.cat(r["jc"]), id=ids, first=ids != prev))
        else:
            streams.append(None)
    longest = max((s["id"].numel() for s in streams if s is not None), default=0)
    for c in range(0, longest, seq_len):
        img = torch.zeros(n_rows, seq_len, 128, 128, 3, dtype=torch.uint8, device=dev)
        first = torch.ones(n_rows, seq_len, dtype=torch.bool, device=dev)
        acts = torch.zeros(2, n_rows, seq_len, dtype=torch.int64, device=dev)
        ids = torch.full((n_rows, seq_len), -1, dtype=torch.int64, device=dev)
        weight = torch.zeros(n_rows, seq_len, dtype=torch.float32, device=dev)
        for b, s in enumerate(streams):
            m = 0 if s is None else max(0, min(seq_len, s["id"].numel() - c))
            if m:
                img[b, :m], first[b, :m], ids[b, :m], weight[b, :m] = s["img"][c:c + m], s["first"][c:c + m], s["id"][c:c + m], 1.0
                acts[0, b, :m], acts[1, b, :m] = s["jb"][c:c + m], s["jc"][c:c + m]
        yield dict(img=img, first=first, act_buttons=acts[0], act_camera=acts[1], episode_id=ids, weight=weight)
