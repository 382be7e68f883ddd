"""[B, T] training chunks from the contractor loader  (`from vpt_amd.sequence_batcher import SequenceBatcher`).

`clip_loader.DataLoader` yields the reference's protocol: one kept frame per lane per batch, for its T = 1 loop
(behavioural_cloning.py:86-122).  The fused step (`training.BCTrainer.step`) wants [B, T] chunks.  A SequenceBatcher turns the one
into the other: row b of every chunk is the loader's lane b, T consecutive kept frames of it.  Recordings have arbitrary lengths
after the null-action filter, so a row moves to its next recording anywhere inside a chunk; `first[b, t]` marks those frames, and a
trainer built with `episode_starts="frame"` keeps attention from crossing them -- which is what the reference's loop computes with
its one hidden state per episode (behavioural_cloning.py:95-112)."""
from typing import Callable, List, Optional

import numpy as np
import torch

CAMERA_MAXVAL, CAMERA_BINSIZE, CAMERA_MU = 10, 2, 10        # agent.py ACTION_TRANSFORMER_KWARGS (mu-law quantisation)
N_CAMERA_BINS = 11


def default_action_encoder(device) -> Callable[[List[dict]], tuple]:
    """env actions -> (joint buttons int64 [N], joint camera int64 [N]) on `device`: ActionTransformer.env2policy (lib/actions.py:
    171-178) followed by CameraHierarchicalMapping.from_factored (lib/action_mapping.py:179-207), one codec launch each for
    the whole chunk (vpt_camera_discretize, vpt_action_from_factored)."""
    from . import ops
    from .lib.actions import Buttons

    def encode(actions: List[dict]):
        camera = np.stack([np.asarray(a["camera"], dtype=np.float64).reshape(2) for a in actions])
        buttons = np.array([[int(a.get(k, 0)) for k in Buttons.ALL] for a in actions], dtype=np.int64)
        bins = ops.camera_discretize(torch.from_numpy(camera).to(device), CAMERA_MAXVAL, CAMERA_BINSIZE, CAMERA_MU, True)
        return ops.action_from_factored(torch.from_numpy(buttons).to(device), bins, N_CAMERA_BINS)

    return encode


class SequenceBatcher:
    """Iterates over a `clip_loader.DataLoader` in [B, T] chunks; B = loader.n_workers (one row per lane), T = seq_len.  The
    loader's `batch_size` belongs to its own round-robin iteration and does not apply here; do not iterate the loader itself while
    a batcher draws from it.

    Each iteration returns a dict:
      img          uint8 [B, T, 128, 128, 3] on the loader's device
      first        bool  [B, T]: the item's trajectory id differs from the previous item of that row -- across chunk edges too, and
                   true for the very first item of every row.  With it, feeding `state_out` of one BCTrainer.step (built with
                   episode_starts="frame") as `state_in` of the next needs no bookkeeping by the caller.
      act_buttons, act_camera   int64 [B, T]: the policy's joint action indices
      episode_id   int64 [B, T]: the loader's trajectory ids

    action_encoder: callable list[dict] -> (buttons [N], camera [N]) (tensors or arrays); default: default_action_encoder on the
    loader's device.  Iteration ends when any lane cannot supply its T items (the reference stops at the first empty lane,
    data_loader.py:198-217); the incomplete chunk is dropped and its items are counted in `dropped_frames`.

    pad_last=True keeps that chunk instead: every chunk also carries `weight` fp32 [B, T] (BCTrainer's `frame_weight`; all ones for a full
    chunk), and when a lane runs dry the chunk in progress is completed with padding -- zero image, first = True, action indices 0,
    episode_id = -1, weight = 0 -- and returned if it holds at least one real item; the next iteration stops.  `dropped_frames` stays 0, and
    only real items reach the action encoder.

    augment: optional callable chunk dict -> chunk dict applied to every chunk before it is returned (augment.FrameAugmenter: one image transform
    per recording, keyed by episode_id, so it holds across chunk edges; padding frames stay as they are).  None: the chunks are what they were."""

    def __init__(self, loader, seq_len: int, action_encoder: Optional[Callable] = None, pad_last: bool = False, *, augment: Optional[Callable] = None):
        if int(seq_len) < 1:
            raise ValueError("seq_len must be at least 1")
        if getattr(loader, "to_numpy", False):
            raise ValueError("SequenceBatcher needs the loader's frames as tensors (to_numpy=False)")
        self.loader = loader
        self.seq_len = int(seq_len)
        self.pad_last = bool(pad_last)
        self.augment = augment
        self.n_rows = loader.n_workers
        self.device = torch.device(loader._device)
        self._encode = action_encoder or default_action_encoder(self.device)
        self._last_id = [None] * self.n_rows
        self.dropped_frames = 0
        self.n_chunks = 0
        self._done = False

    def __iter__(self):
        return self

    def __next__(self):
        chunk = self._next_chunk()
        return chunk if self.augment is None else self.augment(chunk)

    def _next_chunk(self):
        if self._done:
            raise StopIteration()
        # lanes are served round-robin, one item at a time, exactly as the loader's own iteration serves them: a lane asks for its next
        # recording at the same point of the schedule, so row b IS the loader's lane b
        rows = [[] for _ in range(self.n_rows)]
        for _ in range(self.seq_len):
            for b in range(self.n_rows):
                item = self.loader.next_lane_item(b)
                if item is None:
                    self._done = True
                    if self.pad_last and any(rows):
                        return self._padded_chunk(rows)
                    self.dropped_frames += sum(len(r) for r in rows)
                    raise StopIteration()
                rows[b].append(item)
        chunk = self._chunk(rows)
        if self.pad_last:
            chunk["weight"] = torch.ones(self.n_rows, self.seq_len, dtype=torch.float32, device=self.device)
        return chunk

    def _chunk(self, rows):
        """A full chunk from `rows` (T items per lane)."""
        bsz, t = self.n_rows, self.seq_len
        ids = torch.tensor([[it[0] for it in r] for r in rows], dtype=torch.int64)
        prev = torch.tensor([[-1 if p is None else p] for p in self._last_id], dtype=torch.int64)
        first = ids != torch.cat([prev, ids[:, :-1]], dim=1)
        for b in range(bsz):
            if self._last_id[b] is None:
                first[b, 0] = True
            self._last_id[b] = rows[b][-1][0]
        img = torch.stack([torch.as_tensor(it[1]) for r in rows for it in r]).to(self.device).view(bsz, t, 128, 128, 3)
        buttons, camera = self._encode([it[2] for r in rows for it in r])
        to_bt = lambda x: torch.as_tensor(x).to(device=self.device, dtype=torch.int64).reshape(bsz, t)
        self.n_chunks += 1
        return dict(img=img, first=first.to(self.device), act_buttons=to_bt(buttons), act_camera=to_bt(camera), episode_id=ids.to(self.device))

    def _padded_chunk(self, rows):
        """The last, incomplete chunk (pad_last): the real items of every lane followed by padding."""
        bsz, t = self.n_rows, self.seq_len
        ids = torch.full((bsz, t), -1, dtype=torch.int64)
        first = torch.ones(bsz, t, dtype=torch.bool)
        weight = torch.zeros(bsz, t, dtype=torch.float32)
        img = torch.zeros(bsz, t, 128, 128, 3, dtype=torch.uint8, device=self.device)
        for b, r in enumerate(rows):
            prev = self._last_id[b]
            for i, it in enumerate(r):
                ids[b, i], first[b, i], weight[b, i] = it[0], prev is None or it[0] != prev, 1.0
                img[b, i] = torch.as_tensor(it[1]).to(self.device)
                prev = it[0]
            self._last_id[b] = prev
        real = weight.reshape(-1) > 0
        acts = torch.zeros(2, bsz * t, dtype=torch.int64, device=self.device)
        buttons, camera = self._encode([it[2] for r in rows for it in r])        # real items only, in lane order
        where = real.to(self.device)
        acts[0, where] = torch.as_tensor(buttons).to(device=self.device, dtype=torch.int64).reshape(-1)
        acts[1, where] = torch.as_tensor(camera).to(device=self.device, dtype=torch.int64).reshape(-1)
        self.n_chunks += 1
        return dict(img=img, first=first.to(self.device), act_buttons=acts[0].view(bsz, t), act_camera=acts[1].view(bsz, t),
                    episode_id=ids.to(self.device), weight=weight.to(self.device))
