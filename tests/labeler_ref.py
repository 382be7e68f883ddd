"""The CPU reference of the IDM video labeller's tests  --  TEST INFRASTRUCTURE.

The tiny IDM (uniform synthetic heads, temperature 2.0) on tests.parity.structured_frames, run by the oracle one window at a time and
stitched with packing.label_windows: what InverseActionPolicy.label_video must reproduce.  Computed once per (frames, window, stride)
and shared by every test that needs it; callers must not modify what they get."""
import functools

import torch

from oracle import vpt_oracle as O
from tests import parity as P
from vpt_amd import packing

TEMPERATURE = 2.0


@functools.lru_cache(maxsize=None)
def tiny_idm():
    """-> (constructor kwargs, oracle config, synthetic state dict) of the structure-preserving tiny IDM, seed 0, uniform heads."""
    kw = O.idm_kwargs_for("tiny")
    cfg = O.idm_config_from_kwargs(kw, dict(temperature=TEMPERATURE))
    return kw, cfg, O.idm_synthetic_state_dict(cfg, seed=0, heads="uniform")


@functools.lru_cache(maxsize=None)
def video(n_frames: int, seed: int = 42):
    """uint8 [n_frames, 128, 128, 3]: low-frequency frames whose latent moves from frame to frame."""
    return P.structured_frames(1, n_frames, torch.Generator().manual_seed(seed))[0]


def stitch(per_window, n_frames, window, stride):
    """per_window: list over windows of {"buttons": [L, 20, 2], "camera": [L, 2, n]} -> the same dict with [n_frames, ...] rows, every frame
    taken from the window packing.label_windows assigns it to."""
    starts, length, owner = packing.label_windows(n_frames, window, stride)
    assert len(per_window) == starts.numel()
    out = {}
    for h in ("buttons", "camera"):
        out[h] = torch.stack([per_window[int(owner[f])][h][f - int(starts[int(owner[f])])] for f in range(n_frames)])
    return out


@functools.lru_cache(maxsize=None)
def stitched_oracle(n_frames: int, window: int, stride: int, edge_blind: bool = False):
    """The oracle's log-probs of video(n_frames), window by window (O.idm_forward on each window's own pixels), stitched.
    edge_blind=True is the WRONG labeller a test must be able to tell from the right one: the temporal conv runs once over the whole
    video, so a window's first and last two frames see neighbours from outside the window instead of its zero padding."""
    _, cfg, sd = tiny_idm()
    frames = video(n_frames)
    starts, length, _ = packing.label_windows(n_frames, window, stride)
    per_window = []
    if edge_blind:
        with torch.no_grad():
            whole = O.conv3d_temporal(sd, frames[None].to(torch.float32) / 255.0)
    real_conv = O.conv3d_temporal
    try:
        for s in starts.tolist():
            if edge_blind:
                O.conv3d_temporal = lambda sd_, x, s=s: whole[:, s:s + length]
            out = O.idm_forward(sd, cfg, frames[None, s:s + length])
            per_window.append({h: out[h][0] for h in ("buttons", "camera")})
    finally:
        O.conv3d_temporal = real_conv
    return stitch(per_window, n_frames, window, stride)
