"""Can the labeller's GPU tests see the mistakes they are there for?  Checked with the CPU oracle alone (tests/labeler_ref.py).

tests/test_gpu_labeler.py holds label_video to the stitched oracle within max-abs 3e-2 (bf16) / 4e-3 (fp16).  Two mistakes a labeller that
shares per-frame features can make must move the stitched log-probs by more than the looser of those: ignoring the temporal conv's zero
padding at the window edges, and taking a frame's answer from the wrong window."""
import torch

from tests import labeler_ref as R
from vpt_amd import packing

N, L, S = 31, 12, 6
LOOSEST_TOL = 3e-2


def test_edge_blind_features_are_visible_above_the_gpu_tolerances():
    right = R.stitched_oracle(N, L, S)
    wrong = R.stitched_oracle(N, L, S, edge_blind=True)
    for h in ("buttons", "camera"):
        d = float((right[h] - wrong[h]).abs().max())
        print(f"edge-blind labeller, {h}: max|d| {d:.3f}")
        assert d > LOOSEST_TOL, (h, d)


def test_the_choice_of_window_is_visible_above_the_gpu_tolerances():
    """The same frame seen from its two windows differs by far more than the tolerance: a wrong `sel_rows` cannot hide."""
    _, cfg, sd = R.tiny_idm()
    frames = R.video(N)
    starts, length, owner = packing.label_windows(N, L, S)
    from oracle import vpt_oracle as O
    a = O.idm_forward(sd, cfg, frames[None, 0:length])["buttons"][0]           # window 0: frames 0..11
    b = O.idm_forward(sd, cfg, frames[None, S:S + length])["buttons"][0]       # window 1: frames 6..17
    both = float((a[S:] - b[:length - S]).abs().max())                        # frames 6..11 from either window
    print(f"one frame from two windows: max|d| {both:.3f}")
    assert both > LOOSEST_TOL, both


def test_the_input_carries_distinct_decisions():
    """Uniform heads on structured frames: the arg-max differs from frame to frame (with peaked heads every frame decides alike, and a
    labeller that returned one frame's labels everywhere would pass an arg-max comparison)."""
    right = R.stitched_oracle(N, L, S)
    rows_b = {tuple(r.tolist()) for r in right["buttons"].argmax(-1)}
    rows_c = {tuple(r.tolist()) for r in right["camera"].argmax(-1)}
    print(f"distinct button rows {len(rows_b)}, camera rows {len(rows_c)}")
    assert len(rows_b) >= 16 and len(rows_c) >= 8
