"""Labelling throughput of the 4x inverse-dynamics model over a whole video: shared per-frame features against window by window.
python tools/label_bench.py [--frames 1024] [--window 128] [--stride 64] [--rounds 5] [--model 4x] [--out label_bench.json]

Both paths of IDMEngine.forward_windows in ONE process per precision, after a warm-up of each, alternating (shared, per-window, shared, ...)
so that a drift of the box's clock hits both alike; every pass is timed with HIP events around the whole call (plan upload, kernels, decode).
The spread reported is the per-window path's own (max - min) / median over its rounds: the shared path is called faster only if it wins by
more than twice that.  Outputs of the two paths are compared on the timed input (labels and log-probs, bit for bit).  Prints one JSON line
per precision; needs a GPU."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

torch.set_grad_enabled(False)
import __graft_entry__ as ge

ge.build()
from bench import BoxSampler
from vpt_amd import configs, packing
from vpt_amd.lib.policy import InverseActionPolicy
from vpt_amd.lib.types import idm_action_space

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1024)
ap.add_argument("--window", type=int, default=128)
ap.add_argument("--stride", type=int, default=64)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--model", default="4x")
ap.add_argument("--precisions", default="bf16,fp16")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("label_bench: no GPU (a labelling rate is a GPU measurement; there is no CPU figure)")

plan = packing.idm_feature_plan(a.frames, a.window, a.stride)
n_win = plan.starts.numel()
slot_ratio = plan.src.numel() / (n_win * plan.length)
g = torch.Generator().manual_seed(1)
frames = torch.randint(0, 256, (a.frames, 128, 128, 3), generator=g, dtype=torch.uint8).to("cuda")
results = []
for prec in a.precisions.split(","):
    pol = InverseActionPolicy(idm_action_space(), pi_head_kwargs=dict(temperature=2.0), idm_net_kwargs=configs.idm_kwargs_for(a.model), precision=prec)
    configs.randomize_(pol, 0)
    pol = pol.to("cuda")
    run = lambda share: pol.label_video(frames, window=a.window, stride=a.stride, share_features=share)
    ref = {share: run(share) for share in (True, False)}           # warm-up: every shape of the timed passes, both paths
    torch.cuda.synchronize()
    same = all(torch.equal(getattr(ref[True], k), getattr(ref[False], k)) for k in ("buttons", "camera", "log_prob", "joint_buttons", "joint_camera", "null"))
    max_d = max(float((ref[True].pd[h] - ref[False].pd[h]).abs().max()) for h in ("buttons", "camera"))
    ms = {True: [], False: []}
    with BoxSampler(torch.cuda.current_device()) as box:
        for _ in range(a.rounds):
            for share in (True, False):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(share)
                e1.record()
                e1.synchronize()
                ms[share].append(e0.elapsed_time(e1))
    med = {s: statistics.median(v) for s, v in ms.items()}
    spread = (max(ms[False]) - min(ms[False])) / med[False]
    ratio = med[False] / med[True]
    rec = dict(tool="label_bench", model=a.model, precision=prec, frames=a.frames, window=a.window, stride=a.stride, windows=n_win, slots=plan.src.numel(),
               slots_over_window_rows=round(slot_ratio, 4), rounds=a.rounds,
               shared_frames_per_s=round(a.frames / med[True] * 1e3, 1), per_window_frames_per_s=round(a.frames / med[False] * 1e3, 1),
               shared_ms=[round(x, 2) for x in ms[True]], per_window_ms=[round(x, 2) for x in ms[False]],
               speedup_shared_over_per_window=round(ratio, 4), per_window_spread=round(spread, 4), shared_wins=bool(ratio - 1.0 > 2.0 * spread),
               labels_bit_equal=bool(same), logprob_max_abs_diff=max_d, box=box.record())
    print(json.dumps(rec), flush=True)
    results.append(rec)
    del pol, ref
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
