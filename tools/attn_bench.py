"""Time the attention entry points alone, at the shapes of the workloads.  Needs an MI355X.
python tools/attn_bench.py [--reps 20] [--rounds 7] [--warmup 3]

  masked_attention, masked_attention_backward   the 2x model's BC shape: B 64, t 128, maxlen 128, heads 16, hid 2048 (vpt_attn_kernel;
                                                vpt_attn_bwd_kernel + its finish kernel + the db_nd slab sum)
  full_attention, full_attention_backward       the 4x inverse-dynamics model's window: B 8, t 128, heads 32, hid 4096 (vpt_attn_kernel with mask
                                                "none"; vpt_full_attn_bwd_kernel + its finish kernel)

Inputs are attention_ref.real_case's distributions (randn, q scaled by 2, 30 % of the memory rows invalid) seeded on the device.  After --warmup
launches of each, the entry points take turns inside every round; a timing is --reps launches back to back between two HIP events, divided by
--reps.  The last line is one JSON record: median, min and max over the rounds per entry point, in ms per launch, and the box's clock while it ran.
VPT_HIP_LIB names another build of the bf16 library (an A/B against the parent commit: one fresh process per library and round, alternating, in
one session -- boxes differ by several per cent)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import vpt_amd  # noqa: E402,F401
from bench import BoxSampler  # noqa: E402
from vpt_amd import _native, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()
dev = "cuda"
dt = torch.bfloat16         # the library VPT_HIP_LIB replaces
g = torch.Generator(device=dev).manual_seed(0)


def randn(*shape):
    return torch.randn(*shape, generator=g, device=dev)


# ---- the 2x model's BC shape (banded attention over [memory ; chunk]) ----
B, T, ML, H = 64, 128, 128, 16
HID = H * 128
qkvr = randn(B * T, 3 * HID + 10 * H)
qkvr[:, :HID] *= 2.0
dout = randn(B * T, HID)
kmem, vmem = randn(B, ML, HID), randn(B, ML, HID)
memvalid = (torch.rand(B, ML, generator=g, device=dev) > 0.3).to(torch.uint8)
b_nd = 0.5 * randn(10, ML)
db_nd = torch.zeros(10, ML, device=dev)
# ---- the 4x inverse-dynamics model's window (mask "none") ----
FB, FT, FH = 8, 128, 32
FHID = FH * 128
qkv = randn(FB * FT, 3 * FHID)
qkv[:, :FHID] *= 2.0
fdout = randn(FB * FT, FHID)

entries = {
    "masked_attention": lambda: ops.masked_attention(qkvr, kmem, vmem, memvalid, b_nd, B, T, H, HID, dtype=dt),
    "masked_attention_backward": lambda: ops.masked_attention_backward(qkvr, kmem, vmem, memvalid, b_nd, dout, db_nd, B, T, H, HID),
    "full_attention": lambda: ops.full_attention(qkv, FB, FT, FH, FHID, dtype=dt),
    "full_attention_backward": lambda: ops.full_attention_backward(qkv, fdout, FB, FT, FH, FHID),
}
for fn in entries.values():
    for _ in range(a.warmup):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in entries}
with BoxSampler(torch.cuda.current_device()) as box:
    for _ in range(a.rounds):
        for k, fn in entries.items():
            fn()                 # one un-timed launch after every switch of entry point
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.reps)
lib = _native.lib_path()
rec = dict(library=os.path.join(os.path.basename(os.path.dirname(lib)), os.path.basename(lib)),
           reps=a.reps, rounds=a.rounds, warmup=a.warmup, shapes=dict(masked=dict(B=B, t=T, maxlen=ML, heads=H, hid=HID), full=dict(B=FB, t=FT, heads=FH, hid=FHID)),
           box=box.record())
for k, v in times.items():
    v = sorted(v)
    rec[k] = dict(ms_median=round(v[len(v) // 2], 4), ms_min=round(v[0], 4), ms_max=round(v[-1], 4))
    print(f"{k:28s} {rec[k]['ms_median']:8.4f} ms per launch (min {v[0]:.4f}, max {v[-1]:.4f})")
print(json.dumps(rec))
