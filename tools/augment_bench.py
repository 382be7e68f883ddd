"""Time the frame augmentation (vpt_augment_frames) against its floor and against the torch route it replaces, interleaved in ONE process.
python tools/augment_bench.py [--batch 64] [--seq 128] [--rounds 5] [--window 0.5] [--bc-steps 3] [--model 2x]

  kernel      ops.augment_frames on uint8 [B, T, 128, 128, 3] with per-recording tables: one read and one write of the frames
  copy        out.copy_(img) of the same tensor: the floor for one read plus one write
  torch       what a user had to write before: uint8 -> fp32 NCHW, affine_grid / grid_sample (bilinear, zeros), colour matmul + mean term, clamp, round, uint8 NHWC
  tables      FrameAugmenter.tables for the chunk's keys: the uniforms kernel + the float64 torch-op builder

Every variant is warmed, then the variants take turns inside every round; a turn is a window of back-to-back calls between two HIP events, sized from the
warm-up to last at least --window seconds.  Peak memory (beyond the resident input, tables and output) is taken for kernel and torch in runs of their own.
With --bc-steps > 0 a BCTrainer step of --model at the same [B, T] is timed too, for the augmentation's share of a training step.  The last line is one JSON record."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import __graft_entry__ as ge
ge.build()
from vpt_amd import ops, configs
from vpt_amd.augment import FrameAugmenter

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64); ap.add_argument("--seq", type=int, default=128); ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window", type=float, default=0.5); ap.add_argument("--bc-steps", type=int, default=3); ap.add_argument("--model", default="2x")
a = ap.parse_args()
dev = "cuda"
B, T, H, W = a.batch, a.seq, 128, 128
F = B * T
g = torch.Generator().manual_seed(1)
img = torch.randint(0, 256, (B, T, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
keys = (torch.arange(B, dtype=torch.int64)[:, None] * 3 + torch.arange(T)[None, :] // 50).to(dev).contiguous()      # a row changes recording every 50 frames
aug = FrameAugmenter(seed=0)
tables = aug.tables(keys, H, W)
out = torch.empty_like(img)


def torch_route():
    x = img.view(F, H, W, 3).permute(0, 3, 1, 2).float()
    mu = (x * torch.tensor([77.0, 150.0, 29.0], device=dev).view(1, 3, 1, 1)).sum(dim=(1, 2, 3)) / (256.0 * H * W)
    gm = tables[:, 10:16].view(F, 2, 3)
    # the table's pixel-index map in affine_grid's normalised coordinates (align_corners=False): xn = (2 x + 1) / W - 1 on both sides
    theta = torch.empty(F, 2, 3, device=dev)
    theta[:, 0, 0] = gm[:, 0, 0]; theta[:, 0, 1] = gm[:, 0, 1] * H / W
    theta[:, 1, 0] = gm[:, 1, 0] * W / H; theta[:, 1, 1] = gm[:, 1, 1]
    theta[:, 0, 2] = (2.0 * (gm[:, 0, 2] + gm[:, 0, 0] * (W - 1) / 2.0 + gm[:, 0, 1] * (H - 1) / 2.0) + 1.0) / W - 1.0
    theta[:, 1, 2] = (2.0 * (gm[:, 1, 2] + gm[:, 1, 0] * (W - 1) / 2.0 + gm[:, 1, 1] * (H - 1) / 2.0) + 1.0) / H - 1.0
    grid = torch.nn.functional.affine_grid(theta, (F, 3, H, W), align_corners=False)
    v = torch.nn.functional.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    o = torch.einsum("fcd,fdhw->fchw", tables[:, :9].view(F, 3, 3), v) + (tables[:, 9] * mu).view(F, 1, 1, 1)
    return o.clamp_(0.0, 255.0).round_().to(torch.uint8).permute(0, 2, 3, 1).contiguous().view(B, T, H, W, 3)


variants = {"kernel": lambda: ops.augment_frames(img, tables, out=out), "copy": lambda: out.copy_(img), "torch": torch_route,
            "tables": lambda: aug.tables(keys, H, W)}


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


# how far the torch route is from the kernel's bytes (its rounding is ATen's, not the kernel's): reported, not asserted
ref = ops.augment_frames(img, tables)
diff = (torch_route().to(torch.int16) - ref.to(torch.int16)).abs()
rec = dict(batch=B, seq=T, frames=F, frame_bytes=H * W * 3, rounds=a.rounds, window_s=a.window,
           torch_route_vs_kernel=dict(max_abs=int(diff.max()), share_differing=float((diff > 0).float().mean())))
del diff, ref
reps = {}
for k, fn in variants.items():
    fn(); fn()
    torch.cuda.synchronize()
    reps[k] = max(1, int(a.window * 1e3 / max(window(fn, 3), 1e-3)) + 1)
times = {k: [] for k in variants}
for _ in range(a.rounds):
    for k, fn in variants.items():
        fn()
        times[k].append(window(fn, reps[k]))
for k, v in times.items():
    v.sort()
    rec[k] = dict(ms_median=round(v[len(v) // 2], 4), ms_min=round(v[0], 4), ms_max=round(v[-1], 4), calls_per_window=reps[k])
    print(f"{k:7s} {rec[k]['ms_median']:9.4f} ms per call (min {v[0]:.4f}, max {v[-1]:.4f}; {reps[k]} calls per window)")
moved = 2.0 * F * H * W * 3
rec["bytes_moved"] = moved
rec["kernel_tb_per_s"] = round(moved / (rec["kernel"]["ms_median"] * 1e-3) / 1e12, 3)
rec["copy_tb_per_s"] = round(moved / (rec["copy"]["ms_median"] * 1e-3) / 1e12, 3)
rec["kernel_over_copy"] = round(rec["kernel"]["ms_median"] / rec["copy"]["ms_median"], 3)
rec["torch_over_kernel"] = round(rec["torch"]["ms_median"] / rec["kernel"]["ms_median"], 2)
print(f"kernel {rec['kernel_tb_per_s']:.2f} TB/s, copy {rec['copy_tb_per_s']:.2f} TB/s over {moved / 1e6:.0f} MB; kernel / copy = {rec['kernel_over_copy']:.2f}; torch / kernel = {rec['torch_over_kernel']:.1f}")

for k in ("kernel", "torch"):
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = variants[k]()
    torch.cuda.synchronize()
    rec[k]["peak_extra_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    del r
    print(f"{k:7s} peak memory beyond the resident input, tables and output: {rec[k]['peak_extra_mb']:.1f} MB")

if a.bc_steps > 0:
    from vpt_amd.training import BCTrainer
    from vpt_amd.lib.policy import MinecraftAgentPolicy
    from vpt_amd.lib.types import minecraft_action_space
    pol = MinecraftAgentPolicy(minecraft_action_space(), configs.policy_kwargs_for(a.model), dict(temperature=2.0), precision="bf16")
    configs.randomize_(pol, 0)
    pol = pol.to(dev)
    tr = BCTrainer(pol, train_cnn=True)
    first = torch.zeros(B, T, dtype=torch.bool, device=dev)
    ab = torch.randint(0, 8641, (B, T), generator=g).to(dev); ac = torch.randint(0, 121, (B, T), generator=g).to(dev)
    step = lambda: tr.step(ops.augment_frames(img, tables, out=out), first, pol.initial_state(B), ab, ac)[0]
    step()
    bc = sorted(window(step, 1) for _ in range(a.bc_steps))
    rec["bc_step"] = dict(model=a.model, ms_median=round(bc[len(bc) // 2], 2), ms_min=round(bc[0], 2), ms_max=round(bc[-1], 2), steps=a.bc_steps)
    rec["kernel_share_of_bc_step"] = round(rec["kernel"]["ms_median"] / rec["bc_step"]["ms_median"], 5)
    print(f"BC step ({a.model}, train_cnn, augmentation inside): {rec['bc_step']['ms_median']:.2f} ms; the augmentation launch is {100 * rec['kernel_share_of_bc_step']:.3f} % of it")
print(json.dumps(rec))
