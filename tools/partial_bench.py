"""Time partial fine-tuning: BCTrainer.step with a trainable subset and with parameter groups against the default step and the
parent commit's, interleaved in ONE process, in the form of tools/rl_bench.py.
python tools/partial_bench.py [--model 2x] [--batch 64] [--seq 128] [--warmup 1] [--steps 3] [--parent-tree DIR] [--skip a,b]

  parent   BCTrainer(train_cnn=False).step of another checkout of the project (--parent-tree: its package directory with its own built libraries),
           loaded beside this one under another module name -- the parent commit's step, on the same box at the same clock
  default  BCTrainer(train_cnn=False).step of this tree, default arguments
  s3       trainable = net.lastlayer, net.final_ln, pi_head and the last transformer block
  s1       trainable = pi_head
  groups   `default` with two parameter groups (the heads at lr_scale 0.1 without decay, the rest at the trainer's values): ops.adam_step_groups_

Every timed step sits between two HIP events; the variants take turns inside every round, each turn one un-timed step (the caching allocator
re-shapes its pools after a switch of variant) and the timed one; the spread of a variant is max - min over its rounds.  Peak memory: the
allocator's peak during the timed step, and the same above what was resident when the step began (the other variants' weights and moments stay
resident all along).  The last line is one JSON record."""
import argparse, importlib.util, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import __graft_entry__ as ge
ge.build()
from bench import BoxSampler
from vpt_amd import configs
from vpt_amd.training import BCTrainer
from vpt_amd.lib.policy import MinecraftAgentPolicy
from vpt_amd.lib.types import minecraft_action_space

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="2x"); ap.add_argument("--batch", type=int, default=64); ap.add_argument("--seq", type=int, default=128)
ap.add_argument("--warmup", type=int, default=1); ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--parent-tree", default=None, help="package directory (video-pre-training_amd/) of another checkout, built, for the parent variant")
ap.add_argument("--skip", default="", help="comma-separated variants to leave out")
a = ap.parse_args()
dev = "cuda"
precision = os.environ.get("VPT_PRECISION", "bf16")
NB, NC = 8641, 121
B, T = a.batch, a.seq
M = B * T


def make_policy(policy_cls=MinecraftAgentPolicy, cfgs=configs, space=minecraft_action_space):
    pol = policy_cls(space(), cfgs.policy_kwargs_for(a.model), dict(temperature=2.0), precision=precision)
    cfgs.randomize_(pol, 0)
    return pol.to(dev)


g = torch.Generator().manual_seed(1)
img = torch.randint(0, 256, (B, T, 128, 128, 3), generator=g, dtype=torch.uint8).to(dev)
first = torch.zeros(B, T, dtype=torch.bool, device=dev)
ab = torch.randint(0, NB, (B, T), generator=g).to(dev); ac = torch.randint(0, NC, (B, T), generator=g).to(dev)
skip = set(filter(None, a.skip.split(",")))
variants, trainers = {}, {}


def add(name, pol, tr):
    trainers[name] = tr
    variants[name] = lambda: tr.step(img, first, pol.initial_state(B), ab, ac)[0]


if a.parent_tree and "parent" not in skip:
    pdir = os.path.abspath(a.parent_tree)
    spec = importlib.util.spec_from_file_location("vpt_amd_parent", os.path.join(pdir, "__init__.py"), submodule_search_locations=[pdir])
    parent = importlib.util.module_from_spec(spec)
    sys.modules["vpt_amd_parent"] = parent
    spec.loader.exec_module(parent)
    from vpt_amd_parent import configs as pconfigs
    from vpt_amd_parent.training import BCTrainer as ParentBCTrainer
    from vpt_amd_parent.lib.policy import MinecraftAgentPolicy as ParentPolicy
    from vpt_amd_parent.lib.types import minecraft_action_space as parent_space
    from vpt_amd_parent import _native as pnative
    print("parent library:", pnative.lib_path())
    pol = make_policy(ParentPolicy, pconfigs, parent_space)
    add("parent", pol, ParentBCTrainer(pol, train_cnn=False))
n_layers = configs.policy_kwargs_for(a.model)["n_recurrence_layers"]
S2 = ["net.lastlayer", "net.final_ln", "pi_head"]
for name, kw in (("default", {}), ("s3", dict(trainable=S2 + [f"net.recurrent_layer.blocks.{n_layers - 1}"])), ("s1", dict(trainable=["pi_head"])),
                 ("groups", dict(param_groups=[dict(params=["pi_head"], lr_scale=0.1, weight_decay=0.0)]))):
    if name not in skip:
        pol = make_policy()
        add(name, pol, BCTrainer(pol, train_cnn=False, **kw))

# ---- interleaved timing -----------------------------------------------------------------------------------------------------------
times, peaks, above = {k: [] for k in variants}, {k: 0.0 for k in variants}, {k: 0.0 for k in variants}
for _ in range(a.warmup):
    for k, fn in variants.items():
        print(f"warm-up {k}: loss {fn():.4f}")
torch.cuda.synchronize()
with BoxSampler(torch.cuda.current_device()) as box:
    for r in range(a.steps):
        for k, fn in variants.items():
            fn()                 # one un-timed step after every switch of variant: the caching allocator re-shapes its pools
            torch.cuda.synchronize()
            resident = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
            peak = torch.cuda.max_memory_allocated()
            peaks[k], above[k] = max(peaks[k], peak / 2 ** 30), max(above[k], (peak - resident) / 2 ** 30)
rec = dict(model=a.model, batch=B, seq=T, precision=precision, train_cnn=False, warmup=a.warmup, rounds=a.steps, box=box.record())
for k, v in times.items():
    rec[k] = dict(ms_median=round(sorted(v)[len(v) // 2], 2), ms_mean=round(sum(v) / len(v), 2), ms_min=round(min(v), 2), ms_max=round(max(v), 2),
                  spread_ms=round(max(v) - min(v), 2), peak_gb=round(peaks[k], 3), peak_above_resident_gb=round(above[k], 3),
                  trainable_tensors=len(trainers[k].trainable), trainable_parameters=sum(trainers[k].params[n].numel() for n in trainers[k].trainable))
    print(f"{k:8s} step {rec[k]['ms_mean']:9.2f} ms  (min {min(v):.2f}, max {max(v):.2f}; {M / (rec[k]['ms_mean'] * 1e-3):.0f} frames/s), "
          f"peak {peaks[k]:.2f} GB, {above[k]:.2f} GB above the resident state, {rec[k]['trainable_tensors']} trainable tensors")
print(json.dumps(rec))
