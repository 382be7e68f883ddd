"""Time low-rank adapters: BCTrainer.step with adapters on every block against dense training of the same blocks, the default
step and the parent commit's, interleaved in ONE process, by the protocol of tools/partial_bench.py.
python tools/lowrank_bench.py [--model 2x] [--batch 64] [--seq 128] [--rank 16] [--warmup 1] [--steps 3] [--parent-tree DIR] [--skip a,b] [--markdown FILE]

  parent    BCTrainer(train_cnn=False).step of another checkout of the project (--parent-tree: its package directory with its own built libraries),
            loaded beside this one under another module name -- the parent commit's step, on the same box at the same clock
  default   BCTrainer(train_cnn=False).step of this tree, default arguments (adapters=None: the code path that has always run)
  dense     trainable = net.recurrent_layer.blocks: every tensor of every block trains densely
  adapters  LowRankAdapters(rank) on every adaptable linear of every block, nothing else trainable

Every timed step sits between two HIP events; the variants take turns inside every round, each turn one un-timed step (the caching allocator
re-shapes its pools after a switch of variant) and the timed one; the spread of a variant is max - min over its rounds.  Peak memory: the
allocator's peak during the timed step above what was resident when the step began.  The saved artefact: what a task checkpoint of the variant
holds -- the policy's state dict (the `.weights` file) for the dense variants, LowRankAdapters.state_dict() for the adapters -- and the Adam moments
next to it.  The last line is one JSON record; --markdown writes the table."""
import argparse, importlib.util, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import __graft_entry__ as ge
ge.build()
from bench import BoxSampler
from vpt_amd import configs
from vpt_amd.adapters import LowRankAdapters
from vpt_amd.training import BCTrainer
from vpt_amd.lib.policy import MinecraftAgentPolicy
from vpt_amd.lib.types import minecraft_action_space

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="2x"); ap.add_argument("--batch", type=int, default=64); ap.add_argument("--seq", type=int, default=128)
ap.add_argument("--rank", type=int, default=16)
ap.add_argument("--warmup", type=int, default=1); ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--parent-tree", default=None, help="package directory (video-pre-training_amd/) of another checkout, built, for the parent variant")
ap.add_argument("--skip", default="", help="comma-separated variants to leave out")
ap.add_argument("--markdown", default=None, help="write the table to this file")
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


def nbytes(tensors):
    return sum(t.numel() * t.element_size() for t in tensors if isinstance(t, torch.Tensor))


g = torch.Generator().manual_seed(1)
img = torch.randint(0, 256, (B, T, 128, 128, 3), generator=g, dtype=torch.uint8).to(dev)
first = torch.zeros(B, T, dtype=torch.bool, device=dev)
ab = torch.randint(0, NB, (B, T), generator=g).to(dev); ac = torch.randint(0, NC, (B, T), generator=g).to(dev)
skip = set(filter(None, a.skip.split(",")))
variants, trainers, artefact = {}, {}, {}


def add(name, pol, tr, saved):
    trainers[name] = tr
    artefact[name] = nbytes(saved.values())
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
    add("parent", pol, ParentBCTrainer(pol, train_cnn=False), pol.state_dict())
for name in ("default", "dense", "adapters"):
    if name in skip:
        continue
    pol = make_policy()
    if name == "adapters":
        ad = LowRankAdapters(pol, targets=("net.recurrent_layer.blocks",), rank=a.rank, alpha=float(a.rank), seed=0)
        add(name, pol, BCTrainer(pol, train_cnn=False, adapters=ad), ad.state_dict())
    else:
        add(name, pol, BCTrainer(pol, train_cnn=False, **(dict(trainable=["net.recurrent_layer.blocks"]) if name == "dense" else {})), pol.state_dict())

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
rec = dict(model=a.model, batch=B, seq=T, precision=precision, train_cnn=False, rank=a.rank, warmup=a.warmup, rounds=a.steps, box=box.record())
rows = []
for k, v in times.items():
    tr = trainers[k]
    rec[k] = dict(ms_median=round(sorted(v)[len(v) // 2], 2), ms_mean=round(sum(v) / len(v), 2), ms_min=round(min(v), 2), ms_max=round(max(v), 2),
                  spread_ms=round(max(v) - min(v), 2), peak_gb=round(peaks[k], 3), peak_above_resident_gb=round(above[k], 3),
                  trainable_tensors=len(tr.trainable), trainable_parameters=sum(tr.params[n].numel() for n in tr.trainable),
                  artefact_bytes=artefact[k], moment_bytes=nbytes(tr.m.values()) + nbytes(tr.v.values()))
    rows.append(f"| `{k}` | {rec[k]['trainable_tensors']} / {rec[k]['trainable_parameters'] / 1e6:.1f} M | {rec[k]['ms_median']:.2f} ({min(v):.2f} - {max(v):.2f}) | "
                f"{above[k]:.2f} | {artefact[k] / 2 ** 20:.1f} | {rec[k]['moment_bytes'] / 2 ** 20:.1f} |")
    print(f"{k:8s} step {rec[k]['ms_mean']:9.2f} ms  (min {min(v):.2f}, max {max(v):.2f}; {M / (rec[k]['ms_mean'] * 1e-3):.0f} frames/s), "
          f"{above[k]:.2f} GB above the resident state, artefact {artefact[k] / 2 ** 20:.1f} MiB, moments {rec[k]['moment_bytes'] / 2 ** 20:.1f} MiB")
table = "\n".join(["| variant | trainable tensors / parameters | ms per step: median (min - max) | GB above the resident state | saved artefact, MiB | Adam moments, MiB |",
                   "|---|---|---|---|---|---|"] + rows)
print(table)
if a.markdown:
    with open(a.markdown, "w") as f:
        f.write(table + "\n")
print(json.dumps(rec))
