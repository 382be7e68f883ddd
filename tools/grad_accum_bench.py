"""Time the BC step with gradient accumulation over micro-batches against the one-piece step and the parent commit's step, interleaved in ONE process,
with each variant's peak memory; then ops.grad_accumulate_ against torch._foreach_add_ on the model's gradient set.
python tools/grad_accum_bench.py [--model 2x] [--batch 64] [--seq 128] [--warmup 1] [--steps 3] [--no-cnn] [--parent-tree DIR] [--micro-batches 2,4]

  bc_parent   BCTrainer.step of another checkout of the project (--parent-tree: its package directory with its own built libraries), loaded beside
              this one under another module name -- the parent commit's step, on the same box at the same clock
  bc          BCTrainer.step of this tree, the default keyword (micro_batches=1): the launches of the parent's step
  bc_k2, ...  BCTrainer.step(micro_batches=K) for every K of --micro-batches: K row groups, their gradients summed by vpt_grad_accumulate_multi

Every timed step sits between two HIP events; the variants take turns inside every round, each turn one un-timed step (the caching allocator re-shapes
its pools after a switch of variant) and the timed one; the spread of a variant is max - min over its rounds.  torch.cuda.max_memory_allocated is reset
before every turn and read after it: a variant's peak is the maximum over its turns, with every variant's policy, moments and the batch resident
(`resident_gb`, the allocation before the first step).  Then, on gradient-shaped tensors of the model (one set as accumulators, one as addends),
ops.grad_accumulate_ and torch._foreach_add_ each --reps times between HIP events after warm-up: GB/s over 12 bytes per element (two reads, one
write).  The last line is one JSON record."""
import argparse, importlib.util, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import __graft_entry__ as ge
ge.build()
from bench import BoxSampler
from vpt_amd import ops, configs
from vpt_amd.training import BCTrainer
from vpt_amd.lib.policy import MinecraftAgentPolicy
from vpt_amd.lib.types import minecraft_action_space

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="2x"); ap.add_argument("--batch", type=int, default=64); ap.add_argument("--seq", type=int, default=128)
ap.add_argument("--warmup", type=int, default=1); ap.add_argument("--steps", type=int, default=3); ap.add_argument("--no-cnn", action="store_true")
ap.add_argument("--parent-tree", default=None, help="package directory (video-pre-training_amd/) of another checkout, built, for the bc_parent variant")
ap.add_argument("--micro-batches", default="2,4", help="comma-separated K of the accumulating variants")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--skip", default="", help="comma-separated variants to leave out")
a = ap.parse_args()
dev = "cuda"
precision = os.environ.get("VPT_PRECISION", "bf16")
NB, NC = 8641, 121
B, T = a.batch, a.seq
M = B * T
GB = 2.0 ** 30


def make_policy(policy_cls=MinecraftAgentPolicy, cfgs=configs, space=minecraft_action_space):
    pol = policy_cls(space(), cfgs.policy_kwargs_for(a.model), dict(temperature=2.0), precision=precision)
    cfgs.randomize_(pol, 0)
    return pol.to(dev)


g = torch.Generator().manual_seed(1)
img = torch.randint(0, 256, (B, T, 128, 128, 3), generator=g, dtype=torch.uint8).to(dev)
first = torch.zeros(B, T, dtype=torch.bool, device=dev)
ab = torch.randint(0, NB, (B, T), generator=g).to(dev); ac = torch.randint(0, NC, (B, T), generator=g).to(dev)
skip = set(filter(None, a.skip.split(",")))
variants = {}

if a.parent_tree:
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
    pol_par = make_policy(ParentPolicy, pconfigs, parent_space)
    tr_par = ParentBCTrainer(pol_par, train_cnn=not a.no_cnn)
    variants["bc_parent"] = lambda: tr_par.step(img, first, pol_par.initial_state(B), ab, ac)[0]

pol_bc = make_policy()
tr_bc = BCTrainer(pol_bc, train_cnn=not a.no_cnn)
variants["bc"] = lambda: tr_bc.step(img, first, pol_bc.initial_state(B), ab, ac)[0]

accum = {}
for k in [int(x) for x in a.micro_batches.split(",") if x]:
    pol_k = make_policy()
    accum[k] = (pol_k, BCTrainer(pol_k, train_cnn=not a.no_cnn))
    variants[f"bc_k{k}"] = (lambda k=k: accum[k][1].step(img, first, accum[k][0].initial_state(B), ab, ac, micro_batches=k)[0])
variants = {k: v for k, v in variants.items() if k not in skip}

# ---- interleaved timing, peak memory per variant --------------------------------------------------------------------------------------
torch.cuda.synchronize()
resident = torch.cuda.memory_allocated()
times, peaks = {k: [] for k in variants}, {k: 0 for k in variants}
for _ in range(a.warmup):
    for k, fn in variants.items():
        print(f"warm-up {k}: loss {fn():.4f}")
torch.cuda.synchronize()
with BoxSampler(torch.cuda.current_device()) as box:
    for r in range(a.steps):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            fn()                 # one un-timed step after every switch of variant (allocator pools), then the timed one
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
            peaks[k] = max(peaks[k], torch.cuda.max_memory_allocated())
rec = dict(model=a.model, batch=B, seq=T, precision=precision, train_cnn=not a.no_cnn, warmup=a.warmup, rounds=a.steps, resident_gb=round(resident / GB, 2),
           box=box.record())
for k, v in times.items():
    rec[k] = dict(ms_median=round(sorted(v)[len(v) // 2], 2), ms_mean=round(sum(v) / len(v), 2), ms_min=round(min(v), 2), ms_max=round(max(v), 2), spread_ms=round(max(v) - min(v), 2),
                  peak_gb=round(peaks[k] / GB, 2), peak_above_resident_gb=round((peaks[k] - resident) / GB, 2))
    print(f"{k:10s} step {rec[k]['ms_mean']:9.2f} ms  (min {min(v):.2f}, max {max(v):.2f}; {M / (rec[k]['ms_mean'] * 1e-3):.0f} frames/s)  peak {rec[k]['peak_gb']:.2f} GB "
          f"({rec[k]['peak_above_resident_gb']:.2f} GB above the {rec['resident_gb']:.2f} GB resident)")
if "bc_parent" in rec and "bc" in rec:
    rec["bc_minus_parent_ms"] = round(rec["bc"]["ms_mean"] - rec["bc_parent"]["ms_mean"], 2)
    print(f"bc - bc_parent: {rec['bc_minus_parent_ms']:+.2f} ms (the parent's own spread: {rec['bc_parent']['spread_ms']:.2f} ms)")
if "bc" in rec:
    for k in accum:
        key = f"bc_k{k}"
        if key in rec:
            rec[key].update(ms_above_bc=round(rec[key]["ms_mean"] - rec["bc"]["ms_mean"], 2), peak_saved_gb=round(rec["bc"]["peak_gb"] - rec[key]["peak_gb"], 2))
            print(f"{key} - bc: {rec[key]['ms_above_bc']:+.2f} ms, peak memory {rec[key]['peak_saved_gb']:+.2f} GB saved")

# ---- the accumulate launch alone, beside torch._foreach_add_ on the same tensors --------------------------------------------------------
names = tr_bc.trainable
accs = [torch.randn(tr_bc.params[n].numel(), device=dev) for n in names]
adds = [torch.randn(tr_bc.params[n].numel(), device=dev) for n in names]
numel = sum(x.numel() for x in accs)
rec.update(tensors=len(accs), parameters=numel, table_blocks=sum((x.numel() + 1023) // 1024 for x in accs))
for key, fn in (("grad_accumulate", lambda: ops.grad_accumulate_(accs, adds)), ("foreach_add", lambda: torch._foreach_add_(accs, adds))):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1))
    ms = sorted(per_call)[len(per_call) // 2]
    rec[key] = dict(ms_median=round(ms, 4), ms_min=round(min(per_call), 4), ms_max=round(max(per_call), 4), gb_per_s=round(12.0 * numel / (ms * 1e-3) / 1e9, 1), calls=a.reps)
    print(f"{key}: {ms:.4f} ms per call (min {min(per_call):.4f}, max {max(per_call):.4f}; HIP events around the whole front-end call, table upload included) "
          f"over {12.0 * numel / 1e6:.1f} MB -> {rec[key]['gb_per_s']:.0f} GB/s")
# ... and the launch alone (HIP events around the C-ABI call, ops.TIMER: no table build, no upload)
ops.TIMER.enabled = True
ops.TIMER.reset()
for _ in range(a.reps):
    ops.grad_accumulate_(accs, adds)
summ = ops.TIMER.summary()["vpt_grad_accumulate_multi"]
ops.TIMER.enabled = False
ms = summ["ms"] / summ["calls"]
rec["vpt_grad_accumulate_multi"] = dict(ms=round(ms, 4), gb_per_s=round(12.0 * numel / (ms * 1e-3) / 1e9, 1), calls=summ["calls"])
print(f"vpt_grad_accumulate_multi: {ms:.4f} ms per launch -> {rec['vpt_grad_accumulate_multi']['gb_per_s']:.0f} GB/s ({summ['calls']} launches)")
print(json.dumps(rec))
