"""Time the BC step with global-norm gradient clipping against the unclipped step, the parent commit's step and torch's clip, interleaved in ONE process.
python tools/grad_clip_bench.py [--model 2x] [--batch 64] [--seq 128] [--warmup 1] [--steps 3] [--no-cnn] [--parent-tree DIR]

  bc_parent   BCTrainer.step of another checkout of the project (--parent-tree: its package directory with its own built libraries), loaded beside
              this one under another module name -- the parent commit's step, on the same box at the same clock
  bc          BCTrainer.step of this tree, max_grad_norm=None: the launches of the parent's step
  bc_clip     BCTrainer.step, max_grad_norm=5.0: vpt_grad_norm_multi over the Adam table + the coefficient inside the Adam launch
  torch_clip  loss_and_grads + torch.nn.utils.clip_grad_norm_(params, 5.0) + ops.adam_step_multi_: what a user had to write before

Every timed step sits between two HIP events; the variants take turns inside every round, each turn one un-timed step (the caching allocator re-shapes
its pools after a switch of variant) and the timed one; the spread of a variant is max - min over its rounds.  Then, on the last step's gradients,
the norm launches alone (kernel + the two finish launches) and vpt_grads_nonfinite_multi -- the same bytes read with no reduction, the yardstick --
each between HIP events, --reps times; and the three optimiser tails alone on those gradients (Adam; norm + clipped Adam; clip_grad_norm_ + Adam), --reps calls
back to back between two HIP events: a whole step is 99.7 % network and cannot resolve them.  The last line is one JSON record."""
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
ap.add_argument("--max-grad-norm", type=float, default=5.0); ap.add_argument("--reps", type=int, default=20)
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

pol_clip = make_policy()
tr_clip = BCTrainer(pol_clip, train_cnn=not a.no_cnn, max_grad_norm=a.max_grad_norm)
variants["bc_clip"] = lambda: tr_clip.step(img, first, pol_clip.initial_state(B), ab, ac)[0]

pol_t = make_policy()
tr_t = BCTrainer(pol_t, train_cnn=not a.no_cnn)
last = {}


def torch_clip_step():
    loss, grads, _ = tr_t.loss_and_grads(img, first, pol_t.initial_state(B), ab, ac)
    names = [n for n in tr_t.trainable if n in grads]
    params = [tr_t.params[n] for n in names]
    for p, n in zip(params, names):
        p.grad = grads[n].reshape(p.shape)
    last["norm"] = torch.nn.utils.clip_grad_norm_(params, a.max_grad_norm)
    ops.adam_step_multi_([p.data.view(-1) for p in params], [p.grad.contiguous().view(-1) for p in params], [tr_t.m[n].view(-1) for n in names],
                         [tr_t.v[n].view(-1) for n in names], tr_t.step_count + 1, lr=tr_t.lr, beta1=tr_t.betas[0], beta2=tr_t.betas[1], eps=tr_t.eps,
                         weight_decay=tr_t.wd)
    for p in params:
        p.grad = None
    tr_t.step_count += 1
    pol_t._packed_key = None
    last["grads"], last["names"] = [grads[n].contiguous().view(-1) for n in names], names
    return float(loss)


variants["torch_clip"] = torch_clip_step
variants = {k: v for k, v in variants.items() if k not in skip}

# ---- interleaved timing -----------------------------------------------------------------------------------------------------------
times = {k: [] for k in variants}
for _ in range(a.warmup):
    for k, fn in variants.items():
        print(f"warm-up {k}: loss {fn():.4f}")
torch.cuda.synchronize()
print("peak mem GB", torch.cuda.max_memory_allocated() / 2 ** 30)
with BoxSampler(torch.cuda.current_device()) as box:
    for r in range(a.steps):
        for k, fn in variants.items():
            fn()                 # one un-timed step after every switch of variant (allocator pools), then the timed one
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
rec = dict(model=a.model, batch=B, seq=T, precision=precision, train_cnn=not a.no_cnn, warmup=a.warmup, rounds=a.steps, max_grad_norm=a.max_grad_norm,
           box=box.record())
for k, v in times.items():
    rec[k] = dict(ms_median=round(sorted(v)[len(v) // 2], 2), ms_mean=round(sum(v) / len(v), 2), ms_min=round(min(v), 2), ms_max=round(max(v), 2), spread_ms=round(max(v) - min(v), 2))
    print(f"{k:10s} step {rec[k]['ms_mean']:9.2f} ms  (min {min(v):.2f}, max {max(v):.2f}; {M / (rec[k]['ms_mean'] * 1e-3):.0f} frames/s)")
if "bc_parent" in rec and "bc" in rec:
    rec["bc_minus_parent_ms"] = round(rec["bc"]["ms_mean"] - rec["bc_parent"]["ms_mean"], 2)
    print(f"bc - bc_parent: {rec['bc_minus_parent_ms']:+.2f} ms (the parent's own spread: {rec['bc_parent']['spread_ms']:.2f} ms)")
if "bc_clip" in rec and "torch_clip" in rec:
    rec["torch_clip_minus_bc_clip_ms"] = round(rec["torch_clip"]["ms_mean"] - rec["bc_clip"]["ms_mean"], 2)
    print(f"torch_clip - bc_clip: {rec['torch_clip_minus_bc_clip_ms']:+.2f} ms (torch_clip's spread: {rec['torch_clip']['spread_ms']:.2f} ms)")
if tr_clip.last_grad_norm is not None:
    rec["grad_norm_last_step"] = float(tr_clip.last_grad_norm)

# ---- the norm launches alone, beside the non-finite check over the same bytes ------------------------------------------------------
if "grads" not in last:
    torch_clip_step()
grads = last["grads"]
numel = sum(x.numel() for x in grads)
blocks = sum((x.numel() + 1023) // 1024 for x in grads)
rec.update(tensors=len(grads), parameters=numel, table_blocks=blocks)
for _ in range(3):
    ops.grad_norm(grads, max_norm=a.max_grad_norm); ops.grads_nonfinite(grads)
torch.cuda.synchronize()
ops.TIMER.enabled = True
ops.TIMER.reset()
for _ in range(a.reps):
    ops.grad_norm(grads, max_norm=a.max_grad_norm)
    ops.grads_nonfinite(grads)
summ = ops.TIMER.summary()
ops.TIMER.enabled = False
for key, nbytes in (("vpt_grad_norm_multi", 4.0 * numel + 8.0 * blocks + 16.0 * len(grads)), ("vpt_grads_nonfinite_multi", 4.0 * numel)):
    ms = summ[key]["ms"] / summ[key]["calls"]
    rec[key] = dict(ms=round(ms, 4), tb_per_s=round(nbytes / (ms * 1e-3) / 1e12, 3), bytes=nbytes, calls=summ[key]["calls"])
    print(f"{key}: {ms:.4f} ms per call over {nbytes / 1e6:.1f} MB -> {rec[key]['tb_per_s']:.2f} TB/s ({summ[key]['calls']} calls)")

# ---- the optimiser tails alone, on the same gradients: what a whole step (99.7 % network) cannot resolve -------------------------------------
names = last["names"]


def tail_of(tr, **kw):
    args = ([tr.params[n].data.view(-1) for n in names], grads, [tr.m[n].view(-1) for n in names], [tr.v[n].view(-1) for n in names], tr.step_count + 1)
    return lambda: ops.adam_step_multi_(*args, lr=tr.lr, beta1=tr.betas[0], beta2=tr.betas[1], eps=tr.eps, weight_decay=tr.wd, **kw)


def torch_tail():
    params = [tr_t.params[n] for n in names]
    for p, x in zip(params, grads):
        p.grad = x.view(p.shape)
    torch.nn.utils.clip_grad_norm_(params, a.max_grad_norm)
    tail_of(tr_t)()
    for p in params:
        p.grad = None


flag = torch.zeros(1, dtype=torch.int32, device=dev)
for key, fn in (("tail_adam", tail_of(tr_bc)), ("tail_norm_adam_clip", tail_of(tr_clip, max_grad_norm=a.max_grad_norm, found_inf=flag)),
                ("tail_torch_clip_adam", torch_tail)):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    rec[key + "_ms"] = round(e0.elapsed_time(e1) / a.reps, 4)
    print(f"{key}: {rec[key + '_ms']:.4f} ms per call ({a.reps} calls back to back between two HIP events, table upload included)")
print(json.dumps(rec))
