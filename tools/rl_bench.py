"""Time the PPO fine-tuning step and the PPG auxiliary step against the same losses written in torch on the autograd boundary and against the BC step,
interleaved in ONE process.
python tools/rl_bench.py [--model 2x] [--batch 64] [--seq 128] [--warmup 1] [--steps 2] [--no-cnn] [--parent-tree DIR]

  ppo        PPOTrainer.step with kl_coef > 0 (the prior's log-probs precomputed): ONE vpt_rl_loss launch between forward and backward
  torch      the same loss written in torch on get_output_for_observation's outputs, .backward() through the autograd boundary, torch.optim.Adam
  aux        PPOTrainer.aux_step (the PPG auxiliary phase; the snapshot precomputed, outside the timing): ONE vpt_ppg_aux_loss launch
  aux_torch  the auxiliary loss written in torch on the same boundary, the same torch.optim.Adam
  bc         BCTrainer.step of this tree
  bc_parent  BCTrainer.step of another checkout of the project (--parent-tree: its package directory with its own built libraries), loaded beside
             this one under another module name -- the parent commit's step, on the same box at the same clock
  ppo_parent PPOTrainer.step of that checkout

Every timed step sits between two HIP events; the variants take turns inside every round (warm-up and round counts as tools/bc_bench.py: 1 and 2 by
default), each turn one un-timed step (the caching allocator re-shapes its pools after a switch of variant: seconds, measured) and the timed one; the
spread of a variant is max - min over its rounds.  Then one instrumented PPO step, one auxiliary step and one weighted BC step give the three loss
kernels' own times.  The last line is one JSON record."""
import argparse, importlib.util, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import __graft_entry__ as ge
ge.build()
from bench import BoxSampler
from vpt_amd import ops, configs
from vpt_amd.training import BCTrainer
from vpt_amd.rl_training import PPOTrainer
from vpt_amd.lib.policy import MinecraftAgentPolicy
from vpt_amd.lib.types import minecraft_action_space

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="2x"); ap.add_argument("--batch", type=int, default=64); ap.add_argument("--seq", type=int, default=128)
ap.add_argument("--warmup", type=int, default=1); ap.add_argument("--steps", type=int, default=2); ap.add_argument("--no-cnn", action="store_true")
ap.add_argument("--parent-tree", default=None, help="package directory (video-pre-training_amd/) of another checkout, built, for the bc_parent variant")
ap.add_argument("--no-settle", action="store_true", help="time the first step after every switch of variant too (allocator re-shaping included)")
ap.add_argument("--skip", default="", help="comma-separated variants to leave out")
a = ap.parse_args()
dev = "cuda"
precision = os.environ.get("VPT_PRECISION", "bf16")
COEF = dict(clip=0.2, kl_coef=0.2, entropy_coef=0.01, value_coef=0.5)
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
adv = torch.randn(B, T, generator=g).to(dev); target = (torch.randn(B, T, generator=g) * 2).to(dev)
skip = set(filter(None, a.skip.split(",")))
variants = {}

# ---- (i) PPOTrainer.step -------------------------------------------------------------------------------------------------------
pol_ppo = make_policy()
tr_ppo = PPOTrainer(pol_ppo, train_cnn=not a.no_cnn, normalize_advantages=False, **COEF)
qb, qc, _ = tr_ppo.prior_logprobs(pol_ppo, img, first, pol_ppo.initial_state(B))
prior = (qb.clone(), qc.clone())
old = (prior[0].gather(1, ab.reshape(M, 1)) + prior[1].gather(1, ac.reshape(M, 1))).reshape(B, T) + 0.1 * torch.randn(B, T, generator=g).to(dev)
del qb, qc
variants["ppo"] = lambda: tr_ppo.step(img, first, pol_ppo.initial_state(B), ab, ac, old, adv, target, prior_lp=prior)[0]
# the auxiliary phase runs on the SAME trainer (one network, one optimiser); its snapshot is the log-probs taken above, before any step
variants["aux"] = lambda: tr_ppo.aux_step(img, first, pol_ppo.initial_state(B), prior, target)[0]

# ---- (ii) the same loss in torch on the autograd boundary + torch.optim.Adam ---------------------------------------------------
if "torch" not in skip:
    pol_t = make_policy()
    if a.no_cnn:
        for n, p in pol_t.named_parameters():
            p.requires_grad_(not n.startswith("net.img_process.cnn."))
    opt = torch.optim.Adam([p for p in pol_t.parameters() if p.requires_grad], lr=0.000181, weight_decay=0.039428)

    def torch_step():
        (pd, vpred, _), _ = pol_t({"img": img}, first, pol_t.initial_state(B))
        lb, lc = pd["buttons"].reshape(M, NB), pd["camera"].reshape(M, NC)
        lp = lb.gather(1, ab.reshape(M, 1))[:, 0] + lc.gather(1, ac.reshape(M, 1))[:, 0]
        rho, A = torch.exp(lp - old.reshape(M)), adv.reshape(M)
        pg = -torch.min(rho * A, torch.clamp(rho, 1 - COEF["clip"], 1 + COEF["clip"]) * A)
        kl = (lb.exp() * (lb - prior[0])).sum(-1) + (lc.exp() * (lc - prior[1])).sum(-1)
        ent = -(lb.exp() * lb).sum(-1) - (lc.exp() * lc).sum(-1)
        that = pol_t.value_head.normalizer.normalize(target.reshape(M, 1)).reshape(M)
        loss = (pg + COEF["kl_coef"] * kl - COEF["entropy_coef"] * ent + COEF["value_coef"] * (vpred.reshape(M) - that) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return float(loss.detach())
    variants["torch"] = torch_step

    def torch_aux_step():
        (pd, vpred, _), _ = pol_t({"img": img}, first, pol_t.initial_state(B))
        lb, lc = pd["buttons"].reshape(M, NB), pd["camera"].reshape(M, NC)
        kl = (prior[0].exp() * (prior[0] - lb)).sum(-1) + (prior[1].exp() * (prior[1] - lc)).sum(-1)
        that = pol_t.value_head.normalizer.normalize(target.reshape(M, 1)).reshape(M)
        loss = (tr_ppo.clone_coef * kl + tr_ppo.aux_value_coef * (vpred.reshape(M) - that) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return float(loss.detach())
    variants["aux_torch"] = torch_aux_step

# ---- (iii) BCTrainer.step, this tree and the parent's ---------------------------------------------------------------------------
pol_bc = make_policy()
tr_bc = BCTrainer(pol_bc, train_cnn=not a.no_cnn)
variants["bc"] = lambda: tr_bc.step(img, first, pol_bc.initial_state(B), ab, ac)[0]
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
    from vpt_amd_parent.rl_training import PPOTrainer as ParentPPOTrainer
    pol_ppar = make_policy(ParentPolicy, pconfigs, parent_space)
    tr_ppar = ParentPPOTrainer(pol_ppar, train_cnn=not a.no_cnn, normalize_advantages=False, **COEF)
    variants["ppo_parent"] = lambda: tr_ppar.step(img, first, pol_ppar.initial_state(B), ab, ac, old, adv, target, prior_lp=prior)[0]
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
            if not a.no_settle:      # the variants' activation footprints differ (tens of GB each): the first step after a switch re-shapes the caching
                fn()                 # allocator's pools (device allocations, synchronising frees) -- one un-timed step, then the timed one
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
rec = dict(model=a.model, batch=B, seq=T, precision=precision, train_cnn=not a.no_cnn, warmup=a.warmup, rounds=a.steps, coef=COEF, box=box.record())
for k, v in times.items():
    rec[k] = dict(ms_median=round(sorted(v)[len(v) // 2], 2), ms_mean=round(sum(v) / len(v), 2), ms_min=round(min(v), 2), ms_max=round(max(v), 2), spread_ms=round(max(v) - min(v), 2))
    print(f"{k:10s} step {rec[k]['ms_mean']:9.2f} ms  (min {min(v):.2f}, max {max(v):.2f}; {M / (rec[k]['ms_mean'] * 1e-3):.0f} frames/s)")

# ---- the three loss kernels' own times --------------------------------------------------------------------------------------------
ops.TIMER.enabled = True
for name, fn, key in (("ppo", variants["ppo"], "vpt_rl_loss"), ("aux", variants["aux"], "vpt_ppg_aux_loss"),
                      ("bc", lambda: tr_bc.step(img, first, pol_bc.initial_state(B), ab, ac, frame_weight=torch.ones(B, T, device=dev), metrics={}), "vpt_bc_loss")):
    ops.TIMER.reset()
    fn()
    torch.cuda.synchronize()
    summ = ops.TIMER.summary()
    rec[key + "_ms"] = round(summ[key]["ms"], 4)
    rec[key + "_bytes"] = summ[key]["bytes"]
    rec[name + "_kernel_total_ms"] = round(sum(v["ms"] for v in summ.values()), 2)
    print(f"{key}: {summ[key]['ms']:.4f} ms of {rec[name + '_kernel_total_ms']:.1f} ms kernel time in an instrumented {name} step "
          f"({summ[key]['bytes'] / (summ[key]['ms'] * 1e-3) / 1e12:.2f} TB/s over its own bytes)")
ops.TIMER.enabled = False
print(json.dumps(rec))
