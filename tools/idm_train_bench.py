"""One IDM fine-tuning step against one IDM forward on the same batch: how much the trained part (everything behind the frozen CNN) adds.
python tools/idm_train_bench.py [--batch 8] [--window 128] [--rounds 5] [--model 4x] [--precisions bf16,fp16] [--train-cnn] [--boundary]
                                [--parent-tree DIR] [--out idm_train_bench.json]

IDMTrainer.step (frozen temporal conv + CNN through the inference path, saving forward of the trunk, ops.idm_loss, the hand-written backward,
one-launch Adam) and IDMEngine.forward in ONE process per precision, after a warm-up of each, alternating (step, forward, forward, step, ...) so
that a drift of the box's clock hits both alike; every pass is timed with HIP events around the whole call.  The forward right behind a step
re-packs the weights the step changed; the second forward is the steady one, and their difference is what a loop of steps pays per step on top
of `step_ms`.  The spread reported is the first forward's own (max - min) / median over its rounds.  --profile-steps N instead runs N untimed steps and nothing else: the pass to put under
`rocprofv3 --kernel-trace --stats` for the attention backward's own time (a run of its own, never together with the timing above).
--boundary adds the variant "boundary + torch.optim.Adam" to every round: the same mean NLL written through pi_head.logprob on a gradient-enabled
InverseActionPolicy.forward (lib/policy.py:_IDMForwardFn, CNN frozen with requires_grad_(False)), loss.backward(), torch's unfused Adam, on a policy of
its own.  --parent-tree DIR (the package directory of another checkout of the project with its own built libraries, tools/rl_bench.py's practice) adds
IDMTrainer.step of THAT checkout, loaded beside this one under another module name: the parent commit's step on the same box at the same clock.  With it
each of the two steps is preceded by an un-timed steady forward of its own policy (the parent's weights re-packed there, as this tree's are by the forward
behind `step`): both start from packed weights, behind the same kind of pass -- without that the parent's step paid its re-pack inside the timing and
sat behind the boundary's backward (measured: 3.0 ms and 1.2 ms of apparent difference).  Both
report their rounds, median and min - max spread next to `step`'s.  The boundary's time INCLUDES the re-pack of the weights torch's Adam changed (a loop of
boundary steps pays it inside the next forward); compare it with step + repack_ms.
Prints one JSON line per precision; needs a GPU."""
import argparse
import importlib.util
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
from vpt_amd import configs
from vpt_amd.idm_training import IDMTrainer
from vpt_amd.lib.policy import InverseActionPolicy
from vpt_amd.lib.types import idm_action_space

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--window", type=int, default=128)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--model", default="4x")
ap.add_argument("--precisions", default="bf16,fp16")
ap.add_argument("--profile-steps", type=int, default=0)
ap.add_argument("--train-cnn", action="store_true")
ap.add_argument("--boundary", action="store_true")
ap.add_argument("--parent-tree", default=None, help="package directory (video-pre-training_amd/) of another checkout, built, for the step_parent variant")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("idm_train_bench: no GPU (a step time is a GPU measurement; there is no CPU figure)")
# --train-cnn: the same protocol with IDMTrainer(train_cnn=True).step -- the whole network trained -- alternating with the train_cnn=False step and the two
# forwards in one process (step_full, step, forward, forward_steady per round); also reported: peak allocated HBM of a full step, and from one extra
# untimed full step under the op timer the new kernels' own times (ops.conv3d_t5_backward, and the conv wgrad / prepare per layer shape: the 128-wide
# stack-0 layer is the largest of each).

g = torch.Generator().manual_seed(1)
img = torch.randint(0, 256, (a.batch, a.window, 128, 128, 3), generator=g, dtype=torch.uint8).to("cuda")
buttons = torch.randint(0, 2, (a.batch, a.window, 20), generator=g).to("cuda")
camera = torch.randint(0, 11, (a.batch, a.window, 2), generator=g).to("cuda")
parent = None
if a.parent_tree:
    pdir = os.path.abspath(a.parent_tree)
    spec = importlib.util.spec_from_file_location("vpt_amd_parent", os.path.join(pdir, "__init__.py"), submodule_search_locations=[pdir])
    parent = importlib.util.module_from_spec(spec)
    sys.modules["vpt_amd_parent"] = parent
    spec.loader.exec_module(parent)
    from vpt_amd_parent import _native as pnative, configs as pconfigs
    from vpt_amd_parent.idm_training import IDMTrainer as ParentIDMTrainer
    from vpt_amd_parent.lib.policy import InverseActionPolicy as ParentPolicy
    from vpt_amd_parent.lib.types import idm_action_space as parent_space
    print("parent library:", pnative.lib_path(), file=sys.stderr)


def make_policy(prec, policy_cls=InverseActionPolicy, cfgs=configs, space=idm_action_space):
    pol = policy_cls(space(), pi_head_kwargs=dict(temperature=2.0), idm_net_kwargs=cfgs.idm_kwargs_for(a.model), precision=prec)
    cfgs.randomize_(pol, 0)
    return pol.to("cuda")


def spread(v):
    return dict(ms=[round(x, 2) for x in v], ms_median=round(statistics.median(v), 2), ms_min=round(min(v), 2), ms_max=round(max(v), 2),
                spread_ms=round(max(v) - min(v), 2))


results = []
for prec in a.precisions.split(","):
    pol = make_policy(prec)
    tr = IDMTrainer(pol, lr=1e-5, weight_decay=0.0)
    run = {"step": lambda: tr.step(img, buttons, camera), "forward": lambda: (pol._ensure_packed(), pol._engine.forward(img))}
    order = ("step", "forward", "forward_steady")
    before = {}                 # un-timed calls in front of a timed pass
    if a.train_cnn:
        tr_full = IDMTrainer(pol, lr=1e-5, weight_decay=0.0, train_cnn=True)
        run["stepfull"] = lambda: tr_full.step(img, buttons, camera)
        order = ("stepfull",) + order
    if a.boundary:
        pol_b = make_policy(prec)
        for n, p in pol_b.named_parameters():
            p.requires_grad_(not n.startswith(("net.conv3d_layer.", "net.img_process.cnn.")))
        opt = torch.optim.Adam([p for p in pol_b.parameters() if p.requires_grad], lr=1e-5)

        def boundary_step():
            with torch.enable_grad():
                (pd, _, _), _ = pol_b({"img": img}, None, None)
                loss = -pol_b.pi_head.logprob({"buttons": buttons, "camera": camera}, pd).mean()
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
        run["boundary"] = boundary_step
        order = order + ("boundary",)
    if parent is not None:
        pol_p = make_policy(prec, ParentPolicy, pconfigs, parent_space)
        tr_p = ParentIDMTrainer(pol_p, lr=1e-5, weight_decay=0.0)
        run["stepparent"] = lambda: tr_p.step(img, buttons, camera)
        before["step"] = lambda: pol._engine.forward(img)
        before["stepparent"] = lambda: (pol_p._ensure_packed(), pol_p._engine.forward(img))
        order = order + ("stepparent",)
    if a.profile_steps:
        for _ in range(a.profile_steps):
            run["stepfull" if a.train_cnn else "step"]()
        torch.cuda.synchronize()
        continue
    for k in dict.fromkeys(o.split("_")[0] for o in order):          # warm-up: every shape of the timed passes, every path
        if k == "stepfull":
            torch.cuda.reset_peak_memory_stats()
        run[k]()
        if k == "stepfull":
            torch.cuda.synchronize()
            peak_full = torch.cuda.max_memory_allocated()
    torch.cuda.synchronize()
    # a step leaves the packed weights stale and the NEXT call re-packs them (IDMEngine.pack): in the alternation that is the forward right behind
    # the step, so a second forward is timed behind it -- "forward" carries one pack, "forward_steady" none, and a loop of steps pays step + pack
    ms = {k: [] for k in order}
    with BoxSampler(torch.cuda.current_device()) as box:
        for _ in range(a.rounds):
            for k in order:
                before.get(k, lambda: None)()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run[k.split("_")[0]]()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in ms.items()}
    pack_ms = med["forward"] - med["forward_steady"]
    rec = dict(tool="idm_train_bench", model=a.model, precision=prec, batch=a.batch, window=a.window, rounds=a.rounds,
               trainable_params=int(sum(tr.params[n].numel() for n in tr.trainable)), params=int(sum(p.numel() for p in tr.params.values())),
               step_ms=[round(x, 2) for x in ms["step"]], forward_ms=[round(x, 2) for x in ms["forward"]],
               step_ms_median=round(med["step"], 2), forward_ms_median=round(med["forward"], 2),
               step_over_forward=round(med["step"] / med["forward"], 4),
               forward_steady_ms=[round(x, 2) for x in ms["forward_steady"]], forward_steady_ms_median=round(med["forward_steady"], 2),
               repack_ms=round(pack_ms, 2), step_plus_repack_over_forward_steady=round((med["step"] + pack_ms) / med["forward_steady"], 4),
               forward_spread=round((max(ms["forward"]) - min(ms["forward"])) / med["forward"], 4),
               step_frames_per_s=round(a.batch * a.window / med["step"] * 1e3, 1), steps_taken=tr.step_count, steps_skipped=tr.skipped_steps, box=box.record())
    rec["step"] = spread(ms["step"])
    if a.boundary:
        rec["boundary"] = dict(spread(ms["boundary"]), over_step=round(med["boundary"] / med["step"], 4), overflows=pol_b.grad_overflows)
    if parent is not None:
        rec["step_parent"] = dict(spread(ms["stepparent"]), step_minus_parent_ms=round(med["step"] - med["stepparent"], 2), steps_taken=tr_p.step_count)
    if a.train_cnn:
        from vpt_amd import ops
        ops.TIMER.reset()
        ops.TIMER.enabled = True
        run["stepfull"]()
        ops.TIMER.enabled = False
        kern = {k: v for k, v in ops.TIMER.summary().items() if k == "vpt_conv3d_t5_backward"}
        for pre in ("vpt_conv3x3_wgrad", "vpt_conv_backward_prepare"):
            kern.update({f"{n} [{w:.4g}]": v for (n, w), v in ops.TIMER.by_shape(pre).items()})
        ops.TIMER.reset()
        rec.update(step_full_ms=[round(x, 2) for x in ms["stepfull"]], step_full_ms_median=round(med["stepfull"], 2),
                   step_full_over_step=round(med["stepfull"] / med["step"], 4), step_full_over_forward_steady=round(med["stepfull"] / med["forward_steady"], 4),
                   step_full_frames_per_s=round(a.batch * a.window / med["stepfull"] * 1e3, 1), step_full_peak_allocated_gb=round(peak_full / 2 ** 30, 2),
                   full_trainable_params=int(sum(tr_full.params[n].numel() for n in tr_full.trainable)), full_steps_taken=tr_full.step_count,
                   full_steps_skipped=tr_full.skipped_steps,
                   kernels={k: dict(ms=round(v["ms"], 3), calls=v["calls"], gb_s=round(v["bytes"] / v["ms"] * 1e-6, 1) if v["bytes"] else None,
                                    tf_s=round(v["flops"] / v["ms"] * 1e-9, 1) if v["flops"] else None) for k, v in kern.items()})
    print(json.dumps(rec), flush=True)
    results.append(rec)
    del pol, tr, run
    if a.boundary:
        del pol_b, opt
    if parent is not None:
        del pol_p, tr_p
    if a.train_cnn:
        del tr_full
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
