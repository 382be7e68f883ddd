"""Environment steps per second of a rollout: RolloutBuffer against INTEGRATION.md's hand loop around policy.act(), taking turns in ONE process.
python tools/rollout_bench.py [--model 2x] [--envs 1,8] [--horizon 128] [--chunk 32] [--rounds 5] [--warmup 1]

  collector     RolloutBuffer.begin / act / add_reward / finish (begin() turns on the aliased step graph; one record launch and one reward launch per step;
                the recurrent state copied once per chunk; one host read per rollout)
  hand          the hand loop written against the API that existed before the collector: policy.act() as it comes (its automatic step graph hands out a
                copy of the whole recurrent state on every step and its NaN assert reads the device on every step), six per-step scatters into [B, T]
                tensors, policy.v() and trainer.advantages() at the end.  The state references kept at chunk starts are valid because of those copies
  hand_aliased  the same loop after enable_step_graph(B, alias_state=True), with the clone of the state at every chunk start that mode needs to be correct:
                separates the per-step state copy from the per-step host read and scatters

The environment is synthetic and lives on the device: a pre-generated uint8 frame table, reward and resets cheap torch functions of the action and the step
(the same for every variant, nothing read back).  One policy object per variant (same weights) so that switching variants re-captures nothing.  Every variant
runs --warmup whole rollouts, then the variants take turns inside every round; a turn is one whole rollout (finish / v / advantages included) between two
HIP events.  The last line is one JSON record: steps per second (B T / rollout time) per variant and B, median / min / max over the rounds."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import __graft_entry__ as ge
ge.build()
from vpt_amd import configs
from vpt_amd.rl_training import PPOTrainer
from vpt_amd.rollout import RolloutBuffer
from vpt_amd.lib.policy import MinecraftAgentPolicy
from vpt_amd.lib.types import minecraft_action_space

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="2x"); ap.add_argument("--envs", default="1,8"); ap.add_argument("--horizon", type=int, default=128)
ap.add_argument("--chunk", type=int, default=32); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--table", type=int, default=32, help="frames per environment in the synthetic frame table")
a = ap.parse_args()
assert torch.cuda.is_available(), "rollout_bench needs a GPU"
dev = "cuda"
precision = os.environ.get("VPT_PRECISION", "bf16")
T, L = a.horizon, a.chunk


def make_policy():
    pol = MinecraftAgentPolicy(minecraft_action_space(), configs.policy_kwargs_for(a.model), dict(temperature=2.0), precision=precision)
    configs.randomize_(pol, 0)
    return pol.to(dev)


class SyntheticEnv:
    def __init__(self, b):
        self.table = torch.randint(0, 256, (a.table, b, 128, 128, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).to(dev)
        self.b, self.s = b, 0

    def reset(self):
        self.s = 0
        return self.table[0], torch.ones(self.b, dtype=torch.bool, device=dev)

    def step(self, action):
        bt, cam = action["buttons"][:, 0], action["camera"][:, 0]
        self.s += 1
        return self.table[self.s % a.table], (bt % 7).float() * 0.25 - cam.float() * 0.01, (bt + self.s) % 97 == 0


def clone_state(state):
    return [(None if m is None else m.clone(), (k.clone(), v.clone())) for m, (k, v) in state]


def collector_rollout(c):
    buf, env, tr = c["buf"], c["env"], c["trainer"]
    obs, first, state = c["obs"], c["first"], c["state"]
    buf.begin(state)
    for t in range(T):
        action, state = buf.act(obs, first, state, stochastic=True)
        obs, reward, first = env.step(action)
        buf.add_reward(reward, first)
    buf.finish(tr, obs, first, state)
    c["obs"], c["first"], c["state"] = obs, first, state


def hand_rollout(c):
    pol, env, tr, d = c["pol"], c["env"], c["trainer"], c["bufs"]
    obs, first, state = c["obs"], c["first"], c["state"]
    states = []
    for t in range(T):
        if t % L == 0:
            states.append(clone_state(state) if c["clone"] else state)
        action, state, info = pol.act({"img": obs}, first, state, stochastic=True)
        d["img"][:, t], d["first"][:, t] = obs, first
        d["act_b"][:, t], d["act_c"][:, t] = action["buttons"][:, 0], action["camera"][:, 0]
        d["old_lp"][:, t], d["vpred"][:, t] = info["log_prob"], info["vpred"].reshape(-1)
        obs, d["reward"][:, t], first = env.step(action)
    last_value = pol.v({"img": obs}, first, state)
    c["adv"], c["ret"] = tr.advantages(d["reward"], d["vpred"], d["first"], last_value, next_first=first)
    c["obs"], c["first"], c["state"], c["states"] = obs, first, state, states


def make_variant(name, b):
    pol = make_policy()
    c = dict(pol=pol, env=SyntheticEnv(b), trainer=PPOTrainer(pol, episode_starts="frame", optimizer_state=False), state=pol.initial_state(b))
    c["obs"], c["first"] = c["env"].reset()
    if name == "collector":
        c["buf"], c["run"] = RolloutBuffer(pol, num_envs=b, horizon=T, chunk_len=L), collector_rollout
        return c
    z = lambda dtype, *shape: torch.zeros(b, T, *shape, dtype=dtype, device=dev)
    c["bufs"] = dict(img=z(torch.uint8, 128, 128, 3), first=z(torch.bool), act_b=z(torch.int64), act_c=z(torch.int64), old_lp=z(torch.float32),
                     vpred=z(torch.float32), reward=z(torch.float32))
    c["clone"], c["run"] = name == "hand_aliased", hand_rollout
    if name == "hand_aliased":
        pol.enable_step_graph(b, alias_state=True)
    return c


def timed(c):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    c["run"](c)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


rec = dict(model=a.model, precision=precision, horizon=T, chunk=L, rounds=a.rounds, warmup=a.warmup, envs={})
for b in [int(x) for x in a.envs.split(",")]:
    variants = {name: make_variant(name, b) for name in ("collector", "hand", "hand_aliased")}
    for c in variants.values():
        for _ in range(a.warmup):
            c["run"](c)
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, c in variants.items():
            ms[name].append(timed(c))
    out = {}
    for name, xs in ms.items():
        sps = [b * T / (x * 1e-3) for x in xs]
        out[name] = dict(steps_per_s_median=round(statistics.median(sps), 1), steps_per_s_min=round(min(sps), 1), steps_per_s_max=round(max(sps), 1),
                         rollout_ms_median=round(statistics.median(xs), 2))
        sg = variants[name]["pol"]._step_graph
        out[name]["step_graph"] = None if sg is None else ("aliased" if sg["alias"] else "copies")
        print(f"B={b} {name:13s} {out[name]['steps_per_s_median']:9.1f} steps/s  (min {out[name]['steps_per_s_min']:.1f}, max {out[name]['steps_per_s_max']:.1f}; "
              f"{out[name]['rollout_ms_median']:.1f} ms per rollout of {T}; step graph: {out[name]['step_graph']})", flush=True)
    out["collector_over_hand"] = round(out["collector"]["steps_per_s_median"] / out["hand"]["steps_per_s_median"], 4)
    out["collector_over_hand_aliased"] = round(out["collector"]["steps_per_s_median"] / out["hand_aliased"]["steps_per_s_median"], 4)
    rec["envs"][str(b)] = out
    del variants
    torch.cuda.empty_cache()
print(json.dumps(rec))
