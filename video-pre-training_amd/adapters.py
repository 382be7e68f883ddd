"""Low-rank adapters for the trunk: a frozen linear y = x W^T (+ b) gains  s (x A^T) B^T,  A fp32 [r, K], B fp32 [n, r], s = alpha / r.

    ad = LowRankAdapters(policy, targets=("net.recurrent_layer.blocks",), rank=16, alpha=16.0, seed=0)
    tr = BCTrainer(policy, train_cnn=False, adapters=ad, trainable=("pi_head",))        # also PPOTrainer, IDMTrainer
    ad.state_dict() / ad.load_state_dict()      the per-task artefact: the A / B tensors by name + rank, alpha, targets
    ad.merge_(policy) / ad.unmerge_(policy)     W <- W + s B A on the fp32 masters (ops.lowrank_merge) / the saved masters back, bit for bit
    ad.merged_state_dict(policy)                a `.weights`-compatible state dict

Adaptable are the linears of the transformer blocks, named as the reference names them: r.orc_block.{q,k,v,r}_layer (r_layer where the fused
projection holds it), r.orc_block.proj_layer, mlp0.layer, mlp1.layer.  Their parameters are `<module>.lora_A` / `<module>.lora_B`.  The policy
object stays the BASE until merge_: act(), RolloutBuffer and label_video see the update only after it; the trainers' saving forward and backward
(trainer_base.adapted_linear / adapted_linear_backward) run base GEMM + low-rank slice through the split-K epilogue.

Everything above the `ops` calls of merge_ / merged_state_dict is host code on names and small tensors and runs without a GPU."""
import math
from typing import Dict, Iterable, List, Sequence, Tuple

import torch

from . import ops
from .trainer_base import _selector_list, name_matches, stack_operands, unstack_gradients  # noqa: F401  (the index algebra lives beside the GEMMs)

MAX_RANK = ops.LOWRANK_MAX_RANK      # one 64-wide K step of the GEMM per adapter
_BLOCKS = "net.recurrent_layer.blocks."
_PROJECTIONS = ("q", "k", "v", "r")
LEAVES = tuple(f"r.orc_block.{c}_layer" for c in _PROJECTIONS) + ("r.orc_block.proj_layer", "mlp0.layer", "mlp1.layer")


def adaptable_modules(param_names: Iterable[str], fused: str = "qkvr") -> List[str]:
    """The adaptable module names among a policy's parameter names, in parameter order.  fused: the projections the block's first GEMM holds
    ("qkvr" the policy, "qkv" the IDM, whose r_layer no GEMM reaches)."""
    leaves = tuple(f"r.orc_block.{c}_layer" for c in _PROJECTIONS if c in fused) + LEAVES[len(_PROJECTIONS):]
    out = []
    for n in param_names:
        if n.startswith(_BLOCKS) and n.endswith(".weight"):
            mod = n[:-len(".weight")]
            rest = mod[len(_BLOCKS):].split(".", 1)
            if len(rest) == 2 and rest[0].isdigit() and rest[1] in leaves:
                out.append(mod)
    return out


def resolve_targets(param_names: Sequence[str], targets, fused: str = "qkvr") -> List[str]:
    """targets (selector strings, name_matches semantics on MODULE names: an exact module or a prefix ending at a `.` boundary) -> the adaptable
    modules they select, sorted by name.  ValueError: a selector that matches nothing; a selector that matches only modules that are not
    adaptable (net.lastlayer, net.img_process.linear, the heads, the CNN: those train densely through trainable=); an empty selection."""
    sel = _selector_list(targets, "LowRankAdapters(targets=)")
    names = list(param_names)
    able = adaptable_modules(names, fused)
    picked = []
    for s in sel:
        hit = [m for m in able if name_matches(s, m)]
        if not hit:
            if any(name_matches(s, n) for n in names):
                raise ValueError(f"LowRankAdapters(targets=): {s!r} is not adaptable (adaptable: {', '.join(LEAVES)} of a transformer block; "
                                 f"everything else trains densely through trainable=)")
            raise ValueError(f"LowRankAdapters(targets=): {s!r} matches no module")
        picked += hit
    if not picked:
        raise ValueError("LowRankAdapters(targets=): the selection is empty")
    return sorted(set(picked))


def init_tensors(shapes: Dict[str, Tuple[int, int]], rank: int, seed: int) -> Dict[str, torch.Tensor]:
    """{module: (n, K)} -> {"<module>.lora_A": U(-1/sqrt K, 1/sqrt K) fp32 [r, K], "<module>.lora_B": zeros [n, r]} on the CPU; the A's are
    drawn from ONE seeded CPU generator in name order (so a (targets, rank, seed) triple names one initialisation on every machine)."""
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    out = {}
    for mod in sorted(shapes):
        n, k = shapes[mod]
        bound = 1.0 / math.sqrt(k)
        out[mod + ".lora_A"] = (torch.rand(rank, k, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * bound
        out[mod + ".lora_B"] = torch.zeros(n, rank, dtype=torch.float32)
    return out


class LowRankAdapters:
    def __init__(self, policy, targets=("net.recurrent_layer.blocks",), rank: int = 16, alpha: float = 16.0, seed: int = 0):
        """policy: a MinecraftAgentPolicy or InverseActionPolicy (anything with named_parameters()); the adapters live on its device.
        targets: selector strings (resolve_targets); rank: 1 <= r <= 64; alpha: s = alpha / r; seed: init_tensors' generator seed."""
        if int(rank) != rank or not 1 <= int(rank) <= MAX_RANK:
            raise ValueError(f"LowRankAdapters: rank must be an integer in 1..{MAX_RANK}, got {rank!r}")
        if not (float(alpha) == float(alpha) and abs(float(alpha)) != float("inf")):
            raise ValueError(f"LowRankAdapters: alpha must be finite, got {alpha!r}")
        self.rank, self.alpha, self.seed = int(rank), float(alpha), int(seed)
        self.scale = self.alpha / self.rank
        self.fused = getattr(getattr(policy, "_engine", None), "_QKV", "qkvr")
        named = dict(policy.named_parameters())
        self.modules = resolve_targets(list(named), targets, self.fused)
        self.shapes = {m: tuple(named[m + ".weight"].shape) for m in self.modules}
        dev = next(iter(named.values())).device
        self.params: Dict[str, torch.Tensor] = {n: t.to(dev) for n, t in init_tensors(self.shapes, self.rank, self.seed).items()}
        self.merged = False
        self._policy_id = id(policy)
        self._saved: Dict[str, torch.Tensor] = {}

    # ---- names ------------------------------------------------------------------------------------
    @property
    def adapted_weights(self) -> List[str]:
        """The frozen base weights under an adapter (a trainer refuses them in trainable=)."""
        return [m + ".weight" for m in self.modules]

    def pair(self, module: str):
        return self.params[module + ".lora_A"], self.params[module + ".lora_B"]

    def operands(self, blocks: Sequence[Tuple[str, int]], k: int):
        """blocks: [(module, its rows)] -- the row blocks of ONE GEMM's [n, K] weight, in order (one module, or the fused projection's layers) ->
        (a_stack, sb, spans, the adapted modules among them) by stack_operands, or None when none of them is adapted."""
        entries, mods, row0 = [], [], 0
        for m, ni in blocks:
            if m in self.shapes:
                a, b = self.pair(m)
                entries.append((a, b, self.scale, row0))
                mods.append(m)
            row0 += ni
        if not entries:
            return None
        return stack_operands(entries, row0, k, device=entries[0][0].device) + (mods,)

    # ---- the artefact -----------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """The tensors by name + rank, alpha, targets (the resolved module names): a few MB per task."""
        sd = {n: t.detach().clone() for n, t in self.params.items()}
        sd.update(rank=self.rank, alpha=self.alpha, targets=list(self.modules))
        return sd

    def load_state_dict(self, sd: dict):
        """Refuses another target set, rank or policy shape (ValueError naming the difference); alpha is taken from the dict."""
        if list(sd.get("targets", ())) != list(self.modules):
            diff = sorted(set(sd.get("targets", ())) ^ set(self.modules))
            raise ValueError(f"LowRankAdapters.load_state_dict: another target set ({diff[:4]}{' ...' if len(diff) > 4 else ''} differ)")
        if int(sd["rank"]) != self.rank:
            raise ValueError(f"LowRankAdapters.load_state_dict: rank {sd['rank']} does not fit these rank-{self.rank} adapters")
        tensors = {n: t for n, t in sd.items() if n not in ("rank", "alpha", "targets")}
        if set(tensors) != set(self.params):
            raise ValueError(f"LowRankAdapters.load_state_dict: tensor names differ: {sorted(set(tensors) ^ set(self.params))[:4]} ...")
        bad = [n for n, t in tensors.items() if tuple(t.shape) != tuple(self.params[n].shape)]
        if bad:
            raise ValueError(f"LowRankAdapters.load_state_dict: another policy shape: {bad[0]} is {tuple(tensors[bad[0]].shape)}, "
                             f"expected {tuple(self.params[bad[0]].shape)}")
        if self.merged:
            raise RuntimeError("LowRankAdapters.load_state_dict: the adapters are merged into the policy; unmerge_ first")
        self.alpha = float(sd["alpha"])
        self.scale = self.alpha / self.rank
        for n, t in tensors.items():
            self.params[n].copy_(t)

    # ---- merge / unmerge / export -------------------------------------------------------------------
    def _weights_of(self, policy) -> Dict[str, torch.Tensor]:
        named = dict(policy.named_parameters())
        bad = [m for m in self.modules if m + ".weight" not in named or tuple(named[m + ".weight"].shape) != self.shapes[m]]
        if bad:
            raise ValueError(f"LowRankAdapters: the policy has no weight of shape {self.shapes[bad[0]]} at {bad[0]}.weight (another policy shape)")
        return {m: named[m + ".weight"] for m in self.modules}

    @torch.no_grad()
    def merge_(self, policy):
        """W <- W + s B A on the fp32 masters of `policy` (the policy these adapters were built on), by ops.lowrank_merge; the masters are kept
        for unmerge_.  The in-place writes move the parameters' version counters, so the packed weights and a captured acting graph refresh on
        the next forward (policy._ensure_packed).  While merged, a trainer holding these adapters refuses to step."""
        if id(policy) != self._policy_id:
            raise ValueError("LowRankAdapters.merge_: these adapters belong to another policy object (merged_state_dict exports into any policy of the same shape)")
        if self.merged:
            raise RuntimeError("LowRankAdapters.merge_: already merged")
        weights = self._weights_of(policy)
        for m, w in weights.items():
            a, b = self.pair(m)
            self._saved[m] = w.detach().clone()
            w.copy_(ops.lowrank_merge(self._saved[m], a.contiguous(), b.contiguous(), self.scale))
        self.merged = True
        return policy

    @torch.no_grad()
    def unmerge_(self, policy):
        """The saved masters back, bit for bit (a copy, no arithmetic)."""
        if id(policy) != self._policy_id:
            raise ValueError("LowRankAdapters.unmerge_: these adapters belong to another policy object")
        if not self.merged:
            raise RuntimeError("LowRankAdapters.unmerge_: not merged")
        for m, w in self._weights_of(policy).items():
            w.copy_(self._saved.pop(m))
        self.merged = False
        return policy

    @torch.no_grad()
    def merged_state_dict(self, policy) -> dict:
        """policy.state_dict() with every adapted weight replaced by W + s B A (ops.lowrank_merge on the base masters, also while merged): loads
        strict=True into a fresh policy of the same shape and saves as a `.weights` file."""
        weights = self._weights_of(policy)
        sd = {n: t.detach().clone() for n, t in policy.state_dict().items()}
        for m, w in weights.items():
            a, b = self.pair(m)
            base = self._saved[m] if (self.merged and id(policy) == self._policy_id) else w.detach()
            sd[m + ".weight"] = ops.lowrank_merge(base.contiguous(), a.contiguous(), b.contiguous(), self.scale)
        return sd

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.params.values())
