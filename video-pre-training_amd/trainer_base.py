"""What BCTrainer, PPOTrainer and IDMTrainer share behind the CNN (ONE copy each): the optimiser state and its checkpoint, the frame-weight check and
the record-based loss, the fp16 un-scaling, the optimiser tail of step(), and the trunk -- its saving forward from the dense layer's output `d` to
`x_trunk`, and its backward from the head logits' gradient down to `dd` = d loss / d `d`.

The two trunks differ in five places, each a class attribute or a hook of TrainerBase:
    attention        _attention_backward (BC: the masked kernel + the b_nd gradient; IDM: the mask-"none" kernel), the `attend` argument of the forward
    fused_qkv        "qkvr": r_layer sits in the fused projection, its gradients come out of that GEMM's wgrad and bias sum; "qkv": r_layer is unreached
    head_params      the rows of the fused head matrix (BC: buttons, camera, value; IDM: buttons, camera)
    has_lastlayer    net.lastlayer between x_trunk and final_ln (BC)
    final_ln_relu    final_ln reads relu(x_trunk) (IDM)
The CNN's part of either pass stays with cnn_training.CnnTrainingMixin and the trainers' own chunk loops.

Partial fine-tuning lives here too: which tensors train (select_trainable, resolve_param_groups: host code on names), the trunk
backward that stops at the first unit holding a trainable tensor, and the per-group Adam launch of the optimiser tail.

So do low-rank adapters (adapters.LowRankAdapters): the adapted GEMMs (adapted_linear, adapted_linear_backward: base product + low-rank
slice through the split-K epilogue), the stacked operands of the fused projection, and the places in the trunk's two passes that take them."""
import contextlib
from typing import Dict, List, Optional

import torch

from . import ops
from .cnn_training import CnnTrainingMixin


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def linear_backward(dy16: torch.Tensor, n: int, x16: Optional[torch.Tensor], weight: torch.Tensor, need_dx: bool = True,
                    res: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                    dx_f32: bool = True, dx_bf16_ld: Optional[int] = None, need_dw: bool = True):
    """Backward of y = x W^T on the MFMA GEMM kernel.
    dy16: bf16 [M, Np] (Np >= n, Np % 64 == 0, padding zero); x16: bf16 [M, K]; weight fp32 [n, K].
    Returns (dx fp32 or None, dx bf16 or None, dW fp32 [n, K] or None).
    dgrad:  dx = dy W      -> GEMM(A = dy, weights = W^T packed), optional ReLU gate `mask` and skip-sum `res`;
    wgrad:  dW = dy^T x    -> the TN GEMM (ops.linear_wgrad): both operands row-major over the M frames, no transposes."""
    np_ = dy16.shape[1]
    k = weight.shape[1]
    dx32 = dx16 = dw = None
    if need_dx:   # W^T packed straight from the fp32 master by one kernel (was: zero, transpose, cast, permute -- four tensor ops)
        wt = ops.pack_linear(weight.contiguous(), transposed=True, k_pad=np_, dtype=dy16.dtype)
        dx32, dx16 = ops.linear(dy16, wt, k, res=res, mask=mask, out_f32=dx_f32,
                                out_bf16=dx_bf16_ld is not None, out_bf16_ld=dx_bf16_ld)
        del wt
    if need_dw:       # dW = dy^T x straight from the row-major activations (vpt_gemm_tn_kernel: LDS transpose reads, no copies)
        dw = ops.linear_wgrad(dy16, x16, np_)[:n]
    return dx32, dx16, dw


# ---- low-rank adapters: the operands of one adapted GEMM, its forward and its backward, built from the existing kernels ----------
def stack_operands(entries, n: int, k: int, device=None):
    """entries: [(A fp32 [r_i, K], B fp32 [n_i, r_i], s_i, row0_i)] -- adapter i acts on output rows row0_i .. row0_i + n_i of an [n, K] weight ->
    (a_stack fp32 [R, K]: the A's stacked, zero rows up to R = sum r_i rounded up to 64, the GEMM's K step; sb fp32 [n, R]: s_i B_i placed
    block-diagonally, zeros elsewhere; spans [(row0_i, n_i, col0_i, r_i)]).  Then  sum_i s_i (x A_i^T) B_i^T  at its rows  ==  (x a_stack^T) sb^T.
    s is applied HERE, on fp32, never to a 16-bit activation.  Plain torch on small tensors: runs on the CPU as well."""
    rp = _round_up(sum(a.shape[0] for a, _, _, _ in entries), 64)
    a_stack = torch.zeros(rp, k, dtype=torch.float32, device=device)
    sb = torch.zeros(n, rp, dtype=torch.float32, device=device)
    spans, c0 = [], 0
    for a, b, s, row0 in entries:
        r, ni = a.shape[0], b.shape[0]
        a_stack[c0:c0 + r] = a
        sb[row0:row0 + ni, c0:c0 + r] = b * s
        spans.append((row0, ni, c0, r))
        c0 += r
    return a_stack, sb, spans


def unstack_gradients(da_stack: torch.Tensor, db_stack: torch.Tensor, spans):
    """The inverse on the gradients: da_stack [R, K] = d / d a_stack, db_stack [n, R] = dy^T u (d / d sb) -> [(dA_i [r_i, K], dy^T u's DIAGONAL
    block [n_i, r_i])] -- dB_i is s_i times the latter; the off-diagonal blocks of a fused projection belong to no parameter and are dropped."""
    return [(da_stack[c0:c0 + r], db_stack[row0:row0 + ni, c0:c0 + r]) for row0, ni, c0, r in spans]


def adapted_linear(x16: torch.Tensor, wpk: torch.Tensor, n: int, a_stack: torch.Tensor, sb: torch.Tensor, bias=None, res=None, relu: bool = False,
                   out_f32: bool = True, out_bf16: bool = False, mask=None, out_bf16_ld: Optional[int] = None, splitk=1, tiling: str = "auto"):
    """y = epi(x W^T (+) u16 (sB)^T),  u16 = rnd16(x A^T)  -> (fp32 [M, n] or None, 16-bit or None, u16 [M, R]) with ops.linear's options.
    Three GEMMs and the split-K epilogue: u16 (ops.linear, 16-bit output); the base product to raw fp32 slice(s), by the kernel and K split the
    unadapted call takes (ops.linear_partials); the low-rank product into one more slice; vpt_linear_splitk_epilogue sums the slices in order and
    applies bias -> ReLU -> gate -> + res.  With B = 0 the extra slice is exact zeros and the result is ops.linear's, bit for bit."""
    dt = x16.dtype
    rp = a_stack.shape[0]
    _, u16 = ops.linear(x16, ops.pack_linear(a_stack, dtype=dt), rp, out_f32=False, out_bf16=True, splitk=splitk, tiling=tiling)
    part, sk = ops.linear_partials(x16, wpk, n, extra=1, splitk=splitk, tiling=tiling)
    ops.linear(u16, ops.pack_linear(sb, dtype=dt), n, out=part[sk], tiling=tiling)
    o32, o16 = ops.splitk_epilogue(part, bias=bias, res=res, relu=relu, out_f32=out_f32, out_bf16=out_bf16, mask=mask, out_bf16_ld=out_bf16_ld, dtype=dt)
    return o32, o16, u16


def adapted_linear_backward(dy16: torch.Tensor, n: int, x16: torch.Tensor, weight: torch.Tensor, a_stack: torch.Tensor, sb: torch.Tensor,
                            u16: torch.Tensor, need_dx: bool = True, res=None, mask=None, dx_f32: bool = True, dx_bf16_ld: Optional[int] = None,
                            need_dw: bool = False):
    """Backward of adapted_linear on the same kernels; arguments as linear_backward's + the forward's operands and its saved u16.
    -> (dx fp32 or None, dx 16-bit or None, dW or None, da_stack fp32 [R, K], dy^T u16 fp32 [n, R]):
        du16 = rnd16(dy (sB));   dx = epi(dy W (+) du16 A) with linear_backward's gate and skip;   d a_stack = du16^T x;   d sb = dy^T u16.
    need_dw: the dense [n, K] wgrad GEMM as well -- a fused projection in which a layer WITHOUT an adapter trains; a frozen adapted weight
    launches none."""
    np_, k, rp, dt = dy16.shape[1], weight.shape[1], a_stack.shape[0], dy16.dtype
    _, du16 = ops.linear(dy16, ops.pack_linear(sb, transposed=True, k_pad=np_, dtype=dt), rp, out_f32=False, out_bf16=True)
    dx32 = dx16 = dw = None
    if need_dx:
        wt = ops.pack_linear(weight.contiguous(), transposed=True, k_pad=np_, dtype=dt)
        part, sk = ops.linear_partials(dy16, wt, k, extra=1)
        ops.linear(du16, ops.pack_linear(a_stack, transposed=True, k_pad=rp, dtype=dt), k, out=part[sk])
        dx32, dx16 = ops.splitk_epilogue(part, res=res, mask=mask, out_f32=dx_f32, out_bf16=dx_bf16_ld is not None, out_bf16_ld=dx_bf16_ld, dtype=dt)
        del wt, part
    if need_dw:
        dw = ops.linear_wgrad(dy16, x16, np_)[:n]
    db_stack = ops.linear_wgrad(dy16, u16, np_)[:n]
    da_stack = ops.linear_wgrad(du16, x16, rp)
    return dx32, dx16, dw, da_stack, db_stack


# ---- which tensors train: name selection and parameter groups, plain host code on names only ---------------------------------
def name_matches(selector: str, name: str) -> bool:
    """A selector is an exact parameter name or a module prefix ending at a `.` boundary: "net.recurrent_layer.blocks.1" matches
    "net.recurrent_layer.blocks.1.mlp0.layer.weight", never "net.recurrent_layer.blocks.10...".  (A trailing "." is accepted and means the same.)"""
    s = selector[:-1] if selector.endswith(".") else selector
    return name == s or name.startswith(s + ".")


def _selector_list(selection, what: str) -> List[str]:
    sel = [selection] if isinstance(selection, str) else list(selection)
    bad = [s for s in sel if not isinstance(s, str) or not s.strip(".")]
    if bad:
        raise ValueError(f"{what}: selectors must be non-empty parameter names or module prefixes, got {bad!r}")
    return sel


def select_trainable(names: List[str], rule, selection, who: str = "trainer") -> List[str]:
    """The effective trainable set, in the order of `names`: the trainer's own rule(name) AND the selection.
    selection: None (the rule alone), an iterable of selector strings (name_matches) or a callable name -> bool.
    ValueError, naming the offenders: a string that matches no parameter; a string that selects a tensor the rule excludes; an empty result.
    (A callable is a filter: what it accepts outside the rule is left out silently -- `lambda n: True` is the rule's own set.)"""
    names = list(names)
    ruled = [n for n in names if rule(n)]
    if selection is None:
        return ruled
    if callable(selection):
        out = [n for n in ruled if selection(n)]
    else:
        sel = _selector_list(selection, f"{who}(trainable=)")
        unmatched = [s for s in sel if not any(name_matches(s, n) for n in names)]
        if unmatched:
            raise ValueError(f"{who}(trainable=): {unmatched!r} match no parameter")
        picked = [n for n in names if any(name_matches(s, n) for s in sel)]
        ruled_set = set(ruled)
        excluded = [n for n in picked if n not in ruled_set]
        if excluded:
            raise ValueError(f"{who}(trainable=): this trainer does not train {excluded[:6]!r}{' ...' if len(excluded) > 6 else ''} "
                             f"({len(excluded)} selected tensors are outside its own rule)")
        out = picked
    if not out:
        raise ValueError(f"{who}(trainable=): the selection leaves no trainable parameter")
    return out


def resolve_param_groups(names: List[str], trainable: List[str], param_groups, who: str = "trainer"):
    """param_groups = [dict(params=<selector strings>, lr_scale=1.0, weight_decay=<the trainer's>), ...] ->
    (the groups normalised to dict(params=[strings], lr_scale=float, weight_decay=float | None) -- what state_dict() carries --,
     {trainable name: index of its group}).  Names in no group use the trainer's values.  ValueError: an unknown key, a selector that matches no
    parameter, a group naming a tensor that is not trainable, a name in two groups."""
    groups, owner = [], {}
    tset = set(trainable)
    for gi, grp in enumerate(param_groups or ()):
        if not isinstance(grp, dict) or "params" not in grp or set(grp) - {"params", "lr_scale", "weight_decay"}:
            raise ValueError(f"{who}(param_groups=): group {gi} must be dict(params=..., lr_scale=..., weight_decay=...), got {grp!r}")
        sel = _selector_list(grp["params"], f"{who}(param_groups=)[{gi}]")
        unmatched = [s for s in sel if not any(name_matches(s, n) for n in names)]
        if unmatched:
            raise ValueError(f"{who}(param_groups=): group {gi}: {unmatched!r} match no parameter")
        picked = [n for n in names if any(name_matches(s, n) for s in sel)]
        frozen = [n for n in picked if n not in tset]
        if frozen:
            raise ValueError(f"{who}(param_groups=): group {gi} names tensors that are not trainable: {frozen[:6]!r}{' ...' if len(frozen) > 6 else ''}")
        twice = [n for n in picked if n in owner]
        if twice:
            raise ValueError(f"{who}(param_groups=): {twice[:6]!r} are in group {owner[twice[0]]} and in group {gi}")
        lr_scale = float(grp.get("lr_scale", 1.0))
        wd = grp.get("weight_decay")
        if not (lr_scale >= 0.0 and lr_scale != float("inf")) or (wd is not None and not (float(wd) >= 0.0 and float(wd) != float("inf"))):
            raise ValueError(f"{who}(param_groups=): group {gi}: lr_scale and weight_decay must be finite and non-negative, got {grp!r}")
        for n in picked:
            owner[n] = gi
        groups.append(dict(params=sel, lr_scale=lr_scale, weight_decay=None if wd is None else float(wd)))
    return groups, owner


class TrainerBase(CnnTrainingMixin):
    fused_qkv = "qkvr"           # the fused projection's name in the engine's packed weights and in saved[l]; "qkv": without r_layer (mask "none")
    head_params = ("pi_head.buttons.linear_layer", "pi_head.camera.linear_layer", "value_head.linear")      # the fused head matrix, row blocks in order
    has_lastlayer = True         # net.lastlayer between the blocks and final_ln
    final_ln_relu = False        # final_ln reads relu(its input)
    max_grad_norm = None         # None: no clipping (what the reference's script does); 5.0: what it meant; float("inf"): measure, never clip
    last_grad_norm = None        # fp32 device scalar of the last step that measured (max_grad_norm set)
    # partial fine-tuning.  The class values are the default-constructed trainer's: everything its own rule trains, one group
    _subset = None               # None: trainable=None, today's set on today's code path; else the frozenset of the effective names
    _cut = -1                    # the trunk unit (see _unit_level) the backward stops at; -1: it runs down to dd
    _cnn_backward = True         # with train_cnn: some CNN-side tensor is trainable, so the CNN activations are kept and its backward runs
    param_groups = ()            # the normalised groups of resolve_param_groups
    _group_of: Dict[str, int] = {}
    decoupled_weight_decay = False
    adapters = None              # low-rank adapters (adapters.LowRankAdapters); None: the code path that has always run

    def _init_trainer(self, policy, lr, weight_decay, betas, eps, train_cnn, optimizer_state, loss_scale, scale_growth_interval, max_grad_norm,
                      trainable=None, param_groups=None, decoupled_weight_decay=False, adapters=None):
        """The state every trainer keeps (the constructors' docstrings say what the arguments mean).
        trainable / param_groups / decoupled_weight_decay: partial fine-tuning, shared by the three trainers --
        trainable: None (default: the trainer's own rule, on the code path that has always run), an iterable of strings -- exact parameter names
        or module prefixes ending at a `.` boundary, e.g. "pi_head", "net.lastlayer", "net.recurrent_layer.blocks.3" -- or a callable name -> bool.
        The effective set is the rule AND the selection (select_trainable: ValueError on a string that matches nothing, on a string that selects
        what the rule excludes, on an empty set).  self.trainable, the Adam moments, the arenas, the norm and the clip cover the effective set only.
        The backward then stops at the first trunk unit (in forward order: net.img_process.linear, net.pre_lstm_ln, the blocks, net.lastlayer,
        net.final_ln, the heads) that holds a trainable tensor -- and inside that unit where nothing trainable is left --, launches no wgrad GEMM
        and no bias sum for a frozen tensor above it, and the saving forward keeps nothing the shortened backward does not read.  Inside the CNN
        nothing is cut: if any CNN tensor is trainable its whole backward runs and the frozen CNN tensors' gradients are dropped.
        param_groups: [dict(params=<strings as above>, lr_scale=1.0, weight_decay=<the trainer's>), ...]; lr_scale multiplies self.lr at step time.
        decoupled_weight_decay: torch.optim.AdamW's decay instead of Adam's L2 term.  Either makes step() use ops.adam_step_groups_ (one launch).
        adapters: an adapters.LowRankAdapters built on this policy.  Its `<module>.lora_A` / `.lora_B` tensors join self.params and
        always train; trainable=None then means "no base tensor", strings (or a callable) add base tensors as above, and an adapted weight among
        them is a ValueError (it is frozen under its adapter).  The moments, the norm and clip, the overflow check, micro-batches, loss scaling and
        state_dict() run over adapters + selection through the same code; adapter names are selectable in param_groups; the cut is the lowest
        level holding a trainable base tensor or an adapted module.  The saving forward and the backward take the adapted GEMMs (adapted_linear,
        adapted_linear_backward) for adapted modules and the unchanged calls everywhere else."""
        self.train_cnn = bool(train_cnn)
        self.max_grad_norm = self._checked_max_grad_norm(max_grad_norm)
        self.policy = policy
        self.engine = policy._engine
        self.dtype = self.engine.dtype
        self.scaled = self.engine.precision == "fp16"
        self.loss_scale = float(loss_scale) if loss_scale is not None else (256.0 if self.scaled else 1.0)
        self.scale_growth_interval, self._clean_steps, self.skipped_steps = int(scale_growth_interval), 0, 0
        self.lr, self.wd, self.betas, self.eps = lr, weight_decay, betas, eps
        self.step_count = 0
        self._cnn_flags_from_env()       # gated_dgrad, fused_pool, fold_n_backward, fold_n_backward0 (cnn_training.py)
        self.params: Dict[str, torch.nn.Parameter] = dict(policy.named_parameters())
        names = self._selectable_names()
        if adapters is None:
            self.trainable = select_trainable(list(self.params) if trainable is None else names, self._is_trainable, trainable, type(self).__name__)
        else:
            who = type(self).__name__
            if getattr(adapters, "_policy_id", None) != id(policy):
                raise ValueError(f"{who}(adapters=): these adapters were built on another policy object")
            if adapters.fused != self.fused_qkv:
                raise ValueError(f"{who}(adapters=): the adapters were resolved for a fused {adapters.fused!r} projection, this trainer runs {self.fused_qkv!r}")
            base = [] if trainable is None else select_trainable(names, self._is_trainable, trainable, who)
            clash = sorted(set(base) & set(adapters.adapted_weights))
            if clash:
                raise ValueError(f"{who}(trainable=): {clash[:6]!r}{' ...' if len(clash) > 6 else ''} are frozen under an adapter; train the adapter or the weight, not both")
            self.adapters = adapters
            self.params.update(adapters.params)      # the same tensor objects: the Adam launch updates the adapters in place
            names = names + list(adapters.params)
            self.trainable = base + list(adapters.params)
        if trainable is not None or adapters is not None:
            self._subset = frozenset(self.trainable)
            self._cut = min(self._unit_level(n) for n in self.trainable)
            self._cnn_backward = self.train_cnn and self._cut < 0
        self.param_groups, self._group_of = resolve_param_groups(names, self.trainable, param_groups, type(self).__name__)
        self.decoupled_weight_decay = bool(decoupled_weight_decay)
        self.m ={n: torch.zeros_like(self.params[n], dtype=torch.float32) for n in self.trainable} if optimizer_state else {}
        self.v = {n: torch.zeros_like(self.params[n], dtype=torch.float32) for n in self.trainable} if optimizer_state else {}

    def _is_trainable(self, name: str) -> bool:
        """The trainer's own rule (reads self.train_cnn and self.params only)."""
        raise NotImplementedError

    @classmethod
    def rule_trainable(cls, params: Dict[str, torch.Tensor], train_cnn: bool) -> List[str]:
        """The names a cls(policy, train_cnn=train_cnn) trains by default, without building one (the autograd boundary compares them with the
        parameters that require grad)."""
        probe = object.__new__(cls)
        probe.train_cnn, probe.params = bool(train_cnn), params
        return [n for n in params if probe._is_trainable(n)]

    def _selectable_names(self) -> List[str]:
        """The names a selector string is matched against: the parameters minus what no optimiser could ever move -- an empty tensor (the IDM's
        b_nd [10, 0]) and the value normaliser's statistics (Parameters only so that they travel with the state_dict; they move by update()).
        So "value_head" under PPOTrainer and a whole block under IDMTrainer select what there is to train instead of raising."""
        return [n for n, p in self.params.items() if p.numel() and not n.startswith("value_head.normalizer.") and not n.endswith((".lora_A", ".lora_B"))]

    def _unit_level(self, name: str) -> int:
        """The trunk unit a parameter belongs to, in forward order: 0 net.img_process.linear, 1 net.pre_lstm_ln, 2 + l block l, 2 + n net.lastlayer,
        3 + n net.final_ln, 4 + n the fused heads; -1: in front of the trunk (the CNN, the IDM's temporal conv)."""
        n = self.engine.cfg["n_layers"]
        blocks = "net.recurrent_layer.blocks."
        if name.startswith(blocks):
            return 2 + int(name[len(blocks):].split(".", 1)[0])
        for prefix, level in (("net.img_process.linear.", 0), ("net.pre_lstm_ln.", 1), ("net.lastlayer.", 2 + n), ("net.final_ln.", 3 + n),
                              ("pi_head.", 4 + n), ("value_head.", 4 + n)):
            if name.startswith(prefix):
                return level
        return -1

    @staticmethod
    def _checked_max_grad_norm(max_grad_norm):
        if max_grad_norm is None:
            return None
        v = float(max_grad_norm)
        if not v > 0:
            raise ValueError(f"max_grad_norm must be positive (float('inf'): measure only) or None, got {max_grad_norm!r}")
        return v

    # ---- checkpoint / resume ---------------------------------------------------
    def state_dict(self) -> dict:
        """Optimizer state next to the policy's own `.weights` state_dict (behavioural_cloning.py:131-132 saves only the
        latter): Adam moments keyed by the reference's parameter names, the step count and the hyper-parameters."""
        self._need_optimizer_state()
        sd = dict(step=self.step_count, lr=self.lr, weight_decay=self.wd, betas=tuple(self.betas), eps=self.eps,
                  loss_scale=self.loss_scale, train_cnn=self.train_cnn, max_grad_norm=self.max_grad_norm,
                  exp_avg={n: t.detach().clone() for n, t in self.m.items()},
                  exp_avg_sq={n: t.detach().clone() for n, t in self.v.items()})
        # partial fine-tuning: what a default-constructed trainer does not have it does not write (its dict is the one it always wrote)
        if self._subset is not None:
            sd["trainable"] = list(self.trainable)
        if self.param_groups or self.decoupled_weight_decay:
            sd["param_groups"] = [dict(g, params=list(g["params"])) for g in self.param_groups]
            sd["decoupled_weight_decay"] = self.decoupled_weight_decay
        return sd

    def _need_optimizer_state(self):
        if not self.m and self.trainable:
            raise RuntimeError(f"this {type(self).__name__} was built with optimizer_state=False (gradients only): step / state_dict / load_state_dict need the Adam moments")

    def load_state_dict(self, sd: dict):
        self._need_optimizer_state()
        if self.scaled and "loss_scale" in sd:
            self.loss_scale = float(sd["loss_scale"])
        if "max_grad_norm" in sd:           # (dicts written before the key existed keep the constructor's value)
            self.max_grad_norm = self._checked_max_grad_norm(sd["max_grad_norm"])
        if set(sd["exp_avg"]) != set(self.m):
            raise KeyError(f"optimizer state does not match the trainable parameters: {sorted(set(sd['exp_avg']) ^ set(self.m))[:4]} ...")
        if "param_groups" in sd:            # (a dict without them leaves the constructor's groups and flag in place)
            self.param_groups, self._group_of = resolve_param_groups(self._selectable_names() + (list(self.adapters.params) if self.adapters is not None else []),
                                                                          self.trainable, sd["param_groups"], type(self).__name__)
            self.decoupled_weight_decay = bool(sd.get("decoupled_weight_decay", False))
        self.step_count = int(sd["step"])
        self.lr, self.wd, self.betas, self.eps = sd["lr"], sd["weight_decay"], tuple(sd["betas"]), sd["eps"]
        for n in self.m:
            self.m[n].copy_(sd["exp_avg"][n])
            self.v[n].copy_(sd["exp_avg_sq"][n])

    # ---- fp16 loss scaling ------------------------------------------------------------------------
    def grad_unscale(self, global_frames: float) -> float:
        """What loss_and_grads(unscaled=False)'s gradients must be multiplied by to be d(mean loss)/d(parameter): 1 in bf16.  (global_frames: the
        global weight sum when the step carries frame weights.)"""
        return 1.0 / (self.loss_scale * global_frames) if self.scaled else 1.0

    def _unscale_(self, g: Dict[str, torch.Tensor], global_frames: float):
        """loss_and_grads(unscaled=True) in the fp16 mode: the loss-scaled gradients -> those of the mean loss, in place."""
        f = self.grad_unscale(global_frames)
        for t_ in g.values():
            t_.mul_(f)

    # ---- frame weights, the loss and the metrics from the loss kernels' records ----------------------
    @staticmethod
    def _weights_on_device(frame_weight, img_u8):
        """[B, T] weights -> (fp32 [M] on the images' device, [their fp64 sum, their fp64 minimum] as device scalars for the caller's ONE host transfer)."""
        m = img_u8.shape[0] * img_u8.shape[1]
        w = torch.as_tensor(frame_weight)
        if w.numel() != m:
            raise ValueError(f"frame_weight must hold one weight per frame ([{img_u8.shape[0]}, {img_u8.shape[1]}]), got {tuple(w.shape)}")
        w = w.reshape(m).to(device=img_u8.device, dtype=torch.float32).contiguous()
        w64 = w.to(torch.float64)
        return w, [w64.sum(), w64.min()]

    @staticmethod
    def _check_weight_probe(wsum: float, wmin: float):
        """The host half: a negative or non-finite weight raises ValueError (a NaN makes the minimum NaN, an infinity the sum infinite)."""
        if not (wmin >= 0.0) or wsum != wsum or wsum in (float("inf"), float("-inf")):
            raise ValueError(f"frame_weight must be finite and non-negative (min {wmin}, sum {wsum})")

    @staticmethod
    def _checked_weights(frame_weight, img_u8):
        """[B, T] weights -> (fp32 [M] on the images' device, their fp64 sum as a host float).  The sum and the minimum come to the host in ONE
        transfer; a negative or non-finite weight raises ValueError."""
        w, probe = TrainerBase._weights_on_device(frame_weight, img_u8)
        wsum, wmin = torch.stack(probe).tolist()
        TrainerBase._check_weight_probe(wsum, wmin)
        return w, wsum

    @staticmethod
    def _record_loss(frame_out, w, wsum):
        """sum w nll / sum w of one rank from the kernel's per-frame records, in the ARITHMETIC OF THE DEFAULT PATH: per frame nll_b + nll_c (the
        negated sum of the two picked log-probs, exactly), then torch's mean over the frames, then the factor M / sum w.  With every weight 1 each
        step is the default path's own -- w x is x, the mean of the negated values is the negated mean, the factor is 1.0 -- so frame_weight=ones (and
        metrics={} alone) returns the default path's loss bit for bit; the totals' fixed tree adds the same terms in another association and lands an
        ulp away, which is why the returned loss is not read from them (they feed the metrics and the reduction over ranks).  M floats per step."""
        nll = frame_out[:, 0] + frame_out[:, 1]
        if w is None:
            return nll.mean()
        wn = torch.where(w != 0, w * nll, torch.zeros_like(nll))          # a zero-weight frame counts an exact zero whatever its record holds
        return wn.mean() * (nll.numel() / wsum if wsum else float("nan"))

    @staticmethod
    def _fill_metrics(metrics: dict, totals, frame_out, bsz: int, t: int):
        """totals [8] (ops.bc_loss's / ops.idm_loss's, or their sum over ranks) + this rank's records -> the metrics dict; device arithmetic only."""
        ws = totals[6]
        metrics.update(loss=(totals[0] + totals[1]) / ws, nll_buttons=totals[0] / ws, nll_camera=totals[1] / ws,
                       entropy_buttons=totals[2] / ws, entropy_camera=totals[3] / ws, acc_buttons=totals[4] / ws, acc_camera=totals[5] / ws,
                       weight_sum=ws, frames=totals[7])
        if frame_out is not None:
            metrics.update(frame_nll=(frame_out[:, 0] + frame_out[:, 1]).view(bsz, t), frame_out=frame_out.view(bsz, t, 8))

    # ---- gradient accumulation over micro-batches: a micro-batch is a data-parallel rank that runs later on the same card --------
    @staticmethod
    def micro_batch_rows(bsz: int, micro_batches: int) -> List[tuple]:
        """The [begin, end) row groups the batch's `bsz` sequences are cut into: distributed.shard_range, the cut of the data-parallel step.
        ValueError unless 1 <= micro_batches <= bsz (every group holds at least one sequence)."""
        from .distributed import shard_range
        k = int(micro_batches)
        if k != micro_batches or k < 1 or k > int(bsz):
            raise ValueError(f"micro_batches must be an integer in 1..{int(bsz)} (the batch's sequences), got {micro_batches!r}")
        return [shard_range(int(bsz), i, k) for i in range(k)]

    @staticmethod
    def sum_totals(totals: List[torch.Tensor]) -> torch.Tensor:
        """The micro-batches' totals vectors (8 of ops.bc_loss / ops.idm_loss, 16 of ops.rl_loss) summed in fp64 IN ORDER, then rounded to fp32 --
        what the data-parallel step's final reduction does with the ranks' totals."""
        acc = totals[0].to(torch.float64)
        for t_ in totals[1:]:
            acc = acc + t_.to(torch.float64)
        return acc.to(torch.float32)

    @staticmethod
    def _tree_rows(tree, lo: int, hi: int):
        """Rows [lo, hi) of every tensor in a nest of tuples / lists (the recurrent state: [B, ...] leaves, None passes through)."""
        if tree is None:
            return None
        if isinstance(tree, torch.Tensor):
            return tree[lo:hi]
        return type(tree)(TrainerBase._tree_rows(x, lo, hi) for x in tree)

    @staticmethod
    def _tree_cat_rows(trees: list):
        """The inverse: the row-wise concatenation of nests of one structure, in order."""
        head = trees[0]
        if head is None:
            return None
        if isinstance(head, torch.Tensor):
            return torch.cat(trees, 0)
        return type(head)(TrainerBase._tree_cat_rows([tr[i] for tr in trees]) for i in range(len(head)))

    def _accumulate_grads(self, acc: Optional[Dict[str, torch.Tensor]], g: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """acc None: the first micro-batch's gradient tensors become the accumulators as they are (no arithmetic).  Otherwise acc[n] += g[n] for
        every trainable tensor in ONE ops.grad_accumulate_ launch."""
        names = [n for n in self.trainable if n in g]
        if acc is None:
            return {n: g[n].contiguous() for n in names}
        ops.grad_accumulate_([acc[n].view(-1) for n in names], [g[n].contiguous().view(-1) for n in names])
        return acc

    def _accumulated_window(self, rows: List[tuple], run_micro_batch, accumulate=None):
        """The loop every trainer's micro_batches=K shares.  run_micro_batch(k, lo, hi) -> (grads of rows [lo, hi) carrying the WINDOW's frame
        count, its totals vector, its frame records, anything else the trainer wants back), one micro-batch at a time: its gradient dict is
        folded into the accumulators and released -- with its activations, which run_micro_batch let go -- before the next forward starts.
        accumulate(k, acc, g) -> acc replaces _accumulate_grads (the data-parallel step accumulates in its arenas).
        -> (accumulated grads, totals summed by sum_totals, records concatenated to [M, .], the list of the extras)."""
        acc, totals, records, extras = None, [], [], []
        for k, (lo, hi) in enumerate(rows):
            g, tot, rec, extra = run_micro_batch(k, lo, hi)
            acc = self._accumulate_grads(acc, g) if accumulate is None else accumulate(k, acc, g)
            del g
            totals.append(tot); records.append(rec); extras.append(extra)
        return acc, self.sum_totals(totals), torch.cat(records, 0), extras

    # ---- the optimiser tail of every trainer's step(): the Adam launch, gradient-norm clipping and the loss-scale bookkeeping --------------
    def _optimizer_tail(self, loss, grads, grad_scale: float, device, metrics=None):
        """The Adam launch for every trainable tensor of `grads` + the bookkeeping -> (float(loss), skipped).
        One launch for all tensors (th.optim.Adam(policy.parameters()).step(), behavioural_cloning.py:122); in the fp16 mode it un-scales the
        gradients and is a no-op on the device when the overflow check (same table, one launch before) fired.
        max_grad_norm set (clip_grad_norm_ as behavioural_cloning.py:121 meant it): the norm of grads * grad_scale -- the gradients of the MEAN loss,
        after the all-reduce, whatever the loss scale -- is taken over the same table (that launch replaces the overflow check), the Adam launch
        multiplies by the clip coefficient on the device.  A non-finite norm skips the step on the device in BOTH formats (skipped_steps counts it;
        fp16 also halves its loss scale): torch.nn.utils.clip_grad_norm_ would instead write NaN into every parameter -- a deliberate difference.
        `metrics` (when given and max_grad_norm is set) gains grad_norm, clip_coef and grad_norm_per_tensor {name: norm}: device tensors."""
        self._check_adapters_ready()
        names = [n for n in self.trainable if n in grads]
        clip = self.max_grad_norm is not None
        found_inf = torch.zeros(1, dtype=torch.int32, device=device) if (self.scaled or clip) else None
        per = torch.empty(len(names), dtype=torch.float32, device=device) if (clip and metrics is not None) else None
        norm_out = torch.empty(4, dtype=torch.float32, device=device) if clip else None
        tensors = ([self.params[n].data.view(-1) for n in names], [grads[n].contiguous().view(-1) for n in names],
                   [self.m[n].view(-1) for n in names], [self.v[n].view(-1) for n in names])
        if self.param_groups or self.decoupled_weight_decay:
            # parameter groups / AdamW decay: the same launches in front, then ONE vpt_adam_step_groups launch with (lr, weight_decay) per tensor;
            # lr_scale multiplies the lr of THIS step (a host schedule that assigns trainer.lr keeps working)
            grp = [self.param_groups[self._group_of[n]] if n in self._group_of else None for n in names]
            ops.adam_step_groups_(*tensors, self.step_count + 1, [self.lr if g_ is None else self.lr * g_["lr_scale"] for g_ in grp],
                                  [self.wd if g_ is None or g_["weight_decay"] is None else g_["weight_decay"] for g_ in grp],
                                  beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, grad_scale=grad_scale, decoupled=self.decoupled_weight_decay,
                                  found_inf=found_inf, max_grad_norm=self.max_grad_norm, norm_out=norm_out, per_tensor_norms=per)
        else:
            ops.adam_step_multi_(*tensors, self.step_count + 1,
                                 lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, weight_decay=self.wd,
                                 grad_scale=grad_scale, found_inf=found_inf, max_grad_norm=self.max_grad_norm, norm_out=norm_out, per_tensor_norms=per)
        if clip and names:
            self.last_grad_norm = norm_out[0]
            if metrics is not None:
                metrics.update(grad_norm=norm_out[0], clip_coef=norm_out[1], grad_norm_per_tensor={n: per[i] for i, n in enumerate(names)})
        loss = float(loss)                     # (synchronises: the flag below is ready)
        if found_inf is not None and int(found_inf.item()):
            self.skipped_steps += 1            # data-parallel: the ranks agree, every rank checked the same all-reduced gradients
            if self.scaled:
                self._clean_steps = 0
                self.loss_scale = max(self.loss_scale * 0.5, 1.0)
            return loss, True
        self.step_count += 1
        if self.scaled:
            self._clean_steps += 1
            if self._clean_steps >= self.scale_growth_interval:
                self._clean_steps, self.loss_scale = 0, min(self.loss_scale * 2.0, 65536.0)
        self.policy._packed_key = None  # weights changed (in place, behind autograd's version counters): re-pack before the next forward
        return loss, False

    # ---- low-rank adapters ---------------------------------------------------------------------------------------------
    def _check_adapters_ready(self):
        """Before a saving forward or an optimiser launch: merged adapters would be applied twice (the masters hold W + s B A), and the
        data-parallel exchange does not carry adapter tensors."""
        if self.adapters is None:
            return
        if self.adapters.merged:
            raise RuntimeError(f"{type(self).__name__}: the adapters are merged into the policy (LowRankAdapters.merge_); unmerge_ before training")
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError(f"{type(self).__name__}(adapters=): data-parallel steps with adapters are not built "
                                      "(torch.distributed is initialised with more than one rank)")

    @contextlib.contextmanager
    def _adapters_applied(self):
        """For the forward-only paths (evaluate), which run the engine's inference forward on the packed policy weights: the adapters merged
        into the masters for the duration (merge_ ... unmerge_, the masters restored bit for bit).  Nothing to do without adapters, or where the
        caller has merged them already."""
        ad = self.adapters
        if ad is None or ad.merged:
            yield
            return
        ad.merge_(self.policy)
        try:
            yield
        finally:
            ad.unmerge_(self.policy)

    # ---- the trunk: ImgObsProcess.linear, pre_lstm_ln, the transformer blocks ------------------------------------------------------------
    def _trunk_forward_saving(self, d: torch.Tensor, attend, **linear_kw) -> dict:
        """d fp32 [M, 256] (the dense layer's pre-ReLU output) -> dict(dn, x_lin16, x_pre, saved, x_trunk): S's entries for the trunk, `saved` holding
        per block what the backward reads.  attend(l, p, qkv) -> (att, the block's own saved entries) runs the attention of block l on the fused
        projection's output.  linear_kw: `tiling` / `splitk` of every ops.linear here (none: the row count decides)."""
        eng = self.engine
        cfg, w, dt = eng.cfg, eng.w, self.dtype
        hid, ratio = cfg["hidsize"], cfg["pointwise_ratio"]
        pl, fq = "net.img_process.linear.", self.fused_qkv
        _, dn = ops.layernorm(d, w[pl + "g"], w[pl + "b"], relu_in=True, dtype=dt)          # 16-bit
        x, x_lin16 = ops.linear(dn, w[pl + "w"], hid, relu=True, out_f32=True, out_bf16=True, **linear_kw)
        x_pre = None
        if cfg["use_pre_lstm_ln"]:     # MinecraftPolicy.pre_lstm_ln (lib/policy.py:202-203)
            x_pre = x
            x, _ = ops.layernorm(x_pre, w["prelstm.g"], w["prelstm.b"], out_f32=True, out_bf16=False, dtype=dt)
        saved: List[dict] = []
        ad = self.adapters
        self._check_adapters_ready()

        def linear(key, blocks, x16, wpk, n, lo_saved, **kw):
            """ops.linear, or -- where an adapter sits on one of the weight's row blocks [(module, rows)] -- adapted_linear, its
            operands and u16 kept in lo_saved[key] for the backward.  Without adapters this IS the ops.linear call that has always run."""
            lo = ad.operands(blocks, x16.shape[1]) if ad is not None else None
            if lo is None:
                return ops.linear(x16, wpk, n, **kw, **linear_kw)
            o32, o16, u16 = adapted_linear(x16, wpk, n, lo[0], lo[1], **kw, **linear_kw)
            lo_saved[key] = dict(a=lo[0], sb=lo[1], spans=lo[2], mods=lo[3], u16=u16)
            return o32, o16

        for l in range(cfg["n_layers"]):
            p = f"net.recurrent_layer.blocks.{l}."
            o = p + "r.orc_block."
            los: dict = {}
            x1, x1b = ops.layernorm(x, w[p + "ln1.g"], w[p + "ln1.b"], out_f32=True, dtype=dt)
            qkv, _ = linear("lo_qkv", [(f"{o}{c}_layer", hid) for c in fq], x1b, w[p + fq + ".w"], eng.n_qkvr, los, bias=w[p + fq + ".b"])
            att, own = attend(l, p, qkv)
            x2, _ = linear("lo_proj", [(o + "proj_layer", hid)], att, w[p + "proj.w"], hid, los, bias=w[p + "proj.b"], res=x1)      # x2 = x1 + proj (engine._block)
            _, hb = ops.layernorm(x2, w[p + "ln2.g"], w[p + "ln2.b"], dtype=dt)
            _, h2 = linear("lo_mlp0", [(p + "mlp0.layer", hid * ratio)], hb, w[p + "mlp0.w"], hid * ratio, los, relu=True, out_f32=False, out_bf16=True)
            xo, _ = linear("lo_mlp1", [(p + "mlp1.layer", hid)], h2, w[p + "mlp1.w"], hid, los, bias=w[p + "mlp1.b"], res=x2)
            # a block below the cut is never walked by the backward: its activations go as the forward leaves them (None keeps the index)
            saved.append(dict(own, x=x, x1b=x1b, att=att, x2=x2, hb=hb, h2=h2, **{fq: qkv}, **los) if 2 + l >= self._cut else None)
            x = xo
        if self._cut > 0:       # the backward stops above ImgObsProcess.linear (and, from 2 on, above pre_lstm_ln): their inputs are not read
            dn = x_lin16 = None
            if self._cut > 1:
                x_pre = None
        return dict(dn=dn, x_lin16=x_lin16, x_pre=x_pre, saved=saved, x_trunk=x)

    def _release_unread(self, S: dict) -> dict:
        """Drop from a forward_saving dict what a backward cut above it does not read: `d` (ImgObsProcess.linear's LayerNorm), `xb` / `y16`
        (net.lastlayer), `y` (net.final_ln's input where there is a lastlayer).  The default set (cut -1) keeps everything."""
        n = self.engine.cfg["n_layers"]
        for key, level in (("d", 0), ("xb", 2 + n), ("y16", 2 + n), ("y", 3 + n)):
            if self._cut > level and key in S:
                S[key] = None
        return S

    def _attention_backward(self, S: dict, l: int, datt: torch.Tensor, g: Dict[str, torch.Tensor]) -> torch.Tensor:
        """datt fp32 [M, hid] -> d loss / d (the fused projection's output of block l); adds to `g` what the attention itself trains."""
        raise NotImplementedError

    def _trunk_backward(self, S: dict, dz: torch.Tensor, P: Dict[str, torch.Tensor], value_grads: bool = False, debug: Optional[dict] = None):
        """dz: 16-bit [M, ldz] = d loss / d (fused head logits) -> (g, dd): the gradient of every trainable tensor behind the CNN, and
        dd fp32 [M, 256] = d loss / d (the dense layer's pre-activation output).  Launch order: heads (dgrad, wgrad, bias sums) -> final_ln ->
        lastlayer (has_lastlayer) -> per block, last to first: mlp1, mlp0, its LayerNorm (+ skip), proj, _attention_backward, the fused projection's
        GEMM (+ skip), pre_r_ln -> pre_lstm_ln -> ImgObsProcess.linear and its LayerNorm.  P: the parameters, detached.
        value_grads: also return the value head's gradients (non-zero only when dz's value column is).  debug: a dict that receives clones of the
        intermediate gradients (tools/bc_grad_diag.py).
        With a trainable subset (trainable=) the SAME launches run in the same order with the same operands, minus those nothing
        trainable needs: a wgrad GEMM whose weights are all frozen (a fused GEMM -- heads, q/k/v/r -- loses it only when every tensor in it is),
        the bias sum of a frozen bias, and every launch below the last trainable tensor -- the walk returns (g, None) there, so the dgrad into the
        unit below the cut is never launched.  A LayerNorm backward that only carries the gradient on keeps its launch; its gain / bias sums are
        discarded.  g holds exactly the trainable names, each bit-equal to the full run's tensor.  The default set takes every branch."""
        cfg = self.engine.cfg
        dev, saved, x_trunk = S["dev"], S["saved"], S["x_trunk"]
        hid, ratio, n_layers = cfg["hidsize"], cfg["pointwise_ratio"], cfg["n_layers"]
        nq, r_fused = self.engine.n_qkvr, self.fused_qkv == "qkvr"
        pl = "net.img_process.linear."
        sub, cut = self._subset, self._cut
        want = (lambda name: True) if sub is None else sub.__contains__
        any_of = lambda *names: any(want(n_) for n_ in names)
        g: Dict[str, torch.Tensor] = {}
        zeros = lambda n_: torch.zeros(n_, dtype=torch.float32, device=dev)

        def keep(name, tensor):
            if want(name):
                g[name] = tensor

        def backward_of(lo, dy16, n_, x16, weight, **kw):
            """linear_backward, or -- lo: what the forward kept of an adapted GEMM -- adapted_linear_backward + the adapters' gradients into g:
            dA_i = the rows of du16^T x, dB_i = s times the diagonal block of dy^T u16 (fp32 results)."""
            if lo is None:
                return linear_backward(dy16, n_, x16, weight, **kw)
            dx32_, dx16_, dw_, da_stack, db_stack = adapted_linear_backward(dy16, n_, x16, weight, lo["a"], lo["sb"], lo["u16"], **kw)
            for mod, (da, db) in zip(lo["mods"], unstack_gradients(da_stack, db_stack, lo["spans"])):
                g[mod + ".lora_A"] = da.contiguous()
                g[mod + ".lora_B"] = db * self.adapters.scale
            return dx32_, dx16_, dw_

        lora = (lambda *mods: [m_ + sfx for m_ in mods for sfx in (".lora_A", ".lora_B")]) if self.adapters is not None else (lambda *mods: [])

        def layernorm_backward(x, prefix, dy, **kw):      # prefix + "weight" / "bias"; a frozen LayerNorm's sums are computed and dropped
            dgain, dbias = zeros(x.shape[1]), zeros(x.shape[1])
            dx_ = ops.layernorm_backward(x, P[prefix + "weight"], dy, dgain, dbias, **kw)
            keep(prefix + "weight", dgain); keep(prefix + "bias", dbias)
            return dx_

        # heads (one fused GEMM over head_params' row blocks): dlat, dW, db
        hw = [P[h + ".weight"] for h in self.head_params]
        nb, nc = hw[0].shape[0], hw[1].shape[0]
        wh = torch.cat(hw, 0)
        nh = wh.shape[0]
        bw, cw, bb, cb = ("pi_head.buttons.linear_layer.weight", "pi_head.camera.linear_layer.weight",
                          "pi_head.buttons.linear_layer.bias", "pi_head.camera.linear_layer.bias")
        # the value head: the caller's choice where the trainer's rule leaves it out (BCTrainer, the autograd boundary), else a tensor like any other
        vw, vb = [value_grads and (want(n_) or not self._is_trainable(n_)) for n_ in ("value_head.linear.weight", "value_head.linear.bias")]
        below = cut < 4 + n_layers
        dlat, _, dwh = linear_backward(dz, nh, S["lb"], wh, need_dx=below, need_dw=vw or any_of(bw, cw))
        if debug is not None:
            debug['dlatent'] = dlat.clone(); debug['latent'] = S["lb"].float().clone()
        if vb or any_of(bb, cb):
            dbh = zeros(nh)
            ops.column_sum_(dbh, dz, nh)
            keep(bb, dbh[:nb]); keep(cb, dbh[nb:nb + nc])
            if vb:
                g["value_head.linear.bias"] = dbh[nb + nc:nh].clone()
        if dwh is not None:
            keep(bw, dwh[:nb]); keep(cw, dwh[nb:nb + nc])
            if vw:
                g["value_head.linear.weight"] = dwh[nb + nc:nh].clone()
        del dz, dwh
        if not below:
            return g, None
        # final_ln
        dx = layernorm_backward(S["y"] if self.has_lastlayer else x_trunk, "net.final_ln.", dlat, relu_in=self.final_ln_relu)
        del dlat
        if cut >= 3 + n_layers:
            return g, None
        if self.has_lastlayer:      # y = relu(xb Wl^T); gate dy by y > 0 while casting to the GEMM operand
            below = cut < 2 + n_layers
            lw = "net.lastlayer.layer.weight"
            go_on = below or any_of("net.lastlayer.norm.weight", "net.lastlayer.norm.bias")
            dy = dx
            dy16 = ops.gate_cast(dy, hid, mask=S["y16"])
            dxb, _, dw = linear_backward(dy16, hid, S["xb"], P[lw], need_dx=go_on, need_dw=want(lw))
            keep(lw, dw)
            if not go_on:
                return g, None
            dx = layernorm_backward(x_trunk, "net.lastlayer.norm.", dxb, relu_in=True)
            if debug is not None:
                debug['y'] = S["y"].clone(); debug['dy'] = dy.clone(); debug['dx_trunk'] = dx.clone(); debug['x_trunk'] = x_trunk.clone()
            del dy, dy16, dxb, dw
            if not below:
                return g, None
        # transformer blocks, last to first
        for l in reversed(range(n_layers)):
            p = f"net.recurrent_layer.blocks.{l}."
            o = p + "r.orc_block."
            s = saved[l]
            below = cut < 2 + l
            # the block's tensors in the order the walk meets them; ahead(k): something trainable is left after stage k (or below the block)
            stages = () if below else (
                [p + "mlp1.layer.weight", p + "mlp1.layer.bias"] + lora(p + "mlp1.layer"), [p + "mlp0.layer.weight"] + lora(p + "mlp0.layer"),
                [p + "mlp0.norm.weight", p + "mlp0.norm.bias"], [o + "proj_layer.weight", o + "proj_layer.bias"] + lora(o + "proj_layer"), [o + "b_nd"],
                [f"{o}{c}_layer.weight" for c in "qkvr"] + [o + "q_layer.bias", o + "r_layer.bias"] + lora(*[f"{o}{c}_layer" for c in "qkvr"]),
                [p + "pre_r_ln.weight", p + "pre_r_ln.bias"])
            ahead = lambda k: below or any(any_of(*names) for names in stages[k + 1:])
            dout16 = ops.gate_cast(dx, hid, dtype=self.dtype)
            # mlp1: out = x2 + h2 W1^T + b1
            _, dh16, dw = backward_of(s.get("lo_mlp1"), dout16, hid, s["h2"], P[p + "mlp1.layer.weight"], mask=s["h2"], dx_f32=False, dx_bf16_ld=hid * ratio,
                                      need_dx=ahead(0), need_dw=want(p + "mlp1.layer.weight"))
            keep(p + "mlp1.layer.weight", dw)
            if want(p + "mlp1.layer.bias"):
                g[p + "mlp1.layer.bias"] = zeros(hid)
                ops.column_sum_(g[p + "mlp1.layer.bias"], dout16, hid)
            if not ahead(0):
                return g, None
            # mlp0: h2 = relu(hb W0^T)  (the ReLU gate was applied by the mask above)
            dhb, _, dw = backward_of(s.get("lo_mlp0"), dh16, hid * ratio, s["hb"], P[p + "mlp0.layer.weight"], need_dx=ahead(1), need_dw=want(p + "mlp0.layer.weight"))
            keep(p + "mlp0.layer.weight", dw)
            if not ahead(1):
                return g, None
            dx2 = layernorm_backward(s["x2"], p + "mlp0.norm.", dhb, dx_add=dx)
            if debug is not None:
                debug[f'dout16_{l}'] = dout16.clone(); debug[f'dh16_{l}'] = dh16.clone(); debug[f'dhb_{l}'] = dhb.clone()
            del dh16, dhb, dout16, dw
            if not ahead(2):
                return g, None
            # proj: x2 = x1 + att Wp^T + bp
            dx2_16 = ops.gate_cast(dx2, hid, dtype=self.dtype)
            datt, _, dw = backward_of(s.get("lo_proj"), dx2_16, hid, s["att"], P[o + "proj_layer.weight"], need_dx=ahead(3), need_dw=want(o + "proj_layer.weight"))
            keep(o + "proj_layer.weight", dw)
            if want(o + "proj_layer.bias"):
                g[o + "proj_layer.bias"] = zeros(hid)
                ops.column_sum_(g[o + "proj_layer.bias"], dx2_16, hid)
            if not ahead(3):
                return g, None
            # attention, then the fused projection: dx1 = dx2 (skip) + dqkv Wqkv
            dqkv = self._attention_backward(S, l, datt, g)
            if not want(o + "b_nd"):
                g.pop(o + "b_nd", None)
            if not ahead(4):
                return g, None
            dq16 = ops.gate_cast(dqkv, _round_up(nq, 64), dtype=self.dtype)
            wq = torch.cat([P[f"{o}{c}_layer.weight"] for c in self.fused_qkv], 0)      # q_layer, k_layer, v_layer (, r_layer)
            dx1, _, dwq = backward_of(s.get("lo_qkv"), dq16, nq, s["x1b"], wq, res=dx2, need_dx=ahead(5),
                                      need_dw=any_of(*[f"{o}{c}_layer.weight" for c in self.fused_qkv]))
            if dwq is not None:
                keep(o + "q_layer.weight", dwq[:hid]); keep(o + "k_layer.weight", dwq[hid:2 * hid]); keep(o + "v_layer.weight", dwq[2 * hid:3 * hid])
            # bias sums over the fused columns (k_layer and v_layer have none).  r_layer outside the fused projection is unreached: exact zeros
            if r_fused:
                if dwq is not None:
                    keep(o + "r_layer.weight", dwq[3 * hid:])
            else:
                keep(o + "r_layer.weight", torch.zeros_like(P[o + "r_layer.weight"]) if want(o + "r_layer.weight") else None)
                keep(o + "r_layer.bias", torch.zeros_like(P[o + "r_layer.bias"]) if want(o + "r_layer.bias") else None)
            if any_of(o + "q_layer.bias", *([o + "r_layer.bias"] if r_fused else [])):
                dbq = zeros(nq if r_fused else hid)
                ops.column_sum_(dbq, dq16, dbq.numel())
                keep(o + "q_layer.bias", dbq[:hid])
                if r_fused:
                    keep(o + "r_layer.bias", dbq[3 * hid:])
            if not ahead(5):
                return g, None
            dx = layernorm_backward(s["x"], p + "pre_r_ln.", dx1)
            if debug is not None:
                debug[f'dx_block{l}'] = dx.clone(); debug[f'dx2_block{l}'] = dx2.clone(); debug[f'datt{l}'] = datt.clone(); debug[f'dqkvr{l}'] = dqkv.clone()
                debug[f'dx1_block{l}'] = dx1.clone(); debug[f'dq16_{l}'] = dq16.clone(); debug[f'dx2_16_{l}'] = dx2_16.clone()
            del dx2, dx2_16, datt, dqkv, dq16, dx1, dwq
            if not below:
                return g, None
        if cfg["use_pre_lstm_ln"]:
            dx = layernorm_backward(S["x_pre"], "net.pre_lstm_ln.", dx)
            if cut >= 1:
                return g, None
        # ImgObsProcess.linear: x = relu(dn Wlin^T); its LayerNorm sits on relu(d), d being the CNN's output
        go_on = cut < 0 or any_of(pl + "norm.weight", pl + "norm.bias")
        dx16 = ops.gate_cast(dx, hid, mask=S["x_lin16"])
        ddn, _, dw = linear_backward(dx16, hid, S["dn"], P[pl + "layer.weight"], need_dx=go_on, need_dw=want(pl + "layer.weight"))
        keep(pl + "layer.weight", dw)
        if not go_on:
            return g, None
        dd = layernorm_backward(S["d"], pl + "norm.", ddn, relu_in=True)
        return g, dd
