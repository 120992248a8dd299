"""The flat parameter arenas under TrainEngine and optim.ArenaOptimizer: f32 master, gradients and moments that mh_optim_step /
mh_optim_groups update in one launch, their bf16 copies (functional.ArenaShadows), the device step state, the group byte of each block
and the torch.optim-shaped state dict.  The layout is decided here; the clients decide the parameters' order and all of a step."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from . import functional as Fn
from . import kernels as K
from ._lib import OPT_ADAM, OPT_ADAMW, OPT_SGD, OptimCfg

f32, bf16 = torch.float32, torch.bfloat16
ALIGN = 8  # elements: keeps every parameter 32-B aligned in f32 and 16-B aligned in the bf16 shadow (and its transposes)


def pad(n: int) -> int:
    return (n + ALIGN - 1) // ALIGN * ALIGN


def lay_out(sizes: Sequence[int]) -> Tuple[List[int], int]:
    """(offsets, total) of tensors of `sizes` elements laid out back to back, each padded to ALIGN elements."""
    ends = [0]
    for n in sizes:
        ends.append(ends[-1] + pad(n))
    return ends[:-1], ends[-1]


# timm's --opt values that create_optimizer_v2 maps to the three rules of mh_optim_step: name -> (rule, nesterov)
OPTS = {"adam": ("adam", False), "adamw": ("adamw", False), "sgd": ("sgd", True), "nesterov": ("sgd", True), "momentum": ("sgd", False)}


def check_opt(opt: str, momentum: Optional[float] = None, nesterov: Optional[bool] = None) -> Tuple[str, bool]:
    """(rule, nesterov) of timm's --opt value, refusing what is not built; nesterov: the live setting, where it may differ from the name's."""
    if opt not in OPTS:
        raise NotImplementedError(f"opt {opt!r}: only {', '.join(map(repr, OPTS))} are implemented (timm's other optimizers are not)")
    rule, nesterov = OPTS[opt][0], OPTS[opt][1] if nesterov is None else bool(nesterov)
    if momentum is not None and rule == "sgd" and nesterov and momentum <= 0.0:
        raise ValueError("Nesterov momentum requires a momentum and zero dampening")        # torch.optim.SGD's own refusal
    return rule, nesterov


def group_settings(rule: str, lr, betas, eps, weight_decay, momentum, nesterov) -> dict:
    """torch.optim's param-group entries for the rule, in torch's key order."""
    if rule != "sgd":
        return {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": weight_decay, "amsgrad": False}
    return {"lr": lr, "momentum": momentum, "dampening": 0, "weight_decay": weight_decay, "nesterov": nesterov}


def rule_cfg(rule: str, betas, eps: float, momentum: float, nesterov) -> OptimCfg:
    """The launch settings of mh_optim_step / mh_optim_groups; a rule ignores the fields that are not its own."""
    code = {"adam": OPT_ADAM, "adamw": OPT_ADAMW, "sgd": OPT_SGD}[rule]
    return OptimCfg(code, float(betas[0]), float(betas[1]), float(eps), float(momentum), int(bool(nesterov)))


def decay_groups(model: torch.nn.Module, weight_decay: float, filter_bias_and_bn: bool = True):
    """The parameter groups timm's create_optimizer_v2 hands to torch.optim (train_mirror.py:742-746), as [(weight_decay, [(name,
    parameter), ...]), ...] over the trainable parameters in model.parameters() order.  With weight_decay > 0 and the filter on:
    param_groups_weight_decay's [no_decay, decay], no_decay = `p.ndim <= 1 or name.endswith(".bias")` at weight_decay 0 (neither
    model defines no_weight_decay()); otherwise one group that carries weight_decay."""
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    if not (weight_decay and filter_bias_and_bn):
        return [(weight_decay, named)]
    no_decay = [(n, p) for n, p in named if p.ndim <= 1 or n.endswith(".bias")]
    decay = [(n, p) for n, p in named if not (p.ndim <= 1 or n.endswith(".bias"))]
    return [(0.0, no_decay), (weight_decay, decay)]


def _fill(arena: torch.Tensor, items) -> None:
    """arena[o : o + n] = x for (o, x) in items: tensors on the device in one mh_gather_many launch, the others (a CPU checkpoint) by copy_."""
    there = [(o, x.detach()) for o, x in items if x.device == arena.device and x.dtype in (f32, bf16) and x.is_contiguous()]
    if there:
        K.gather_many(arena, K.gather_table(arena, there))
    for o, x in items:
        if not (x.device == arena.device and x.dtype in (f32, bf16) and x.is_contiguous()):
            arena[o:o + x.numel()].copy_(x.reshape(-1))


class ParamArena:
    """params: the parameters in arena order; rule: "adam" / "adamw" / "sgd"; momentum_buffer: whether SGD keeps one; precision: the
    forward's policy (the bf16 ones get an ArenaShadows); lr: the initial state[3].  Construction makes every `p.data` a view of `master`.
    It neither publishes the bf16 copies nor assigns `p.grad` (grad_views[i] is params[i]'s): the client does both, and keeps the
    transposes' staleness.  The arena holds no reference to its client."""

    def __init__(self, params, rule: str, momentum_buffer: bool, precision: str, lr: float):
        self.params, self.rule = list(params), rule
        self.offsets, self.numel = lay_out([p.numel() for p in self.params])
        self.off_of = {id(p): o for p, o in zip(self.params, self.offsets)}
        self.device = dev = self.params[0].device
        self.master = torch.zeros(self.numel, device=dev, dtype=f32)
        self.grad = torch.zeros(self.numel, device=dev, dtype=f32)
        # exp_avg / momentum_buffer and exp_avg_sq: SGD has no second moment, and no buffer at all without momentum
        self.m = torch.zeros(self.numel, device=dev, dtype=f32) if rule != "sgd" or momentum_buffer else None
        self.v = torch.zeros(self.numel, device=dev, dtype=f32) if rule != "sgd" else None
        bf = self.bf = Fn.ArenaShadows(self.master, zip(self.params, self.offsets)) if Fn.POLICIES[precision].act == bf16 else None
        self.shadow, self.shadow_t, self.t_params = (bf.flat, bf.flat_t, bf.t_params) if bf is not None else (None, None, [])
        self.grad_views: List[torch.Tensor] = []
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                n = p.numel()
                self.master[o:o + n].copy_(p.detach().reshape(-1))
                p.data = self.master[o:o + n].view(p.shape)
                self.grad_views.append(self.grad[o:o + n].view(p.shape))
        # {t, 1 - b1^t, 1 - b2^t, lr, clip, |g|}: advanced by the optimizer launch itself, so a step replays from a HIP graph
        self.state = torch.tensor([0.0, 0.0, 0.0, float(lr), 1.0, 0.0], device=dev, dtype=f32)

    def set_step(self, t: float, b1: float, b2: float, lr: float, keep_clip: bool = False) -> None:
        """Reload the step state for step count t; keep_clip leaves the clip factor and |g| as they are (else 1 and 0)."""
        head = [t, 1.0 - b1 ** t, 1.0 - b2 ** t, float(lr)]
        self.state[:4 if keep_clip else 6].copy_(torch.tensor(head if keep_clip else head + [1.0, 0.0]))

    def sync_shadows(self, owner=None) -> None:
        """Rebuild the bf16 copies and publish them at the parameters' present addresses; owner: who keeps the transposes current."""
        if self.bf is not None:
            self.bf.refresh()
            self.bf.publish(owner=owner)

    def span(self, p: torch.Tensor) -> Tuple[int, int]:
        """(first, end) of the ALIGN-element blocks of parameter p: its padding shares its last block (and stays zero: p = g = m = 0)."""
        o = self.off_of[id(p)]
        return o // ALIGN, pad(o + p.numel()) // ALIGN

    def group_bytes(self, group_of_param: Sequence[int]) -> torch.Tensor:
        """The kernels' group map, on the host: one uint8 per block, group_of_param[i] over the blocks of params[i]."""
        gmap = torch.zeros(self.numel // ALIGN, dtype=torch.uint8)
        for p, gi in zip(self.params, group_of_param):
            a, b = self.span(p)
            gmap[a:b] = gi
        return gmap

    def range_of(self, i0: int, i1: int) -> Tuple[int, int]:
        """The element range [start, end) of params[i0 .. i1], padding included."""
        return self.offsets[i0], self.offsets[i1] + pad(self.params[i1].numel())

    # ------------------------------------------------------------------ state (torch.optim's shape and entry order)
    def state_dict(self, rule_groups, t: float, skip=()) -> dict:
        """The torch.optim-shaped state dict, on the CPU.  rule_groups: [(the group's settings in torch's key order for the rule, without
        "params", [parameters]), ...]; t: the step count.  State indices run through the groups.  Adam / AdamW: {step, exp_avg,
        exp_avg_sq} per parameter; SGD: {momentum_buffer}, no state without momentum; parameters whose id is in `skip` (never updated)
        have no entry, as in torch.  SGD keeps no step in torch: the arena's travels as the extra top-level "step", which
        torch.optim.SGD.load_state_dict ignores."""
        state, out_groups, i = {}, [], 0
        for settings, members in rule_groups:
            first = i
            for p in members:
                o, n = self.off_of[id(p)], p.numel()
                if id(p) in skip:
                    pass
                elif self.rule != "sgd":
                    state[i] = {"step": torch.tensor(t), "exp_avg": self.m[o:o + n].view(p.shape).cpu().clone(),
                                "exp_avg_sq": self.v[o:o + n].view(p.shape).cpu().clone()}
                elif self.m is not None and t > 0:          # torch creates the buffer at a parameter's first step
                    state[i] = {"momentum_buffer": self.m[o:o + n].view(p.shape).cpu().clone()}
                i += 1
            out_groups.append({**settings, "params": list(range(first, i))})
        return {"state": state, "param_groups": out_groups, **({"step": t} if self.rule == "sgd" else {})}

    def load_state(self, who: str, sd: dict, members, expect: Optional[int]) -> float:
        """Check a torch.optim-shaped state dict against the client `who` (its name, for the messages) and copy its moments into m, v.
        members: [[parameters of group 0], ...]; expect: how many state entries a non-empty state must have (None: any number;
        parameters without an entry keep their moments).  Returns the step count the dict holds."""
        rule = self.rule
        order = [p for group in members for p in group]
        pg = sd.get("param_groups") or []
        want = "momentum" if rule == "sgd" else "betas"
        if pg and any(want not in g for g in pg):
            raise ValueError(f"optimizer state of another rule: {who} loads param groups that hold "
                             f"{want!r}, these hold {sorted(k for k in pg[0] if k != 'params')}")
        if pg and [len(g["params"]) for g in pg] != [len(group) for group in members]:
            raise ValueError(f"optimizer state has param groups of {[len(g['params']) for g in pg]} parameters, those of {who} "
                             f"have {[len(group) for group in members]}")
        if expect is not None and len(sd["state"]) not in (0, expect):
            raise ValueError(f"optimizer state has {len(sd['state'])} entries, the model has {expect} parameters")
        t = float(sd.get("step", 0.0)) if rule == "sgd" else 0.0
        keys = ("exp_avg", "exp_avg_sq") if rule != "sgd" else ("momentum_buffer",) if self.m is not None else ()
        into = {k: [] for k in keys}
        for i, p in enumerate(order):
            st = sd["state"].get(i)
            if st is None:
                continue
            if rule != "sgd" and "exp_avg" not in st:
                raise ValueError(f"optimizer state of another rule: entry {i} holds {sorted(st)}, not Adam's exp_avg / exp_avg_sq")
            for k in keys:
                if st[k].numel() != p.numel():
                    raise ValueError(f"optimizer state entry {i} holds {tuple(st[k].shape)} for a parameter of shape {tuple(p.shape)}")
                into[k].append((self.off_of[id(p)], st[k]))
            if rule != "sgd":
                t = float(st["step"])
        for k, arena in zip(keys, (self.m, self.v)):
            if into[k]:
                _fill(arena, into[k])
        return t
