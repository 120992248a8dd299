"""The arena optimizer behind torch.optim's interface, for the downstream trainers (train_subtyping.py:742-763, :1226-1260;
train_survival.py the same): what they hold is `optimizer = create_optimizer_v2(...)`, and what they call on it is zero_grad(),
step(), utils.dispatch_clip_grad(...), lr_scheduler.step() (which writes optimizer.param_groups[i]["lr"]) and state_dict().

ArenaOptimizer is that object over the kernel TrainEngine steps with: f32 master parameters, gradients and moments in flat arenas, the
parameters and their .grad views of them, and ONE launch (mh_optim_groups) that updates parameter, moments and bf16 shadow, with the
learning rate and weight decay of each parameter group read from device tables — so timm's and torch's lr schedulers drive it
unchanged, and step() replays from a captured HIP graph.  There is no CPU path and no torch.optim fallback.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from . import kernels as K
from ._lib import OPT_SKIP_GROUP, MirrorHipError
from .arena import ParamArena, check_opt, decay_groups, group_settings, rule_cfg
from .functional import POLICIES

f32, bf16 = torch.float32, torch.bfloat16


class ArenaOptimizer(torch.optim.Optimizer):
    """torch.optim.Adam / AdamW / SGD over flat arenas, one HIP launch per step.

    params: parameters or parameter groups in torch's form, CUDA float32 tensors that require gradients (anything else raises
    MirrorHipError).  opt: timm's name — "adam", "adamw", "sgd" / "nesterov" (both SGD with Nesterov momentum, as timm maps them) or
    "momentum"; timm's other optimizers raise NotImplementedError.  lr, betas, eps, momentum, weight_decay: torch's.
    precision: the policy of the model's forward; under the bf16 policies the update also writes the bf16 copies the GEMMs read
    (functional.shadow) and step() rebuilds the transposed copies behind it.

    Construction moves the parameters: `p.data` becomes a view of the master arena and `p.grad` a view of the gradient arena (offsets
    are multiples of 8 elements), so autograd accumulates straight into the arena.  Whoever writes the parameters afterwards through
    anything but step() — model.load_state_dict — calls sync_shadows() (load_state_dict() here does).

    param_groups are live dicts with torch's keys for the rule.  "lr" and "weight_decay" may differ between groups and change at any
    time: step() compares them with the device tables and uploads those when a value changed.  betas / eps / momentum are one setting
    for the whole arena (groups that disagree raise NotImplementedError).

    Gradients.  A parameter whose .grad is its arena view costs nothing.  A .grad that is another tensor (set by hand, or allocated by
    autograd after something set .grad to None) is copied into the arena at step() / clip_grad() — all such tensors in one
    mh_gather_many launch — and .grad is pointed back at the view.  A parameter whose .grad is None at the first step() belongs to the
    skipped group from then on: parameter, moments and shadow keep their bits, as torch.optim leaves a parameter without a gradient
    alone, weight decay included.  The arena has ONE step count where torch keeps one per parameter, so a parameter that changes
    between "has a gradient" and "has none" after the first step raises ValueError.  Note that zero_grad() keeps the views: a
    parameter the forward did not use then has a zero gradient, not None, and is updated as torch updates a zero gradient (decay and
    momentum move it); set its .grad to None before the first step to have it skipped.

    Graph capture: step() with arena-resident gradients is capturable with torch.cuda.graph after one eager step — nothing that
    changes from step to step is a launch argument.  A replay runs no host code: after writing param_groups[i]["lr"], call
    publish_groups() before the replay (an eager step() does it itself)."""

    def __init__(self, params, opt: str = "adam", lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, momentum: float = 0.9,
                 weight_decay: float = 0.0, precision: str = "bf16"):
        self._rule, nesterov = check_opt(opt)
        if precision not in POLICIES:
            raise ValueError(f"unknown precision {precision!r}")
        self.opt = opt
        if lr < 0.0 or weight_decay < 0.0 or momentum < 0.0 or eps < 0.0:
            raise ValueError(f"lr {lr}, weight_decay {weight_decay}, momentum {momentum} and eps {eps} must not be negative")
        defaults = group_settings(self._rule, lr, betas, eps, weight_decay, float(momentum), nesterov)
        self._keys = tuple(defaults)          # torch's keys for the rule
        self._laid_out = False
        super().__init__(params, defaults)
        self._cfg_key = None
        self._settings()          # refuses groups whose betas / eps / momentum differ, before anything is moved
        order = [p for g in self.param_groups for p in g["params"]]
        for p in order:
            if not (p.is_cuda and p.dtype == f32 and p.requires_grad):
                raise MirrorHipError("ArenaOptimizer needs trainable float32 parameters on an MI355X device (model.to('cuda') first), got "
                                     f"{tuple(p.shape)} {p.dtype} on {p.device}, requires_grad={p.requires_grad}: there is no CPU path")
        if len(self.param_groups) > OPT_SKIP_GROUP:
            raise NotImplementedError(f"{len(self.param_groups)} parameter groups: the group byte holds {OPT_SKIP_GROUP}")
        pa = self.arena = ParamArena(order, self._rule, float(momentum) > 0.0, precision, lr)
        self.params, self.offsets, self.numel, self.device = pa.params, pa.offsets, pa.numel, pa.device
        self.master, self.grad, self.m, self.v, self._state = pa.master, pa.grad, pa.m, pa.v, pa.state
        self._bf, self.shadow, self._gviews = pa.bf, pa.shadow, pa.grad_views
        for p, view in zip(order, self._gviews):
            p.grad = view
        self.sync_shadows()
        # one byte per block names its parameter group (ParamArena.group_bytes); OPT_SKIP_GROUP once a parameter is known to have no gradient.
        # The tables [weight decay; lr] live in one fixed device buffer (state[3] is not read): a captured launch follows the schedulers
        self._gmap_host = pa.group_bytes([gi for gi, g in enumerate(self.param_groups) for _ in g["params"]])
        self._gmap = self._gmap_host.to(self.device)
        self._tab = torch.zeros(2, len(self.param_groups), device=self.device, dtype=f32)
        self._tab_host = None                 # what the device tables hold (None: nothing yet)
        self._has: Optional[List[bool]] = None      # per parameter: has a gradient (fixed by the first step)
        self._clipped = False
        self._laid_out = True

    # ------------------------------------------------------------------ groups
    def add_param_group(self, param_group) -> None:
        if self._laid_out:
            raise NotImplementedError("ArenaOptimizer lays its arenas out at construction: build a new optimizer for more parameters")
        super().add_param_group(param_group)

    def _settings(self) -> None:
        """The launch settings from the live groups: betas / eps / momentum / nesterov are one setting for the whole arena."""
        keys = ("momentum", "nesterov", "dampening") if self._rule == "sgd" else ("betas", "eps", "amsgrad")
        key = tuple(tuple(self.param_groups[0][k]) if k == "betas" else self.param_groups[0][k] for k in keys)
        if key == self._cfg_key and all(g[k] == self.param_groups[0][k] for g in self.param_groups[1:] for k in keys):
            return
        for g in self.param_groups:
            if any((tuple(g[k]) if k == "betas" else g[k]) != v for k, v in zip(keys, key)):
                raise NotImplementedError(f"parameter groups with different {keys}: one setting for the whole arena")
        if self._rule == "sgd":
            mu, nesterov, damp = key
            if damp != 0:
                raise NotImplementedError("SGD dampening is not built (timm passes 0)")
            check_opt(self.opt, mu, nesterov)
            if self._cfg_key is not None and (mu > 0.0) != (self.m is not None):
                raise NotImplementedError("momentum cannot change between zero and non-zero: the buffer arena is laid out at construction")
            cfg = rule_cfg("sgd", (0.0, 0.0), 0.0, mu, nesterov)
        else:
            (b1, b2), eps, amsgrad = key
            if amsgrad:
                raise NotImplementedError("amsgrad is not built")
            cfg = rule_cfg(self._rule, (b1, b2), eps, 0.0, False)
        if self._cfg_key is not None and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("betas / eps / momentum changed: they are launch arguments, capture step() again")
        self._opt_cfg, self._cfg_key = cfg, key

    def publish_groups(self) -> None:
        """Bring the device tables up to the live param_groups: every group's "weight_decay" and "lr" are compared with what the
        tables hold and uploaded (one small host-to-device copy on the current stream) only when a value changed.  An eager step()
        calls this; call it yourself between writing an lr and replaying a captured step()."""
        self._settings()
        vals = [[float(g["weight_decay"]) for g in self.param_groups], [float(g["lr"]) for g in self.param_groups]]
        if vals == self._tab_host:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a learning rate or weight decay changed inside a captured region: the tables are refreshed by a host-side "
                               "copy — run one eager step() first, and call publish_groups() outside the capture")
        self._tab.copy_(torch.tensor(vals, dtype=f32))
        self._tab_host = vals

    # ------------------------------------------------------------------ gradients
    def _gather(self) -> None:
        """Fix which parameters have a gradient (first call), and bring gradients that live outside the arena into it."""
        has = [p.grad is not None for p in self.params]
        if self._has is not None and has != self._has:
            i = next(k for k, (a, b) in enumerate(zip(has, self._has)) if a != b)
            raise ValueError(f"parameter {i} of shape {tuple(self.params[i].shape)} {'has a gradient now' if has[i] else 'has no gradient now'}"
                             " and it was the other way at the first step: the arena keeps one step count, torch.optim one per parameter")
        items = []
        for p, view, o in zip(self.params, self._gviews, self.offsets):
            g = p.grad
            if g is None or g is view:
                continue
            if g.is_sparse or not g.is_cuda or g.device != self.device or g.dtype not in (f32, bf16) or g.shape != p.shape:
                raise MirrorHipError(f"a gradient of shape {tuple(g.shape)}, {g.dtype} on {g.device} for a parameter of shape "
                                     f"{tuple(p.shape)}: dense f32 / bf16 on the arena's device")
            if g.data_ptr() != view.data_ptr():
                items.append((o, g.detach().contiguous()))
            p.grad = view
        if self._has is None:
            if not all(has):
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("run one eager step() before capturing: the first step fixes which parameters have gradients")
                for p, h in zip(self.params, has):
                    if not h:
                        first, end = self.arena.span(p)
                        self._gmap_host[first:end] = OPT_SKIP_GROUP
                self._gmap.copy_(self._gmap_host)
            self._has = has
        if items:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("a gradient outside the arena cannot be gathered inside a captured region (its address is a launch argument)")
            K.gather_many(self.grad, K.gather_table(self.grad, items))

    def zero_grad(self, set_to_none: bool = True) -> None:
        """Zero the gradient arena with one memset.  The .grad views are KEPT whatever set_to_none says — autograd then accumulates into
        the arena and step() has nothing to gather; a .grad that is another tensor is dropped for its view.  A .grad that is None stays
        None (the skipped group)."""
        self.grad.zero_()
        for p, view in zip(self.params, self._gviews):
            if p.grad is not None and p.grad is not view:
                p.grad = view

    def clip_grad(self, value: float, mode: str = "norm") -> None:
        """timm's dispatch_clip_grad over the arena, after gathering outside gradients.  "norm": the global L2 norm goes to `grad_norm`
        and the factor min(1, value / (norm + 1e-6)) stays on the device — the next step() applies it inside the update, p.grad is NOT
        rescaled.  "value": the arena is clamped to [-value, value] in place.  "agc" is not built."""
        if mode == "agc":
            raise NotImplementedError("clip mode 'agc' is not implemented (timm's adaptive gradient clipping)")
        if mode not in ("norm", "value"):
            raise ValueError(f"unknown clip mode {mode!r}")
        self._gather()
        if mode == "norm":
            K.grad_clip(self.grad, 1.0, float(value), self._state)
            self._clipped = True
        else:
            self.grad.clamp_(-float(value), float(value))

    @property
    def grad_norm(self) -> torch.Tensor:
        """The gradient norm the last clip_grad(mode="norm") measured: a device scalar (a view of the step state), no host sync."""
        return self._state[5]

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._gather()
        self.publish_groups()
        K.optim_groups(self.master, self.grad, self.m, self.v, self.shadow, self._opt_cfg, self._state, self._gmap, self._tab[0],
                       self._tab[1])
        if self._clipped:             # the factor belongs to the step it was measured for
            self._state[4:5].fill_(1.0)
            self._clipped = False
        if self._bf is not None:
            self._bf.refresh_t()      # the transposed bf16 copies the backward's data gradients stream
        return loss

    def sync_shadows(self) -> None:
        """(Re)publish the bf16 copies after the master arena was written by anything but step()."""
        self.arena.sync_shadows()

    # ------------------------------------------------------------------ state (torch.optim's shape and entry order)
    def state_dict(self) -> dict:
        """torch.optim's dict for the same groups (ParamArena.state_dict); a skipped parameter has no entry.  Group entries beyond
        torch's keys for the rule (a scheduler's "initial_lr") follow them."""
        groups = []
        for g in self.param_groups:
            settings = {k: g[k] for k in self._keys}
            settings.update({k: v for k, v in g.items() if k not in self._keys and k != "params"})
            groups.append((settings, g["params"]))
        skip = () if self._has is None else {id(p) for p, h in zip(self.params, self._has) if not h}
        return self.arena.state_dict(groups, float(self._state[0].item()), skip=skip)

    def load_state_dict(self, state_dict: dict) -> None:
        """Load this optimizer's dict, or torch.optim.Adam / AdamW / SGD's over the same groups (tensors on the device arrive in one
        mh_gather_many launch per arena).  Every entry must hold the same step; the groups' settings are taken over as torch does."""
        sd = state_dict
        steps = {float(st["step"]) for st in sd["state"].values() if "step" in st}
        if len(steps) > 1:
            raise ValueError(f"optimizer state with step counts {sorted(steps)}: the arena keeps one")
        pg = sd.get("param_groups") or []
        if any(g.get("amsgrad") or g.get("maximize") for g in pg):
            raise NotImplementedError("amsgrad and maximize are not built")
        expect = None if self._has is None else sum(self._has)
        t = self.arena.load_state(f"ArenaOptimizer(opt={self.opt!r})", sd, [g["params"] for g in self.param_groups], expect)
        if self._rule == "sgd" and sd["state"] and t == 0.0:
            t = 1.0                       # torch.optim.SGD's dict has no step; buffers mean that at least one was taken
        for g, new in zip(self.param_groups, pg):
            g.update({k: v for k, v in new.items() if k in self._keys or k == "initial_lr"})
        self._settings()
        b1, b2 = (self._opt_cfg.beta1, self._opt_cfg.beta2) if self._rule != "sgd" else (0.0, 0.0)
        self.arena.set_step(t, b1, b2, self.param_groups[0]["lr"])
        self._clipped = False
        self.sync_shadows()


def param_groups_of(model: torch.nn.Module, weight_decay: float = 0.0, filter_bias_and_bn: bool = True) -> List[dict]:
    """timm's parameter groups (arena.decay_groups) in torch's form, over the parameters that require gradients."""
    return [{"params": [p for _, p in members], "weight_decay": wd}
            for wd, members in decay_groups(model, weight_decay, filter_bias_and_bn)]


def create_optimizer_v2(model_or_params, opt: str = "adam", lr: Optional[float] = None, weight_decay: float = 0.0,
                        momentum: float = 0.9, filter_bias_and_bn: bool = True, **kw) -> ArenaOptimizer:
    """timm.optim.create_optimizer_v2 (train_subtyping.py:742-763: `create_optimizer_v2(model, **optimizer_kwargs(cfg=args))`) for
    --opt adam / adamw / sgd / nesterov / momentum, returning an ArenaOptimizer.  A module is grouped as timm groups it: with
    weight_decay > 0 and the filter on, 1-D and `.bias` parameters form a group without decay.  Only parameters that require
    gradients enter: a linear probe's arena holds the head alone.  kw: betas, eps (timm's opt_args) and precision (default: the
    module's own `precision`, else "bf16")."""
    if isinstance(model_or_params, torch.nn.Module):
        groups = param_groups_of(model_or_params, weight_decay, filter_bias_and_bn)
        kw.setdefault("precision", getattr(model_or_params, "precision", None) or "bf16")
        if weight_decay and filter_bias_and_bn:
            weight_decay = 0.0          # the groups carry it
    else:
        groups = list(model_or_params)
        if groups and not isinstance(groups[0], dict):
            groups = [p for p in groups if p.requires_grad]
    return ArenaOptimizer(groups, opt=opt.lower(), lr=1e-3 if lr is None else lr, weight_decay=weight_decay, momentum=momentum, **kw)


def dispatch_clip_grad(parameters, value: float, mode: str = "norm", norm_type: float = 2.0, optimizer=None) -> None:
    """timm.utils.dispatch_clip_grad (train_subtyping.py:1243-1247) plus `optimizer`.  With an ArenaOptimizer the clipping runs over
    its gradient arena (`parameters` is not read).  One visible difference from timm: in "norm" mode p.grad is not rescaled by this
    call — the factor stays on the device and the optimizer's next step() applies it; the norm is `optimizer.grad_norm`.  Without an
    ArenaOptimizer it is timm's own dispatch over torch.nn.utils.  norm_type other than 2 and mode "agc" raise NotImplementedError."""
    if mode == "norm" and float(norm_type) != 2.0:
        raise NotImplementedError(f"norm_type {norm_type}: only the L2 norm is implemented")
    if mode == "agc":
        raise NotImplementedError("clip mode 'agc' is not implemented (timm's adaptive gradient clipping)")
    if isinstance(optimizer, ArenaOptimizer):
        optimizer.clip_grad(value, mode)
    elif mode == "norm":
        torch.nn.utils.clip_grad_norm_(parameters, value, norm_type=norm_type)
    elif mode == "value":
        torch.nn.utils.clip_grad_value_(parameters, value)
    else:
        raise ValueError(f"unknown clip mode {mode!r}")
