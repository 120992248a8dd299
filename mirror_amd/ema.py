"""Model EMA: timm's `utils.ModelEmaV3` as the three reference trainers use it behind --model-ema.

  * built at train_mirror.py:787-799 (train_subtyping.py:867-879, train_survival.py:879-891):
    `ModelEmaV3(model, decay=args.model_ema_decay, use_warmup=args.model_ema_warmup, device=...)`;
  * updated behind every optimizer update, :1283-1284 (:1293, :1322): `model_ema.update(model, step=num_updates)`;
  * validated, and checkpoints selected on it, :1022-1037 (:1119-1130, :1139); reloaded with
    `load_checkpoint(model_ema.module, args.resume, use_ema=True)` (:797, `mirror_amd.checkpoint.load_checkpoint`).

The EMA weights live in one flat, 16-B-aligned f32 arena; the parameters of `.module` are views of it.  Two update paths:
  * standalone (`update(model, step)`, e.g. downstream fine-tuning under a plain torch.optim optimizer): ONE mh_ema_update_many
    launch over a table of (EMA offset, source address, n) rows;
  * attached to a TrainEngine (`TrainEngine(..., model_ema=ema)`): the arena takes the master arena's layout and mh_optim_step lerps
    every updated parameter inside the optimizer pass (+8 B per parameter, no launch of its own, decay from the device step: the
    update is part of the captured whole-step graph).  `update(model, step=num_updates)` is then a checked no-op.

A kernel write does not bump torch's version counter: the bf16 weight copies of `.module` (bf16 policies) are rebuilt by a forward
pre-hook whenever the arena was updated or written through torch since the last forward — one refresh per validation, not per step.
"""
from __future__ import annotations

import copy
from typing import List, Optional, Tuple

import numpy as np
import torch
from torch import nn

from . import functional as Fn
from . import kernels as K
from ._lib import EmaCfg, MirrorHipError
from .arena import ALIGN, lay_out

f32, bf16 = torch.float32, torch.bfloat16
_ROW = 16384        # elements per mh_ema_update_many row (a multiple of 4: the rows of one tensor keep its 16-B alignment)


def _unwrap(model: nn.Module) -> nn.Module:
    from torch.nn.parallel import DataParallel, DistributedDataParallel
    while isinstance(model, (DistributedDataParallel, DataParallel)):
        model = model.module
    return model


def _rows(off: int, t: torch.Tensor) -> List[int]:
    """mh_ema_update_many rows {ema offset, source address, n} covering tensor t (f32, contiguous) stored at EMA offset `off`."""
    n, ptr, out = t.numel(), t.data_ptr(), []
    for s in range(0, n, _ROW):
        out += [off + s, ptr + 4 * s, min(_ROW, n - s)]
    return out


def ema_decay(step: Optional[int], decay: float, min_decay: float = 0.0, update_after_step: int = 0, use_warmup: bool = False,
              warmup_gamma: float = 1.0, warmup_power: float = 2 / 3) -> float:
    """timm's ModelEmaV3.get_decay (the kernels restate it on the device from the step counter: include/mirror_hip.h)."""
    if step is None:
        return decay
    step = max(0, step - update_after_step - 1)
    if step <= 0:
        return 0.0          # the first update copies the model
    if use_warmup:
        d = 1 - (1 + step / warmup_gamma) ** -warmup_power
        return max(min(d, decay), min_decay)
    return decay


class ModelEmaV3(nn.Module):
    """timm.utils.ModelEmaV3 (same constructor, `get_decay`, `update`, `set`, `forward`, `.module`, state_dict keys `module.*`).
    `foreach` is accepted for compatibility: every path is one launch.  `device="cpu"` (--model-ema-force-cpu) raises: this build has
    no CPU path.  Floating-point state must be f32."""

    def __init__(self, model: nn.Module, decay: float = 0.9999, min_decay: float = 0.0, update_after_step: int = 0,
                 use_warmup: bool = False, warmup_gamma: float = 1.0, warmup_power: float = 2 / 3, device=None,
                 foreach: bool = True, exclude_buffers: bool = False):
        super().__init__()
        if device is not None and torch.device(device).type == "cpu":
            raise NotImplementedError("ModelEmaV3(device='cpu') / --model-ema-force-cpu: mirror_amd has no CPU path; keep the EMA "
                                      "on the GPU")
        if warmup_gamma <= 0:
            raise ValueError("warmup_gamma must be > 0")
        model = _unwrap(model)
        self.decay, self.min_decay, self.update_after_step = float(decay), float(min_decay), int(update_after_step)
        self.use_warmup, self.warmup_gamma, self.warmup_power = bool(use_warmup), float(warmup_gamma), float(warmup_power)
        self.foreach, self.exclude_buffers = foreach, exclude_buffers
        src = model.state_dict(keep_vars=True)
        first = next(iter(src.values()), None)
        self.device = torch.device(device) if device is not None else (first.device if first is not None else torch.device("cpu"))
        if self.device.type != "cuda":
            raise MirrorHipError("ModelEmaV3 needs the model (or `device`) on an MI355X: mirror_amd has no CPU path")
        pnames = {n for n, _ in model.named_parameters()}
        for k, v in src.items():
            if v.is_floating_point() and v.dtype != f32:
                raise NotImplementedError(f"ModelEmaV3: {k} is {v.dtype}; the EMA kernels take f32 state only")
        # one flat arena: every f32 state_dict entry (parameters and floating buffers), state_dict order, 8-element aligned
        keys = [k for k, v in src.items() if v.is_floating_point()]
        offs, total = lay_out([src[k].numel() for k in keys])
        lay = list(zip(keys, offs))
        self.arena = torch.zeros(max(total, ALIGN), device=self.device, dtype=f32)
        off = dict(lay)
        # .module: the model's structure with its tensors replaced WITHOUT copying the storages they view (a parameter of an
        # engine-managed model is a view of the whole master arena, its .grad one of the grad arena) nor the captured graphs and
        # process groups a TrainEngine hangs on the modules
        memo = {}
        with torch.no_grad():
            for mod_name, mod in model.named_modules():
                for attr in ("_rna_graph", "_align_gather"):
                    if mod.__dict__.get(attr) is not None:
                        memo[id(mod.__dict__[attr])] = None
                pre = mod_name + "." if mod_name else ""
                for n, p in mod._parameters.items():
                    if p is None or id(p) in memo:
                        continue
                    o = off[pre + n]
                    view = self.arena[o:o + p.numel()].view(p.shape)
                    view.copy_(p.detach().to(self.device).reshape(p.shape))
                    memo[id(p)] = nn.Parameter(view, requires_grad=p.requires_grad)
                for n, b in mod._buffers.items():
                    if b is None or id(b) in memo:
                        continue
                    if pre + n in off:
                        o = off[pre + n]
                        view = self.arena[o:o + b.numel()].view(b.shape)
                        view.copy_(b.detach().to(self.device))
                        memo[id(b)] = view
                    else:
                        memo[id(b)] = b.detach().to(self.device).clone()
            self.module = copy.deepcopy(model, memo)
        self.module.eval()
        self._names = list(self.module.state_dict(keep_vars=True).keys())
        self._param_names = pnames
        self._lay = lay
        self._engine = None
        self._table_key = self._table = None
        self._nrows = 0
        # bf16 copies of the EMA weights (bf16 policies), refreshed by the forward pre-hook
        self._bf = None
        self._dirty = True
        self._ver = -1
        self.module.register_forward_pre_hook(self._refresh_shadows)
        self.module.register_load_state_dict_post_hook(lambda *_: self._touch())

    # ------------------------------------------------------------------ timm's API
    def get_decay(self, step: Optional[int] = None) -> float:
        return ema_decay(step, self.decay, self.min_decay, self.update_after_step, self.use_warmup, self.warmup_gamma,
                         self.warmup_power)

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)

    @torch.no_grad()
    def set(self, model: nn.Module) -> None:
        for e, s in zip(self.module.state_dict().values(), _unwrap(model).state_dict().values()):
            e.copy_(s.to(self.device))
        self._touch()

    @torch.no_grad()
    def update(self, model: nn.Module, step: Optional[int] = None) -> None:
        if self._engine is not None:
            eng = self._engine
            if step is None:
                raise ValueError("ModelEmaV3 is attached to a TrainEngine, which updates it inside its step: call "
                                 "update(model, step=num_updates) with the update count (engine.step_count)")
            if int(step) != eng.step_count:
                raise ValueError(f"ModelEmaV3.update(step={step}): the attached TrainEngine has made {eng.step_count} updates; "
                                 "the EMA it keeps is that of its own step count")
            return
        model = _unwrap(model)
        w = float(np.float32(1.0 - self.get_decay(step)))      # torch rounds timm's Python weight to f32 the same way
        src = list(model.state_dict(keep_vars=True).values())
        ema = list(self.module.state_dict(keep_vars=True).values())
        if len(src) != len(ema):
            raise ValueError(f"ModelEmaV3.update: the model has {len(src)} state entries, the EMA {len(ema)}")
        lerp, copies, seen = [], [], set()
        for k, e, s in zip(self._names, ema, src):
            s = s.detach()
            if e.data_ptr() in seen:          # a tied tensor appears under several names: one update
                continue
            seen.add(e.data_ptr())
            if e.is_floating_point() and (not self.exclude_buffers or k in self._param_names):
                if s.dtype != f32 or s.device != self.device or not s.is_contiguous() or s.numel() != e.numel():
                    raise MirrorHipError(f"ModelEmaV3.update: {k} must be a contiguous f32 tensor of {e.numel()} elements on "
                                         f"{self.device}, got {s.dtype} {tuple(s.shape)} on {s.device}")
                lerp.append(((e.data_ptr() - self.arena.data_ptr()) // 4, s))
            else:
                copies.append((e, s))
        key = tuple((o, s.data_ptr(), s.numel()) for o, s in lerp)
        if key != self._table_key:
            rows = []
            for o, s in lerp:
                rows += _rows(o, s)
            self._nrows = len(rows) // 3
            self._table = torch.tensor(rows, dtype=torch.int64).to(self.device) if rows else None
            self._table_key = key
        if self._nrows:
            K.ema_update_many(self.arena, self._table, self._nrows, w)
        for e, s in copies:
            e.detach().copy_(s.to(self.device))
        self._touch()

    # ------------------------------------------------------------------ TrainEngine attachment
    def _attach(self, pa, model: nn.Module, engine) -> Tuple[torch.Tensor, Optional[torch.Tensor], int]:
        """Re-lay the arena out like the master of `pa`, the ParamArena of `model` (same offsets; parameters outside it, and f32 buffers,
        behind it) and return (arena, table of the entries behind the master range or None, its row count).  Called once, by `engine`."""
        if self._engine is not None:
            raise ValueError("this ModelEmaV3 is already attached to a TrainEngine")
        src = dict(model.state_dict(keep_vars=True))
        if list(src.keys()) != self._names:
            raise ValueError("ModelEmaV3 attached to an engine whose model has other state entries than the EMA's")
        name_of = {id(v): k for k, v in src.items()}
        off = {name_of[id(p)]: o for p, o in zip(pa.params, pa.offsets)}
        tail = [k for k, _ in self._lay if k not in off]
        offs, total = lay_out([pa.numel] + [src[k].numel() for k in tail])      # (pa.numel is a multiple of ALIGN)
        off.update(zip(tail, offs[1:]))
        arena = torch.zeros(max(total, ALIGN), device=pa.device, dtype=f32)
        ema_sd = self.module.state_dict(keep_vars=True)
        with torch.no_grad():
            for k, _ in self._lay:
                e = ema_sd[k]
                o = off[k]
                arena[o:o + e.numel()].copy_(e.detach().reshape(-1))
                e.data = arena[o:o + e.numel()].view(e.shape)
        self.arena = arena
        self._lay = [(k, off[k]) for k, _ in self._lay]
        self._bf = None          # (its copies were published for the blocks the parameters have just left: not served any more)
        rows, cp = [], []
        for k in tail:
            s = src[k].detach()
            if self.exclude_buffers and k not in self._param_names:
                cp.append((ema_sd[k], s))
                continue
            if not s.is_contiguous() or s.device != pa.device:
                raise MirrorHipError(f"ModelEmaV3: {k} must be a contiguous f32 tensor on {pa.device}")
            rows += _rows(off[k], s)
        self._engine_copies = cp + [(ema_sd[k], src[k].detach()) for k in self._names if not ema_sd[k].is_floating_point()]
        self._engine = engine
        self._touch()
        table = torch.tensor(rows, dtype=torch.int64).to(pa.device) if rows else None
        return arena, table, len(rows) // 3

    def _cfg(self) -> EmaCfg:
        return EmaCfg(self.decay, self.min_decay, self.warmup_gamma, self.warmup_power, self.update_after_step, int(self.use_warmup))

    # ------------------------------------------------------------------ bf16 copies of the EMA weights
    def _touch(self) -> None:
        self._dirty = True

    def _refresh_shadows(self, module, args) -> None:
        from .models.mirror import resolve_precision
        if resolve_precision(getattr(module, "precision", None)).act != bf16:
            return
        ver = self._versions()
        if not self._dirty and self._ver == ver:
            return
        if self._bf is None:
            base = self.arena.data_ptr()
            self._bf = Fn.ArenaShadows(self.arena, [(p, (p.data_ptr() - base) // 4) for p in module.parameters()])
            self._bf.publish()
        self._bf.refresh()
        self._dirty = False
        self._ver = ver

    def _versions(self) -> int:
        """Sum of the version counters of the EMA tensors: grows with every write through torch (load_state_dict, set, copy_)."""
        return sum(t._version for t in self.module.state_dict(keep_vars=True).values())

    # ------------------------------------------------------------------ state
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        if assign:
            raise NotImplementedError("ModelEmaV3.load_state_dict(assign=True): the EMA parameters are views of its arena")
        out = super().load_state_dict(state_dict, strict=strict)
        self._touch()
        return out
