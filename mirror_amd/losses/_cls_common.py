"""Input checks shared by the classification losses of train_subtyping.py (label_smoothing.py, cross_entropy.py)."""
from __future__ import annotations

import torch

from .. import functional as Fn

REDUCTIONS = ("mean", "sum", "none")


def check_smoothing(s: float, name: str) -> float:
    s = float(s)
    if not 0.0 <= s <= 1.0:
        raise ValueError(f"{name} must lie in [0, 1], got {s}")
    return s


def check_reduction(reduction: str) -> str:
    if reduction not in REDUCTIONS:
        raise ValueError(f"{reduction} is not a valid value for reduction")
    return reduction


def cls_loss(logits: torch.Tensor, target: torch.Tensor, smoothing: float, ignore_index: int, reduction: str) -> torch.Tensor:
    if target.is_floating_point() or target.is_complex():
        raise NotImplementedError("class-probability targets are not built: pass integer class labels")
    return Fn.ClsCELossFn.apply(logits, target, smoothing, ignore_index, check_reduction(reduction))
