"""LabelSmoothingCrossEntropy on HIP kernels — timm's loss of the same name (timm.loss), the subtyping template's training loss
(train_subtyping.py:981-984, configs/subtyping/mirror.template.yaml:106: smoothing 0.1).  Same signature and attributes
(`smoothing`, `confidence`); forward(x, target) returns the mean over the rows of

    loss_r = confidence * (lse_r - x[r, y_r]) + smoothing * (lse_r - mean_c x[r, c]),   lse_r = logsumexp(x[r, :]).

`x` must be f32 device logits [N, C]; `target` int32 / int64 labels [N] on the device or the host (host labels are copied
without blocking; a graph capture needs device labels).  A label outside [0, C) gives NaN where timm's gather raises.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import kernels as K
from ._cls_common import check_smoothing, cls_loss

__all__ = ["LabelSmoothingCrossEntropy"]


class LabelSmoothingCrossEntropy(nn.Module):
    """NLL loss with label smoothing (timm's signature)."""

    def __init__(self, smoothing=0.1):
        super().__init__()
        if float(smoothing) >= 1.0:
            raise ValueError(f"smoothing must be below 1.0, got {smoothing}")
        self.smoothing = check_smoothing(smoothing, "smoothing")
        self.confidence = 1.0 - self.smoothing

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return cls_loss(x, target, self.smoothing, K.NO_IGNORE, "mean")
