"""CrossEntropyLoss on HIP kernels — nn.CrossEntropyLoss's signature for integer class labels, the subtyping trainer's loss without
smoothing (train_subtyping.py:986) and its validation loss (:990).  Per row

    loss_r = (1 - label_smoothing) * (lse_r - x[r, y_r]) + label_smoothing * (lse_r - mean_c x[r, c]),

0 for rows labelled `ignore_index`; "mean" divides the sum by the number of the other rows.  `x` must be f32 device logits [N, C];
`target` int32 / int64 labels [N] on the device or the host.  Not built: class `weight` (NotImplementedError), class-probability
targets (NotImplementedError) and inputs of another rank.  A label that is neither `ignore_index` nor in [0, C) gives NaN in its
row where torch raises (CPU) or device-asserts (GPU).
"""
from __future__ import annotations

import torch
from torch import nn

from ._cls_common import check_reduction, check_smoothing, cls_loss

__all__ = ["CrossEntropyLoss"]


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss(weight=None, size_average=None, ignore_index=-100, reduce=None, reduction="mean", label_smoothing=0.0)."""

    def __init__(self, weight=None, size_average=None, ignore_index=-100, reduce=None, reduction="mean", label_smoothing=0.0):
        super().__init__()
        if weight is not None:
            raise NotImplementedError("CrossEntropyLoss: class weights are not built")
        if size_average is not None or reduce is not None:
            reduction = nn.modules.loss._Reduction.legacy_get_string(size_average, reduce)
        self.weight = None
        self.ignore_index = int(ignore_index)
        self.reduction = check_reduction(reduction)
        self.label_smoothing = check_smoothing(label_smoothing, "label_smoothing")

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return cls_loss(input, target, self.label_smoothing, self.ignore_index, self.reduction)
