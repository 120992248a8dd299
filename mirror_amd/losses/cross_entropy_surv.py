"""CrossEntropySurvLoss on HIP kernels — host-side mirror of the reference's `losses/cross_entropy_surv.py` (same kwargs,
attributes and `forward(logits, event_times, censoring)`); the loss and its logit gradient are one launch each
(`csrc/survival.hip`).

Logits must be f32 device tensors.  Floating-point `event_times` raise TypeError (stated deviation, as for NLLSurvLoss).  Where the
reference's `gather` raises (an uncensored row whose event time lies outside [0, M]), that row's loss and gradient are NaN here:
the check would cost a host sync.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import functional as Fn
from .. import kernels as K
from .nll_surv import check_event_times

__all__ = ["CrossEntropySurvLoss"]


class CrossEntropySurvLoss(nn.Module):
    """Cross-entropy over the M + 1 outcomes (event in bin t, or no event) built from the sigmoid hazards; `reduction="none"`
    returns [N, 1], as the reference's gather does."""

    def __init__(self, eps=1e-7, reduction="mean"):
        super().__init__()
        self.eps = eps
        self.reduction = reduction

    def forward(self, logits: torch.Tensor, event_times: torch.Tensor, censoring: torch.Tensor) -> torch.Tensor:
        check_event_times(event_times)
        return Fn.SurvLossFn.apply(logits, event_times, censoring, K.SURV_CE, float(self.eps), 0.0, self.reduction)
