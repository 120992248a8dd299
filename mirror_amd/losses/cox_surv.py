"""CoxSurvLoss on HIP kernels: the Cox proportional-hazards partial likelihood of a one-logit head on the follow-up time itself
(the `CoxSurvLoss` of MIL survival code, DeepSurv, pycox), with Breslow or Efron handling of tied event times.  The loss and its
logit gradient are all-pairs passes in `csrc/cox.hip`: nothing N x N is stored and exp never sees a positive argument.

`forward(logits, event_times, censoring)` has the argument order of the other two survival losses, with `censoring == 1` the
event flag as there.  Unlike them it takes floating-point or integer `event_times`: these are times, not bins.  Logits are f32
device tensors [N] or [N, 1] (a column view is read in place), 1 <= N <= 65536, with max - min <= 700.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import functional as Fn
from .. import kernels as K

__all__ = ["CoxSurvLoss"]


class CoxSurvLoss(nn.Module):
    """loss_i = e_i (log den_i - r_i), den_i the sum of exp(r_j) over the risk set {t_j >= t_i}, less Efron's share of the tied
    events.  reduction: "mean" divides the sum by max(n_events, 1) (DeepSurv / pycox), "batch" by N (MCAT), "sum", "none" ([N])."""

    def __init__(self, ties="efron", reduction="mean"):
        super().__init__()
        if ties not in K.COX_TIES:
            raise ValueError(f"ties must be one of {sorted(K.COX_TIES)}, got {ties!r}")
        if reduction not in K.COX_RED:
            raise ValueError(f"reduction must be one of {sorted(K.COX_RED)}, got {reduction!r}")
        self.ties = ties
        self.reduction = reduction

    def forward(self, logits: torch.Tensor, event_times: torch.Tensor, censoring: torch.Tensor) -> torch.Tensor:
        if self.ties not in K.COX_TIES or self.reduction not in K.COX_RED:
            raise ValueError(f"unknown ties / reduction: {self.ties!r} / {self.reduction!r}")
        if event_times.is_complex() or event_times.dtype == torch.bool:
            raise TypeError(f"event_times must be real-valued times, got {event_times.dtype}")
        return Fn.CoxLossFn.apply(logits, event_times, censoring, self.ties, self.reduction)
