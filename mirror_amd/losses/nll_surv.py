"""NLLSurvLoss on HIP kernels — host-side mirror of the reference's `losses/nll_surv.py` (same kwargs, attributes and
`forward(logits, event_times, censoring)`); the loss and its logit gradient are one launch each (`csrc/survival.hip`).

Logits must be f32 device tensors (train_survival.py passes `output.float()`).  Floating-point `event_times` raise TypeError
(the trainer always passes the dataset's integer `disc_label`); the reference would compare them with the bin index as floats.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import functional as Fn
from .. import kernels as K

__all__ = ["NLLSurvLoss"]


def check_event_times(event_times: torch.Tensor) -> None:
    if event_times.is_floating_point() or event_times.is_complex():
        raise TypeError(f"event_times must be an integer tensor (discrete time bins), got {event_times.dtype}")


class NLLSurvLoss(nn.Module):
    """Negative log-likelihood of discrete-time survival from logits (sigmoid hazards clamped to [eps, 1 - eps]); censored rows
    weighted (1 - alpha), uncensored rows 1, rows whose censoring is neither 0 nor 1 contribute 0."""

    def __init__(self, alpha=0.0, eps=1e-7, reduction="mean"):
        super().__init__()
        self.alpha = alpha
        self.eps = eps
        self.reduction = reduction

    def forward(self, logits: torch.Tensor, event_times: torch.Tensor, censoring: torch.Tensor) -> torch.Tensor:
        check_event_times(event_times)
        return Fn.SurvLossFn.apply(logits, event_times, censoring, K.SURV_NLL, float(self.eps), float(self.alpha), self.reduction)
