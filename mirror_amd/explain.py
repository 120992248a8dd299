"""Presentation of the slide attention map that `FeatureTransMIL.forward_with_attention` / `MIRRORClassifier.forward_with_attention`
return (the CLS row of [3P] NystromAttention's `return_attn=True`, from csrc/nystrom_cls.hip).  Plain torch ops on [B, heads, N]
tensors, on whatever device the map lives on: this is display code, not the product path.
"""
from __future__ import annotations

import torch

_REDUCE = ("mean", "max")


def slide_attention(attn: torch.Tensor, layer: int = -1, reduce: str = "mean") -> torch.Tensor:
    """attn [B, layers, heads, N] -> [B, N] heat map: the chosen layer's heads reduced by `reduce` ("mean" or "max"), then min-max
    normalised per slide to [0, 1] (a constant slide maps to 0)."""
    if not isinstance(attn, torch.Tensor) or attn.dim() != 4:
        got = tuple(attn.shape) if isinstance(attn, torch.Tensor) else type(attn).__name__
        raise ValueError(f"slide_attention: attn must be [B, layers, heads, N] (4 dims), got {got}")
    if reduce not in _REDUCE:
        raise ValueError(f"slide_attention: unknown reduce {reduce!r}; choose from {_REDUCE}")
    if not -attn.shape[1] <= layer < attn.shape[1]:
        raise ValueError(f"slide_attention: layer {layer} outside the {attn.shape[1]} layers of attn")
    a = attn[:, layer].to(torch.float32)
    a = a.mean(dim=1) if reduce == "mean" else a.amax(dim=1)
    lo, hi = a.amin(dim=1, keepdim=True), a.amax(dim=1, keepdim=True)
    return (a - lo) / (hi - lo).clamp_min(torch.finfo(torch.float32).tiny)
