"""InfoNCE on HIP kernels — host-side mirror of the reference's `losses/info_nce.py` (same kwargs and checks).

`negative_keys=None` (losses/info_nce.py:144-164): the other samples' positive keys are the negatives; `symmetric` adds the
transposed term.

Explicit `negative_keys` (losses/info_nce.py:126-143): the reference builds `logits = cat([pos, neg], 1)` and `labels = 0` and never
assigns `loss`, so its `return loss` raises UnboundLocalError.  The line it forgets is the
`F.cross_entropy(logits / temperature, labels, reduction=reduction)` of the info-nce-pytorch package the file was copied from, and
that is what runs here:  with q^, k^, n^ = F.normalize(.., dim=-1),
    pos[i] = q^[i].k^[i];   neg[i, j] = q^[i].n^[j] ("unpaired", negative_keys [M, D]) or q^[i].n^[i, j] ("paired", [N, M, D]);
    row[i] = logsumexp([pos[i] | neg[i, :]] / temperature) - pos[i] / temperature;   reduction "mean" / "sum" -> 0-d, "none" -> [N].
`symmetric` is ignored when `negative_keys` is given: the reference reads that flag only inside its implicit-negatives branch
(:153-164).  `negative_keys` may be f32 or bf16 and is read in place in its own dtype (its gradient comes back in that dtype);
norms, products and the log-sum-exp are f32.  A `negative_keys` that does not require grad costs no backward pass over it.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import functional as Fn
from .. import kernels as K

__all__ = ["InfoNCE"]
f32 = torch.float32


class InfoNCE(nn.Module):
    def __init__(self, temperature=0.1, reduction="mean", negative_mode="unpaired", symmetric=False):
        super().__init__()
        self.temperature = temperature
        self.reduction = reduction
        self.negative_mode = negative_mode
        self.symmetric = symmetric

    def forward(self, query, positive_key, negative_keys=None):
        return self.info_nce(query, positive_key, negative_keys, temperature=self.temperature,
                             reduction=self.reduction, negative_mode=self.negative_mode, symmetric=self.symmetric)

    def info_nce(self, query, positive_key, negative_keys=None, temperature=0.1, reduction="mean",
                 negative_mode="unpaired", symmetric=False):
        # input checks: same conditions and messages as losses/info_nce.py:85-120
        if query.dim() != 2:
            raise ValueError("<query> must have 2 dimensions.")
        if positive_key.dim() != 2:
            raise ValueError("<positive_key> must have 2 dimensions.")
        if negative_keys is not None:
            if negative_mode == "unpaired" and negative_keys.dim() != 2:
                raise ValueError("<negative_keys> must have 2 dimensions if <negative_mode> == 'unpaired'.")
            if negative_mode == "paired" and negative_keys.dim() != 3:
                raise ValueError("<negative_keys> must have 3 dimensions if <negative_mode> == 'paired'.")
        if len(query) != len(positive_key):
            raise ValueError("<query> and <positive_key> must must have the same number of samples.")
        if negative_keys is not None:
            if negative_mode == "paired" and len(query) != len(negative_keys):
                raise ValueError("If negative_mode == 'paired', then <negative_keys> must have the same number of samples as <query>.")
        if query.shape[-1] != positive_key.shape[-1]:
            raise ValueError("Vectors of <query> and <positive_key> should have the same number of components.")
        if negative_keys is not None:
            if query.shape[-1] != negative_keys.shape[-1]:
                raise ValueError("Vectors of <query> and <negative_keys> should have the same number of components.")
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f"{reduction} is not a valid value for reduction")
        if negative_keys is not None:
            return self._explicit_negatives(query, positive_key, negative_keys, temperature, reduction, negative_mode)
        n = query.shape[0]
        q = Fn.L2NormRowFn.apply(query.float(), 1e-12, f32)          # F.normalize(dim=-1), losses/info_nce.py:171-172
        k = Fn.L2NormRowFn.apply(positive_key.float(), 1e-12, f32)
        coef = (1.0 / n) if reduction == "mean" else 1.0
        per_row = reduction == "none"
        half = 0.5 if symmetric else 1.0
        loss = Fn.CERowsFn.apply(Fn.MatmulNTFn.apply(q, k), None, 1.0 / temperature, 0, coef * half, per_row)
        if symmetric:
            loss = loss + Fn.CERowsFn.apply(Fn.MatmulNTFn.apply(k, q), None, 1.0 / temperature, 0, coef * half, per_row)
        return loss if per_row else loss.reshape(())

    def _explicit_negatives(self, query, positive_key, negative_keys, temperature, reduction, negative_mode):
        # CE(cat([pos, neg], 1) / temperature, 0): losses/info_nce.py:126-143 with the missing cross-entropy supplied
        if negative_mode not in ("unpaired", "paired"):
            raise ValueError(f"{negative_mode} is not a valid value for negative_mode")
        if negative_keys.shape[-2] == 0:
            raise ValueError("<negative_keys> must hold at least one negative key.")
        K._chk(query, positive_key, negative_keys)
        q = Fn.L2NormRowFn.apply(query.float(), 1e-12, f32)          # F.normalize(dim=-1), losses/info_nce.py:171-172
        k = Fn.L2NormRowFn.apply(positive_key.float(), 1e-12, f32)
        fn = Fn.InfoNCEPairedFn if negative_mode == "paired" else Fn.InfoNCEUnpairedFn
        return fn.apply(q, k, negative_keys, 1.0 / temperature, reduction)

    def transpose(self, x):
        return x.transpose(-2, -1)

    def normalize(self, *xs):
        return [None if x is None else Fn.L2NormRowFn.apply(x.float(), 1e-12, f32) for x in xs]
