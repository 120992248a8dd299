"""kNN probe of frozen embeddings: the training-free check of a pre-trained encoder.  A bank of labelled embeddings votes for every
query with its k nearest neighbours, each weighted by exp(similarity / temperature) (Wu et al. 2018, as DINO evaluates):

    score[i, c] = sum over the k neighbours j of query i with label c of exp((s_ij - max_j' s_ij') / T), divided by the row's total.

The neighbours come from `mh_retrieval_topk` (the exact-f32 product of the retrieval ranks with a selecting epilogue: the
[nq, n] similarities are never stored), the vote from `mh_knn_scores`, and the scores go to the metrics of `mirror_amd.metrics`
(`accuracy`, `MulticlassAUROC`, `MulticlassF1Score`), so nothing returns to the host between the product and the metrics.

A cohort has several slides per patient.  With `group` ids (the patient of every row) a neighbour of the query's own group never
votes: `leave_one_out()` over a bank with groups is leave-one-PATIENT-out, and without them leave-one-row-out.

Not built: bf16 keys, k > 64, a bank gathered over DDP ranks (`merge_state` merges states the caller has gathered).
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Iterable, List, Optional

import torch

from . import kernels as K
from ._lib import MirrorHipError
from .metrics import MulticlassAUROC, MulticlassF1Score, accuracy
from .retrieval import _l2

__all__ = ["KNNProbe"]


def _ids(t, n: int, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.numel() != n or t.dtype not in (torch.int32, torch.int64):
        got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{what} must be an int32 / int64 [{n}] tensor, got {got}")
    return t


class KNNProbe:
    """`fit(emb, labels, group=None)` adds rows to the bank (f32 copies on the device, no host wait; calls concatenate);
    `scores(query_emb, query_group=None)` returns the class scores f32 [nq, C] on the device; `evaluate(query_emb, query_labels,
    query_group=None)` and `leave_one_out()` (the bank against itself) return an OrderedDict of `knn_acc` (top-1 accuracy in percent,
    as `metrics.accuracy`), `knn_auroc` (macro one-vs-rest), `knn_f1` (`average`), `knn_k` and `knn_n` (the bank size, which the values
    depend on); the host is first waited for when those three results are read back.

    k: neighbours per query, 1..64.  temperature: T of the vote; math.inf is the unweighted vote.  normalize: compare cosines (both
    sides through mh_l2norm_fwd), the usual choice; False compares raw dot products."""

    def __init__(self, num_classes: int, k: int = 20, temperature: float = 0.07, normalize: bool = True, average: Optional[str] = "weighted",
                 device=None):
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not (2 <= num_classes <= 1024):
            raise ValueError(f"num_classes must be an int in [2, 1024], got {num_classes!r}")
        if isinstance(k, bool) or not isinstance(k, int) or not (1 <= k <= 64):
            raise ValueError(f"k must be an int in [1, 64], got {k!r}")
        t = float(temperature)
        if not t > 0.0:
            raise ValueError(f"temperature must be positive (math.inf: the unweighted vote), got {temperature!r}")
        if average not in ("micro", "macro", "weighted"):
            raise ValueError(f'average must be "micro", "macro" or "weighted", got {average!r}')
        d = torch.device("cuda") if device is None else torch.device(device)
        if d.type != "cuda":
            raise MirrorHipError(f"mirror_amd metrics keep their state on a HIP device, got {d}")
        self.num_classes = num_classes
        self.k = k
        self.temperature = t
        self.inv_temperature = 0.0 if math.isinf(t) else 1.0 / t
        self.normalize = bool(normalize)
        self.average = average
        self.device = d
        self.emb: List[torch.Tensor] = []             # f32 [n_i, D] per fit
        self.labels: List[torch.Tensor] = []          # int64 [n_i]
        self.group: List[torch.Tensor] = []           # int64 [n_i] per fit, or none at all

    # ------------------------------------------------------------------ the bank
    def fit(self, emb: torch.Tensor, labels: torch.Tensor, group: Optional[torch.Tensor] = None) -> "KNNProbe":
        """emb: embeddings [n, D]; labels: integer [n] in [0, num_classes) (not checked here: that would wait on the host; a label
        outside never votes); group: integer [n], e.g. the patient of every slide (every fit, or none)."""
        if not isinstance(emb, torch.Tensor) or emb.dim() != 2 or not emb.is_floating_point():
            got = f"{emb.dtype} {tuple(emb.shape)}" if isinstance(emb, torch.Tensor) else type(emb).__name__
            raise ValueError(f"emb must be floating point [n, D], got {got}")
        n = emb.shape[0]
        _ids(labels, n, "labels")
        if group is not None:
            _ids(group, n, "group")
        if self.emb and self.emb[0].shape[1] != emb.shape[1]:
            raise ValueError(f"embedding width changed from {self.emb[0].shape[1]} to {emb.shape[1]}")
        if self.emb and (group is not None) != bool(self.group):
            raise ValueError("either every fit() passes `group` or none does: this one " +
                             ("does, the earlier ones did not" if group is not None else "does not, the earlier ones did"))
        self.emb.append(emb.detach().to(device=self.device, dtype=torch.float32, non_blocking=True, copy=True))
        self.labels.append(labels.detach().to(device=self.device, dtype=torch.int64, non_blocking=True, copy=True))
        if group is not None:
            self.group.append(group.detach().to(device=self.device, dtype=torch.int64, non_blocking=True, copy=True))
        return self

    def _bank(self):
        n = sum(t.shape[0] for t in self.emb)
        if n == 0:
            raise ValueError("KNNProbe: the bank is empty (call fit() first)")
        cat = lambda ts: ts[0] if len(ts) == 1 else torch.cat(ts)      # noqa: E731
        return cat(self.emb), cat(self.labels), (cat(self.group) if self.group else None)

    # ------------------------------------------------------------------ the vote
    def _vote(self, query: torch.Tensor, bank: torch.Tensor, labels: torch.Tensor, qgroup, kgroup) -> torch.Tensor:
        if self.normalize:
            query = _l2(query)
            bank = query if bank is None else _l2(bank)
        elif bank is None:
            bank = query
        val, idx = K.retrieval_topk(query, bank, self.k, qgroup, kgroup)
        return K.knn_scores(idx, val, labels, self.num_classes, self.inv_temperature)

    def _query(self, query_emb: torch.Tensor, width: int) -> torch.Tensor:
        if not isinstance(query_emb, torch.Tensor) or query_emb.dim() != 2 or not query_emb.is_floating_point() or query_emb.shape[1] != width:
            got = f"{query_emb.dtype} {tuple(query_emb.shape)}" if isinstance(query_emb, torch.Tensor) else type(query_emb).__name__
            raise ValueError(f"query_emb must be floating point [nq, {width}], got {got}")
        if query_emb.shape[0] == 0:
            raise ValueError("query_emb has no rows")
        return query_emb.detach().to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous()

    def scores(self, query_emb: torch.Tensor, query_group: Optional[torch.Tensor] = None) -> torch.Tensor:
        """f32 [nq, num_classes] on the device, no host wait: every row sums to 1 (all zeros if no neighbour could vote).
        query_group [nq]: the bank rows of a query's own group do not vote (needs a bank fitted with `group`)."""
        bank, labels, group = self._bank()
        q = self._query(query_emb, bank.shape[1])
        if query_group is not None:
            if group is None:
                raise ValueError("query_group needs a bank fitted with `group`")
            query_group = _ids(query_group, q.shape[0], "query_group")
            return self._vote(q, bank, labels, query_group, group)
        return self._vote(q, bank, labels, None, None)

    def _report(self, scores: torch.Tensor, labels: torch.Tensor, n_bank: int) -> "OrderedDict[str, float]":
        acc = accuracy(scores, labels)[0]
        auroc = MulticlassAUROC(num_classes=self.num_classes, average="macro", device=self.device).update(scores, labels)
        f1 = MulticlassF1Score(num_classes=self.num_classes, average=self.average, device=self.device).update(scores, labels)
        out: "OrderedDict[str, float]" = OrderedDict()      # every launch is queued: the readbacks below are the first host waits
        out["knn_acc"] = float(acc.item())
        out["knn_auroc"] = float(auroc.compute().item())
        out["knn_f1"] = float(f1.compute().item())
        out["knn_k"] = self.k
        out["knn_n"] = n_bank
        return out

    def evaluate(self, query_emb: torch.Tensor, query_labels: torch.Tensor, query_group: Optional[torch.Tensor] = None):
        """The metrics of the bank's vote on labelled queries (a validation split against the training bank)."""
        if not isinstance(query_emb, torch.Tensor) or query_emb.dim() != 2:
            raise ValueError("query_emb must be [nq, D]")
        labels = _ids(query_labels, query_emb.shape[0], "query_labels").to(device=self.device, dtype=torch.int64, non_blocking=True)
        return self._report(self.scores(query_emb, query_group), labels, sum(t.shape[0] for t in self.emb))

    def leave_one_out(self) -> "OrderedDict[str, float]":
        """Every bank row queries the bank without its own group: the bank's `group`, or the row itself when it has none."""
        bank, labels, group = self._bank()
        if group is None:
            group = torch.arange(bank.shape[0], device=self.device, dtype=torch.int64)
        return self._report(self._vote(bank, None, labels, group, group), labels, bank.shape[0])

    # ------------------------------------------------------------------ state
    def reset(self) -> "KNNProbe":
        self.emb, self.labels, self.group = [], [], []
        return self

    def merge_state(self, probes: Iterable["KNNProbe"]) -> "KNNProbe":
        for m in probes:
            if m.emb and self.emb and m.emb[0].shape[1] != self.emb[0].shape[1]:
                raise ValueError(f"cannot merge kNN banks of widths {m.emb[0].shape[1]} and {self.emb[0].shape[1]}")
            if m.emb and self.emb and bool(m.group) != bool(self.group):
                raise ValueError("cannot merge a kNN bank with group ids and one without")
            self.emb.extend(t.to(self.device) for t in m.emb)
            self.labels.extend(t.to(self.device) for t in m.labels)
            self.group.extend(t.to(self.device) for t in m.group)
        return self
