"""Validation metrics of train_subtyping.py on HIP kernels, with torcheval's surface: `MulticlassAUROC`, `MulticlassF1Score` and
`sync_and_compute` (train_subtyping.py:1355-1360, :1391-1392, :1419-1424), and timm's top-1 `accuracy` (:1390).  torcheval and
timm are not dependencies: the definitions are restated from their documented behaviour.

Every metric keeps its state on its device; `update()` launches kernels and never waits on the host.  `compute()` reads the
state back once and returns an f64 tensor on the device: a scalar, or a [C] vector for `average=None`.

* `MulticlassF1Score`: the state is an int64 [C, C] confusion matrix (`mh_cls_confusion`).  Per class F1_c = 2 tp_c /
  (n_label_c + n_pred_c), 0 where that is 0 / 0.  "micro": correct rows / rows; "macro": mean of F1_c over the classes with
  n_label_c + n_pred_c > 0; "weighted": sum F1_c n_label_c / sum n_label_c over the same classes; None / "none": the vector.
* `MulticlassAUROC`: the state is every score row and label seen.  One-vs-rest per class c with the raw column scores[:, c]:
  AUROC_c = (#{pos > neg} + 0.5 #{pos == neg}) / (P_c Q_c) from exact pair counts (`mh_auroc_counts`); 0.5 when P_c or Q_c is
  0 (torcheval's rule); NaN when the column holds a NaN score (torcheval's value there depends on where its sort puts NaN).
  "macro": the mean over the classes; None / "none": the vector.

A label outside [0, C) makes `compute()` raise ValueError (torcheval raises on it in `update()`, which would need a host read).
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import kernels as K
from ._lib import MirrorHipError

__all__ = ["MulticlassAUROC", "MulticlassF1Score", "accuracy", "sync_and_compute"]


def _device(device) -> torch.device:
    d = torch.device("cuda") if device is None else torch.device(device)
    if d.type != "cuda":
        raise MirrorHipError(f"mirror_amd metrics keep their state on a HIP device, got {d}")
    return d


def _scores(x: torch.Tensor, device: torch.device) -> torch.Tensor:
    """Scores as f32 [N, C] on `device` (bf16 / fp16 convert exactly)."""
    if not (x.is_floating_point() and x.dim() == 2):
        raise ValueError(f"input must be floating-point scores [N, C], got {x.dtype} {tuple(x.shape)}")
    return x.detach().to(device=device, dtype=torch.float32, non_blocking=True)


def _labels(t: torch.Tensor, n: int) -> torch.Tensor:
    if t.dim() != 1 or t.numel() != n:
        raise ValueError(f"target must be [{n}], got {tuple(t.shape)}")
    if t.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"target must be int32 or int64, got {t.dtype}")
    return t


def _result(v: np.ndarray, device: torch.device) -> torch.Tensor:
    return torch.from_numpy(np.asarray(v, dtype=np.float64)).to(device)


class MulticlassF1Score:
    """torcheval.metrics.MulticlassF1Score(*, num_classes=None, average="micro", device=None).  `num_classes` is required unless
    average is "micro"; without it the class count is taken from the first [N, C] score input."""

    AVERAGES = ("micro", "macro", "weighted", "none", None)

    def __init__(self, *, num_classes: Optional[int] = None, average: Optional[str] = "micro", device=None):
        if average not in self.AVERAGES:
            raise ValueError(f"`average` was not in the allowed value of {self.AVERAGES}, got {average}.")
        if num_classes is None and average != "micro":
            raise ValueError(f"num_classes should be a positive number when average={average}, got num_classes=None.")
        if num_classes is not None and int(num_classes) < 1:
            raise ValueError(f"num_classes should be a positive number, got {num_classes}.")
        self.num_classes = None if num_classes is None else int(num_classes)
        self.average = average
        self.device = _device(device)
        self.conf: Optional[torch.Tensor] = None      # int64 [C, C], [label, prediction]
        self.bad: Optional[torch.Tensor] = None       # int64 [1]: rows with a label / prediction outside [0, C)

    def _state(self, C: int) -> None:
        if self.conf is None:
            self.conf = torch.zeros((C, C), dtype=torch.int64, device=self.device)
            self.bad = torch.zeros((1,), dtype=torch.int64, device=self.device)

    def update(self, input: torch.Tensor, target: torch.Tensor) -> "MulticlassF1Score":
        """input: scores [N, C] (prediction = argmax) or predicted labels [N]; target: labels [N]."""
        target = _labels(target, input.shape[0])
        if input.dim() == 2:
            C = self.num_classes if self.num_classes is not None else (self.conf.shape[0] if self.conf is not None else input.shape[1])
            if input.shape[1] != C:
                raise ValueError(f"input has {input.shape[1]} classes, the metric {C}")
            input = _scores(input, self.device)
        elif input.dim() == 1 and input.dtype in (torch.int32, torch.int64):
            if self.num_classes is None and self.conf is None:
                raise ValueError("predicted-label input needs num_classes (or an earlier [N, C] score input)")
            C = self.num_classes if self.num_classes is not None else self.conf.shape[0]
            input = input.to(self.device, non_blocking=True)
        else:
            raise ValueError(f"input must be scores [N, C] or integer labels [N], got {input.dtype} {tuple(input.shape)}")
        self._state(C)
        K.cls_confusion(input, target, self.conf, self.bad)
        return self

    def compute(self) -> torch.Tensor:
        if self.conf is None:
            raise ValueError("MulticlassF1Score.compute(): no samples (call update() first)")
        host = torch.cat((self.bad, self.conf.reshape(-1))).cpu().numpy()
        bad, conf = int(host[0]), host[1:].reshape(self.conf.shape)
        if bad:
            raise ValueError(f"MulticlassF1Score: {bad} samples had a label or predicted label outside [0, {conf.shape[0]})")
        total = int(conf.sum())
        if total == 0:
            raise ValueError("MulticlassF1Score.compute(): no samples (call update() first)")
        tp = np.diag(conf).astype(np.float64)
        n_label, n_pred = conf.sum(1).astype(np.float64), conf.sum(0).astype(np.float64)
        if self.average == "micro":
            return _result(tp.sum() / total, self.device)
        den = n_label + n_pred
        f1 = np.divide(2.0 * tp, den, out=np.zeros_like(tp), where=den > 0)
        if self.average in (None, "none"):
            return _result(f1, self.device)
        seen = den > 0
        if self.average == "macro":
            return _result(f1[seen].mean(), self.device)
        return _result((f1[seen] * n_label[seen]).sum() / n_label[seen].sum(), self.device)

    def reset(self) -> "MulticlassF1Score":
        self.conf = self.bad = None
        return self

    def merge_state(self, metrics: Iterable["MulticlassF1Score"]) -> "MulticlassF1Score":
        for m in metrics:
            if m.conf is None:
                continue
            self._state(m.conf.shape[0])
            if m.conf.shape != self.conf.shape:
                raise ValueError(f"cannot merge F1 states of {m.conf.shape[0]} and {self.conf.shape[0]} classes")
            self.conf += m.conf.to(self.device)
            self.bad += m.bad.to(self.device)
        return self


class MulticlassAUROC:
    """torcheval.metrics.MulticlassAUROC(*, num_classes, average="macro", device=None): one-vs-rest AUROC over every sample
    accumulated so far, from the raw scores."""

    AVERAGES = ("macro", "none", None)

    def __init__(self, *, num_classes: int, average: Optional[str] = "macro", device=None):
        if average not in self.AVERAGES:
            raise ValueError(f"`average` was not in the allowed value of {self.AVERAGES}, got {average}.")
        if num_classes is None or int(num_classes) < 2:
            raise ValueError(f"`num_classes` has to be at least 2, got {num_classes}.")
        self.num_classes = int(num_classes)
        self.average = average
        self.device = _device(device)
        self.inputs: List[torch.Tensor] = []          # f32 [n_i, C] per update
        self.targets: List[torch.Tensor] = []         # int64 [n_i]

    def update(self, input: torch.Tensor, target: torch.Tensor) -> "MulticlassAUROC":
        """input: scores [N, C] (logits as the trainer passes them); target: labels [N]."""
        target = _labels(target, input.shape[0])
        if input.dim() != 2 or input.shape[1] != self.num_classes:
            raise ValueError(f"input must be [N, {self.num_classes}], got {tuple(input.shape)}")
        self.inputs.append(_scores(input, self.device).clone())
        self.targets.append(target.to(device=self.device, dtype=torch.int64, non_blocking=True).clone())
        return self

    def compute(self) -> torch.Tensor:
        n = sum(t.numel() for t in self.targets)
        if n == 0:
            raise ValueError("MulticlassAUROC.compute(): no samples (call update() first)")
        x = self.inputs[0] if len(self.inputs) == 1 else torch.cat(self.inputs)
        y = self.targets[0] if len(self.targets) == 1 else torch.cat(self.targets)
        counts = K.auroc_counts(x, y).cpu().numpy()
        u2, P, Q, nan = (counts[:, q] for q in range(4))
        bad = n - int(P.sum())
        if bad:
            raise ValueError(f"MulticlassAUROC: {bad} samples had a label outside [0, {self.num_classes})")
        pq = P.astype(np.float64) * Q.astype(np.float64)
        auc = np.divide(u2.astype(np.float64), 2.0 * pq, out=np.full(pq.shape, 0.5), where=pq > 0)
        auc[(nan > 0) & (pq > 0)] = np.nan
        return _result(auc if self.average in (None, "none") else auc.mean(), self.device)

    def reset(self) -> "MulticlassAUROC":
        self.inputs, self.targets = [], []
        return self

    def merge_state(self, metrics: Iterable["MulticlassAUROC"]) -> "MulticlassAUROC":
        for m in metrics:
            if m.num_classes != self.num_classes:
                raise ValueError(f"cannot merge AUROC states of {m.num_classes} and {self.num_classes} classes")
            self.inputs.extend(t.to(self.device) for t in m.inputs)
            self.targets.extend(t.to(self.device) for t in m.targets)
        return self


def _gather_var(t: torch.Tensor, group, via_host: bool) -> List[torch.Tensor]:
    """all_gather of tensors whose first dim differs by rank: a size exchange, then a gather padded to the largest."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    dev = torch.device("cpu") if via_host else t.device
    n = torch.tensor([t.shape[0]], dtype=torch.int64, device=dev)
    sizes = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(sizes, n, group=group)
    sizes = [int(s) for s in sizes]
    pad = torch.zeros((max(sizes),) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
    pad[:t.shape[0]] = t.to(dev)
    outs = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(outs, pad, group=group)
    return [o[:s].to(t.device) for o, s in zip(outs, sizes)]


def sync_and_compute(metric, process_group=None):
    """torcheval.metrics.toolkit.sync_and_compute: merge the metric's state over the ranks of `process_group` (torch.distributed)
    and compute it on every rank.  The caller's metric is left as it was.  On a gloo group the state goes through the host.
    Also takes a `retrieval.CrossModalRetrieval` (both embedding sets, and the group ids if it has them, are gathered; the result is
    its OrderedDict)."""
    import copy

    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(process_group) == 1:
        return metric.compute()
    via_host = dist.get_backend(process_group) == "gloo"
    merged = copy.copy(metric)
    if isinstance(metric, MulticlassF1Score):
        if metric.conf is None:
            if metric.num_classes is None:
                raise ValueError("sync_and_compute: an F1 metric without num_classes needs an update() on every rank")
            merged._state(metric.num_classes)
        state = torch.cat((merged.bad, merged.conf.reshape(-1)))
        state = state.cpu() if via_host else state.clone()
        dist.all_reduce(state, group=process_group)
        state = state.to(metric.device)
        merged.bad, merged.conf = state[:1].clone(), state[1:].reshape(merged.conf.shape).clone()
        return merged.compute()
    if isinstance(metric, MulticlassAUROC):
        C = metric.num_classes
        x = torch.cat(metric.inputs) if metric.inputs else torch.empty((0, C), dtype=torch.float32, device=metric.device)
        y = torch.cat(metric.targets) if metric.targets else torch.empty((0,), dtype=torch.int64, device=metric.device)
        merged.inputs = _gather_var(x, process_group, via_host)
        merged.targets = _gather_var(y, process_group, via_host)
        return merged.compute()
    from .retrieval import CrossModalRetrieval
    if isinstance(metric, CrossModalRetrieval):
        # every rank ranks over the UNION: the gallery size is part of the metric, so per-rank values averaged afterwards would be
        # another (easier) metric.  A rank without samples learns the width from the others.
        # The same for the group ids: a rank with samples either has them or not, and all such ranks must agree.
        D = torch.tensor([metric.wsi[0].shape[1] if metric.wsi else 0, int(bool(metric.group)), int(bool(metric.wsi) and not metric.group)],
                         dtype=torch.int64, device="cpu" if via_host else metric.device)
        dist.all_reduce(D, op=dist.ReduceOp.MAX, group=process_group)
        D, grouped, plain = (int(v) for v in D.cpu())
        if grouped and plain:
            raise ValueError("sync_and_compute: some ranks fed the retrieval metric group ids and others did not")
        empty = torch.empty((0, D), dtype=torch.float32, device=metric.device)
        w, r = metric._cat() if metric.wsi else (empty, empty)
        merged.wsi = [t for t in _gather_var(w, process_group, via_host) if t.shape[0]]
        merged.rna = [t for t in _gather_var(r, process_group, via_host) if t.shape[0]]
        merged.group = []
        if grouped:       # ids mean the same on every rank: a sample whose slides sit on different ranks is one group of the union
            g = torch.cat(metric.group) if metric.group else torch.empty((0,), dtype=torch.int64, device=metric.device)
            merged.group = [t for t in _gather_var(g, process_group, via_host) if t.shape[0]]
        return merged.compute()
    raise TypeError(f"sync_and_compute: unsupported metric {type(metric).__name__}")


def accuracy(output: torch.Tensor, target: torch.Tensor, topk: Sequence[int] = (1,)) -> List[torch.Tensor]:
    """timm.utils.accuracy for topk=(1,): [100 * (rows whose first argmax equals the label) / N] as a 0-d f32 device tensor, no
    host sync.  Labels outside [0, C) count as wrong, as in timm.  Other `topk` raise NotImplementedError."""
    if tuple(topk) != (1,):
        raise NotImplementedError(f"accuracy: only topk=(1,) is built, got {tuple(topk)}")
    if output.dim() != 2:
        raise ValueError(f"output must be [N, C], got {tuple(output.shape)}")
    N, C = output.shape
    target = _labels(target, N)
    K._chk(output)
    conf = torch.zeros((C, C), dtype=torch.int64, device=output.device)
    bad = torch.zeros((1,), dtype=torch.int64, device=output.device)
    K.cls_confusion(output.detach().float(), target, conf, bad)
    return [conf.diagonal().sum().float() * 100.0 / N]
