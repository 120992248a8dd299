"""Few-shot prototype probe of frozen embeddings: the training-free few-shot figure of a pre-trained encoder.

The reference's few-shot protocol (tools/gen_few_shot_files.py, tools/downstream_tasks_evaluator.py) takes `shots` training slides per
class, drawn with random.choices, as support and the fold's validation slides as queries; it draws ONE support set per fold and
fine-tunes on it.  This probe keeps the protocol and replaces the fine-tune by SimpleShot's nearest-centroid classifier (Wang et al.
2019), over many support draws ("episodes") at once, reported as mean, standard deviation and 95 % interval over the episodes:

    y      = (x - mu) / max(|x - mu|, 1e-12)       mu: the column mean of the labelled pool (center=False: only the normalisation)
    p[e,c] = mean over the K support rows of class c in episode e of y          ("cosine": normalised again)
    pred   = argmax_c  q . p[e,c] - |p[e,c]|^2 / 2   ("euclidean": the nearest prototype)   or   argmax_c q . p[e,c]   ("cosine")

The draw is `mh_sample_rows` over the class-sorted pool (class c is "slide" c; slot e C + c draws K rows with draw id offset + e C + c:
without replacement when the class has >= K members, with replacement below, which is random.choices).  It is the Philox stream of the
data feed's token draws: under an equal seed and overlapping draw ids the two draw the same words, so give the probe its own seed.
The prototypes of all episodes are the keys of `mh_fewshot_predict` (the retrieval kernels' exact-f32 tile product with a per-episode
argmax as epilogue: no [E, nq, C] scores in memory), the per-episode confusion counts and summaries come from `mh_fewshot_tally`; the
host is first waited for when `evaluate` reads the [E, 3] table back (`draw` reads the C class counts once per fitted pool).

Not built: patient-group exclusion, bf16 embeddings, C > 64, a pool gathered over DDP ranks (`merge_state` merges states the caller has
gathered), transductive variants.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Iterable, List, Optional

import torch

from . import kernels as K
from ._lib import MirrorHipError
from .knn import _ids
from .retrieval import _l2

__all__ = ["FewShotProbe"]


def _int_in(v, lo: int, hi: int, what: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not (lo <= v <= hi):
        raise ValueError(f"{what} must be an int in [{lo}, {hi}], got {v!r}")
    return v


class FewShotProbe:
    """`fit(emb, labels)` adds rows to the labelled pool the supports are drawn from (f32 copies on the device, no host wait; calls
    concatenate); `draw()` returns the support rows int64 [E, C, K] of the pool; `predict(query_emb, support=None)` the classes
    int32 [E, nq] (-1: no class eligible), both on the device; `evaluate(query_emb, query_labels, support=None)` an OrderedDict of
    `fewshot_acc`, `fewshot_bacc` (percent, as `metrics.accuracy`) and `fewshot_f1` (macro, in [0, 1]), each with `_std` (sample standard
    deviation over the episodes, 0 for one episode) and `_ci95` (1.96 std / sqrt(E)), then `fewshot_shots`, `fewshot_episodes` and
    `fewshot_n` (the pool size).  `run(...)` is evaluate without the read-back: every launch queued, nothing waits on the host, so it can
    be captured in a graph once the pool's class table exists (after one eager call).  After either, `per_episode` (f64 [E, 3]:
    accuracy, balanced accuracy, macro F1), `confusion` (int32 [E, C, C], [label, prediction]), `bad` (int32 [E]: rows with a label
    outside [0, C) or without a prediction) and `pred` stay on the device.

    support: an explicit int64 [E', C, K'] tensor of pool rows instead of the draw, e.g. E' = 1 with the rows of a reference split file;
    an entry outside the pool makes that prototype NaN, and a NaN prototype is never predicted."""

    def __init__(self, num_classes: int, shots: int = 10, episodes: int = 1000, center: bool = True, metric: str = "euclidean",
                 seed: int = 0, offset: int = 0, device=None):
        _int_in(num_classes, 2, 64, "num_classes")
        _int_in(shots, 1, 1024, "shots")
        _int_in(episodes, 1, (1 << 20) // K.fewshot_cp(num_classes), f"episodes (episodes x {K.fewshot_cp(num_classes)} key slots <= 2^20)")
        if metric not in K.FEWSHOT_METRIC:
            raise ValueError(f'metric must be "euclidean" or "cosine", got {metric!r}')
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed must be an int, got {seed!r}")
        _int_in(offset, 0, (1 << 62), "offset")
        d = torch.device("cuda") if device is None else torch.device(device)
        if d.type != "cuda":
            raise MirrorHipError(f"mirror_amd metrics keep their state on a HIP device, got {d}")
        self.num_classes = num_classes
        self.shots = shots
        self.episodes = episodes
        self.center = bool(center)
        self.metric = metric
        self.seed = seed
        self.offset = offset
        self.device = d
        self.emb: List[torch.Tensor] = []             # f32 [n_i, D] per fit
        self.labels: List[torch.Tensor] = []          # int64 [n_i]
        self._prep = None                             # what the pool gives every call: built once per pool
        self.pred = self.per_episode = self.confusion = self.bad = None

    # ------------------------------------------------------------------ the pool
    def fit(self, emb: torch.Tensor, labels: torch.Tensor) -> "FewShotProbe":
        """emb: embeddings [n, D]; labels: integer [n] in [0, num_classes) (not checked here: that would wait on the host; a row with a
        label outside belongs to no class and is never drawn, but counts in the pool's mean)."""
        if not isinstance(emb, torch.Tensor) or emb.dim() != 2 or not emb.is_floating_point():
            got = f"{emb.dtype} {tuple(emb.shape)}" if isinstance(emb, torch.Tensor) else type(emb).__name__
            raise ValueError(f"emb must be floating point [n, D], got {got}")
        _ids(labels, emb.shape[0], "labels")
        if self.emb and self.emb[0].shape[1] != emb.shape[1]:
            raise ValueError(f"embedding width changed from {self.emb[0].shape[1]} to {emb.shape[1]}")
        self.emb.append(emb.detach().to(device=self.device, dtype=torch.float32, non_blocking=True, copy=True))
        self.labels.append(labels.detach().to(device=self.device, dtype=torch.int64, non_blocking=True, copy=True))
        self._prep = None
        return self

    def _pool(self) -> dict:
        """The prepared pool: its rows y, the mean mu, and the class-sorted permutation with the tables mh_sample_rows reads.  The class
        counts are read back here (the one host wait before evaluate's): an empty class cannot be drawn from."""
        if self._prep is not None:
            return self._prep
        n = sum(t.shape[0] for t in self.emb)
        if n == 0:
            raise ValueError("FewShotProbe: the pool is empty (call fit() first)")
        cat = lambda ts: ts[0] if len(ts) == 1 else torch.cat(ts)      # noqa: E731
        x, labels = cat(self.emb), cat(self.labels)
        C = self.num_classes
        key = torch.where((labels >= 0) & (labels < C), labels, torch.full_like(labels, C))
        perm = torch.sort(key, stable=True)[1].contiguous()            # class c is the run of its rows, in pool order
        counts = torch.bincount(key, minlength=C + 1)[:C].contiguous()
        starts = (torch.cumsum(counts, 0) - counts).contiguous()
        if self.center:
            mu = K.colmean(x)
            y = K.center_l2norm(x, mu)
        else:
            mu, y = None, _l2(x)
        slots = (torch.arange(self.episodes * C, device=self.device, dtype=torch.int64) % C).contiguous()
        host = counts.cpu()
        empty = [c for c in range(C) if int(host[c]) == 0]
        if empty:
            raise ValueError(f"FewShotProbe: the pool has no row of class(es) {empty}: nothing to draw a support from")
        self._prep = dict(n=n, D=x.shape[1], y=y, mu=mu, perm=perm, counts=counts, starts=starts, slots=slots)
        return self._prep

    # ------------------------------------------------------------------ the draw
    def _draw_sorted(self, P: dict) -> torch.Tensor:
        rows = K.sample_rows(P["slots"], P["counts"], P["starts"], self.shots, self.seed, self.offset)
        return rows.view(self.episodes, self.num_classes, self.shots)

    def draw(self) -> torch.Tensor:
        """int64 [E, C, K] on the device: the support rows of the pool.  The same (seed, offset) gives the same tensor; slot e C + c uses
        draw id offset + e C + c of the data feed's token stream (tests/datafeed_ref.py restates it)."""
        P = self._pool()
        return P["perm"][self._draw_sorted(P)]

    # ------------------------------------------------------------------ prediction
    def _query(self, query_emb: torch.Tensor, P: dict) -> torch.Tensor:
        D = P["D"]
        if not isinstance(query_emb, torch.Tensor) or query_emb.dim() != 2 or not query_emb.is_floating_point() or query_emb.shape[1] != D:
            got = f"{query_emb.dtype} {tuple(query_emb.shape)}" if isinstance(query_emb, torch.Tensor) else type(query_emb).__name__
            raise ValueError(f"query_emb must be floating point [nq, {D}], got {got}")
        if not (1 <= query_emb.shape[0] <= (1 << 20)):
            raise ValueError(f"query_emb must have 1 .. 2^20 rows, got {query_emb.shape[0]}")
        q = query_emb.detach().to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous()
        return K.center_l2norm(q, P["mu"]) if self.center else _l2(q)

    def _support(self, support) -> torch.Tensor:
        C = self.num_classes
        if (not isinstance(support, torch.Tensor) or support.dtype != torch.int64 or support.dim() != 3 or support.shape[1] != C
                or not (1 <= support.shape[2] <= 1024) or support.shape[0] < 1 or support.shape[0] * K.fewshot_cp(C) > (1 << 20)):
            got = f"{support.dtype} {tuple(support.shape)}" if isinstance(support, torch.Tensor) else type(support).__name__
            raise ValueError(f"support must be an int64 [E, {C}, K] tensor of pool rows (1 <= K <= 1024), got {got}")
        return support.to(device=self.device, non_blocking=True).contiguous()

    def prototypes(self, support: Optional[torch.Tensor] = None):
        """(protos f32 [E, Cp, D], bias f32 [E, Cp] or None for "cosine") of the draw, or of an explicit support."""
        P = self._pool()
        if support is None:
            return K.fewshot_protos(P["y"], self._draw_sorted(P), P["perm"], self.metric)
        return K.fewshot_protos(P["y"], self._support(support), None, self.metric)

    def predict(self, query_emb: torch.Tensor, support: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int32 [E, nq] on the device, no host wait once the pool is prepared."""
        P = self._pool()
        if support is not None:
            support = self._support(support)                            # before anything is launched
        q = self._query(query_emb, P)
        protos, bias = self.prototypes(support)
        self.pred = K.fewshot_predict(q, protos, bias, self.num_classes)
        return self.pred

    def run(self, query_emb: torch.Tensor, query_labels: torch.Tensor, support: Optional[torch.Tensor] = None) -> torch.Tensor:
        """evaluate without its read-back: returns `per_episode` f64 [E, 3] on the device."""
        if not isinstance(query_emb, torch.Tensor) or query_emb.dim() != 2:
            raise ValueError("query_emb must be [nq, D]")
        _ids(query_labels, query_emb.shape[0], "query_labels")
        self._pool()                                                    # an empty pool is refused before anything goes to the device
        labels = query_labels.to(device=self.device, dtype=torch.int64, non_blocking=True)
        pred = self.predict(query_emb, support)
        self.confusion, self.bad, self.per_episode = K.fewshot_tally(pred, labels, self.num_classes)
        return self.per_episode

    def evaluate(self, query_emb: torch.Tensor, query_labels: torch.Tensor, support: Optional[torch.Tensor] = None):
        """The metrics of the episodes on labelled queries (a validation split against supports from the training pool)."""
        table = self.run(query_emb, query_labels, support).cpu()        # the first host wait
        E = table.shape[0]
        out: "OrderedDict[str, float]" = OrderedDict()
        for j, name in enumerate(("fewshot_acc", "fewshot_bacc", "fewshot_f1")):
            col = table[:, j]
            std = float(col.std(unbiased=True)) if E > 1 else 0.0
            out[name] = float(col.mean())
            out[name + "_std"] = std
            out[name + "_ci95"] = 1.96 * std / math.sqrt(E)
        out["fewshot_shots"] = self.shots if support is None else int(support.shape[2])
        out["fewshot_episodes"] = E
        out["fewshot_n"] = self._pool()["n"]
        return out

    # ------------------------------------------------------------------ state
    def reset(self) -> "FewShotProbe":
        self.emb, self.labels, self._prep = [], [], None
        self.pred = self.per_episode = self.confusion = self.bad = None
        return self

    def merge_state(self, probes: Iterable["FewShotProbe"]) -> "FewShotProbe":
        for m in probes:
            if m.emb and self.emb and m.emb[0].shape[1] != self.emb[0].shape[1]:
                raise ValueError(f"cannot merge few-shot pools of widths {m.emb[0].shape[1]} and {self.emb[0].shape[1]}")
            self.emb.extend(t.to(self.device) for t in m.emb)
            self.labels.extend(t.to(self.device) for t in m.labels)
        self._prep = None
        return self
