"""Cluster probe of frozen embeddings: the label-free figure of a pre-trained encoder.

Every other probe of this package (`retrieval`, `knn`, `fewshot`, `survival`) has labels in the loop.  This one asks whether the slide
embeddings fall into the cohort's subtypes on their own: k-means (Lloyd's iteration) on the frozen embeddings, R restarts at once,
scored against the subtype labels with NMI, ARI and purity.

    y        = the prepared rows (see ClusterProbe: centred and / or normalised, or as they are)
    assign   = argmax_k  y . c[r,k] - |c[r,k]|^2 / 2   ("euclidean": the nearest centroid)   or   argmax_k y . c[r,k]   ("cosine")
    c[r,k]   = the mean of the rows assigned to k, summed in row order in f64   ("cosine": normalised again; empty: unchanged)

until no row of any restart changes its cluster.  The assignment is `mh_kmeans_assign` (the retrieval kernels' exact-f32 tile product
with a running argmax over the key tiles as epilogue: no [R, n, K] scores in memory), the update `mh_kmeans_update` (deterministic: no
float atomics, the same assignment gives the same centroids bit for bit, so a converged restart is a fixed point and running it further
is harmless), the inertia `mh_kmeans_inertia`, the contingency counts and the three scores `mh_kmeans_tally`.  Nothing waits on the
host inside an iteration: the per-iteration change counts go to an int32 [max_iter, R] table that is read back every 8 iterations.
A restart without explicit start begins at K distinct rows drawn by `mh_sample_rows` (the Philox stream of the data feed: the pool is
one "slide" of n rows, restart r uses draw id offset + r), gathered by `mh_gather_rows`; with `seeding="kmeans++"` the start is
`mh_kmeanspp_init` on the prepared rows instead: plain k-means++ (Arthur and Vassilvitskii: D^2 sampling, one draw per centre, NOT
sklearn's greedy variant with local trials), every restart at once, draw id offset + r of the same stream under kind 2.

Beside NMI, ARI and purity: `evaluate(..., matched=True)` adds the accuracy under the best one-to-one matching of clusters to classes
(`mh_cluster_match` on the contingency counts: the Hungarian assignment, exact in integers), and `silhouette()` /
`evaluate(..., silhouette=True)` the one figure that needs no labels (`mh_silhouette`: the same tile product over all pairs of rows
with an f64 distance-sum epilogue, no [n, n] matrix; `silhouette_score` is the same for labels from elsewhere).

Not built: relocating empty clusters (an empty cluster keeps its centroid; `cluster_empty` reports them), bf16 embeddings, a pool
gathered over DDP ranks.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import torch

from . import kernels as K
from ._lib import MirrorHipError

__all__ = ["ClusterProbe", "silhouette_score"]

_CHECK_EVERY = 8          # iterations between two read-backs of the change table
_SEEDING = ("random", "kmeans++")


def _int_in(v, lo: int, hi: int, what: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not (lo <= v <= hi):
        raise ValueError(f"{what} must be an int in [{lo}, {hi}], got {v!r}")
    return v


class ClusterProbe:
    """`fit(emb, init=None)` clusters the rows; `predict(emb)` assigns new rows under the best restart, `assign(emb, centroids)` under
    explicit centroids f32 [R', K, D] (int32 [R', n']); `evaluate(labels, num_classes)` scores the fitted clusters against labels.

    The preparation of the rows (the pool's, and every later query's with the POOL's mean):

        center=True,  either metric     y = (x - mu) / max(|x - mu|, 1e-12), mu the pool's column mean     (mh_colmean, mh_center_l2norm)
        center=False, "cosine"          y = x / max(|x|, 1e-12)                                            (mh_center_l2norm with mu = 0)
        center=False, "euclidean"       y = x, the rows as they are

    After `fit`, on the device: `centroids_` f32 [R, K, D] (in the prepared space), `assign_` int32 [R, n], `inertia_` f64 [R]
    (sum of squared distances of the prepared rows to their centroids, also for "cosine"), `counts_` int32 [R, K], `n_iter_` int64 [R]
    (the assignment steps up to and including the first that changed nothing; max_iter when there was none), `best_` (a 0-d int64
    tensor: the restart of least inertia, ties to the smaller index), `labels_` = `assign_[best_]`, `changed_` (the int32 table) and,
    for a drawn start, `init_rows_` int64 [R, K].  `fit` waits on the host once per 8 iterations, for the change table alone.

    seeding: "random" (K distinct rows drawn uniformly, the default) or "kmeans++" (mh_kmeanspp_init on the prepared rows: Euclidean
    D^2 sampling in the prepared space for both metrics); either sets `init_rows_`, neither is used when `init=` is given.

    init: an f32 [R', K, D] tensor of starting centroids in the prepared space (R' replaces `restarts`), or None for the draw, which
    needs K <= n.  After `evaluate`: `per_restart` f64 [R, 3] (NMI, ARI, purity), `contingency` int32 [R, K, C] ([cluster, label])
    and `bad` int32 [R] (rows with a label outside [0, C) or without a cluster) stay on the device; with `matched=True` also `match_`
    int32 [R, K] (the class every cluster is matched to, or -1) and `hits_` int64 [R]."""

    def __init__(self, num_clusters: int, restarts: int = 16, max_iter: int = 100, metric: str = "cosine", center: bool = True,
                 seed: int = 0, offset: int = 0, device=None, seeding: str = "random"):
        _int_in(num_clusters, 1, 1024, "num_clusters")
        _int_in(restarts, 1, min(65535, (1 << 20) // num_clusters), f"restarts (restarts x {num_clusters} centroids <= 2^20)")
        _int_in(max_iter, 1, 1 << 16, "max_iter")
        if metric not in K.KMEANS_METRIC:
            raise ValueError(f'metric must be "cosine" or "euclidean", got {metric!r}')
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed must be an int, got {seed!r}")
        _int_in(offset, 0, (1 << 62), "offset")
        if seeding not in _SEEDING:
            raise ValueError(f'seeding must be "random" or "kmeans++", got {seeding!r}')
        d = torch.device("cuda") if device is None else torch.device(device)
        if d.type != "cuda":
            raise MirrorHipError(f"mirror_amd metrics keep their state on a HIP device, got {d}")
        self.num_clusters = num_clusters
        self.restarts = restarts
        self.max_iter = max_iter
        self.metric = metric
        self.center = bool(center)
        self.seed = seed
        self.offset = offset
        self.seeding = seeding
        self.device = d
        self._clear()

    def _clear(self) -> None:
        self.mu_ = self._y = None
        self.centroids_ = self.bias_ = self.assign_ = self.inertia_ = self.counts_ = self.n_iter_ = self.best_ = self.labels_ = None
        self.changed_ = self.init_rows_ = None
        self.per_restart = self.contingency = self.bad = self.match_ = self.hits_ = None

    # ------------------------------------------------------------------ preparation
    def _rows(self, emb, what: str, D: Optional[int] = None) -> torch.Tensor:
        ok = isinstance(emb, torch.Tensor) and emb.dim() == 2 and emb.is_floating_point() and (D is None or emb.shape[1] == D)
        if not ok:
            got = f"{emb.dtype} {tuple(emb.shape)}" if isinstance(emb, torch.Tensor) else type(emb).__name__
            raise ValueError(f"{what} must be floating point [n, {'D' if D is None else D}], got {got}")
        n, d = emb.shape
        if not (1 <= n <= (1 << 20)) or not (1 <= d <= 4096):
            raise MirrorHipError(f"{what}: n = {n} (1..2^20), D = {d} (1..4096)")
        return emb

    def _prepare(self, x: torch.Tensor) -> torch.Tensor:
        if self.center:
            return K.center_l2norm(x, self.mu_)
        if self.metric == "cosine":
            return K.center_l2norm(x, torch.zeros((x.shape[1],), device=self.device, dtype=torch.float32))
        return x

    def _centroids(self, cent, D: int, what: str) -> torch.Tensor:
        Kk = self.num_clusters
        if not isinstance(cent, torch.Tensor) or cent.dtype != torch.float32 or cent.dim() != 3 or tuple(cent.shape[1:]) != (Kk, D):
            got = f"{cent.dtype} {tuple(cent.shape)}" if isinstance(cent, torch.Tensor) else type(cent).__name__
            raise ValueError(f"{what} must be an f32 [R, {Kk}, {D}] tensor of centroids in the prepared space, got {got}")
        R = cent.shape[0]
        if not (1 <= R <= 65535) or R * Kk > (1 << 20):
            raise MirrorHipError(f"{what}: R = {R} restarts of {Kk} centroids (1..65535, R * K <= 2^20)")
        return cent

    # ------------------------------------------------------------------ fit
    def fit(self, emb: torch.Tensor, init: Optional[torch.Tensor] = None) -> "ClusterProbe":
        self._rows(emb, "emb")
        n, D = emb.shape
        Kk = self.num_clusters
        if init is not None:
            self._centroids(init, D, "init")
        elif Kk > n:
            raise ValueError(f"ClusterProbe: {Kk} distinct starting rows cannot be drawn from {n} rows (num_clusters <= n, or pass init=)")
        self._clear()
        x = emb.detach().to(device=self.device, dtype=torch.float32, non_blocking=True, copy=True).contiguous()
        self.mu_ = K.colmean(x) if self.center else None
        y = self._y = self._prepare(x)
        if init is None and self.seeding == "kmeans++":
            R = self.restarts
            self.init_rows_, cent = K.kmeanspp_init(y, R, Kk, self.seed, self.offset)
        elif init is None:
            R = self.restarts
            slots = torch.zeros((R,), device=self.device, dtype=torch.int64)          # every restart draws from the one "slide"
            lengths = torch.full((1,), n, device=self.device, dtype=torch.int64)
            starts = torch.zeros((1,), device=self.device, dtype=torch.int64)
            self.init_rows_ = K.sample_rows(slots, lengths, starts, Kk, self.seed, self.offset)
            cent = K.gather_rows(y, self.init_rows_)
        else:
            cent = init.detach().to(device=self.device, non_blocking=True, copy=True).contiguous()
            R = cent.shape[0]
        euclid = self.metric == "euclidean"
        bias = K.kmeans_bias(cent) if euclid else None
        assign = torch.full((R, n), -1, device=self.device, dtype=torch.int32)
        counts = torch.empty((R, Kk), device=self.device, dtype=torch.int32)
        changed = torch.zeros((self.max_iter, R), device=self.device, dtype=torch.int32)
        done = 0
        for it in range(self.max_iter):
            K.kmeans_assign(y, cent, bias, prev=assign, changed=changed[it], out=assign)
            K.kmeans_update(y, assign, cent, bias, self.metric, count=counts)
            done = it + 1
            if done % _CHECK_EVERY == 0 and done < self.max_iter:
                if bool((changed[done - _CHECK_EVERY:done] == 0).all(1).any()):      # the one host wait of these iterations
                    break
        table = changed[:done]
        still = table != 0
        first = torch.argmax((~still).to(torch.int8), dim=0) + 1                      # the first step without a change
        self.n_iter_ = torch.where((~still).any(0), first, torch.full_like(first, self.max_iter))
        self.changed_ = table
        self.centroids_, self.bias_, self.assign_, self.counts_ = cent, bias, assign, counts
        self.inertia_ = K.kmeans_inertia(y, cent, assign)
        self.best_ = torch.argmin(self.inertia_)
        self.labels_ = assign.index_select(0, self.best_.view(1))[0]
        return self

    def _fitted(self) -> None:
        if self.centroids_ is None:
            raise ValueError("ClusterProbe: nothing is fitted (call fit() first)")

    # ------------------------------------------------------------------ assignment of further rows
    def assign(self, emb: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
        """int32 [R', n'] on the device: the rows of emb, prepared as the pool was, under explicit centroids f32 [R', K, D]."""
        self._fitted()
        D = self.centroids_.shape[2]
        self._rows(emb, "emb", D)
        self._centroids(centroids, D, "centroids")
        q = self._prepare(emb.detach().to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous())
        cent = centroids.detach().to(device=self.device, non_blocking=True).contiguous()
        bias = K.kmeans_bias(cent) if self.metric == "euclidean" else None
        return K.kmeans_assign(q, cent, bias)[0]

    def predict(self, emb: torch.Tensor) -> torch.Tensor:
        """int32 [n'] on the device: the clusters of the best restart, no host wait."""
        self._fitted()
        return self.assign(emb, self.centroids_.index_select(0, self.best_.view(1)))[0]

    def silhouette(self, restarts: str = "best", samples: bool = False):
        """The silhouette of the fitted clusters over the prepared rows under the probe's metric, on the device, no host wait:
        restarts="best" scores `labels_` (a 0-d f64 tensor), "all" every restart (f64 [R]).  samples=True returns (mean, per-row values)
        instead: f64 [n], or [R, n] for "all"."""
        self._fitted()
        if restarts not in ("best", "all"):
            raise ValueError(f'restarts must be "best" or "all", got {restarts!r}')
        lab = self.assign_ if restarts == "all" else self.labels_.view(1, -1)
        mean, _, sil = K.silhouette(self._y, lab, self.num_clusters, self.metric, samples=bool(samples))
        if restarts == "best":
            mean, sil = mean[0], (None if sil is None else sil[0])
        return (mean, sil) if samples else mean

    # ------------------------------------------------------------------ scores
    def evaluate(self, labels: torch.Tensor, num_classes: int, matched: bool = False, silhouette: bool = False):
        """The fitted clusters against labels (integer [n], the pool's rows in order): an OrderedDict of `cluster_nmi` (arithmetic
        normalisation, natural log), `cluster_ari`, `cluster_purity` of the best restart, each with `_mean` and `_std` (sample standard
        deviation, 0 for one restart) over the restarts, then `cluster_inertia`, `cluster_empty` (the empty clusters of the best
        restart), `cluster_k`, `cluster_restarts` and `cluster_n`.  matched=True appends `cluster_acc`, `cluster_acc_mean`,
        `cluster_acc_std` (per cent of the tallied rows that fall into the class their cluster is matched to, under the best one-to-one
        matching; NaN when no row is tallied) and `match_` (int32 [R, K], on the device); silhouette=True appends `cluster_silhouette`
        (the best restart's).  One host copy either way."""
        self._fitted()
        R, n = self.assign_.shape
        if not isinstance(labels, torch.Tensor) or labels.dim() != 1 or labels.numel() != n or labels.dtype not in (torch.int32, torch.int64):
            got = f"{labels.dtype} {tuple(labels.shape)}" if isinstance(labels, torch.Tensor) else type(labels).__name__
            raise ValueError(f"labels must be an int32 / int64 [{n}] tensor, got {got}")
        _int_in(num_classes, 1, 1024, "num_classes")
        for v, name in ((matched, "matched"), (silhouette, "silhouette")):
            if not isinstance(v, bool):
                raise ValueError(f"{name} must be a bool, got {v!r}")
        if num_classes * self.num_clusters > 65536:
            raise MirrorHipError(f"ClusterProbe: {self.num_clusters} clusters x {num_classes} classes = "
                                 f"{num_classes * self.num_clusters} contingency cells, 65536 at the most")
        labels = labels.detach().to(device=self.device, dtype=torch.int64, non_blocking=True)
        self.contingency, self.bad, self.per_restart = K.kmeans_tally(self.assign_, labels, self.num_clusters, num_classes)
        best = self.best_.view(1)
        parts = [self.per_restart.reshape(-1), best.double(), self.inertia_.index_select(0, best),
                 (self.counts_.index_select(0, best) == 0).sum().double().view(1)]
        self.match_ = self.hits_ = None
        if matched:
            self.match_, self.hits_ = K.cluster_match(self.contingency)
            parts += [self.hits_.double(), self.bad.double()]                  # counts <= 2^20: exact in f64
        if silhouette:
            parts.append(self.silhouette().view(1))
        flat = torch.cat(parts).cpu()                                         # the one host wait
        table, best = flat[:3 * R].view(R, 3), int(flat[3 * R])
        out: "OrderedDict[str, float]" = OrderedDict()
        for j, name in enumerate(("cluster_nmi", "cluster_ari", "cluster_purity")):
            col = table[:, j]
            out[name] = float(col[best])
            out[name + "_mean"] = float(col.mean())
            out[name + "_std"] = float(col.std(unbiased=True)) if R > 1 else 0.0
        out["cluster_inertia"] = float(flat[3 * R + 1])
        out["cluster_empty"] = int(flat[3 * R + 2])
        out["cluster_k"] = self.num_clusters
        out["cluster_restarts"] = R
        out["cluster_n"] = n
        at = 3 * R + 3
        if matched:
            acc = 100.0 * flat[at:at + R] / (n - flat[at + R:at + 2 * R])      # 0 / 0 = NaN: no row was tallied
            out["cluster_acc"] = float(acc[best])
            out["cluster_acc_mean"] = float(acc.mean())
            out["cluster_acc_std"] = float(acc.std(unbiased=True)) if R > 1 else 0.0
            out["match_"] = self.match_
            at += 2 * R
        if silhouette:
            out["cluster_silhouette"] = float(flat[at])
        return out


def silhouette_score(emb: torch.Tensor, labels: torch.Tensor, num_clusters: int, metric: str = "cosine", center: bool = False,
                     samples: bool = False, device=None):
    """The silhouette of labels that did not come from a probe: emb floating point [n, D], labels integer [n] or [R, n] (cluster ids in
    [0, num_clusters); a row outside takes no part and has sample NaN).  The rows are prepared as ClusterProbe prepares them
    (center=False: "euclidean" as they are, "cosine" normalised, which is sklearn's silhouette_score with that metric).  Returns device
    tensors without a host wait: the mean (0-d f64, or [R]), and with samples=True (mean, per-row values f64 [n] or [R, n])."""
    if isinstance(num_clusters, bool) or not isinstance(num_clusters, int):
        raise ValueError(f"num_clusters must be an int in [1, 1024], got {num_clusters!r}")
    p = ClusterProbe(num_clusters, restarts=1, metric=metric, center=center, device=device)
    p._rows(emb, "emb")
    n = emb.shape[0]
    if (not isinstance(labels, torch.Tensor) or labels.dtype not in (torch.int32, torch.int64) or labels.dim() not in (1, 2)
            or labels.shape[-1] != n):
        got = f"{labels.dtype} {tuple(labels.shape)}" if isinstance(labels, torch.Tensor) else type(labels).__name__
        raise ValueError(f"labels must be an int32 / int64 [{n}] or [R, {n}] tensor, got {got}")
    x = emb.detach().to(device=p.device, dtype=torch.float32, non_blocking=True).contiguous()
    p.mu_ = K.colmean(x) if p.center else None
    y = p._prepare(x)
    lab = labels.detach().to(device=p.device, non_blocking=True)
    if lab.dtype == torch.int64:
        lab = lab.clamp(-1, num_clusters).to(torch.int32)                     # outside stays outside
    mean, _, sil = K.silhouette(y, lab.view(-1, n).contiguous(), num_clusters, metric, samples=bool(samples))
    if labels.dim() == 1:
        mean, sil = mean[0], (None if sil is None else sil[0])
    return (mean, sil) if samples else mean
