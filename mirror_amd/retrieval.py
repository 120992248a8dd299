"""Zero-shot cross-modal retrieval of the alignment heads: for each slide, where its own RNA profile ranks among all validation
profiles, and the reverse (recall@1/5/10, median and mean rank).  Unlike the alignment loss these do not depend on `logit_scale`
(positive, so irrelevant to ranks), the batch size, the world size or `gather_distributed`: only on the gallery.

The ranks come from `mh_retrieval_ranks` (csrc/retrieval.hip): a fused exact-f32 MFMA product with a comparing epilogue, so the
[n, n] similarity matrix never exists.  The rule is pessimistic: a key that ties with the positive, or a NaN on either side,
counts against the query, so a collapsed encoder scores rank n everywhere, never rank 1.

Several positives per query (`mh_retrieval_ranks_grouped`): the pretraining set has one item per SLIDE and looks its RNA row up by the
sample barcode, so a sample with three slides is in a validation set three times with the same RNA vector.  Given a group id per
pair (the sample's row in the RNA table), a query's positives are all keys of its group and its rank is that of the best of them
among the keys of other groups; the slide -> RNA gallery is the distinct samples, and RNA -> slide counts each sample once.

The neighbours themselves (`mh_retrieval_topk`, csrc/retrieval_topk.hip): the same product with a selecting epilogue, for qualitative
review, hard-negative mining and the kNN probe of `mirror_amd.knn`; `retrieval_topk` below and `CrossModalRetrieval.topk`.

Not built: bf16 keys, both directions from one pass over the similarities, more than 64 neighbours.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import kernels as K
from ._lib import MirrorHipError

__all__ = ["retrieval_ranks", "retrieval_topk", "summarize_ranks", "first_of_group", "CrossModalRetrieval"]


def _l2(x: torch.Tensor) -> torch.Tensor:
    """Rows scaled to unit length by mh_l2norm_fwd (F.normalize's eps), as InfoNCE normalises its operands."""
    x = x.detach().contiguous()
    rows, D = x.shape
    y, _ = K.l2norm_fwd(x, rows, D, D, 1e-12, torch.float32)
    return y


def retrieval_ranks(query: torch.Tensor, key: torch.Tensor, target: Optional[torch.Tensor] = None,
                    query_group: Optional[torch.Tensor] = None, key_group: Optional[torch.Tensor] = None,
                    key_count: Optional[torch.Tensor] = None, normalize: bool = False) -> torch.Tensor:
    """int32 [nq] on the device, no host sync: the rank (1 = best) of key[target[i]] among all keys by query[i] . key[j]; `target`
    None pairs row i with row i.  normalize=True compares cosines (both sides through mh_l2norm_fwd first), which is what
    `InfoNCE` trains; the default compares the raw dot products, as `ClipLoss` does with the projected embeddings.
    See kernels.retrieval_ranks for the checks and the pessimistic tie / NaN rule.
    query_group [nq], key_group [nk] (integer ids, both or neither; not together with `target`): the positives of query i are all
    keys of its group and the rank is that of the best of them among the keys of OTHER groups for which key_count [nk] (None: all)
    is not 0; see kernels.retrieval_ranks_grouped."""
    grouped = query_group is not None or key_group is not None
    if grouped and target is not None:
        raise ValueError("retrieval_ranks: `target` names one positive per query, the groups name several: pass one or the other")
    if grouped and (query_group is None or key_group is None):
        raise ValueError("retrieval_ranks: query_group and key_group go together")
    if key_count is not None and not grouped:
        raise ValueError("retrieval_ranks: key_count needs query_group and key_group")
    if normalize:
        if query.dim() != 2 or key.dim() != 2:
            raise ValueError(f"retrieval_ranks: query and key must be [n, D], got {tuple(query.shape)} and {tuple(key.shape)}")
        K._chk(query, key)
        if query.dtype != torch.float32 or key.dtype != torch.float32:
            raise MirrorHipError(f"retrieval_ranks: query and key must be f32, got {query.dtype}, {key.dtype}")
        if query.shape[0] and key.shape[0] and query.shape[1] == key.shape[1] and query.shape[1] >= 1:
            query, key = _l2(query), _l2(key)
    if grouped:
        return K.retrieval_ranks_grouped(query, key, query_group, key_group, key_count)
    return K.retrieval_ranks(query, key, target)


def retrieval_topk(query: torch.Tensor, key: torch.Tensor, k: int, query_group: Optional[torch.Tensor] = None,
                   key_group: Optional[torch.Tensor] = None, normalize: bool = False, parts: int = 0):
    """(values f32 [nq, k], indices int32 [nq, k]) on the device, no host sync: for every query the k keys with the largest
    query[i] . key[j], best first, equal similarities by the smaller key index.  normalize=True compares cosines (both sides through
    mh_l2norm_fwd first), as `retrieval_ranks` does.  query_group [nq], key_group [nk] (integer ids, both or neither): a key of the
    query's own group is left out, so `arange(n)` on both sides is leave-one-out over one set and a patient id leaves out the
    patient's other slides.  A key whose similarity is NaN is never listed; slots beyond the eligible keys hold index -1 and value
    -inf.  1 <= k <= 64.  The values are the numbers `retrieval_ranks` decides by, bit for bit; `parts` (the number of key strips,
    0: chosen by the library) does not change the result.  See kernels.retrieval_topk for the checks."""
    if (query_group is None) != (key_group is None):
        raise ValueError("retrieval_topk: query_group and key_group go together")
    if normalize:
        if query.dim() != 2 or key.dim() != 2:
            raise ValueError(f"retrieval_topk: query and key must be [n, D], got {tuple(query.shape)} and {tuple(key.shape)}")
        K._chk(query, key)
        if query.dtype != torch.float32 or key.dtype != torch.float32:
            raise MirrorHipError(f"retrieval_topk: query and key must be f32, got {query.dtype}, {key.dtype}")
        if query.shape[0] and key.shape[0] and query.shape[1] == key.shape[1] and query.shape[1] >= 1:
            query, key = _l2(query), _l2(key)
    return K.retrieval_topk(query, key, k, query_group, key_group, parts)


def summarize_ranks(ranks, ks: Sequence[int] = (1, 5, 10)) -> "OrderedDict[str, float]":
    """`r@{k}` = the fraction of ranks <= k for every k of `ks`, then `medr` (np.median) and `meanr`, from a host array of ranks."""
    r = np.asarray(ranks).reshape(-1)
    if r.size == 0:
        raise ValueError("summarize_ranks: no ranks")
    out: "OrderedDict[str, float]" = OrderedDict()
    for k in ks:
        out[f"r@{int(k)}"] = float(np.mean(r <= int(k)))
    out["medr"] = float(np.median(r))
    out["meanr"] = float(np.mean(r.astype(np.float64)))
    return out


def first_of_group(sorted_ids, perm):
    """bool [n] in the original order: True on the first row of every group, from a STABLE ascending sort of the ids (the sorted
    ids and the permutation, as torch.sort or numpy's argsort(kind="stable") give them).  Torch tensors or numpy arrays."""
    if isinstance(sorted_ids, torch.Tensor):
        head = torch.ones_like(sorted_ids, dtype=torch.bool)
        head[1:] = sorted_ids[1:] != sorted_ids[:-1]
        return torch.zeros_like(head).scatter_(0, perm, head)
    sorted_ids, perm = np.asarray(sorted_ids), np.asarray(perm)
    head = np.ones(sorted_ids.shape, dtype=bool)
    head[1:] = sorted_ids[1:] != sorted_ids[:-1]
    out = np.zeros(sorted_ids.shape, dtype=bool)
    out[perm] = head
    return out


class CrossModalRetrieval:
    """Slide -> RNA and RNA -> slide retrieval over every pair accumulated so far, shaped like the classes of `metrics`:
    `update(wsi_emb, rna_emb)` keeps f32 copies on the device and never waits on the host; `compute()` launches both directions,
    reads the two rank vectors back in one sync and returns an OrderedDict of `wsi2rna_r@k..`, `wsi2rna_medr`, `wsi2rna_meanr`,
    the same for `rna2wsi_`, `r_mean` (the mean of all r@k over both directions: the scalar to select checkpoints on) and
    `retrieval_n` (the gallery size, which the values depend on).  Recalls are fractions in [0, 1].

    With `update(..., group=ids)` (every update, or none) pairs of one group are slides of one sample.  wsi2rna: every slide is a
    query, its positives are its group's RNA rows and the gallery is the first RNA row of each of the G groups.  rna2wsi: the keys
    are all slides, a query's positives are its group's slides, and the ranks are summarised over the first row of each group, so a
    sample counts once however many slides it has.  `retrieval_groups` = G follows `retrieval_n` = the number of slides.  With
    all-distinct ids every value equals the ungrouped one."""

    def __init__(self, ks: Sequence[int] = (1, 5, 10), normalize: bool = False, device=None):
        ks = tuple(int(k) for k in ks)
        if not ks or any(k < 1 for k in ks):
            raise ValueError(f"ks must be positive ranks, got {ks}")
        d = torch.device("cuda") if device is None else torch.device(device)
        if d.type != "cuda":
            raise MirrorHipError(f"mirror_amd metrics keep their state on a HIP device, got {d}")
        self.ks = ks
        self.normalize = bool(normalize)
        self.device = d
        self.wsi: List[torch.Tensor] = []             # f32 [n_i, D] per update
        self.rna: List[torch.Tensor] = []
        self.group: List[torch.Tensor] = []           # int64 [n_i] per update, or none at all

    def update(self, wsi_emb: torch.Tensor, rna_emb: torch.Tensor, group: Optional[torch.Tensor] = None) -> "CrossModalRetrieval":
        """wsi_emb, rna_emb: the two alignment embeddings [B, D] of the same B pairs, row i with row i.  group: an integer [B]
        tensor on the device or the host, the sample each pair belongs to (ids that mean the same on every rank)."""
        if wsi_emb.dim() != 2 or tuple(wsi_emb.shape) != tuple(rna_emb.shape):
            raise ValueError(f"wsi_emb and rna_emb must both be [B, D], got {tuple(wsi_emb.shape)} and {tuple(rna_emb.shape)}")
        if not (wsi_emb.is_floating_point() and rna_emb.is_floating_point()):
            raise ValueError(f"embeddings must be floating point, got {wsi_emb.dtype} and {rna_emb.dtype}")
        if self.wsi and self.wsi[0].shape[1] != wsi_emb.shape[1]:
            raise ValueError(f"embedding width changed from {self.wsi[0].shape[1]} to {wsi_emb.shape[1]}")
        if group is not None and (not isinstance(group, torch.Tensor) or group.dim() != 1 or group.numel() != wsi_emb.shape[0]
                                  or group.dtype not in (torch.int32, torch.int64)):
            got = f"{group.dtype} {tuple(group.shape)}" if isinstance(group, torch.Tensor) else type(group).__name__
            raise ValueError(f"group must be an int32 / int64 [{wsi_emb.shape[0]}] tensor, got {got}")
        if self.wsi and (group is not None) != bool(self.group):
            raise ValueError("either every update() passes `group` or none does: this one " +
                             ("does, the earlier ones did not" if group is not None else "does not, the earlier ones did"))
        if group is not None:
            self.group.append(group.detach().to(device=self.device, dtype=torch.int64, non_blocking=True, copy=True))
        for store, x in ((self.wsi, wsi_emb), (self.rna, rna_emb)):
            store.append(x.detach().to(device=self.device, dtype=torch.float32, non_blocking=True, copy=True))
        return self

    def _cat(self):
        w = self.wsi[0] if len(self.wsi) == 1 else torch.cat(self.wsi)
        r = self.rna[0] if len(self.rna) == 1 else torch.cat(self.rna)
        return w, r

    def compute(self) -> "OrderedDict[str, float]":
        n = sum(t.shape[0] for t in self.wsi)
        if n == 0:
            raise ValueError("CrossModalRetrieval.compute(): no samples (call update() first)")
        w, r = self._cat()
        if self.normalize:
            w, r = _l2(w), _l2(r)
        groups = None
        if self.group:
            g = self.group[0] if len(self.group) == 1 else torch.cat(self.group)
            order = torch.sort(g, stable=True)
            first = first_of_group(*order)
            both = torch.stack((K.retrieval_ranks_grouped(w, r, g, g, first, key_order=order),
                                K.retrieval_ranks_grouped(r, w, g, g, None, key_order=order), first.to(torch.int32))).cpu().numpy()
            heads = both[2] != 0
            both, groups = (both[0], both[1][heads]), int(heads.sum())
        else:
            both = torch.stack((K.retrieval_ranks(w, r), K.retrieval_ranks(r, w))).cpu().numpy()
        out: "OrderedDict[str, float]" = OrderedDict()
        recalls = []
        for name, ranks in (("wsi2rna", both[0]), ("rna2wsi", both[1])):
            for k, v in summarize_ranks(ranks, self.ks).items():
                out[f"{name}_{k}"] = v
                if k.startswith("r@"):
                    recalls.append(v)
        out["r_mean"] = float(np.mean(recalls))
        out["retrieval_n"] = n
        if groups is not None:
            out["retrieval_groups"] = groups
        return out

    def topk(self, k: int, direction: str = "wsi2rna", exclude_own_group: bool = False):
        """(values f32 [n, k], indices int32 [n, k]) on the device, no host sync: for every accumulated slide the k RNA profiles it
        retrieves ("wsi2rna"), or for every RNA profile the k slides ("rna2wsi"), best first; indices count the accumulated pairs in
        update() order.  By default nothing is excluded, so a query's positive appears where it ranks.  exclude_own_group=True leaves
        the query's own sample out of its list: every pair of its group with group ids, its own pair without.  The state and
        compute() are untouched."""
        if direction not in ("wsi2rna", "rna2wsi"):
            raise ValueError(f'direction must be "wsi2rna" or "rna2wsi", got {direction!r}')
        if sum(t.shape[0] for t in self.wsi) == 0:
            raise ValueError("CrossModalRetrieval.topk(): no samples (call update() first)")
        w, r = self._cat()
        if self.normalize:
            w, r = _l2(w), _l2(r)
        g = None
        if exclude_own_group:
            if self.group:
                g = self.group[0] if len(self.group) == 1 else torch.cat(self.group)
            else:
                g = torch.arange(w.shape[0], device=self.device, dtype=torch.int64)
        query, key = (w, r) if direction == "wsi2rna" else (r, w)
        return K.retrieval_topk(query, key, k, g, g)

    def reset(self) -> "CrossModalRetrieval":
        self.wsi, self.rna, self.group = [], [], []
        return self

    def merge_state(self, metrics: Iterable["CrossModalRetrieval"]) -> "CrossModalRetrieval":
        for m in metrics:
            if m.wsi and self.wsi and m.wsi[0].shape[1] != self.wsi[0].shape[1]:
                raise ValueError(f"cannot merge retrieval states of widths {m.wsi[0].shape[1]} and {self.wsi[0].shape[1]}")
            if m.wsi and self.wsi and bool(m.group) != bool(self.group):
                raise ValueError("cannot merge a retrieval state with group ids and one without")
            self.wsi.extend(t.to(self.device) for t in m.wsi)
            self.rna.extend(t.to(self.device) for t in m.rna)
            self.group.extend(t.to(self.device) for t in m.group)
        return self
