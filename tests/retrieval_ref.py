"""The grouped retrieval ranks of include/mirror_hip.h (mh_retrieval_ranks_grouped) restated in float64 numpy, and the metric built
on them (mirror_amd/retrieval.py: CrossModalRetrieval with group ids).  Shared by tests/test_retrieval_grouped_{cpu,gpu}.py.

    P_i      = { j : kgroup[j] == qgroup[i] }
    d_i      = max_{j in P_i} s_ij          (NaN if P_i is empty or holds a NaN)
    ranks[i] = 1 + #{ j not in P_i, kcount[j] != 0 : not (s_ij < d_i) }
"""
from collections import OrderedDict

import numpy as np


def similarities(q, k, same=()):
    """q k^T in float64.  same: (src, dst) key-row pairs that are copies of each other, whose columns are forced to be the same
    number (a float64 BLAS may sum two equal columns in different orders)."""
    S = np.asarray(q, dtype=np.float64) @ np.asarray(k, dtype=np.float64).T
    for src, dst in same:
        S[:, dst] = S[:, src]
    return S


def best_positive(S, qgroup, kgroup):
    """d [nq] and the positives' mask [nq, nk]."""
    pos = np.asarray(qgroup, dtype=np.int64)[:, None] == np.asarray(kgroup, dtype=np.int64)[None, :]
    d = np.full(S.shape[0], np.nan)
    for i in range(S.shape[0]):
        s = S[i, pos[i]]
        if s.size and not np.isnan(s).any():
            d[i] = s.max()
    return d, pos


def grouped_ranks_np(q, k, qgroup, kgroup, kcount=None, same=()):
    S = similarities(q, k, same)
    d, pos = best_positive(S, qgroup, kgroup)
    counted = np.ones(S.shape[1], dtype=bool) if kcount is None else np.asarray(kcount) != 0
    with np.errstate(invalid="ignore"):
        beats = ~(S < d[:, None])                      # a NaN on either side: not below, so it counts
    beats &= ~pos & counted[None, :]
    return (1 + beats.sum(1)).astype(np.int64)


def grouped_undecided_np(q, k, qgroup, kgroup, kcount=None):
    """Queries with a counted competitor inside the float64 margin 1e-5 |q_i| |k_j| of the best positive.  Which of two close
    positives is the best moves d_i by less than the f32 error the margin already allows for, so only competitors are looked at.
    A competitor whose row is an exact copy of one of the query's positives is a tie by construction, not a near miss."""
    q, k = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64)
    S = q @ k.T
    d, pos = best_positive(S, qgroup, kgroup)
    counted = np.ones(S.shape[1], dtype=bool) if kcount is None else np.asarray(kcount) != 0
    close = np.abs(S - d[:, None]) <= 1e-5 * np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(k, axis=1)[None, :]
    close &= ~pos & counted[None, :]
    copies = (k[:, None, :] == k[None, :, :]).all(-1)
    close &= ~((pos.astype(np.int64) @ copies.astype(np.int64)) > 0)
    return int(close.any(1).sum())


def first_of_group_np(group):
    """True on the first row of every group, in the order given."""
    group = np.asarray(group, dtype=np.int64)
    seen, out = set(), np.zeros(group.shape, dtype=bool)
    for i, g in enumerate(group.tolist()):
        if g not in seen:
            seen.add(g)
            out[i] = True
    return out


def summarize_np(ranks, ks):
    r = np.asarray(ranks).reshape(-1)
    out = OrderedDict((f"r@{int(k)}", float(np.mean(r <= int(k)))) for k in ks)
    out["medr"] = float(np.median(r))
    out["meanr"] = float(np.mean(r.astype(np.float64)))
    return out


def grouped_metric_np(w, r, group, ks=(1, 5, 10)):
    """The dictionary of CrossModalRetrieval.compute() with group ids: slide -> RNA over all slides against the first RNA row of
    each group, RNA -> slide over the first row of each group against all slides."""
    first = first_of_group_np(group)
    w2r = grouped_ranks_np(w, r, group, group, first)
    r2w = grouped_ranks_np(r, w, group, group)[first]
    out, rec = OrderedDict(), []
    for name, ranks in (("wsi2rna", w2r), ("rna2wsi", r2w)):
        for key, v in summarize_np(ranks, ks).items():
            out[f"{name}_{key}"] = v
            if key.startswith("r@"):
                rec.append(v)
    out["r_mean"] = float(np.mean(rec))
    out["retrieval_n"] = int(len(first))
    out["retrieval_groups"] = int(first.sum())
    return out
