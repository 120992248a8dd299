"""mh_retrieval_topk and mh_knn_scores of include/mirror_hip.h restated in float64 numpy.  Shared by tests/test_retrieval_topk_{cpu,gpu}.py
and tests/test_knn_gpu.py.

    eligible(i, j) = s_ij is not NaN  and  (no groups  or  kgroup[j] != qgroup[i])
    idx[i, :]      = the eligible j by descending s_ij, equal s_ij by ascending j, cut or padded (-1, -inf) to kk
    score[i, c]    = sum_s [labels[idx[i, s]] == c] exp((val[i, s] - val[i, 0]) inv_t) / the row's total
"""
import numpy as np

MARGIN = 1e-5          # the project's margin 1e-5 |q_i| |k_j| (about 30x the f32 fmaf-chain error at D <= 1024)


def similarities(q, k):
    with np.errstate(invalid="ignore"):
        return np.asarray(q, dtype=np.float64) @ np.asarray(k, dtype=np.float64).T


def topk_np(q, k, kk, qgroup=None, kgroup=None, S=None):
    """(idx int64 [nq, kk], val float64 [nq, kk]).  S: similarities the caller already has."""
    S = similarities(q, k) if S is None else np.asarray(S, dtype=np.float64)
    nq, nk = S.shape
    out = np.isnan(S)
    if qgroup is not None:
        out |= np.asarray(qgroup, dtype=np.int64)[:, None] == np.asarray(kgroup, dtype=np.int64)[None, :]
    M = np.where(out, -np.inf, S)
    # ineligible columns go behind every eligible one, a real -inf similarity included: sort on (eligible first, larger S, smaller j)
    order = np.argsort(-M, axis=1, kind="stable")                    # the stable sort is the smaller-index tie rule
    order = np.take_along_axis(order, np.argsort(np.take_along_axis(out, order, 1), axis=1, kind="stable"), 1)
    idx = np.full((nq, kk), -1, dtype=np.int64)
    val = np.full((nq, kk), -np.inf)
    m = min(kk, nk)
    idx[:, :m] = order[:, :m]
    val[:, :m] = np.take_along_axis(S, order[:, :m], 1)
    gone = np.take_along_axis(out, order[:, :m], 1)
    idx[:, :m][gone] = -1
    val[:, :m][gone] = -np.inf
    return idx, val


def knn_scores_np(idx, val, labels, C, inv_t):
    idx, val, labels = np.asarray(idx, dtype=np.int64), np.asarray(val, dtype=np.float64), np.asarray(labels, dtype=np.int64)
    nq, kk = idx.shape
    out = np.zeros((nq, C))
    for i in range(nq):
        total = 0.0
        for s in range(kk):
            j = idx[i, s]
            if j < 0 or j >= labels.shape[0]:
                continue
            c = labels[j]
            if c < 0 or c >= C:
                continue
            d = 0.0 if val[i, s] == val[i, 0] else val[i, s] - val[i, 0]
            w = np.exp(d * inv_t)
            out[i, c] += w
            total += w
        if total > 0:
            out[i] /= total
    return out


def unit(x):
    x = np.asarray(x, dtype=np.float64)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)


def gauss_pairs(n, D, seed):
    """The Gaussian pairs of the ranks' tests: q Gaussian, k_i = a_i q_i + sqrt(1 - a_i^2) noise with a_i spread over [0, 0.5]."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n, D)).astype(np.float32)
    a = rng.permutation(np.linspace(0.0, 0.5, n)).astype(np.float32)[:, None]
    k = (a * q + np.sqrt(1 - a * a) * rng.standard_normal((n, D)).astype(np.float32)).astype(np.float32)
    return q, k


def undecided_rows(q, k, kk):
    """bool [nq]: two consecutive entries of the float64 top-(kk + 1) lie within the margin 1e-5 |q_i| |k_j| (the larger of the pair's)."""
    q, k = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64)
    idx, val = topk_np(q, k, min(kk + 1, k.shape[0]))
    qn, kn = np.linalg.norm(q, axis=1), np.linalg.norm(k, axis=1)
    m = MARGIN * qn[:, None] * kn[idx]
    gap = val[:, :-1] - val[:, 1:]
    return (gap <= np.maximum(m[:, :-1], m[:, 1:])).any(1)
