"""The cluster probe (include/mirror_hip.h "k-means of frozen embeddings"; mirror_amd/cluster.py) restated in float64 numpy.
Shared by tests/test_cluster_{cpu,gpu}.py; shares no code with mirror_amd.

    1. y       = the prepared rows: center: (x - mu) / max(|x - mu|, 1e-12) with the POOL's column mean; "cosine" without centring:
                 x / max(|x|, 1e-12); "euclidean" without centring: x
    2. assign  = the k of the largest y . c[r, k] + bias[r, k]; NaN not eligible, equal scores to the smaller k, -1 when none is eligible
    3. update  : c[r, k] = the mean of the member rows SUMMED IN ROW ORDER (np.cumsum, never np.sum: pairwise); "cosine": c / max(|c|,
                 1e-12); "euclidean": bias = -|c|^2 / 2; an empty cluster keeps centroid and bias.  f32=True rounds where the device
                 rounds (the mean once; the normalised centroid and the bias once more) and adds |c|^2 in the device's stated order
                 (device_sumsq), for the bit-for-bit comparison
    4. inertia = sum over the assigned rows of |y_i - c[r, assign]|^2
    5. tally   : cont[cluster, label]; bad = rows with a label outside [0, C) or assign outside [0, K); NMI (arithmetic mean, natural
                 log), ARI, purity, with sklearn's degenerate cases
    6. lloyd   : assign, update, until an assign step changes nothing; per step the share of rows whose two best scores lie within the
                 margin of each other
"""
import math

import numpy as np

from tests import datafeed_ref
from tests.retrieval_topk_ref import MARGIN


def clusters(C, D, per_class, noise, seed):
    """Gaussian class clusters (the generator of tests/fewshot_ref.py restated, without its queries): centres ~ N(0, I), per_class rows
    per class (shuffled) with N(0, noise^2 I) around their centre plus a common offset (so that centring matters).  f32 rows, int64
    labels."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((C, D))
    shift = 3.0 * rng.standard_normal(D)
    yl = rng.permutation(np.repeat(np.arange(C), per_class))
    pool = centres[yl] + noise * rng.standard_normal((len(yl), D)) + shift
    return pool.astype(np.float32), yl.astype(np.int64)


def prepare(pool, x, metric, center=True):
    """(y float64 [n, D], mu float64 [D] or None) of rows x under the pool's mean."""
    pool, x = np.asarray(pool, dtype=np.float64), np.asarray(x, dtype=np.float64)
    if not center and metric == "euclidean":
        return x.copy(), None
    mu = pool.mean(0) if center else np.zeros(pool.shape[1])
    with np.errstate(invalid="ignore"):
        d = x - mu
        return d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12), (mu if center else None)


def bias_of(cent, metric):
    """float64 [R, K]: -|c|^2 / 2 ("euclidean"), 0 ("cosine": no bias, which decides the same)."""
    cent = np.asarray(cent, dtype=np.float64)
    return -0.5 * (cent * cent).sum(2) if metric == "euclidean" else np.zeros(cent.shape[:2])


def scores(y, cent, bias):
    """float64 [R, n, K]."""
    with np.errstate(invalid="ignore"):
        return np.einsum("id,rkd->rik", np.asarray(y, dtype=np.float64), np.asarray(cent, dtype=np.float64)) + np.asarray(bias)[:, None, :]


def assign_step(S):
    """int64 [R, n] from scores [R, n, K]: the first largest non-NaN, -1 when all are NaN."""
    S = np.asarray(S, dtype=np.float64)
    R, n, K = S.shape
    out = np.full((R, n), -1, dtype=np.int64)
    for r in range(R):
        for i in range(n):
            best = -1
            for k in range(K):
                v = S[r, i, k]
                if v == v and (best < 0 or v > S[r, i, best]):
                    best = k
            out[r, i] = best
    return out


def top_two_gap(S):
    """float64 [R, n]: best minus second best (NaN counted as -inf; inf when fewer than two are eligible)."""
    S = np.asarray(S, dtype=np.float64)
    if S.shape[2] < 2:
        return np.full(S.shape[:2], np.inf)
    M = np.sort(np.where(np.isnan(S), -np.inf, S), axis=2)
    with np.errstate(invalid="ignore"):
        gap = M[:, :, -1] - M[:, :, -2]
    return np.where(np.isnan(gap) | np.isinf(M[:, :, -2]), np.inf, gap)


def margin_of(y, cent, bias, metric):
    """float64 [R, n]: the project's margin on a score, 1e-5 (|y_i| max_k |c_k| + max_k |bias_k|), the bias term for "euclidean"."""
    y, cent = np.asarray(y, dtype=np.float64), np.asarray(cent, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        m = np.linalg.norm(y, axis=1)[None, :] * np.nanmax(np.linalg.norm(cent, axis=2), axis=1)[:, None]
        if metric == "euclidean":
            m = m + np.nanmax(np.abs(np.asarray(bias, dtype=np.float64)), axis=1)[:, None]
    return MARGIN * m


def device_sumsq(c):
    """|c|^2 of an f32-valued centroid (D <= 4096) in the order the header states for mh_kmeans_update and mh_kmeans_bias: thread t of 256
    adds the squares of its columns t, t + 256, .. in that order (the squares of f32 values are exact in f64, so a fused multiply-add
    is a multiply and an add), the 64 lanes of a wave are added by the xor butterfly 32, 16, .., 1 (lane l takes v[l] + v[l ^ o]:
    every lane ends with the same bits), the four waves in order."""
    c = np.asarray(c, dtype=np.float64)
    sq = np.zeros(4096)
    sq[:len(c)] = c * c
    v = np.cumsum(sq.reshape(16, 256), axis=0)[-1].reshape(4, 64)        # [wave, lane]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return float(((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0])


def update_step(y, assign, cent, bias, metric, f32=False):
    """(cent, bias, count) after one update; the inputs are left alone.  Members are summed in ascending row order."""
    y, assign = np.asarray(y, dtype=np.float64), np.asarray(assign, dtype=np.int64)
    cent, bias = np.array(cent, dtype=np.float64), np.array(bias, dtype=np.float64)
    R, K, D = cent.shape
    count = np.zeros((R, K), dtype=np.int64)
    rnd = (lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)) if f32 else (lambda a: a)
    for r in range(R):
        for k in range(K):
            rows = np.flatnonzero(assign[r] == k)                  # ascending
            count[r, k] = len(rows)
            if len(rows) == 0:
                continue
            c = rnd(np.cumsum(y[rows], axis=0)[-1] / float(len(rows)))      # cumsum: one addition after the other, in row order
            ss = device_sumsq(c) if f32 else float(np.cumsum(c * c)[-1])
            if metric == "cosine":
                cent[r, k], bias[r, k] = rnd(c / max(math.sqrt(ss), 1e-12)), 0.0
            else:
                cent[r, k], bias[r, k] = c, float(rnd(-0.5 * ss))
    return cent, bias, count


def inertia(y, cent, assign):
    """float64 [R]."""
    y, cent, assign = np.asarray(y, dtype=np.float64), np.asarray(cent, dtype=np.float64), np.asarray(assign, dtype=np.int64)
    out = np.zeros(cent.shape[0])
    for r in range(cent.shape[0]):
        ok = (assign[r] >= 0) & (assign[r] < cent.shape[1])
        d = y[ok] - cent[r][assign[r][ok]]
        out[r] = float((d * d).sum())
    return out


def contingency(assign, labels, K, C):
    """(cont int64 [R, K, C], bad int64 [R])."""
    assign, labels = np.asarray(assign, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    R, n = assign.shape
    cont = np.zeros((R, K, C), dtype=np.int64)
    bad = np.zeros(R, dtype=np.int64)
    for r in range(R):
        for i in range(n):
            a, y = assign[r, i], labels[i]
            if 0 <= a < K and 0 <= y < C:
                cont[r, a, y] += 1
            else:
                bad[r] += 1
    return cont, bad


def _entropy(m, N):
    m = [int(v) for v in m if v > 0]
    return -sum((v / N) * (math.log(v) - math.log(N)) for v in m)


def scores_of(cont):
    """(NMI, ARI, purity) of one contingency table [K, C] of integers."""
    cont = np.asarray(cont, dtype=np.int64)
    a, b = cont.sum(1), cont.sum(0)
    N = int(cont.sum())
    nk, nc = int((a > 0).sum()), int((b > 0).sum())
    if nk <= 1 and nc <= 1:
        nmi = 1.0
    elif nk == 1 or nc == 1:
        nmi = 0.0
    else:
        mi = 0.0
        for k in range(cont.shape[0]):
            for c in range(cont.shape[1]):
                v = int(cont[k, c])
                if v > 0:
                    t = (v / N) * (math.log(v) - math.log(int(a[k])) - math.log(int(b[c])) + math.log(N))
                    mi += 0.0 if abs(t) < np.finfo(np.float64).eps else t
        mi = max(mi, 0.0)
        nmi = 0.0 if mi == 0.0 else mi / (0.5 * (_entropy(a, N) + _entropy(b, N)))
    sq = sum(int(v) ** 2 for v in cont.ravel())
    tp, fp, fn = sq - N, sum(int(v) ** 2 for v in b) - sq, sum(int(v) ** 2 for v in a) - sq
    tn = N * N - fp - fn - sq
    ari = 1.0 if fp == 0 and fn == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    purity = float(cont.max(1).sum()) / N if N > 0 else float("nan")
    return nmi, ari, purity


def tally(assign, labels, K, C):
    """(cont, bad, summary float64 [R, 3])."""
    cont, bad = contingency(assign, labels, K, C)
    return cont, bad, np.array([scores_of(cont[r]) for r in range(cont.shape[0])], dtype=np.float64).reshape(-1, 3)


def lloyd(y, init, metric, max_iter=100):
    """Lloyd's iteration of every restart from init [R, K, D]: assign, then update, until an assign step changes nothing (that step
    counts) or max_iter.  Returns a dict: assign int64 [R, n], cent, bias, count, n_iter int64 [R], inertia float64 [R] (of the last
    assignment against the centroids updated from it), undecided: per restart the list over its steps of the share of rows whose two
    best scores lie within margin_of(...) of each other, trace: per restart the list of inertia after every step."""
    y, init = np.asarray(y, dtype=np.float64), np.asarray(init, dtype=np.float64)
    R, K, D = init.shape
    n = y.shape[0]
    out = dict(assign=np.full((R, n), -1, dtype=np.int64), cent=init.copy(), bias=bias_of(init, metric), count=np.zeros((R, K), dtype=np.int64),
               n_iter=np.full(R, max_iter, dtype=np.int64), undecided=[[] for _ in range(R)], trace=[[] for _ in range(R)])
    for r in range(R):
        cent, bias, prev = out["cent"][r:r + 1], out["bias"][r:r + 1], out["assign"][r:r + 1]
        for it in range(max_iter):
            S = scores(y, cent, bias)
            out["undecided"][r].append(float((top_two_gap(S) <= margin_of(y, cent, bias, metric)).mean()))
            a = assign_step(S)
            same = np.array_equal(a, prev)
            prev = a
            cent, bias, count = update_step(y, a, cent, bias, metric)
            out["trace"][r].append(float(inertia(y, cent, a)[0]))
            if same:
                out["n_iter"][r] = it + 1
                break
        out["assign"][r], out["cent"][r], out["bias"][r], out["count"][r] = prev[0], cent[0], bias[0], count[0]
    out["inertia"] = inertia(y, out["cent"], out["assign"])
    return out


def random_rows(n, K, R, seed):
    """int64 [R, K]: K distinct rows per restart, for explicit starts."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(n, size=K, replace=False) for _ in range(R)]).astype(np.int64)


def drawn_rows(n, K, R, seed, offset):
    """int64 [R, K]: the rows ClusterProbe draws without init: restart r is draw id offset + r over one slide of n rows."""
    return np.stack([datafeed_ref.sample_local(n, K, seed, offset + r) for r in range(R)]).astype(np.int64)


def report(summary, best, inertia_best, empty_best, K, n):
    """The dict of ClusterProbe.evaluate from the [R, 3] table."""
    summary = np.asarray(summary, dtype=np.float64)
    R = summary.shape[0]
    out = {}
    for j, name in enumerate(("cluster_nmi", "cluster_ari", "cluster_purity")):
        out[name] = float(summary[best, j])
        out[name + "_mean"] = float(summary[:, j].mean())
        out[name + "_std"] = float(summary[:, j].std(ddof=1)) if R > 1 else 0.0
    out["cluster_inertia"], out["cluster_empty"] = float(inertia_best), int(empty_best)
    out["cluster_k"], out["cluster_restarts"], out["cluster_n"] = K, R, n
    return out


#        (classes, D, per class, noise, K): the end-to-end inputs; tests/test_cluster_cpu.py checks from float64 alone that no step of any
#        of their starts has an undecided row
E2E = [(5, 24, 26, 0.5, 5), (7, 515, 43, 1.0, 7), (4, 64, 75, 2.0, 12)]
E2E_STARTS = 4


def e2e_case(shape, metric):
    """(pool f32, labels, y float64, init f32 [4, K, D]: rows of y rounded to f32) of one end-to-end input."""
    C, D, per, noise, K = shape
    pool, yl = clusters(C, D, per, noise, seed=C * 1000 + D)
    y, _ = prepare(pool, pool, metric)
    rows = random_rows(len(yl), K, E2E_STARTS, seed=D + K)
    return pool, yl, y, y[rows].astype(np.float32)
