"""The cluster probe's seeding, silhouette and matched accuracy (include/mirror_hip.h "cluster probe: seeding, silhouette, matched
accuracy"; csrc/cluster_ext.hip) restated in float64 numpy from the header text.  Shared by tests/test_cluster_ext_{cpu,gpu}.py; shares
no code with mirror_amd.

    silhouette   d_ij = sqrt(max(q_i + q_j - 2 s_ij, 0)) ("euclidean") or 1 - s_ij ("cosine"), the pair i = j left out by index;
                 a_i, b_i, s_i as sklearn's silhouette_samples; a row with an id outside [0, K) takes no part and is NaN
    match        the maximum-weight one-to-one assignment of clusters to classes, by shortest augmenting paths on Python integers
    kmeanspp     D^2 sampling with the data feed's Philox stream under kind 2, the sums in strip order then row order
"""
import numpy as np

from tests import datafeed_ref

KIND_SEED = 2
MAXPARTS = 128


# ------------------------------------------------------------------ silhouette
def distances(y, metric):
    """float64 [n, n] from float64 products; the diagonal is whatever the formula gives (it is never used)."""
    y = np.asarray(y, dtype=np.float64)
    s = y @ y.T
    if metric == "cosine":
        return 1.0 - s
    q = (y * y).sum(1)
    t = q[:, None] + q[None, :] - 2.0 * s
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.where(t < 0.0, 0.0, t))


def silhouette(y, lab, K, metric, dist=None):
    """(s float64 [n], mean, bad, scale float64 [n]): scale = max(a_i, b_i), what a distance error is divided by."""
    lab = np.asarray(lab, dtype=np.int64)
    n = len(lab)
    d = distances(y, metric) if dist is None else dist
    ok = (lab >= 0) & (lab < K)
    sizes = np.array([int((lab == k).sum()) for k in range(K)])
    s, scale = np.full(n, np.nan), np.full(n, np.nan)
    if (sizes > 0).sum() >= 2:
        for i in np.flatnonzero(ok):
            S = np.zeros(K)
            for k in range(K):
                m = lab == k
                m[i] = False                                # by index
                S[k] = d[i, m].sum()
            li = lab[i]
            b = min(S[k] / sizes[k] for k in range(K) if k != li and sizes[k] > 0)
            if sizes[li] == 1:
                s[i], scale[i] = 0.0, b
                continue
            a = S[li] / (sizes[li] - 1)
            scale[i] = max(a, b)
            s[i] = 0.0 if scale[i] == 0.0 else (b - a) / scale[i]
    mean = float(np.mean(s[ok])) if ok.any() and (sizes > 0).sum() >= 2 else float("nan")
    return s, mean, int((~ok).sum()), scale


# ------------------------------------------------------------------ matching
def match(cont):
    """(match int64 [K], hits int) of one table [K, C] of non-negative integers: min(K, C) pairs of the largest sum."""
    cont = np.asarray(cont, dtype=np.int64)
    K, C = cont.shape
    tr = K > C
    w = (cont.T if tr else cont).astype(object)             # Python integers; the smaller side as rows
    n, m = w.shape
    INF = 1 << 60
    u, v, p, way = [0] * (n + 1), [0] * (m + 1), [0] * (m + 1), [0] * (m + 1)
    for i in range(1, n + 1):
        p[0], j0 = i, 0
        minv, used = [INF] * (m + 1), [False] * (m + 1)
        while True:
            used[j0] = True
            i0, delta, j1 = p[j0], INF, 0
            for j in range(1, m + 1):
                if not used[j]:
                    cur = -int(w[i0 - 1, j - 1]) - u[i0] - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                    if minv[j] < delta:
                        delta, j1 = minv[j], j
            for j in range(m + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    out = np.full(K, -1, dtype=np.int64)
    for j in range(1, m + 1):
        if p[j]:
            if tr:
                out[j - 1] = p[j] - 1
            else:
                out[p[j] - 1] = j - 1
    return out, int(sum(int(cont[k, out[k]]) for k in range(K) if out[k] >= 0))


# ------------------------------------------------------------------ k-means++
def uniforms(count, seed, draw):
    """float64 [count]: u_j = (((w_2j >> 5) << 26) | (w_2j+1 >> 6)) 2^-53 of draw `draw` under kind 2."""
    w = datafeed_ref.draw_words(2 * count, KIND_SEED, draw, seed)
    bits = ((w[0::2] >> np.uint64(5)) << np.uint64(26)) | (w[1::2] >> np.uint64(6))
    return bits.astype(np.float64) * 2.0 ** -53


def strips(n):
    """[(r0, r1)]: mh_colmean's partition: at least 64 rows a strip, 128 strips at the most."""
    parts = min(MAXPARTS, max(1, (n + 63) // 64))
    return [(p * n // parts, (p + 1) * n // parts) for p in range(parts)]


def sqdist(y, c):
    """float64 [n]: |y_i - c|^2 in ascending d, one addition per column; a NaN counts as 0."""
    e = np.asarray(y, dtype=np.float64) - np.asarray(c, dtype=np.float64)[None, :]
    with np.errstate(invalid="ignore"):
        t = np.cumsum(e * e, axis=1)[:, -1]
    return np.where(np.isnan(t), 0.0, t)


def min_dist(y, chosen):
    m = sqdist(y, y[chosen[0]])
    for c in chosen[1:]:
        m = np.minimum(m, sqdist(y, y[c]))
    return m


def running(m):
    """(before float64 [n], after float64 [n], T): the running sum before and after every row, the strips' own sums added in strip
    order, a strip's rows in row order."""
    n = len(m)
    before, after = np.zeros(n), np.zeros(n)
    acc = 0.0
    for r0, r1 in strips(n):
        local = np.cumsum(m[r0:r1]) if r1 > r0 else np.zeros(0)
        after[r0:r1] = acc + local
        before[r0:r1] = acc + np.concatenate([[0.0], local[:-1]])
        if r1 > r0:
            acc = acc + float(local[-1])
    return before, after, acc


def pick(m, u):
    """The row of one centre from the weights m and the draw u, by the header's rules."""
    n = len(m)
    before, after, T = running(m)
    if not T > 0.0:
        return int(u * float(n))
    t = u * T
    hit = np.flatnonzero((after > t) & (m > 0))
    if len(hit):
        return int(hit[0])
    return int(np.flatnonzero(m > 0)[-1])


def kmeanspp(y, R, K, seed, offset):
    """int64 [R, K]: the rows of every restart."""
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    rows = np.zeros((R, K), dtype=np.int64)
    for r in range(R):
        u = uniforms(K, seed, offset + r)
        rows[r, 0] = int(u[0] * float(n))
        m = sqdist(y, y[rows[r, 0]])
        for j in range(1, K):
            rows[r, j] = pick(m, u[j])
            m = np.minimum(m, sqdist(y, y[rows[r, j]]))
    return rows


# ------------------------------------------------------------------ the inputs both test files use
#            ((classes, D, per class, noise) of kmeans_ref.clusters, K): n = 132, 300, 260
SIL_CASES = [((3, 24, 44, 0.6), 3), ((5, 515, 60, 0.8), 7), ((4, 512, 65, 1.0), 4)]


def sil_case(shape, K):
    """(pool f32 [n, D], lab int32 [n]): the true class mod K with 15 % of the rows reassigned at random, rows in the generator's
    (shuffled) order."""
    from tests import kmeans_ref
    pool, yl = kmeans_ref.clusters(*shape, seed=shape[1] + K)
    rng = np.random.default_rng(shape[1] * 7 + K)
    lab = yl % K
    move = rng.random(len(yl)) < 0.15
    lab = np.where(move, rng.integers(0, K, len(yl)), lab)
    return pool, lab.astype(np.int32)


def index_case():
    """(y f32 [130, 24] of integers in [-2, 2], lab int32 [130], notes): K = 5; cluster 3 is a singleton (row 17), cluster 4 is empty,
    rows 5 and 90 are identical and both in cluster 1, rows 40 and 129 carry ids outside [0, 5)."""
    rng = np.random.default_rng(130)
    y = rng.integers(-2, 3, (130, 24)).astype(np.float32)
    lab = rng.integers(0, 3, 130).astype(np.int32)
    lab[17] = 3
    y[90] = y[5]
    lab[5] = lab[90] = 1
    lab[40], lab[129] = -1, 5
    return y, lab, dict(K=5, singleton=17, twins=(5, 90), outside=(40, 129))
