"""The few-shot prototype probe (include/mirror_hip.h "few-shot prototype probe"; mirror_amd/fewshot.py) restated in float64 numpy.
Shared by tests/test_fewshot_{cpu,gpu}.py; shares no code with mirror_amd.

    1. y      = (x - mu) / max(|x - mu|, 1e-12), mu the column mean of the POOL (center=False: mu = 0)
    2. draw   : slot b = e C + c draws K rows of class c's run of the class-sorted pool, draw id offset + b (tests/datafeed_ref.py)
    3. p[e,c] = mean_k y[support[e, c, k]]; "cosine": p / max(|p|, 1e-12); "euclidean": bias = -|p|^2 / 2; an index outside the pool: NaN
    4. pred   = the class of the largest q . p + bias; NaN not eligible, equal scores to the smaller class, -1 when none is eligible
    5. tally  : conf[label, pred]; bad = rows with a label outside [0, C) or pred -1; accuracy %, balanced accuracy %, macro F1
"""
import numpy as np

from tests import datafeed_ref

# A pair (episode, query) whose two best float64 scores lie within this of each other is "undecided" in the END-TO-END comparison, where
# the device prepares features, prototypes and scores in f32 from the raw embeddings while this file does all of it in f64: unit rows
# carry 2e-6 per element from the preparation, |q| = 1 and |p| <= 1 bound the score's error by a few 1e-6, and 1e-4 leaves an order
# of magnitude above that.  (The kernel-level test compares on the device's own f32 features and uses the project's 1e-5 |q| |p|.)
MARGIN_E2E = 1e-4


def cp_of(C):
    return 1 << (int(C) - 1).bit_length()


def prepare(pool, x, center=True):
    """(y float64 [n, D], mu float64 [D]) of rows x under the pool's mean."""
    pool, x = np.asarray(pool, dtype=np.float64), np.asarray(x, dtype=np.float64)
    mu = pool.mean(0) if center else np.zeros(pool.shape[1])
    with np.errstate(invalid="ignore"):
        d = x - mu
        return d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12), mu


def class_runs(labels, C):
    """[C] arrays: the pool rows of every class in pool order (the runs of the stable class sort)."""
    labels = np.asarray(labels, dtype=np.int64)
    return [np.flatnonzero(labels == c) for c in range(C)]


def draw(labels, C, K, E, seed, offset):
    """int64 [E, C, K]: the support rows of the pool."""
    runs = class_runs(labels, C)
    out = np.empty((E, C, K), dtype=np.int64)
    for e in range(E):
        for c in range(C):
            out[e, c] = runs[c][datafeed_ref.sample_local(len(runs[c]), K, seed, offset + e * C + c)]
    return out


def prototypes(y, support, metric):
    """(p float64 [E, Cp, D], bias float64 [E, Cp]; for "cosine" the bias is 0 on classes and -inf on pads, which decides the same)."""
    y, support = np.asarray(y, dtype=np.float64), np.asarray(support, dtype=np.int64)
    E, C, K = support.shape
    n, D = y.shape
    Cp = cp_of(C)
    p = np.zeros((E, Cp, D))
    bias = np.full((E, Cp), -np.inf)
    for e in range(E):
        for c in range(C):
            idx = support[e, c]
            if ((idx < 0) | (idx >= n)).any():
                p[e, c], bias[e, c] = np.nan, np.nan
                continue
            m = y[idx].sum(0) / K
            if metric == "cosine":
                p[e, c], bias[e, c] = m / max(np.linalg.norm(m), 1e-12), 0.0
            else:
                p[e, c], bias[e, c] = m, -0.5 * float(m @ m)
    return p, bias


def scores(q, p, bias):
    """float64 [E, nq, Cp]."""
    with np.errstate(invalid="ignore"):
        return np.einsum("id,ecd->eic", np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64)) + np.asarray(bias)[:, None, :]


def predict(S, C):
    """int64 [E, nq] from scores [E, nq, >= C]: the first largest non-NaN of the first C columns, -1 when all are NaN."""
    S = np.asarray(S, dtype=np.float64)[:, :, :C]
    E, nq, _ = S.shape
    out = np.full((E, nq), -1, dtype=np.int64)
    for e in range(E):
        for i in range(nq):
            best = -1
            for c in range(C):
                v = S[e, i, c]
                if v == v and (best < 0 or v > S[e, i, best]):
                    best = c
            out[e, i] = best
    return out


def top_two_gap(S, C):
    """float64 [E, nq]: best minus second best of the first C columns (NaN counted as -inf; inf when fewer than two are eligible)."""
    S = np.asarray(S, dtype=np.float64)[:, :, :C]
    M = np.sort(np.where(np.isnan(S), -np.inf, S), axis=2)
    with np.errstate(invalid="ignore"):
        gap = M[:, :, -1] - M[:, :, -2]
    return np.where(np.isnan(gap) | np.isinf(M[:, :, -2]), np.inf, gap)


def tally(pred, labels, C):
    """(conf int64 [E, C, C], bad int64 [E], summary float64 [E, 3])."""
    pred, labels = np.asarray(pred, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    E, nq = pred.shape
    conf = np.zeros((E, C, C), dtype=np.int64)
    bad = np.zeros(E, dtype=np.int64)
    summary = np.full((E, 3), np.nan)
    for e in range(E):
        n = np.zeros(C, dtype=np.int64)
        for i in range(nq):
            y, p = labels[i], pred[e, i]
            yok = 0 <= y < C
            if yok:
                n[y] += 1
            if yok and 0 <= p < C:
                conf[e, y, p] += 1
            else:
                bad[e] += 1
        tp, m = np.diag(conf[e]), conf[e].sum(0)
        if n.sum() > 0:
            summary[e, 0] = 100.0 * float(tp.sum()) / float(n.sum())
        rec = [float(tp[c]) / float(n[c]) for c in range(C) if n[c] > 0]
        if rec:
            summary[e, 1] = 100.0 * (sum(rec) / len(rec))
        f1 = [2.0 * float(tp[c]) / float(n[c] + m[c]) for c in range(C) if n[c] + m[c] > 0]
        if f1:
            summary[e, 2] = sum(f1) / len(f1)
    return conf, bad, summary


def report(summary, shots, n):
    """The dict of FewShotProbe.evaluate from the [E, 3] table."""
    summary = np.asarray(summary, dtype=np.float64)
    E = summary.shape[0]
    out = {}
    for j, name in enumerate(("fewshot_acc", "fewshot_bacc", "fewshot_f1")):
        std = float(summary[:, j].std(ddof=1)) if E > 1 else 0.0
        out[name] = float(summary[:, j].mean())
        out[name + "_std"] = std
        out[name + "_ci95"] = 1.96 * std / np.sqrt(E)
    out["fewshot_shots"], out["fewshot_episodes"], out["fewshot_n"] = shots, E, n
    return out


def clusters(C, D, per_class, nq, noise, seed):
    """Gaussian class clusters: centres ~ N(0, I), pool of per_class rows per class (shuffled), nq queries with cycling labels, all with
    N(0, noise^2 I) around their centre plus a common offset (so that centring matters).  f32 arrays and int64 labels."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((C, D))
    shift = 3.0 * rng.standard_normal(D)
    yl = rng.permutation(np.repeat(np.arange(C), per_class))
    pool = centres[yl] + noise * rng.standard_normal((len(yl), D)) + shift
    ql = np.arange(nq) % C
    query = centres[ql] + noise * rng.standard_normal((nq, D)) + shift
    return pool.astype(np.float32), yl.astype(np.int64), query.astype(np.float32), ql.astype(np.int64)
