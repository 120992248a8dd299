"""MI355X: the cluster probe's silhouette, k-means++ seeding and matched accuracy (csrc/cluster_ext.hip, mirror_amd/cluster.py) against
the float64 restatements of tests/cluster_ext_ref.py.

Silhouette, rounding.  The device's distances come from f32 products; with the project's MARGIN (1e-5 of |y_i| |y_j|) on a product a
distance is off by at most delta = MARGIN (2 max|y|)^2 / d_min ("euclidean": d = sqrt(t), t off by 4 MARGIN max|y|^2 at the most,
|d' - d| = |t' - t| / (d' + d) <= |t' - t| / d_min) or delta = MARGIN max|y|^2 ("cosine"), and to first order |s'_i - s_i| <=
4 delta / max(a_i, b_i) (a and b are means of distances: each is off by delta at the most; s = (b - a) / max(a, b)).  d_min and
max(a_i, b_i) are computed in float64 by the test.  On these inputs the euclidean d_min lies between 0.45 and 28, the bounds between 3e-5 and 4e-3.

Silhouette, indexing.  Integer coordinates: every product and every d^2 is exact, so only the order of the f64 additions differs
from the restatement: 1e-12 relative.

k-means++.  Each pick is checked against the device's own earlier picks: the restatement forms m and the running sums from
rows[r, :j] and asks for before(p) - tau T <= t < after(p) + tau T with tau = (n + D + 2) 2^-52, the bound of a sequential f64 sum of
non-negative terms plus the distance's own rounding, and for m_p > 0."""
import numpy as np
import pytest
import torch

from mirror_amd import ClusterProbe, cluster, kernels as K
from tests import cluster_ext_ref as X, kmeans_ref as R
from tests.retrieval_topk_ref import MARGIN

pytestmark = pytest.mark.gpu

METRICS = ["euclidean", "cosine"]


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()


def host(t):
    return t.detach().cpu().numpy()


def prepared(pool, metric, center):
    """The probe's preparation, on the device."""
    x = dev(pool)
    if center:
        return K.center_l2norm(x, K.colmean(x))
    if metric == "cosine":
        return K.center_l2norm(x, torch.zeros(x.shape[1], device="cuda"))
    return x


# ------------------------------------------------------------------ silhouette: rounding
@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", X.SIL_CASES)
def test_silhouette_against_float64_within_the_derived_bound(case, metric, center):
    shape, Kk = case
    pool, lab = X.sil_case(shape, Kk)
    y = prepared(pool, metric, center)
    mean, bad, sil = K.silhouette(y, dev(lab[None, :]), Kk, metric, samples=True)
    assert mean.dtype == torch.float64 and tuple(mean.shape) == (1,) and sil.dtype == torch.float64 and tuple(sil.shape) == (1, len(lab))
    y64 = host(y).astype(np.float64)
    d = X.distances(y64, metric)
    want, want_mean, want_bad, scale = X.silhouette(y64, lab, Kk, metric, dist=d)
    ymax = np.linalg.norm(y64, axis=1).max()
    if metric == "euclidean":
        q = (y64 * y64).sum(1)
        t = q[:, None] + q[None, :] - 2.0 * (y64 @ y64.T)
        dmin = float(np.sqrt(t[~np.eye(len(lab), dtype=bool)].min()))
        delta = MARGIN * (2.0 * ymax) ** 2 / dmin
    else:
        dmin = float(d[~np.eye(len(lab), dtype=bool)].min())
        delta = MARGIN * ymax ** 2
    bound = 4.0 * delta / scale
    err = np.abs(host(sil)[0] - want)
    print(f"{metric} center={center} {shape}: d_min {dmin:.4g}, max|y| {ymax:.4g}, error {err.max():.3g}, bound {bound.min():.3g} .. "
          f"{bound.max():.3g}, mean {float(mean[0]):.6f} (float64 {want_mean:.6f})")
    assert int(bad[0]) == 0 and want_bad == 0
    assert (err <= bound).all()
    assert abs(float(mean[0]) - want.mean()) <= bound.mean()
    if metric == "euclidean":
        assert 0.4 < dmin < 30.0                                # the bound's denominator is not small on these inputs


# ------------------------------------------------------------------ silhouette: indexing
@pytest.mark.parametrize("metric", METRICS)
def test_silhouette_indexing_on_integer_rows(metric):
    y, lab, note = X.index_case()
    Kk = note["K"]
    mean, bad, sil = K.silhouette(dev(y), dev(lab[None, :]), Kk, metric, samples=True)
    got = host(sil)[0]
    want, want_mean, want_bad, _ = X.silhouette(y, lab, Kk, metric)
    keep = ~np.isnan(want)
    assert int(bad[0]) == 2 and want_bad == 2 and np.isnan(got[list(note["outside"])]).all() and keep.sum() == len(lab) - 2
    assert not np.isnan(got[keep]).any()
    assert (np.abs(got[keep] - want[keep]) <= 1e-12 * np.abs(want[keep])).all()
    assert got[note["singleton"]] == 0.0
    assert abs(float(mean[0]) - want_mean) <= 1e-12 * abs(want_mean)
    # the twins are at distance exactly 0 of each other: with the pair's distance set to 1 in the restatement both samples move
    a, b = note["twins"]
    d = X.distances(y, metric)
    if metric == "euclidean":
        assert d[a, b] == 0.0
        d2 = d.copy()
        d2[a, b] = d2[b, a] = 1.0
        moved = X.silhouette(y, lab, Kk, metric, dist=d2)[0]
        assert abs(moved[a] - got[a]) > 1e-6 and abs(moved[b] - got[b]) > 1e-6
    # a row is left out by index, not by value: each twin counts the other (at distance 0) and not itself, so both see the same
    # distances and their samples agree up to the order of additions
    assert abs(got[a] - got[b]) <= 1e-12 * abs(got[a])


def test_silhouette_of_one_cluster_is_nan():
    y, lab, note = X.index_case()
    one = np.full(len(lab), 2, dtype=np.int32)
    mean, bad, sil = K.silhouette(dev(y), dev(one[None, :]), note["K"], "euclidean", samples=True)
    assert np.isnan(float(mean[0])) and int(bad[0]) == 0 and np.isnan(host(sil)).all()
    none = np.full(len(lab), -1, dtype=np.int32)
    mean, bad, _ = K.silhouette(dev(y), dev(none[None, :]), note["K"], "euclidean")
    assert np.isnan(float(mean[0])) and int(bad[0]) == len(lab)


# ------------------------------------------------------------------ silhouette: general
def test_silhouette_repeats_batches_and_captures():
    shape, Kk = X.SIL_CASES[1]
    pool, lab = X.sil_case(shape, Kk)
    rng = np.random.default_rng(3)
    labs = np.stack([lab, rng.integers(0, Kk, len(lab)).astype(np.int32), (lab + 1) % Kk]).astype(np.int32)
    labs[1, :4] = [-1, Kk, 0, 1]
    y, ld = prepared(pool, "cosine", True), dev(labs)
    mean, bad, sil = K.silhouette(y, ld, Kk, "cosine", samples=True)
    again = K.silhouette(y, ld, Kk, "cosine", samples=True)
    eq = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))  # noqa: E731  (bits: NaN equals NaN)
    assert eq(again[0], mean) and torch.equal(again[1], bad) and eq(again[2], sil)
    assert host(bad).tolist() == [0, 2, 0]
    for r in range(3):
        m1, b1, s1 = K.silhouette(y, ld[r:r + 1], Kk, "cosine", samples=True)
        assert eq(m1[0], mean[r]) and int(b1[0]) == int(bad[r]) and eq(s1[0], sil[r])
    assert eq(K.silhouette(y, ld, Kk, "cosine")[0], mean) and K.silhouette(y, ld, Kk, "cosine")[2] is None
    # a relabelling of the clusters does not change the samples' values beyond the order of additions
    assert np.abs(host(sil)[2] - host(sil)[0]).max() <= 1e-12
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.silhouette(y, ld, Kk, "cosine", samples=True)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cm, cb, cs = K.silhouette(y, ld, Kk, "cosine", samples=True)
    g.replay()
    torch.cuda.synchronize()
    assert eq(cm, mean) and torch.equal(cb, bad) and eq(cs, sil)


def test_probe_silhouette_and_the_functional_form():
    shape, Kk = X.SIL_CASES[0]
    pool, _ = X.sil_case(shape, Kk)
    p = ClusterProbe(Kk, restarts=3, metric="euclidean", center=False, device="cuda").fit(dev(pool))
    best, per = p.silhouette(samples=True)
    every = p.silhouette(restarts="all")
    assert best.dim() == 0 and best.dtype == torch.float64 and tuple(per.shape) == (len(pool),) and tuple(every.shape) == (3,)
    assert torch.equal(every[int(p.best_)], best)
    mean, bad, sil = K.silhouette(p._y, p.labels_.view(1, -1), Kk, "euclidean", samples=True)
    assert torch.equal(mean[0], best) and torch.equal(sil[0], per)
    f_mean, f_per = cluster.silhouette_score(dev(pool), p.labels_, Kk, metric="euclidean", samples=True, device="cuda")
    assert torch.equal(f_mean, best) and torch.equal(f_per, per)
    assert torch.equal(cluster.silhouette_score(dev(pool), p.assign_.long(), Kk, metric="euclidean", device="cuda"), every)
    out = p.evaluate(dev(np.zeros(len(pool), dtype=np.int64)), 1, silhouette=True)
    assert list(out)[-1] == "cluster_silhouette" and out["cluster_silhouette"] == float(best) and len(out) == 15


# ------------------------------------------------------------------ k-means++
#        (n,   K, D,   R)
SEED = [(130, 3, 24, 1), (300, 8, 515, 3), (9000, 4, 16, 2)]            # the last one reaches all 128 strips


def seed_rows(n, D):
    return R.clusters(5, D, n // 5, 0.7, seed=n + D)[0]


@pytest.mark.parametrize("n,Kk,D,Rr", SEED)
def test_kmeanspp_picks_follow_the_stated_rule(n, Kk, D, Rr):
    y = seed_rows(n, D)
    assert y.shape == (n, D)
    seed, offset = 41, (2 << 32) + 7
    rows, cent = K.kmeanspp_init(dev(y), Rr, Kk, seed, offset)
    assert rows.dtype == torch.int64 and tuple(rows.shape) == (Rr, Kk) and cent.dtype == torch.float32 and tuple(cent.shape) == (Rr, Kk, D)
    again = K.kmeanspp_init(dev(y), Rr, Kk, seed, offset)
    assert torch.equal(again[0], rows) and torch.equal(again[1], cent)
    got = host(rows)
    assert np.array_equal(host(cent), y[got])                                # bit copies
    tau = (n + D + 2) * 2.0 ** -52
    closest = np.inf
    for r in range(Rr):
        u = X.uniforms(Kk, seed, offset + r)
        assert got[r, 0] == int(u[0] * float(n))
        for j in range(1, Kk):
            m = X.min_dist(y, list(got[r, :j]))
            before, after, T = X.running(m)
            t, p = u[j] * T, got[r, j]
            assert T > 0 and m[p] > 0, (r, j, p)
            assert before[p] - tau * T <= t < after[p] + tau * T, (r, j, p, before[p], t, after[p])
            closest = min(closest, abs(t - before[p]) / T, abs(after[p] - t) / T)
        assert len(set(got[r])) == Kk                                        # a chosen row has weight 0
    print(f"{(n, Kk, D, Rr)}: no target within {closest:.3g} T of a boundary (slack {tau:.3g})")
    if Rr > 1:
        assert len({tuple(v) for v in got}) == Rr                            # the restarts differ
    other = host(K.kmeanspp_init(dev(y), Rr, Kk, seed, offset + 1)[0])
    assert np.array_equal(other[:-1], got[1:])                               # restart r of one call is restart r + 1 of the other


def test_kmeanspp_without_enough_distinct_rows():
    same = np.full((200, 24), 0.5, dtype=np.float32)
    rows = host(K.kmeanspp_init(dev(same), 3, 4, 5, 9)[0])
    for r in range(3):
        assert list(rows[r]) == [int(v * 200.0) for v in X.uniforms(4, 5, 9 + r)]
    two = np.zeros((200, 24), dtype=np.float32)
    two[77:] = 1.0
    rows = host(K.kmeanspp_init(dev(two), 4, 3, 1, 0)[0])
    for r in range(4):
        u = X.uniforms(3, 1, r)
        assert rows[r, 0] == int(u[0] * 200.0) and (rows[r, 1] >= 77) == (rows[r, 0] < 77) and rows[r, 2] == int(u[2] * 200.0)
        assert rows[r, 1] == X.pick(X.sqdist(two, two[rows[r, 0]]), u[1])   # equal weights: exact sums, the pick is decided
    assert np.array_equal(rows, X.kmeanspp(two, 4, 3, 1, 0))


@pytest.mark.parametrize("metric", METRICS)
def test_fit_with_kmeanspp_is_a_fit_from_those_rows(metric):
    shape = R.E2E[0]
    pool, _ = R.clusters(*shape[:4], seed=3)
    Kk = shape[4]
    p = ClusterProbe(Kk, restarts=5, metric=metric, seed=11, offset=4, seeding="kmeans++", device="cuda").fit(dev(pool))
    rows, cent = K.kmeanspp_init(p._y, 5, Kk, 11, 4)
    assert torch.equal(p.init_rows_, rows) and p.init_rows_.dtype == torch.int64
    q = ClusterProbe(Kk, metric=metric, device="cuda").fit(dev(pool), init=p._y[p.init_rows_])
    assert torch.equal(q.assign_, p.assign_) and torch.equal(q.centroids_, p.centroids_) and torch.equal(q.n_iter_, p.n_iter_)
    rnd = ClusterProbe(Kk, restarts=5, metric=metric, seed=11, offset=4, device="cuda").fit(dev(pool))
    assert not torch.equal(rnd.init_rows_, p.init_rows_)                     # the default draw is another stream


# ------------------------------------------------------------------ matching
MATCH = [(1, 1), (3, 3), (7, 5), (5, 7), (64, 64), (300, 200)]


@pytest.mark.parametrize("hi", [51, 4])
@pytest.mark.parametrize("Kk,Cc", MATCH)
def test_matching_reaches_scipys_optimum(Kk, Cc, hi):
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(Kk * 1000 + Cc + hi)
    cont = rng.integers(0, hi, (3, Kk, Cc)).astype(np.int32)
    cont[2] = 0                                                              # an all-zero table
    match, hits = K.cluster_match(dev(cont))
    assert match.dtype == torch.int32 and tuple(match.shape) == (3, Kk) and hits.dtype == torch.int64 and tuple(hits.shape) == (3,)
    again = K.cluster_match(dev(cont))
    assert torch.equal(again[0], match) and torch.equal(again[1], hits)
    m, h = host(match), host(hits)
    for r in range(3):
        rr, cc = linear_sum_assignment(cont[r], maximize=True)
        assert h[r] == int(cont[r][rr, cc].sum())
        got = m[r][m[r] >= 0]
        assert len(got) == min(Kk, Cc) and len(set(got)) == len(got) and (got < Cc).all() and (m[r] >= -1).all()
        assert h[r] == sum(int(cont[r, k, m[r, k]]) for k in range(Kk) if m[r, k] >= 0)
    assert h[2] == 0


def test_evaluate_reports_the_matched_accuracy():
    shape, metric = R.E2E[2], "cosine"
    C, Kk = shape[0], shape[4]
    pool, yl, y, init = R.e2e_case(shape, metric)
    p = ClusterProbe(Kk, metric=metric, device="cuda").fit(dev(pool), init=dev(init))
    plain = p.evaluate(dev(yl), C)
    assert list(plain) == ["cluster_nmi", "cluster_nmi_mean", "cluster_nmi_std", "cluster_ari", "cluster_ari_mean", "cluster_ari_std",
                           "cluster_purity", "cluster_purity_mean", "cluster_purity_std", "cluster_inertia", "cluster_empty", "cluster_k",
                           "cluster_restarts", "cluster_n"] and p.match_ is None
    yl2 = yl.copy()
    yl2[:3] = [-1, C, C + 7]                                                 # three rows are not tallied
    out = p.evaluate(dev(yl2), C, matched=True, silhouette=True)
    assert list(out) == list(plain) + ["cluster_acc", "cluster_acc_mean", "cluster_acc_std", "match_", "cluster_silhouette"]
    assert out["match_"] is p.match_ and p.match_.is_cuda and tuple(p.match_.shape) == (R.E2E_STARTS, Kk)
    cont, bad = host(p.contingency), host(p.bad)
    want = np.array([100.0 * X.match(cont[r])[1] / (len(yl) - bad[r]) for r in range(R.E2E_STARTS)])
    assert (bad == 3).all() and np.array_equal(host(p.hits_), [X.match(cont[r])[1] for r in range(R.E2E_STARTS)])
    best = int(p.best_)
    assert out["cluster_acc"] == pytest.approx(want[best], rel=1e-12) and out["cluster_acc_mean"] == pytest.approx(want.mean(), rel=1e-12)
    assert out["cluster_acc_std"] == pytest.approx(want.std(ddof=1), rel=1e-9)
    assert out["cluster_acc"] <= 100.0 * out["cluster_purity"] + 1e-9        # one-to-one is never above many-to-one
    assert out["cluster_silhouette"] == float(p.silhouette())
    # K = C and a permuted perfect clustering: 100
    q = ClusterProbe(C, restarts=1, metric=metric, device="cuda").fit(dev(pool), init=dev(init[:1, :C].copy()))
    perm = np.array([2, 0, 3, 1])
    q.assign_ = dev(perm[yl][None, :].astype(np.int32))
    res = q.evaluate(dev(yl), C, matched=True)
    assert res["cluster_acc"] == 100.0 and res["cluster_acc_std"] == 0.0 and res["cluster_purity"] == 1.0
    assert host(q.match_)[0].tolist() == np.argsort(perm).tolist()
