"""MI355X: the cluster probe (csrc/kmeans.hip, mirror_amd/cluster.py) against the float64 restatement of tests/kmeans_ref.py.

Every stage is compared on what the device itself handed to it (rows and centroids -> assignment -> centroids -> inertia -> scores), so a
stage's tolerance is that stage's own rounding.  The assignment is compared where float64 decides by more than the project's margin;
the update's sums are compared BIT FOR BIT (their order is the contract); the tally is integer arithmetic.  The end-to-end test runs on
inputs that tests/test_cluster_cpu.py shows to be decided at every step in float64, and there asks for the same assignment everywhere.

The update is compared BIT FOR BIT for both metrics: the mean is summed in ascending row order in f64 and rounded to f32 once; |c|^2 of
the rounded mean is added in the order the header states (per thread over its columns, the butterfly, the four waves), which
tests/kmeans_ref.py restates (device_sumsq), so the cosine quotient and the bias are the same f64 numbers, rounded once.

Inertia "non-increasing" is asserted as it reads, without slack: the inputs are decided at every step, a mean minimises its cluster's
sum, and rounding that mean to f32 moves the sum in second order only (1e-14 of itself), far below the decrease of any step that
changes a row; steps that change nothing repeat the same bits."""
import functools

import numpy as np
import pytest
import torch

from mirror_amd import ClusterProbe, kernels as K
from tests import datafeed_ref, kmeans_ref as R

pytestmark = pytest.mark.gpu

METRICS = ["euclidean", "cosine"]


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()       # a copy: the shared inputs are read-only


def host(t):
    return t.detach().cpu().numpy()


def unit(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def ulp32(a):
    return np.spacing(np.abs(np.asarray(a, dtype=np.float32))).astype(np.float64)


# ------------------------------------------------------------------ 1. assignment
#             (n,   K,   D,  R)
ASSIGN = [(130, 3, 24, 1),         # a row-tile edge, one key tile, D = 16 + 8: a remainder of the K step
          (300, 129, 515, 3),      # two key tiles (the second holds one key), a D that is no multiple of 4: scalar loads
          (257, 300, 512, 2)]      # three row tiles, three key tiles


def assign_inputs(n, Kk, D, Rr):
    """Unit rows and centroids of norm 0.5 .. 1 (so that the euclidean bias moves the decision), f32."""
    rng = np.random.default_rng(n + Kk + D)
    x = unit(rng.standard_normal((n, D))).astype(np.float32)
    cent = (unit(rng.standard_normal((Rr * Kk, D))) * rng.uniform(0.5, 1.0, (Rr * Kk, 1))).reshape(Rr, Kk, D).astype(np.float32)
    return x, cent


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,Kk,D,Rr", ASSIGN)
def test_assignment_against_float64_scores(metric, n, Kk, D, Rr):
    x, cent = assign_inputs(n, Kk, D, Rr)
    xd, cd = dev(x), dev(cent)
    bias = K.kmeans_bias(cd) if metric == "euclidean" else None
    got, score = K.kmeans_assign(xd, cd, bias, want_score=True)
    assert got.dtype == torch.int32 and tuple(got.shape) == (Rr, n) and score.dtype == torch.float32 and tuple(score.shape) == (Rr, n)
    again, none = K.kmeans_assign(xd, cd, bias)
    assert torch.equal(again, got) and none is None
    b64 = host(bias).astype(np.float64) if bias is not None else np.zeros((Rr, Kk))
    if bias is not None:                                                          # the bias itself: f64 sums, rounded once
        want_b = R.bias_of(cent, "euclidean")
        assert (np.abs(b64 - want_b) <= ulp32(want_b)).all()
    S = R.scores(x, cent, b64)
    want = R.assign_step(S)
    margin = R.margin_of(x, cent, b64, metric)
    decided = R.top_two_gap(S) > margin
    g = host(got).astype(np.int64)
    print(f"{metric} {(n, Kk, D, Rr)}: {decided.mean():.4f} decided, {(g != want)[decided].sum()} of them differ, {(g != want).sum()} differ at all")
    assert (g >= 0).all() and (g < Kk).all()
    assert decided.mean() >= 0.99
    assert np.array_equal(g[decided], want[decided])
    # the winning value is the score of the chosen centroid, to the margin
    chosen = np.take_along_axis(S, g[:, :, None], axis=2)[:, :, 0]
    assert (np.abs(host(score) - chosen) <= margin).all()


@pytest.mark.parametrize("metric", METRICS)
def test_ties_go_to_the_smaller_centroid_across_key_tiles(metric):
    """Small integers: every product, bias and score is exact in f32 and in f64, so the comparison needs no margin.  Centroids 5 (first
    key tile) and 200 (second) are the same vector of +-2, the largest norm there is: a row equal to it scores highest on exactly these."""
    n, Kk, D, Rr = 130, 257, 24, 2
    rng = np.random.default_rng(12)
    cent = rng.integers(-2, 3, (Rr, Kk, D)).astype(np.float32)
    twos = (2 * rng.choice([-1, 1], D)).astype(np.float32)
    cent[:, 5] = cent[:, 200] = twos
    x = rng.integers(-2, 3, (n, D)).astype(np.float32)
    x[::2] = twos
    cd = dev(cent)
    bias = K.kmeans_bias(cd) if metric == "euclidean" else None
    b64 = host(bias).astype(np.float64) if bias is not None else np.zeros((Rr, Kk))
    assert np.array_equal(b64, R.bias_of(cent, metric))                            # exact
    got = host(K.kmeans_assign(dev(x), cd, bias)[0]).astype(np.int64)
    assert (got[:, ::2] == 5).all() and (got != 200).all()
    assert np.array_equal(got, R.assign_step(R.scores(x, cent, b64)))


@pytest.mark.parametrize("metric", METRICS)
def test_nan_is_never_chosen_and_a_nan_row_has_no_cluster(metric):
    n, Kk, D, Rr = 300, 129, 515, 3
    x, cent = assign_inputs(n, Kk, D, Rr)
    x, cent = x.copy(), cent.copy()
    clean = host(K.kmeans_assign(dev(x), dev(cent), K.kmeans_bias(dev(cent)) if metric == "euclidean" else None)[0])
    k0, k1 = int(clean[0, 0]), int(clean[2, 1])                                    # winners of the clean run: poison them
    cent[0, k0, 3] = np.nan
    cent[2, k1, 514] = np.nan
    cent[1, 128] = np.nan                                                          # the lone key of the second tile
    x[7, 0] = np.nan
    cd = dev(cent)
    bias = K.kmeans_bias(cd) if metric == "euclidean" else None
    got, score = K.kmeans_assign(dev(x), cd, bias, want_score=True)
    g, s = host(got), host(score)
    rows = np.arange(n) != 7
    assert (g[:, 7] == -1).all() and np.isnan(s[:, 7]).all()
    assert (g[:, rows] >= 0).all() and not np.isnan(s[:, rows]).any()
    assert (g[0] != k0).all() and (g[2] != k1).all() and (g[1] != 128).all()
    untouched = (clean != np.array([k0, 128, k1])[:, None]) & rows[None, :]
    assert np.array_equal(g[untouched], clean[untouched])


def test_changed_counts_the_differences_from_prev_also_in_place():
    n, Kk, D, Rr = 300, 129, 515, 3
    x, cent = assign_inputs(n, Kk, D, Rr)
    xd, cd = dev(x), dev(cent)
    base, _ = K.kmeans_assign(xd, cd)
    rng = np.random.default_rng(4)
    prev = host(base).copy()
    for r, m in enumerate((0, 1, 77)):                                             # no difference, one, many (in more than one row tile)
        idx = rng.choice(n, m, replace=False)
        prev[r, idx] = (prev[r, idx] + 1) % Kk
    want = (prev != host(base)).sum(1)
    assert list(want) == [0, 1, 77]
    changed = torch.zeros(Rr, device="cuda", dtype=torch.int32)
    got, _ = K.kmeans_assign(xd, cd, prev=dev(prev), changed=changed)
    assert torch.equal(got, base) and np.array_equal(host(changed), want)
    K.kmeans_assign(xd, cd, prev=dev(prev), changed=changed)                       # it is added to, not stored
    assert np.array_equal(host(changed), 2 * want)
    buf, changed = dev(prev), torch.zeros(Rr, device="cuda", dtype=torch.int32)
    out, _ = K.kmeans_assign(xd, cd, prev=buf, changed=changed, out=buf)           # prev is assign itself
    assert out is buf and torch.equal(buf, base) and np.array_equal(host(changed), want)


# ------------------------------------------------------------------ 2. update, bias and inertia
UPD_N, UPD_K, UPD_R = 1000, 7, 2
UPD_SIZES = [700, 1, 0, 75, 75, 75, 74]                                            # a cluster over two 256-row chunks, a single row, none


def update_inputs(D, metric):
    """Well separated groups (0.05 noise around unit centres), shuffled; restart 1 has the centroids in another order."""
    rng = np.random.default_rng(D)
    centres = unit(rng.standard_normal((UPD_K, D)))
    yl = rng.permutation(np.repeat(np.arange(UPD_K), UPD_SIZES))
    x = centres[yl] + 0.05 * rng.standard_normal((UPD_N, D)) / np.sqrt(D)
    if metric == "cosine":
        x = unit(x)
    cent = np.stack([centres, centres[::-1]]) + 0.01 * rng.standard_normal((UPD_R, UPD_K, D)) / np.sqrt(D)
    return x.astype(np.float32), cent.astype(np.float32), yl


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("D", [24, 515])
def test_update_bit_for_bit_against_the_sequential_float64_sums(metric, D):
    x, cent, yl = update_inputs(D, metric)
    xd, cd = dev(x), dev(cent)
    euclid = metric == "euclidean"
    bias = K.kmeans_bias(cd) if euclid else None
    assign, _ = K.kmeans_assign(xd, cd, bias)
    a = host(assign).astype(np.int64)
    assert np.array_equal(a[0], yl) and np.array_equal(a[1], UPD_K - 1 - yl)        # the groups, as constructed
    b0 = host(bias).astype(np.float64) if euclid else np.zeros((UPD_R, UPD_K))
    want_c, want_b, want_n = R.update_step(x, a, cent, b0, metric, f32=True)
    count = K.kmeans_update(xd, assign, cd, bias, metric)                          # cd and bias in place
    got_c, got_n = host(cd), host(count)
    assert count.dtype == torch.int32 and np.array_equal(got_n, want_n)
    assert np.array_equal(got_n[0], UPD_SIZES) and np.array_equal(got_n[1], UPD_SIZES[::-1])
    differ = int((got_c != want_c.astype(np.float32)).sum())
    print(f"{metric} D = {D}: {differ} of {got_c.size} centroid elements are not identical")
    assert differ == 0                                                             # bit for bit, both metrics
    single = int(np.flatnonzero(yl == 1)[0])                                       # one member: that row (a unit f32 row of these inputs
    assert np.array_equal(got_c[0, 1], x[single]) and np.array_equal(got_c[1, UPD_K - 2], x[single])      # normalises to itself)
    if euclid:
        got_b = host(bias).astype(np.float64)
        exact_b = -0.5 * (got_c.astype(np.float64) ** 2).sum(2)
        assert (np.abs(got_b - exact_b) <= ulp32(exact_b)).all()                   # within one f32 ulp of the f64 value
        assert np.array_equal(got_b, want_b)                                       # and the bits of the stated order
        assert torch.equal(K.kmeans_bias(cd), bias)                                # the stand-alone bias repeats the update's bits
        assert np.array_equal(got_b[0, 2], b0[0, 2]) and np.array_equal(got_b[1, UPD_K - 3], b0[1, UPD_K - 3])
    else:
        filled = got_n > 0
        assert np.abs(np.linalg.norm(got_c.astype(np.float64), axis=2)[filled] - 1).max() <= 1e-6
    assert np.array_equal(got_c[0, 2], cent[0, 2]) and np.array_equal(got_c[1, UPD_K - 3], cent[1, UPD_K - 3])   # empty: unchanged
    # the same assignment again: the same bits (a converged restart is a fixed point)
    before = cd.clone()
    K.kmeans_update(xd, assign, cd, bias, metric)
    assert torch.equal(cd, before)
    # rows without a cluster belong to none
    a2 = a.copy()
    a2[0, np.flatnonzero(yl == 0)[:300]] = -1
    a2[1, :10] = UPD_K + 3
    c2 = dev(cent)
    n2 = K.kmeans_update(xd, dev(a2.astype(np.int32)), c2, K.kmeans_bias(c2) if euclid else None, metric)
    w2_c, _, w2_n = R.update_step(x, np.where((a2 < 0) | (a2 >= UPD_K), -1, a2), cent, b0, metric, f32=True)
    assert np.array_equal(host(n2), w2_n) and host(n2)[0, 0] == 400
    assert np.array_equal(host(c2), w2_c.astype(np.float32))


@pytest.mark.parametrize("D", [24, 515])
def test_inertia_against_float64(D):
    x, cent, yl = update_inputs(D, "euclidean")
    a = np.stack([yl, UPD_K - 1 - yl]).astype(np.int32)
    a[0, [0, 500, 999]] = -1                                                        # rows without a cluster add nothing
    a[1, 3] = UPD_K
    got = host(K.kmeans_inertia(dev(x), dev(cent), dev(a)))
    want = R.inertia(x, cent, a)
    print(f"D = {D}: inertia {got}, relative error {np.abs(got - want) / want}")
    assert got.dtype == np.float64 and (np.abs(got - want) <= 1e-10 * want).all()
    assert np.array_equal(host(K.kmeans_inertia(dev(x), dev(cent), dev(a))), got)


# ------------------------------------------------------------------ 3. tally
@pytest.mark.parametrize("Kk,Cc,n", [(129, 64, 3000), (3, 2, 200)])
def test_tally_is_exact_and_scores_are_sklearns(Kk, Cc, n):
    from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score
    rng = np.random.default_rng(Kk)
    labels = rng.integers(0, Cc, n).astype(np.int64)
    a = np.stack([np.where(rng.random(n) < 0.7, labels % Kk, rng.integers(0, Kk, n)),      # agrees with the labels
                  rng.integers(0, Kk, n),                                                   # does not
                  np.zeros(n, dtype=np.int64),                                              # one cluster: NMI 0, ARI 0
                  labels % Kk]).astype(np.int32)
    labels[[0, 1, 2]] = [-1, Cc, 1 << 40]                                          # rows that are left out
    a[:, 5] = -1
    a[1, 6] = Kk
    cont, bad, summary = K.kmeans_tally(dev(a), dev(labels), Kk, Cc)
    assert cont.dtype == torch.int32 and tuple(cont.shape) == (4, Kk, Cc) and summary.dtype == torch.float64
    want_cont, want_bad, want = R.tally(a, labels, Kk, Cc)
    assert np.array_equal(host(cont), want_cont) and np.array_equal(host(bad), want_bad) and list(want_bad) == [4, 5, 4, 4]
    got = host(summary)
    for r in range(4):
        keep = (labels >= 0) & (labels < Cc) & (a[r] >= 0) & (a[r] < Kk)
        sk = [normalized_mutual_info_score(labels[keep], a[r][keep]), adjusted_rand_score(labels[keep], a[r][keep]),
              want_cont[r].max(1).sum() / keep.sum()]
        print(f"K = {Kk} C = {Cc} restart {r}: {got[r]}, against sklearn {np.abs(got[r] - sk)}")
        assert (np.abs(got[r] - sk) <= 1e-12).all() and (np.abs(got[r] - want[r]) <= 1e-12).all()
    assert got[2, 0] == 0.0 and abs(got[2, 1]) <= 1e-12
    # neither side splits the rows: 1, 1, 1
    one = K.kmeans_tally(dev(np.zeros((1, n), dtype=np.int32)), dev(np.zeros(n, dtype=np.int64)), Kk, Cc)[2]
    assert np.array_equal(host(one), [[1.0, 1.0, 1.0]])
    again = K.kmeans_tally(dev(a), dev(labels), Kk, Cc)
    assert torch.equal(again[0], cont) and torch.equal(again[2], summary)


# ------------------------------------------------------------------ 4. end to end
@functools.lru_cache(maxsize=None)
def e2e_reference(shape, metric):
    """The float64 run from the raw embeddings, once per input."""
    pool, yl, y, init = R.e2e_case(shape, metric)
    return pool, yl, y, init, R.lloyd(y, init.astype(np.float64), metric)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", R.E2E)
def test_fit_end_to_end_against_float64(shape, metric):
    Kk = shape[4]
    pool, yl, y, init, L = e2e_reference(shape, metric)
    p = ClusterProbe(Kk, restarts=1, metric=metric, device="cuda").fit(dev(pool), init=dev(init))
    assert tuple(p.centroids_.shape) == (R.E2E_STARTS, Kk, shape[1]) and p.assign_.dtype == torch.int32 and p.inertia_.dtype == torch.float64
    got_inertia = host(p.inertia_)
    print(f"{metric} {shape}: n_iter {host(p.n_iter_)} (float64 {L['n_iter']}), inertia {got_inertia}, "
          f"relative to float64 {np.abs(got_inertia - L['inertia']) / L['inertia']}")
    assert np.array_equal(host(p.assign_), L["assign"])
    assert np.array_equal(host(p.n_iter_), L["n_iter"])
    assert np.array_equal(host(p.counts_), L["count"])
    assert (np.abs(got_inertia - L["inertia"]) <= 1e-5 * L["inertia"]).all()
    assert int(p.best_) == int(np.argmin(got_inertia)) and torch.equal(p.labels_, p.assign_[int(p.best_)])
    assert tuple(p.changed_.shape)[1] == R.E2E_STARTS and p.changed_.dtype == torch.int32
    assert (host(p.changed_)[0] == len(yl)).all() and not host(p.changed_)[-1].any()      # every row is new in step 1, none in the last
    # one further assign + update leaves the centroids bit-identical
    cent, bias = p.centroids_.clone(), None if p.bias_ is None else p.bias_.clone()
    a2, _ = K.kmeans_assign(p._y, cent, bias)
    K.kmeans_update(p._y, a2, cent, bias, metric)
    assert torch.equal(a2, p.assign_) and torch.equal(cent, p.centroids_) and (bias is None or torch.equal(bias, p.bias_))
    # further rows: the pool itself falls where fit left it
    assert torch.equal(p.predict(dev(pool)), p.labels_)
    assert torch.equal(p.assign(dev(pool), p.centroids_), p.assign_)
    if metric == "euclidean":
        # inertia never grows from one step to the next: every prefix of the run, by max_iter (no slack: see the module docstring)
        steps = int(L["n_iter"].max())
        trace = np.stack([host(ClusterProbe(Kk, max_iter=t, metric=metric, device="cuda").fit(dev(pool), init=dev(init)).inertia_)
                          for t in range(1, steps + 1)])
        assert (trace[1:] <= trace[:-1]).all() and np.array_equal(trace[-1], got_inertia)
        assert (trace[0] > trace[-1]).any()


def test_drawn_start_is_the_data_feed_draw_and_repeats():
    shape = R.E2E[0]
    pool, yl = R.clusters(*shape[:4], seed=3)
    n, Kk, Rr, seed, offset = len(yl), shape[4], 6, 77, (3 << 32) + 5
    mk = lambda off: ClusterProbe(Kk, restarts=Rr, metric="euclidean", seed=seed, offset=off, device="cuda").fit(dev(pool))  # noqa: E731
    p = mk(offset)
    rows = host(p.init_rows_)
    assert p.init_rows_.dtype == torch.int64 and rows.shape == (Rr, Kk)
    for r in range(Rr):
        assert np.array_equal(rows[r], datafeed_ref.sample_local(n, Kk, seed, offset + r)) and len(set(rows[r])) == Kk      # bit for bit
    assert np.array_equal(rows, R.drawn_rows(n, Kk, Rr, seed, offset))
    q = mk(offset)
    assert torch.equal(q.assign_, p.assign_) and torch.equal(q.centroids_, p.centroids_) and torch.equal(q.inertia_, p.inertia_)
    other = mk(offset + 1)
    assert np.array_equal(host(other.init_rows_)[:-1], rows[1:])                   # restart r of one draw is restart r + 1 of the other
    # the start is those rows of the prepared pool: an explicit start of the same rows runs the same
    explicit = ClusterProbe(Kk, metric="euclidean", device="cuda").fit(dev(pool), init=p._y[p.init_rows_])
    assert torch.equal(explicit.assign_, p.assign_) and torch.equal(explicit.n_iter_, p.n_iter_)
    with pytest.raises(ValueError, match="cannot be drawn"):
        ClusterProbe(n + 1, restarts=1, device="cuda").fit(dev(pool))


@pytest.mark.parametrize("metric,center", [("euclidean", False), ("cosine", False), ("euclidean", True)])
def test_preparation_of_every_combination(metric, center):
    pool, _ = R.clusters(3, 24, 20, 0.5, seed=9)
    p = ClusterProbe(3, restarts=2, metric=metric, center=center, device="cuda").fit(dev(pool))
    want, mu = R.prepare(pool, pool, metric, center)
    assert (p.mu_ is None) == (not center)
    if metric == "euclidean" and not center:
        assert np.array_equal(host(p._y), pool)                                    # the rows as they are
    else:
        assert np.abs(host(p._y) - want).max() <= 2e-6                             # f32 rounding of unit rows (tests/test_fewshot_gpu.py)


def test_evaluate_against_the_restatement():
    shape, metric = R.E2E[2], "cosine"
    C, Kk = shape[0], shape[4]
    pool, yl, y, init, L = e2e_reference(shape, metric)
    p = ClusterProbe(Kk, metric=metric, device="cuda").fit(dev(pool), init=dev(init))
    out = p.evaluate(dev(yl), C)
    assert np.array_equal(host(p.assign_), L["assign"])
    cont, bad, summary = R.tally(L["assign"], yl, Kk, C)
    assert np.array_equal(host(p.contingency), cont) and not host(p.bad).any() and tuple(p.per_restart.shape) == (R.E2E_STARTS, 3)
    assert (np.abs(host(p.per_restart) - summary) <= 1e-12).all()
    best = int(np.argmin(L["inertia"]))
    assert int(p.best_) == best
    rep = R.report(summary, best, L["inertia"][best], (L["count"][best] == 0).sum(), Kk, len(yl))
    assert list(out) == ["cluster_nmi", "cluster_nmi_mean", "cluster_nmi_std", "cluster_ari", "cluster_ari_mean", "cluster_ari_std",
                         "cluster_purity", "cluster_purity_mean", "cluster_purity_std", "cluster_inertia", "cluster_empty", "cluster_k",
                         "cluster_restarts", "cluster_n"]
    for k, v in rep.items():
        tol = 1e-5 if k == "cluster_inertia" else 1e-9                             # the inertia carries the f32 preparation, as above
        assert out[k] == pytest.approx(v, rel=tol, abs=1e-12), k
    assert out["cluster_nmi_std"] > 0 and 0.5 < out["cluster_nmi"] < 0.9 and out["cluster_restarts"] == R.E2E_STARTS
    # int32 labels, and labels outside the classes
    yl2 = yl.copy()
    yl2[:3] = [-1, C, C + 7]
    p.evaluate(dev(yl2.astype(np.int32)), C)
    cont2, bad2, summary2 = R.tally(L["assign"], yl2, Kk, C)
    assert np.array_equal(host(p.contingency), cont2) and np.array_equal(host(p.bad), bad2) and (bad2 == 3).all()
    assert (np.abs(host(p.per_restart) - summary2) <= 1e-12).all()
    for bad_labels in (dev(yl)[:-1], dev(yl).float()):
        with pytest.raises(ValueError, match="labels must be"):
            p.evaluate(bad_labels, C)
    with pytest.raises(ValueError, match="num_classes must be"):
        p.evaluate(dev(yl), 0)
