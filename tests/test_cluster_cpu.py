"""CPU (no GPU): the float64 restatement of the cluster probe (tests/kmeans_ref.py) against sklearn (NMI, ARI, Lloyd's iteration), the
input conditions of the end-to-end GPU test from float64 alone, the declarations of the new entry points, and the refusals of
ClusterProbe, the launchers and the entry points that need no device (null pointers: nothing is launched)."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import mirror_amd
from mirror_amd import ClusterProbe, _lib, kernels as K
from mirror_amd._lib import MirrorHipError
from tests import kmeans_ref as R


# ------------------------------------------------------------------ the scores
def _sk(labels, clusters):
    from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score
    return normalized_mutual_info_score(labels, clusters), adjusted_rand_score(labels, clusters)


def _check_scores(clusters, labels, Kk, Cc):
    cont, bad, summary = R.tally(clusters[None, :], labels, Kk, Cc)
    assert not bad.any() and cont.sum() == len(labels)
    nmi, ari = _sk(labels, clusters)
    assert abs(summary[0, 0] - nmi) <= 1e-12 and abs(summary[0, 1] - ari) <= 1e-12, (summary[0], nmi, ari)
    return summary[0]


def test_restated_scores_against_sklearn():
    rng = np.random.default_rng(5)
    for Kk, Cc, n, agree in ((3, 2, 200, 0.8), (129, 64, 3000, 0.5), (7, 7, 500, 0.0), (12, 4, 300, 0.95)):
        labels = rng.integers(0, Cc, n)
        clusters = np.where(rng.random(n) < agree, labels % Kk, rng.integers(0, Kk, n))
        s = _check_scores(clusters, labels, Kk, Cc)
        cont = R.contingency(clusters[None, :], labels, Kk, Cc)[0][0]
        assert s[2] == cont.max(1).sum() / n and 0 < s[2] <= 1


def test_restated_scores_on_the_degenerate_partitions():
    n = 40
    one, many, single = np.zeros(n, dtype=np.int64), np.arange(n) % 4, np.arange(n)
    assert tuple(_check_scores(one, one, 3, 2)) == (1.0, 1.0, 1.0)                 # neither side splits the rows
    s = _check_scores(one, many, 3, 4)                                             # one cluster, four classes
    assert s[0] == 0.0 and s[1] == 0.0 and s[2] == 0.25
    s = _check_scores(many, one, 4, 1)                                             # four clusters, one class
    assert s[0] == 0.0 and s[1] == 0.0 and s[2] == 1.0
    s = _check_scores(single, single, n, n)                                        # all singletons on both sides
    assert abs(s[0] - 1.0) <= 1e-12 and s[1] == 1.0 and s[2] == 1.0
    s = _check_scores(single, many, n, 4)                                          # singletons against classes
    assert s[1] == 0.0 and s[2] == 1.0
    # rows outside either range are left out, and the scores are those of the rest
    clusters, labels = many.copy(), (np.arange(n) % 3).astype(np.int64)
    clusters[[0, 1]], labels[[2, 3]] = [-1, 4], [-1, 3]
    cont, bad, summary = R.tally(clusters[None, :], labels, 4, 3)
    assert bad[0] == 4 and cont.sum() == n - 4
    nmi, ari = _sk(labels[4:], clusters[4:])
    assert abs(summary[0, 0] - nmi) <= 1e-12 and abs(summary[0, 1] - ari) <= 1e-12


def test_restated_steps_on_a_hand_worked_example():
    y = np.array([[1, 0], [0, 1], [-1, 0], [0, -1], [np.nan, 0]], dtype=np.float64)
    cent = np.array([[[1, 0], [0, 1], [1, 0]]], dtype=np.float64)                   # centroids 0 and 2 coincide
    bias = R.bias_of(cent, "euclidean")
    assert np.array_equal(bias, [[-.5, -.5, -.5]])
    a = R.assign_step(R.scores(y, cent, bias))
    assert np.array_equal(a, [[0, 1, 1, 0, -1]])                                    # ties to the smaller k; the NaN row has no cluster
    c2, b2, cnt = R.update_step(y, a, cent, bias, "euclidean")
    assert np.array_equal(cnt, [[2, 2, 0]]) and np.array_equal(c2[0], [[.5, -.5], [-.5, .5], [1, 0]])     # the empty cluster is kept
    assert np.array_equal(b2, [[-.25, -.25, -.5]])
    c3, b3, _ = R.update_step(y, a, cent, np.zeros((1, 3)), "cosine")
    h = 1 / np.sqrt(2.0)
    assert np.allclose(c3[0, :2], [[h, -h], [-h, h]], rtol=0, atol=1e-15) and not b3.any()
    assert R.inertia(y, c2, a)[0] == 4 * 0.5
    big = np.array([[1e8], [1.0], [-1e8], [1.0]])                                   # row order matters in f32 rounding, not in the sum
    c4, _, _ = R.update_step(big, np.zeros((1, 4), dtype=np.int64), np.zeros((1, 1, 1)), np.zeros((1, 1)), "euclidean", f32=True)
    assert c4[0, 0, 0] == 0.5


# ------------------------------------------------------------------ Lloyd's iteration on the end-to-end inputs
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("shape", R.E2E)
def test_lloyd_on_the_end_to_end_inputs_is_decided_and_is_sklearns(shape, metric):
    from sklearn.cluster import KMeans
    Kk = shape[4]
    pool, yl, y, init = R.e2e_case(shape, metric)
    L = R.lloyd(y, init.astype(np.float64), metric)
    assert (L["n_iter"] < 100).all() and (L["n_iter"] >= 2).all()
    for r in range(R.E2E_STARTS):
        assert len(L["undecided"][r]) == L["n_iter"][r] and max(L["undecided"][r]) == 0.0      # no undecided row in any iteration
        assert not (L["count"][r] == 0).any()                                       # no empty cluster: sklearn would relocate it
        if metric == "euclidean":
            tr = L["trace"][r]
            assert all(b <= a * (1 + 1e-12) for a, b in zip(tr, tr[1:]))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                km = KMeans(n_clusters=Kk, init=init[r].astype(np.float64), n_init=1, algorithm="lloyd", tol=0, max_iter=100).fit(y)
            assert np.array_equal(km.labels_, L["assign"][r]) and km.n_iter_ == L["n_iter"][r]
            assert abs(km.inertia_ - L["inertia"][r]) <= 1e-9 * L["inertia"][r]
    assert L["inertia"].argmin() == np.argmin(L["inertia"])


def test_drawn_rows_are_the_data_feed_draw():
    from tests import datafeed_ref
    rows = R.drawn_rows(50, 7, 3, seed=11, offset=5)
    assert rows.shape == (3, 7)
    for r in range(3):
        assert np.array_equal(rows[r], datafeed_ref.sample_local(50, 7, 11, 5 + r)) and len(set(rows[r])) == 7


# ------------------------------------------------------------------ the public face
def test_probe_is_exported_and_checks_its_arguments():
    assert mirror_amd.ClusterProbe is ClusterProbe and "ClusterProbe" in mirror_amd.__all__
    for kw in (dict(num_clusters=0), dict(num_clusters=1025), dict(num_clusters=True), dict(num_clusters=4, restarts=0),
               dict(num_clusters=4, restarts=65536), dict(num_clusters=1024, restarts=1025), dict(num_clusters=4, max_iter=0),
               dict(num_clusters=4, metric="l2"), dict(num_clusters=4, seed=1.5), dict(num_clusters=4, offset=-1)):
        with pytest.raises(ValueError):
            ClusterProbe(device="cuda", **kw)
    with pytest.raises(MirrorHipError, match="HIP device"):
        ClusterProbe(4, device="cpu")
    p = ClusterProbe(4, restarts=3, max_iter=7, metric="euclidean", center=False, seed=3, offset=9, device="cuda")
    assert (p.num_clusters, p.restarts, p.max_iter, p.metric, p.center, p.seed, p.offset) == (4, 3, 7, "euclidean", False, 3, 9)
    d = ClusterProbe(3, device="cuda")
    assert (d.restarts, d.max_iter, d.metric, d.center, d.seed, d.offset) == (16, 100, "cosine", True, 0, 0)
    for bad in (torch.zeros((3, 2), dtype=torch.int64), torch.zeros(3), [[0.0]]):
        with pytest.raises(ValueError, match="emb must be"):
            p.fit(bad)
    with pytest.raises(MirrorHipError, match=r"D = 4097"):
        p.fit(torch.zeros((3, 4097)))
    with pytest.raises(ValueError, match="cannot be drawn from 3 rows"):
        p.fit(torch.zeros((3, 2)))                                                  # K > n without init
    for bad in (torch.zeros((1, 4, 3)), torch.zeros((1, 5, 2)), torch.zeros((4, 2)), torch.zeros((1, 4, 2), dtype=torch.float64), [[0.0]]):
        with pytest.raises(ValueError, match="init must be"):
            p.fit(torch.zeros((3, 2)), init=bad)
    with pytest.raises(MirrorHipError, match="R = 0 restarts"):
        p.fit(torch.zeros((3, 2)), init=torch.zeros((0, 4, 2)))
    for call in (lambda: p.predict(torch.zeros((3, 2))), lambda: p.assign(torch.zeros((3, 2)), torch.zeros((1, 4, 2))),
                 lambda: p.evaluate(torch.zeros(3, dtype=torch.int64), 2)):
        with pytest.raises(ValueError, match="nothing is fitted"):
            call()


def test_launchers_check_before_they_launch():
    x, cent = torch.zeros((6, 8)), torch.zeros((2, 3, 8))
    a = torch.zeros((2, 6), dtype=torch.int32)
    for fn in (lambda t: K.kmeans_assign(t, cent), lambda t: K.kmeans_update(t, a, cent, None, "cosine"), lambda t: K.kmeans_inertia(t, cent, a)):
        with pytest.raises(ValueError, match="must be f32"):
            fn(x.double())
        with pytest.raises(ValueError, match="must be f32"):
            fn(x[0])
        with pytest.raises(MirrorHipError, match="HIP device tensors"):             # there is no CPU path
            fn(x)
    for bad in (cent.double(), cent[0], torch.zeros((2, 3, 7))):
        with pytest.raises(ValueError, match="cent must be f32"):
            K.kmeans_assign(x, bad)
    with pytest.raises(MirrorHipError, match=r"K = 1025"):
        K.kmeans_assign(x, torch.zeros((1, 1025, 8)))
    with pytest.raises(MirrorHipError, match=r"R = 0"):
        K.kmeans_assign(x, torch.zeros((0, 3, 8)))
    with pytest.raises(ValueError, match="bias must be f32"):
        K.kmeans_assign(x, cent, torch.zeros((2, 4)))
    with pytest.raises(ValueError, match="prev and changed go together"):
        K.kmeans_assign(x, cent, prev=a)
    with pytest.raises(ValueError, match="prev must be int32"):
        K.kmeans_assign(x, cent, prev=a.long(), changed=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="changed must be"):
        K.kmeans_assign(x, cent, prev=a, changed=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="metric must be"):
        K.kmeans_update(x, a, cent, None, "l2")
    with pytest.raises(ValueError, match="bias goes with the euclidean"):
        K.kmeans_update(x, a, cent, None, "euclidean")
    with pytest.raises(ValueError, match="bias goes with the euclidean"):
        K.kmeans_update(x, a, cent, torch.zeros((2, 3)), "cosine")
    with pytest.raises(ValueError, match="assign must be int32"):
        K.kmeans_update(x, a[:, :5], cent, None, "cosine")
    with pytest.raises(ValueError, match="assign must be int32"):
        K.kmeans_inertia(x, cent, a.long())
    with pytest.raises(ValueError, match="cent must be f32"):
        K.kmeans_bias(cent[0])
    with pytest.raises(MirrorHipError, match="HIP device tensors"):
        K.kmeans_bias(cent)
    y = torch.zeros(6, dtype=torch.int64)
    with pytest.raises(ValueError, match="assign must be"):
        K.kmeans_tally(a.long(), y, 3, 2)
    with pytest.raises(ValueError, match="labels must be"):
        K.kmeans_tally(a, y[:5], 3, 2)
    for bad in (0, 1025, 2.0, True):
        with pytest.raises(ValueError, match="K must be"):
            K.kmeans_tally(a, y, bad, 2)
        with pytest.raises(ValueError, match="C must be"):
            K.kmeans_tally(a, y, 3, bad)
    with pytest.raises(MirrorHipError, match="65536 at the most"):
        K.kmeans_tally(a, y, 1024, 65)
    with pytest.raises(MirrorHipError, match="HIP device tensors"):
        K.kmeans_tally(a, y, 3, 2)


# ------------------------------------------------------------------ the declarations and their refusals
NEW = {"mh_kmeans_assign": 11, "mh_kmeans_update": 11, "mh_kmeans_bias": 5, "mh_kmeans_inertia": 9, "mh_kmeans_tally": 9}


def test_the_entry_points_are_declared_and_bound_within_the_same_abi_generation():
    import os
    import re
    lib = _lib.load()
    assert _lib.ABI_VERSION == 123 and lib.mh_version() == 123
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mirror_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in NEW.items():
        assert name in _lib.EXPORTS and len(_lib._SIGS[name]) == nargs and hasattr(lib, name), name
        decl = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.M | re.S)
        assert decl is not None, name
        params = [q for q in decl.group(1).split(",") if q.strip()]
        assert len(params) == nargs + 1 and params[-1].split()[0] == "mh_stream", (name, params)       # the stream comes last
        for q, t in zip(params, _lib._SIGS[name]):
            want = C.c_void_p if "*" in q else {"int": C.c_int, "int64_t": C.c_int64}[q.split()[0]]
            assert t is want, (name, q, t)
    for name in ("mh_kmeans_update_workspace_bytes", "mh_kmeans_inertia_workspace_bytes"):
        assert name in _lib.EXPORTS and name not in _lib._SIGS and getattr(lib, name).restype is C.c_int64
        assert re.search(r"^int64_t\s+" + name + r"\s*\(", header, flags=re.M)
    assert lib.mh_kmeans_update_workspace_bytes(1000, 16, 32, 512) == 0             # the members are compacted in LDS
    ws = lib.mh_kmeans_inertia_workspace_bytes                                      # one f64 per strip and restart; mh_colmean's strips
    assert ws(130, 2) == 3 * 2 * 8 and ws(1, 1) == 8 and ws(64, 5) == 5 * 8 and ws(65, 5) == 2 * 5 * 8
    assert ws(1 << 20, 16) == 128 * 16 * 8 and ws(0, 5) == 0 and ws(5, 0) == 0


def _refused(name, match, *args):
    with pytest.raises(MirrorHipError, match=match):
        _lib.call(name, *args)


def test_entry_points_refuse_what_lies_outside_their_limits():
    """Null pointers everywhere: each call must stop in its argument check with MH_EINVAL, and say why, before it launches anything."""
    # mh_kmeans_assign(x, cent, bias, n, R, K, D, prev, assign, score, changed)
    asg = lambda n=100, R_=4, K_=5, D=64: ("mh_kmeans_assign", None, None, None, n, R_, K_, D, None, None, None, None)  # noqa: E731
    # mh_kmeans_update(x, assign, n, R, K, D, metric, cent, bias, count, workspace)
    upd = lambda n=100, R_=4, K_=5, D=64, metric=0: ("mh_kmeans_update", None, None, n, R_, K_, D, metric, None, None, None, None)  # noqa: E731
    # mh_kmeans_inertia(x, cent, assign, n, R, K, D, inertia, workspace)
    ine = lambda n=100, R_=4, K_=5, D=64: ("mh_kmeans_inertia", None, None, None, n, R_, K_, D, None, None)  # noqa: E731
    for mk in (asg, upd, ine):
        name = mk()[0]
        _refused(name, r"K = 0 outside \[1, 1024\]", *mk(K_=0)[1:])
        _refused(name, r"K = 1025 outside \[1, 1024\]", *mk(K_=1025)[1:])
        _refused(name, r"D = 0 outside \[1, 4096\]", *mk(D=0)[1:])
        _refused(name, r"D = 4097 outside \[1, 4096\]", *mk(D=4097)[1:])
        _refused(name, "n = 0 outside", *mk(n=0)[1:])
        _refused(name, "n = 1048577 outside", *mk(n=(1 << 20) + 1)[1:])
        _refused(name, "R = 0 restarts", *mk(R_=0)[1:])
        _refused(name, "R = 65536 restarts", *mk(R_=65536, K_=1)[1:])
        _refused(name, r"R = 1025 restarts of K = 1024 keys", *mk(R_=1025, K_=1024)[1:])
        _refused(name, "null pointer", *mk()[1:])                                   # everything in range: the pointers are looked at last
    _refused("mh_kmeans_update", "metric = 2", *upd(metric=2)[1:])
    _refused("mh_kmeans_bias", r"K = 1025 outside", None, 1, 1025, 8, None)
    _refused("mh_kmeans_bias", r"D = 4097 outside", None, 1, 5, 4097, None)
    _refused("mh_kmeans_bias", "null pointer", None, 1, 5, 8, None)
    # mh_kmeans_tally(assign, labels, n, R, K, C, cont, bad, summary)
    tal = lambda n=10, R_=4, K_=3, C_=2: ("mh_kmeans_tally", None, None, n, R_, K_, C_, None, None, None)  # noqa: E731
    _refused("mh_kmeans_tally", r"K = 0 outside \[1, 1024\]", *tal(K_=0)[1:])
    _refused("mh_kmeans_tally", r"C = 0 outside \[1, 1024\]", *tal(C_=0)[1:])
    _refused("mh_kmeans_tally", r"C = 1025 outside \[1, 1024\]", *tal(C_=1025)[1:])
    _refused("mh_kmeans_tally", r"K C = 66560 cells", *tal(K_=1024, C_=65)[1:])
    _refused("mh_kmeans_tally", "R = 0 outside", *tal(R_=0)[1:])
    _refused("mh_kmeans_tally", "n = 0 outside", *tal(n=0)[1:])
    _refused("mh_kmeans_tally", "null pointer", *tal()[1:])
