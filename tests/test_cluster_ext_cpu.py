"""CPU (no GPU): the float64 restatements of tests/cluster_ext_ref.py against sklearn (silhouette), scipy (the assignment) and cases done
by hand (k-means++), the declarations of the new entry points, and the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from mirror_amd import ClusterProbe, _lib, cluster, kernels as K
from mirror_amd._lib import MirrorHipError
from tests import cluster_ext_ref as X, kmeans_ref as R


# ------------------------------------------------------------------ silhouette
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("case", X.SIL_CASES)
def test_restated_silhouette_against_sklearn(case, metric):
    from sklearn.metrics import silhouette_samples
    shape, Kk = case
    pool, lab = X.sil_case(shape, Kk)
    assert len(lab) == shape[0] * shape[2] and len(set(lab)) == Kk
    for center in (False, True):
        y, _ = R.prepare(pool, pool, metric, center)
        s, mean, bad, scale = X.silhouette(y, lab, Kk, metric)
        want = silhouette_samples(y, lab, metric=metric)
        print(f"{metric} center={center} {shape}: largest difference from sklearn {np.abs(s - want).max():.3g}, mean {mean:.6f}")
        assert bad == 0 and np.abs(s - want).max() <= 2e-7 and abs(mean - want.mean()) <= 2e-7
        assert (scale > 0).all()


def test_restated_silhouette_on_the_index_case():
    from sklearn.metrics import silhouette_samples
    y, lab, note = X.index_case()
    for metric in ("euclidean", "cosine"):
        s, mean, bad, _ = X.silhouette(y, lab, note["K"], metric)
        assert bad == 2 and np.isnan(s[list(note["outside"])]).all() and s[note["singleton"]] == 0.0
        keep = np.ones(len(lab), dtype=bool)
        keep[list(note["outside"])] = False
        assert not np.isnan(s[keep]).any() and mean == pytest.approx(s[keep].mean(), abs=1e-15)
        if metric == "euclidean":                               # the rows outside take no part as neighbours either
            want = silhouette_samples(y[keep].astype(np.float64), lab[keep], metric=metric)
            assert np.abs(s[keep] - want).max() <= 1e-12
        a, b = note["twins"]
        assert X.distances(y, "euclidean")[a, b] == 0.0
    one = np.zeros(len(lab), dtype=np.int32)
    s, mean, bad, _ = X.silhouette(y, one, 5, "euclidean")
    assert np.isnan(mean) and bad == 0 and np.isnan(s).all()


# ------------------------------------------------------------------ matching
MATCH = [(1, 1), (3, 3), (7, 5), (5, 7), (64, 64), (300, 200)]


@pytest.mark.parametrize("hi", [51, 4])
@pytest.mark.parametrize("Kk,Cc", MATCH)
def test_restated_matching_against_scipy(Kk, Cc, hi):
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(Kk * 1000 + Cc + hi)
    for cont in (rng.integers(0, hi, (Kk, Cc)), np.zeros((Kk, Cc), dtype=np.int64)):
        m, hits = X.match(cont)
        r, c = linear_sum_assignment(cont, maximize=True)
        assert hits == int(cont[r, c].sum())
        got = m[m >= 0]
        assert len(got) == min(Kk, Cc) and len(set(got)) == len(got) and (got < Cc).all()
        assert hits == sum(int(cont[k, m[k]]) for k in range(Kk) if m[k] >= 0)


# ------------------------------------------------------------------ k-means++
def test_restated_seeding_on_cases_done_by_hand():
    assert X.strips(130) == [(0, 43), (43, 86), (86, 130)] and X.strips(1) == [(0, 1)] and len(X.strips(9000)) == 128
    assert len(X.strips(8128)) == 127 and X.strips(64) == [(0, 64)]
    u = X.uniforms(5, seed=7, draw=3)
    w = [int(v) for v in R.datafeed_ref.draw_words(10, 2, 3, 7)]
    assert all(u[j] == (((w[2 * j] >> 5) << 26) | (w[2 * j + 1] >> 6)) * 2.0 ** -53 for j in range(5)) and ((0 <= u) & (u < 1)).all()
    assert not np.array_equal(u, X.uniforms(5, seed=7, draw=4))
    assert not np.array_equal(R.datafeed_ref.draw_words(10, 2, 3, 7), R.datafeed_ref.draw_words(10, 1, 3, 7))      # a stream of its own
    y = np.array([[0.0], [1.0], [3.0]])
    m = X.sqdist(y, y[0])
    assert np.array_equal(m, [0.0, 1.0, 9.0])
    assert X.pick(m, 0.0) == 1 and X.pick(m, 0.05) == 1 and X.pick(m, 0.1) == 2 and X.pick(m, 0.99) == 2
    m2 = X.min_dist(y, [0, 2])
    assert np.array_equal(m2, [0.0, 1.0, 0.0]) and X.pick(m2, 0.0) == 1 and X.pick(m2, 0.999) == 1
    # no running sum passes t (u T < T for every finite T, so this takes an infinite weight): the last row of positive weight
    top = 1.0 - 2.0 ** -53
    assert top * 3.0 < 3.0 and X.pick(np.array([1.0, 2.0, 0.0]), top) == 1
    assert X.pick(np.array([1.0, np.inf, 0.0]), 0.5) == 1 and X.pick(np.array([np.inf, 1.0, 2.0, 0.0]), 0.0) == 2
    # T = 0: fewer distinct rows than centres
    same = np.ones((10, 4))
    rows = X.kmeanspp(same, 2, 3, seed=5, offset=9)
    for r in range(2):
        uu = X.uniforms(3, 5, 9 + r)
        assert list(rows[r]) == [int(v * 10.0) for v in uu]
    two = np.zeros((10, 4))
    two[3:] = 1.0
    rows = X.kmeanspp(two, 4, 3, seed=1, offset=0)
    for r in range(4):
        uu = X.uniforms(3, 1, r)
        assert rows[r, 0] == int(uu[0] * 10.0) and (rows[r, 1] >= 3) == (rows[r, 0] < 3) and rows[r, 2] == int(uu[2] * 10.0)
    assert X.sqdist(np.array([[np.nan, 0.0], [1.0, 1.0]]), np.zeros(2)).tolist() == [0.0, 2.0]      # a NaN distance counts as 0


# ------------------------------------------------------------------ the declarations
NEW = {"mh_silhouette": 11, "mh_kmeanspp_init": 10, "mh_cluster_match": 6}


def test_the_entry_points_are_declared_and_bound_within_the_same_abi_generation():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 123 and lib.mh_version() == 123
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mirror_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in NEW.items():
        assert name in _lib.EXPORTS and len(_lib._SIGS[name]) == nargs and hasattr(lib, name), name
        decl = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.M | re.S)
        assert decl is not None, name
        params = [q for q in decl.group(1).split(",") if q.strip()]
        assert len(params) == nargs + 1 and params[-1].split()[0] == "mh_stream", (name, params)
        for q, t in zip(params, _lib._SIGS[name]):
            want = C.c_void_p if "*" in q else {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64}[q.split()[0]]
            assert t is want, (name, q, t)
    for name in ("mh_silhouette_workspace_bytes", "mh_kmeanspp_workspace_bytes"):
        assert name in _lib.EXPORTS and name not in _lib._SIGS and getattr(lib, name).restype is C.c_int64
        assert re.search(r"^int64_t\s+" + name + r"\s*\(", header, flags=re.M)
    ws = lib.mh_kmeanspp_workspace_bytes                        # m f64 [R, n] and one f64 per strip and restart
    assert ws(130, 2) == 2 * (130 + 3) * 8 and ws(1 << 20, 1) == ((1 << 20) + 128) * 8 and ws(0, 1) == 0 and ws(5, 0) == 0
    ws = lib.mh_silhouette_workspace_bytes                      # the sorted rows, S f64 [P, n, K], and 20 bytes a row; 16-byte pieces
    assert ws(128, 4, 16) == 128 * 16 * 4 + 128 * 4 * 8 + 128 * 8 + 3 * 128 * 4 + 32 and ws(0, 4, 16) == 0       # one tile: P = 1
    assert ws(300, 7, 515) == 618000 + 3 * 300 * 7 * 8 + 2400 + 3 * 1200 + 32                                    # three tiles: P = 3
    assert ws(8192, 8, 512) == 8192 * 512 * 4 + 16 * 8192 * 8 * 8 + 8192 * 8 + 3 * 8192 * 4 + 48                 # P = 16
    # the slices beyond the first stay within 64 MiB: one more at n K 8 = 64 MiB, none above
    assert ws(8192, 1024, 16) == 8192 * 16 * 4 + 2 * 8192 * 1024 * 8 + 8192 * 8 + 3 * 8192 * 4 + 4112
    assert ws(16384, 1024, 16) == 16384 * 16 * 4 + 16384 * 1024 * 8 + 16384 * 8 + 3 * 16384 * 4 + 4112
    n = 1 << 17                                                 # from here on P = 1 for every K: S is [n, K]
    assert ws(n, 8, 16) == n * 16 * 4 + n * 8 * 8 + n * 8 + 3 * n * 4 + 48


def _refused(name, match, *args):
    with pytest.raises(MirrorHipError, match=match):
        _lib.call(name, *args)


def test_entry_points_refuse_what_lies_outside_their_limits():
    """Null pointers everywhere: each call must stop in its argument check and say why, before it launches anything."""
    # mh_silhouette(y, lab, n, R, K, D, metric, sil, mean, bad, workspace)
    sil = lambda n=100, R_=2, K_=5, D=64, metric=0: ("mh_silhouette", None, None, n, R_, K_, D, metric, None, None, None, None)  # noqa: E731
    # mh_kmeanspp_init(y, n, R, K, D, seed, offset, rows, cent, workspace)
    kpp = lambda n=100, R_=2, K_=5, D=64, offset=0: ("mh_kmeanspp_init", None, n, R_, K_, D, 0, offset, None, None, None)  # noqa: E731
    for mk in (sil, kpp):
        name = mk()[0]
        _refused(name, r"K = 0 outside \[1, 1024\]", *mk(K_=0)[1:])
        _refused(name, r"K = 1025 outside \[1, 1024\]", *mk(K_=1025)[1:])
        _refused(name, r"D = 0 outside \[1, 4096\]", *mk(D=0)[1:])
        _refused(name, r"D = 4097 outside \[1, 4096\]", *mk(D=4097)[1:])
        _refused(name, "n = 0 outside", *mk(n=0)[1:])
        _refused(name, "n = 1048577 outside", *mk(n=(1 << 20) + 1)[1:])
        _refused(name, r"R = 0 outside \[1, 65535\]", *mk(R_=0)[1:])
        _refused(name, r"R = 65536 outside \[1, 65535\]", *mk(R_=65536, K_=1)[1:])
        _refused(name, "null pointer", *mk()[1:])
    _refused("mh_silhouette", "metric = 2", *sil(metric=2)[1:])
    _refused("mh_kmeanspp_init", "R = 1025 restarts of K = 1024", *kpp(R_=1025, K_=1024)[1:])
    _refused("mh_kmeanspp_init", "below 2\\^63", *kpp(offset=(1 << 63) - 1)[1:])
    # mh_cluster_match(cont, R, K, C, match, hits)
    mat = lambda R_=4, K_=3, C_=2: ("mh_cluster_match", None, R_, K_, C_, None, None)  # noqa: E731
    _refused("mh_cluster_match", r"K = 0 outside \[1, 1024\]", *mat(K_=0)[1:])
    _refused("mh_cluster_match", r"C = 1025 outside \[1, 1024\]", *mat(C_=1025)[1:])
    _refused("mh_cluster_match", r"K C = 66560 cells", *mat(K_=1024, C_=65)[1:])
    _refused("mh_cluster_match", "R = 0 outside", *mat(R_=0)[1:])
    _refused("mh_cluster_match", "null pointer", *mat()[1:])


# ------------------------------------------------------------------ the public face
def test_probe_and_launchers_check_their_arguments():
    for bad in ("kmeans", "k-means++", None, 1):
        with pytest.raises(ValueError, match="seeding must be"):
            ClusterProbe(4, seeding=bad, device="cuda")
    assert ClusterProbe(4, device="cuda").seeding == "random" and ClusterProbe(4, seeding="kmeans++", device="cuda").seeding == "kmeans++"
    p = ClusterProbe(4, device="cuda")
    for call in (lambda: p.silhouette(), lambda: p.evaluate(torch.zeros(3, dtype=torch.int64), 2, matched=True)):
        with pytest.raises(ValueError, match="nothing is fitted"):
            call()
    y, lab = torch.zeros((6, 8)), torch.zeros((2, 6), dtype=torch.int32)
    with pytest.raises(ValueError, match="must be f32"):
        K.silhouette(y.double(), lab, 3, "cosine")
    with pytest.raises(ValueError, match="metric must be"):
        K.silhouette(y, lab, 3, "l2")
    with pytest.raises(ValueError, match="lab must be int32"):
        K.silhouette(y, lab.long(), 3, "cosine")
    with pytest.raises(ValueError, match="lab must be int32"):
        K.silhouette(y, lab[:, :5], 3, "cosine")
    for bad in (0, 1025, True, 2.0):
        with pytest.raises(ValueError, match="K must be"):
            K.silhouette(y, lab, bad, "cosine")
        with pytest.raises(ValueError, match="K must be"):
            K.kmeanspp_init(y, 2, bad, 0, 0)
    with pytest.raises(MirrorHipError, match="HIP device tensors"):         # there is no CPU path
        K.silhouette(y, lab, 3, "cosine")
    with pytest.raises(ValueError, match="R must be"):
        K.kmeanspp_init(y, 0, 3, 0, 0)
    with pytest.raises(ValueError, match="seed must be"):
        K.kmeanspp_init(y, 2, 3, 1.5, 0)
    with pytest.raises(ValueError, match="draw ids"):
        K.kmeanspp_init(y, 2, 3, 0, -1)
    with pytest.raises(MirrorHipError, match="HIP device tensors"):
        K.kmeanspp_init(y, 2, 3, 0, 0)
    for bad in (torch.zeros((2, 3)), torch.zeros((2, 3, 2), dtype=torch.int64), [[0]]):
        with pytest.raises(ValueError, match="cont must be int32"):
            K.cluster_match(bad)
    with pytest.raises(MirrorHipError, match="K \\* C <= 65536"):
        K.cluster_match(torch.zeros((1, 1024, 65), dtype=torch.int32))
    with pytest.raises(MirrorHipError, match="HIP device tensors"):
        K.cluster_match(torch.zeros((1, 3, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="labels must be"):
        cluster.silhouette_score(y, lab[:, :5], 3, device="cuda")
    with pytest.raises(ValueError, match="metric must be"):
        cluster.silhouette_score(y, lab, 3, metric="l2", device="cuda")
    with pytest.raises(ValueError, match="num_clusters must be"):
        cluster.silhouette_score(y, lab, 0, device="cuda")


def test_evaluate_keeps_its_default_keys_and_checks_its_flags():
    """evaluate() on a probe whose fitted state is set by hand stops at the device check of the tally: the flags are looked at first."""
    import inspect
    sig = inspect.signature(ClusterProbe.evaluate)
    assert list(sig.parameters) == ["self", "labels", "num_classes", "matched", "silhouette"]
    assert sig.parameters["matched"].default is False and sig.parameters["silhouette"].default is False
    assert list(inspect.signature(ClusterProbe.fit).parameters) == ["self", "emb", "init"]
    assert list(inspect.signature(ClusterProbe.__init__).parameters)[-1] == "seeding"
    assert inspect.signature(ClusterProbe.__init__).parameters["seeding"].default == "random"
    p = ClusterProbe(3, restarts=2, device="cuda")
    p.centroids_ = torch.zeros((2, 3, 4))
    p.assign_ = torch.zeros((2, 5), dtype=torch.int32)
    labels = torch.zeros(5, dtype=torch.int64)
    for kw in (dict(matched=1), dict(silhouette="yes"), dict(matched=None)):
        with pytest.raises(ValueError, match="must be a bool"):
            p.evaluate(labels, 2, **kw)
    with pytest.raises(ValueError, match='restarts must be "best" or "all"'):
        p.silhouette(restarts="every")
