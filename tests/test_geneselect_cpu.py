"""CPU (no device): the float64 restatement of GeneSelect (tests/geneselect_ref.py) against sklearn's RFECV / RFE over LinearSVC on the
planted set, the condition the GPU end-to-end test rests on (the importance gap at every cut), the gradient against central differences,
the size schedule and the closing report against sklearn, the declarations of the new entry points, and the refusals of GeneSelect,
the launchers and the entry points that need no device (null pointers: nothing is launched)."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest
import torch

import mirror_amd
from mirror_amd import _lib, kernels as K
from mirror_amd.geneselect import GeneSelect, size_schedule
from tests import geneselect_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(step=4, min_features=1, max_iter=1024, tol=1e-4)


def svc():
    from sklearn.svm import LinearSVC
    return LinearSVC(C=1, fit_intercept=False, dual=False, tol=1e-10, max_iter=500000)


@pytest.fixture(scope="module")
def planted_run():
    x, lab, fold = R.planted(0)
    return x, lab, fold, R.rfecv(x, lab, fold, 3, fit_intercept=False, **CFG)


# ------------------------------------------------------------------ the restatement against sklearn
def test_restatement_equals_sklearn_rfecv_and_rfe_on_the_planted_set(planted_run):
    from sklearn.feature_selection import RFE, RFECV
    from sklearn.model_selection import PredefinedSplit
    x, lab, fold, o = planted_run
    y, _, _ = R.standardize(x)
    s = RFECV(svc(), step=4, cv=PredefinedSplit(fold)).fit(y, lab)
    assert o["n_features"] == s.n_features_ == 4
    assert np.array_equal(o["support"], s.support_) and np.nonzero(s.support_)[0].tolist() == [0, 3, 5, 16]
    assert np.array_equal(o["ranking"], s.ranking_)
    assert list(s.cv_results_["n_features"]) == o["cv_results"]["n_features"]
    for k in ("mean_test_score", "split0_test_score", "split1_test_score", "split2_test_score", "split3_test_score"):
        assert np.array_equal(o["cv_results"][k], s.cv_results_[k]), k          # integer counts over the same integer: the same f64
    assert np.allclose(o["cv_results"]["std_test_score"], s.cv_results_["std_test_score"], rtol=1e-12, atol=1e-15)
    # plain RFE (no folds) down to 8
    p = R.rfecv(x, lab, None, 3, step=4, min_features=8, fit_intercept=False, max_iter=1024, tol=1e-4)
    r = RFE(svc(), n_features_to_select=8, step=4).fit(y, lab)
    assert np.array_equal(p["ranking"], r.ranking_) and np.array_equal(p["support"], r.support_)
    # the final fit is LinearSVC's on the support
    ref = svc().fit(y[:, s.support_], lab)
    assert np.abs(o["coef"][:, s.support_] - ref.coef_).max() <= 1e-3 * np.abs(ref.coef_).max()
    assert (o["coef"][:, ~s.support_] == 0).all() and (o["intercept"] == 0).all()


def test_the_importance_gap_the_device_test_rests_on(planted_run):
    """The GPU end-to-end test demands identical integer decisions of an f32 run: sound only if no cut falls between nearly equal
    importances.  Fails, never skips, when the planted set does not meet it."""
    o = planted_run[3]
    print(f"smallest relative importance gap over all jobs and rounds: {o['gap']:.3e}")
    assert o["gap"] >= 1e-3
    x, lab, fold = planted_run[:3]
    assert R.rfecv(x, lab, fold, 3, fit_intercept=True, **CFG)["gap"] >= 1e-3


def test_two_mirrored_machines_rank_as_sklearns_single_machine_on_a_binary_set():
    from sklearn.feature_selection import RFE
    x, lab, _ = R.planted(2, C=2)                                             # seeds 0 and 1 need more than 1024 iterations to agree
    y, _, _ = R.standardize(x)
    o = R.rfecv(x, lab, None, 2, step=4, min_features=8, fit_intercept=False, max_iter=1024, tol=1e-4)
    assert o["gap"] >= 1e-3
    assert np.abs(o["coef"][0] + o["coef"][1]).max() <= 1e-9 * np.abs(o["coef"]).max()     # mirror images
    r = RFE(svc(), n_features_to_select=8, step=4).fit(y, lab)
    assert r.estimator_.coef_.shape[0] == 1
    assert np.array_equal(o["ranking"], r.ranking_)


def test_gradient_against_central_differences():
    rng = np.random.default_rng(4)
    n, D, Cn, F = 30, 7, 3, 3
    y = rng.standard_normal((n, D))
    lab = rng.integers(-1, Cn + 1, n)
    fold = rng.integers(-1, F, n)
    fold[:F] = np.arange(F)
    train, _, _, _, _ = R.jobs(lab, fold, Cn)
    J = F + 1
    T = R.targets(lab, Cn)
    ntr = train.sum(1)
    r, lam = 1.0 / ntr, 1.0 / (0.7 * ntr)
    mask = (rng.random((J, D)) < 0.7).astype(np.uint8)
    W = rng.standard_normal((J, Cn, D)) * mask[:, None, :]
    b = rng.standard_normal((J, Cn))
    dW, db = R.gradient(W, b, y, T, train, r, lam, mask)
    h = 1e-6
    for _ in range(40):
        j, c, d = rng.integers(J), rng.integers(Cn), rng.integers(D)
        Wp, Wm = W.copy(), W.copy()
        Wp[j, c, d] += h
        Wm[j, c, d] -= h
        num = (R.objective(Wp, b, y, T, train, r, lam, mask)[j] - R.objective(Wm, b, y, T, train, r, lam, mask)[j]) / (2 * h)
        if mask[j, d]:
            assert abs(num - dW[j, c, d]) <= 1e-6 * max(1.0, abs(num))
        else:
            assert dW[j, c, d] == 0.0
        bp, bm = b.copy(), b.copy()
        bp[j, c] += h
        bm[j, c] -= h
        num = (R.objective(W, bp, y, T, train, r, lam, mask)[j] - R.objective(W, bm, y, T, train, r, lam, mask)[j]) / (2 * h)
        assert abs(num - db[j, c]) <= 1e-6 * max(1.0, abs(num))
    assert (R.gradient(W, b, y, T, train, r, lam, mask, fit_intercept=False)[1] == 0).all()
    # the step size is a bound: 2 rho + lambda dominates the curvature, so one plain gradient step does not raise the objective
    eta = R.step_sizes(y, mask, lam)
    f0 = R.objective(W, b, y, T, train, r, lam, mask)
    f1 = R.objective(W - eta[:, None, None] * dW, b - eta[:, None] * db, y, T, train, r, lam, mask)
    assert (f1 <= f0).all()


@pytest.mark.parametrize("D,step,min_features", [(40, 0.05, 1), (19, 0.05, 1), (40, 4, 1), (41, 7, 3)])
def test_size_schedule_is_sklearns(D, step, min_features):
    from sklearn.feature_selection import RFECV
    from sklearn.svm import LinearSVC
    rng = np.random.default_rng(D)
    x, lab = rng.standard_normal((24, D)), np.arange(24) % 2
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s = RFECV(LinearSVC(dual=False, max_iter=50), step=step, cv=2, min_features_to_select=min_features).fit(x, lab)
    want = list(s.cv_results_["n_features"])[::-1]
    assert size_schedule(D, step, min_features) == want == R.schedule(D, step, min_features)
    assert want[0] == D and want[-1] == min_features


def test_weighted_report_is_sklearns():
    from sklearn.metrics import accuracy_score, precision_recall_fscore_support
    rng = np.random.default_rng(9)
    lab = rng.integers(0, 4, 300)
    pred = np.where(rng.random(300) < 0.6, lab, rng.integers(0, 3, 300))     # class 3 is never predicted by chance alone
    conf = np.array([[((lab == a) & (pred == b)).sum() for b in range(4)] for a in range(4)])
    got = R.report(conf)
    p, r, f, _ = precision_recall_fscore_support(lab, pred, average="weighted", zero_division=0)
    assert abs(got["accuracy"] - accuracy_score(lab, pred)) <= 1e-15
    assert abs(got["precision"] - p) <= 1e-14 and abs(got["recall"] - r) <= 1e-14 and abs(got["f1"] - f) <= 1e-14
    conf[:, 2] = 0                                                            # a class that is never predicted: zero_division = 0
    assert 0 < R.report(conf)["precision"] < 1


# ------------------------------------------------------------------ declarations
NEW = {"mh_colstats": 6, "mh_standardize": 6, "mh_gsel_rowsq": 6, "mh_gsel_grad": 16, "mh_gsel_step": 17, "mh_gsel_eliminate": 11}
NEW_PLAIN = ("mh_colstats_workspace_bytes", "mh_gsel_grad_workspace_bytes", "mh_gsel_slices")


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mirror_hip.h")).read()
    lib = _lib.load()
    for name, nargs in NEW.items():
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in _lib.EXPORTS and len(_lib._SIGS[name]) == nargs and hasattr(lib, name), name
    for name in NEW_PLAIN:
        assert re.search(r"^int(64_t)? %s\(" % name, header, flags=re.M), name
        assert name in _lib.EXPORTS and name not in _lib._SIGS and hasattr(lib, name), name
    assert lib.mh_gsel_grad_workspace_bytes.restype is C.c_int64 and lib.mh_colstats_workspace_bytes.restype is C.c_int64
    assert _lib.ABI_VERSION == 123 == lib.mh_version()
    assert mirror_amd.GeneSelect is GeneSelect and "GeneSelect" in mirror_amd.__all__


def test_slices_and_workspaces_depend_on_the_shape_alone():
    lib = _lib.load()
    assert K.gsel_slices(1, 2, 1) == 1 and K.gsel_slices(300, 20, 256) == 1 and K.gsel_slices(300, 20, 257) == 2
    assert K.gsel_slices(1024, 24, 16384) == 64                               # 8 tiles x 64 slices of 256 columns
    assert K.gsel_slices(1 << 20, 128, 1 << 18) == 1                          # the tiles alone fill the device
    assert K.gsel_slices(0, 2, 1) == 0 and K.gsel_slices(1, 2, (1 << 18) + 1) == 0
    assert lib.mh_gsel_grad_workspace_bytes(1024, 6, 4, 16384) == 64 * 1024 * 24 * 4
    assert lib.mh_gsel_grad_workspace_bytes(0, 6, 4, 16) == 0
    assert lib.mh_colstats_workspace_bytes(1024, 100) == 16 * 100 * 8 and lib.mh_colstats_workspace_bytes(0, 1) == 0


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kw,exc", [
    (dict(num_classes=1), ValueError), (dict(num_classes=65), ValueError), (dict(num_classes=True), ValueError),
    (dict(step=0), ValueError), (dict(step=1.0), ValueError), (dict(step=0.0), ValueError), (dict(step=True), ValueError),
    (dict(step="0.05"), ValueError), (dict(min_features=0), ValueError), (dict(min_features=1.0), ValueError),
    (dict(svm_c=0.0), ValueError), (dict(svm_c=float("inf")), ValueError), (dict(svm_c="1"), ValueError),
    (dict(max_iter=0), ValueError), (dict(tol=-1.0), ValueError), (dict(tol=float("nan")), ValueError),
    (dict(standardize=1), ValueError), (dict(fit_intercept=0), ValueError), (dict(check_every=0), ValueError),
    (dict(device="cpu"), _lib.MirrorHipError)])
def test_geneselect_refuses(kw, exc):
    args = dict(num_classes=3, device="cuda")
    args.update(kw)
    with pytest.raises(exc):
        GeneSelect(**args)


def test_fit_and_methods_refuse_before_touching_a_device():
    g = GeneSelect(3, device="cuda")
    x, lab = torch.zeros((6, 4)), torch.zeros((6,), dtype=torch.int64)
    for bad in (torch.zeros((6,)), torch.zeros((6, 4), dtype=torch.int64), [[0.0]]):
        with pytest.raises(ValueError, match="floating point"):
            g.fit(bad, lab)
    with pytest.raises(ValueError, match="labels must be"):
        g.fit(x, lab.float())
    with pytest.raises(ValueError, match="labels must be"):
        g.fit(x, lab[:5])
    with pytest.raises(ValueError, match="fold must be"):
        g.fit(x, lab, fold=torch.zeros((6,)))
    with pytest.raises(ValueError, match=r"no row of fold\(s\) \[1\]"):
        g.fit(x, lab, fold=torch.tensor([0, 0, 2, 2, -1, 0]))
    with pytest.raises(ValueError, match="every fold value is negative"):
        g.fit(x, lab, fold=torch.full((6,), -1))
    with pytest.raises(ValueError, match="min_features = 5 exceeds D = 4"):
        GeneSelect(3, min_features=5, device="cuda").fit(x, lab)
    with pytest.raises(_lib.MirrorHipError, match="2\\^18"):
        g.fit(torch.zeros((1, (1 << 18) + 1)), lab[:1])
    for call in (lambda: g.predict(x), lambda: g.selected(), lambda: g.transform(x), lambda: g.score(x, lab)):
        with pytest.raises(ValueError, match="nothing is fitted"):
            call()


def test_launchers_refuse():
    f32, u8, i32, i64 = torch.float32, torch.uint8, torch.int32, torch.int64
    n, D, J, Cn, Cp = 5, 6, 2, 3, 4
    y, W, b = torch.zeros((n, D)), torch.zeros((J, Cp, D)), torch.zeros((J, Cp))
    lab, fold, held, r = torch.zeros((n,), dtype=i64), torch.zeros((n,), dtype=i32), torch.zeros((J,), dtype=i32), torch.zeros((J,))
    mask, elim, G = torch.ones((J, D), dtype=u8), torch.zeros((J, D), dtype=i32), torch.zeros((n, J * Cp))
    lam = eta = torch.zeros((J,))
    with pytest.raises(ValueError, match="must be f32"):
        K.colstats(y.double())
    with pytest.raises(_lib.MirrorHipError, match="HIP device"):
        K.colstats(y)
    with pytest.raises(ValueError, match="mu must be f32"):
        K.standardize(y, torch.zeros((D + 1,)), torch.zeros((D,)))
    with pytest.raises(ValueError, match="rstd must be f32"):
        K.standardize(y, torch.zeros((D,)), torch.zeros((D,), dtype=torch.float64))
    with pytest.raises(ValueError, match="out must be"):
        K.standardize(y, torch.zeros((D,)), torch.zeros((D,)), out=torch.zeros((n, D + 1)))
    with pytest.raises(ValueError, match="mask must be"):
        K.gsel_rowsq(y, mask.to(i32))
    with pytest.raises(ValueError, match="mask must be"):
        K.gsel_rowsq(y, torch.ones((J, D + 1), dtype=u8))
    with pytest.raises(_lib.MirrorHipError, match="HIP device"):
        K.gsel_rowsq(y, mask)
    with pytest.raises(ValueError, match="C must be an int"):
        K.gsel_grad(y, W, b, lab, fold, held, r, 65)
    with pytest.raises(ValueError, match="weights must be f32"):
        K.gsel_grad(y, W[:, :3], b, lab, fold, held, r, Cn)
    with pytest.raises(ValueError, match="bias must be f32"):
        K.gsel_grad(y, W, b[:, :3], lab, fold, held, r, Cn)
    with pytest.raises(_lib.MirrorHipError, match="HIP device"):
        K.gsel_grad(y, W, b, lab, fold, held, r, Cn)
    with pytest.raises(ValueError, match="weights must be f32"):
        K.gsel_step(y, G, W, b, W.double(), b, lam, eta, 0.0, mask, True, Cn)
    with pytest.raises(_lib.MirrorHipError, match="HIP device"):
        K.gsel_step(y, G, W, b, W, b, lam, eta, 0.0, mask, True, Cn)
    for kw, msg in ((dict(Wz=W[:1]), "Wz must be"), (dict(mask=mask.to(i32)), "mask must be"), (dict(elim=elim.to(i64)), "elim_round must be"),
                    (dict(k=-1), "k must be"), (dict(k=True), "k must be"), (dict(rnd=-1), "round must be"), (dict(Cn=1), "C must be")):
        a = dict(Wx=W, Wz=W, mask=mask, elim=elim, k=1, rnd=0, Cn=Cn)
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            K.gsel_eliminate(a["Wx"], a["Wz"], a["mask"], a["elim"], a["k"], a["rnd"], a["Cn"])
    with pytest.raises(_lib.MirrorHipError, match="HIP device"):
        K.gsel_eliminate(W, W.clone(), mask, elim, 1, 0, Cn)


def test_entry_points_refuse_outside_their_limits():
    """MH_EINVAL with a message before anything is launched: null pointers stand in for the buffers."""
    lib = _lib.load()

    def refused(name, *args, match):
        with pytest.raises(_lib.MirrorHipError, match=match):
            _lib.call(name, *args, stream=0)

    refused("mh_colstats", None, 0, 4, None, None, None, match="n = 0")
    refused("mh_colstats", None, 4, (1 << 18) + 1, None, None, None, match="D = 262145")
    refused("mh_colstats", None, 4, 4, None, None, None, match="null pointer")
    refused("mh_standardize", None, None, None, None, 4, 0, match="D = 0")
    refused("mh_standardize", None, None, None, None, 4, 4, match="null pointer")
    refused("mh_gsel_rowsq", None, 4, 4, None, 0, None, match="J = 0")
    refused("mh_gsel_rowsq", None, 4, 4, None, 2, None, match="null pointer")
    g = lambda n, D, J, Cn, Cp: ("mh_gsel_grad", None, n, D, None, None, None, None, None, None, J, Cn, Cp, None, None, None, None)
    refused(*g(4, 4, 2, 1, 1), match="C = 1")
    refused(*g(4, 4, 2, 3, 8), match="Cp = 8")
    refused(*g(4, (1 << 18) + 1, 2, 3, 4), match="D = 262145")
    refused(*g((1 << 20) + 1, 4, 2, 3, 4), match="n = 1048577")
    refused(*g(4, 4, (1 << 18) + 1, 3, 4), match="keys")
    refused(*g(1 << 20, 4, 128, 3, 4), match="2\\^28")
    refused(*g(4, 4, 2, 3, 4), match="null pointer")
    s = lambda D, beta, fi: ("mh_gsel_step", None, 4, D, None, None, None, None, None, None, None, beta, None, fi, 2, 3, 4, None)
    refused(*s((1 << 18) + 1, 0.5, 1), match="D = 262145")
    refused(*s(4, 1.5, 1), match="beta")
    refused(*s(4, 0.5, 2), match="fit_intercept")
    refused(*s(4, 0.5, 1), match="null pointer")
    e = lambda D, k, rnd: ("mh_gsel_eliminate", None, None, None, None, 2, 3, 4, D, k, rnd, None)
    refused(*e(0, 1, 0), match="D = 0")
    refused(*e(4, -1, 0), match="k = -1")
    refused(*e(4, 1, -1), match="round = -1")
    refused(*e(4, 1, 0), match="null pointer")
    assert lib.mh_version() == 123
