"""CPU (no GPU): the float64 restatement of the few-shot prototype probe (tests/fewshot_ref.py) against a hand-worked example and against
sklearn, FewShotProbe's argument checks, and the MH_EINVAL refusals of the new entry points (null pointers: nothing is launched)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mirror_amd
from mirror_amd import FewShotProbe, _lib, kernels as K
from mirror_amd._lib import MirrorHipError
from tests import fewshot_ref as R


# ------------------------------------------------------------------ the hand-worked example: 2 classes, D = 2, K = 2
# pool rows (4,1) (1,4) (-2,1) (1,-2): mu = (1,1); centred (3,0) (0,3) (-3,0) (0,-3); unit e1, e2, -e1, -e2; labels 0 0 1 1
POOL = np.array([[4, 1], [1, 4], [-2, 1], [1, -2]], dtype=np.float64)
POOL_Y = np.array([0, 0, 1, 1])
# queries after preparation: e1, (1,1)/sqrt 2, -e2, NaN, -(1,1)/sqrt 2; the last label lies outside the classes
QUERY = np.array([[3, 1], [2, 2], [1, -1], [np.nan, 0], [0, 0]], dtype=np.float64)
QUERY_Y = np.array([0, 0, 1, 1, 5])
# episode 0: p = (.5,.5), -(.5,.5), bias -.25; episode 1: p = e1, e2, bias -.5 (queries 1 and 4 tie EXACTLY); episode 2: class 1 draws
# row 7, which the pool does not have: a NaN prototype
SUPPORT = np.array([[[0, 1], [2, 3]], [[0, 0], [1, 1]], [[0, 1], [2, 7]]])


def test_restatement_on_the_hand_worked_example():
    y, mu = R.prepare(POOL, POOL)
    assert np.array_equal(mu, [1.0, 1.0])
    assert np.array_equal(y, [[1, 0], [0, 1], [-1, 0], [0, -1]])
    q, _ = R.prepare(POOL, QUERY)
    h = 1 / np.sqrt(2.0)
    assert np.allclose(q[[0, 1, 2, 4]], [[1, 0], [h, h], [0, -1], [-h, -h]], rtol=0, atol=1e-15) and np.isnan(q[3]).all()
    p, bias = R.prototypes(y, SUPPORT, "euclidean")
    assert p.shape == (3, 2, 2) and R.cp_of(2) == 2 and R.cp_of(3) == 4 and R.cp_of(33) == 64 and R.cp_of(64) == 64
    assert np.array_equal(p[0], [[.5, .5], [-.5, -.5]]) and np.array_equal(bias[0], [-.25, -.25])
    assert np.array_equal(p[1], [[1, 0], [0, 1]]) and np.array_equal(bias[1], [-.5, -.5])
    assert np.array_equal(p[2, 0], [.5, .5]) and np.isnan(p[2, 1]).all() and np.isnan(bias[2, 1]) and bias[2, 0] == -.25
    S = R.scores(q, p, bias)
    assert S[0, 0, 0] == .25 and S[0, 0, 1] == -.75 and S[1, 0, 0] == .5 and S[1, 0, 1] == -.5
    assert S[1, 1, 0] == S[1, 1, 1] == h - .5 and S[1, 4, 0] == S[1, 4, 1] == -h - .5      # the exact ties
    pred = R.predict(S, 2)
    assert np.array_equal(pred, [[0, 0, 1, -1, 1],         # episode 0
                                 [0, 0, 0, -1, 0],         # episode 1: both ties go to the smaller class
                                 [0, 0, 0, -1, 0]])        # episode 2: the NaN prototype is never predicted
    gap = R.top_two_gap(S, 2)
    assert gap[1, 1] == 0 and gap[1, 4] == 0 and gap[0, 0] == 1.0 and np.isinf(gap[2]).all() and np.isinf(gap[:, 3]).all()
    conf, bad, summary = R.tally(pred, QUERY_Y, 2)
    assert np.array_equal(conf[0], [[2, 0], [0, 1]]) and np.array_equal(conf[1], [[2, 0], [1, 0]]) and np.array_equal(conf[1], conf[2])
    assert np.array_equal(bad, [2, 2, 2])                  # query 3 has no prediction, query 4 no class
    # n = (2, 2): query 3 counts for its label.  Episode 0: 3 of 4; recalls 1, 1/2; F1 1, 2 / 3.  Episode 1: 2 of 4; recalls 1, 0; F1 4 / 5, 0
    assert np.allclose(summary[0], [75.0, 75.0, 5 / 6], rtol=1e-15, atol=0)
    assert np.allclose(summary[1], [50.0, 50.0, 0.4], rtol=1e-15, atol=0) and np.array_equal(summary[1], summary[2])
    rep = R.report(summary, 2, 4)
    assert rep["fewshot_acc"] == pytest.approx(175 / 3) and rep["fewshot_acc_std"] == pytest.approx(np.sqrt(625 / 3))
    assert rep["fewshot_acc_ci95"] == pytest.approx(1.96 * np.sqrt(625 / 3) / np.sqrt(3))
    assert R.report(summary[:1], 2, 4)["fewshot_f1_std"] == 0.0 and R.report(summary[:1], 2, 4)["fewshot_f1_ci95"] == 0.0
    assert (rep["fewshot_shots"], rep["fewshot_episodes"], rep["fewshot_n"]) == (2, 3, 4)


def test_restatement_cosine_and_pads():
    y, _ = R.prepare(POOL, POOL)
    p, bias = R.prototypes(y, SUPPORT[:2], "cosine")
    h = 1 / np.sqrt(2.0)
    assert np.allclose(p[0], [[h, h], [-h, -h]], rtol=0, atol=1e-15) and np.array_equal(bias, np.zeros((2, 2)))
    sup3 = np.array([[[0, 1], [2, 3], [1, 2]]])            # three classes: Cp = 4, one pad
    p, bias = R.prototypes(y, sup3, "euclidean")
    assert p.shape == (1, 4, 2) and np.array_equal(p[0, 3], [0, 0]) and bias[0, 3] == -np.inf
    S = R.scores(np.array([[0.0, 0.0]]), p, bias)          # every class scores its bias: class 2 (p = (-.5, .5)) ties with 0 and 1
    assert R.predict(S, 3)[0, 0] == 0


def test_restatement_draw_is_the_data_feed_draw_through_the_class_runs():
    from tests import datafeed_ref
    labels = np.array([2, 0, 1, 0, 0, 2, 0, 1, 0, 0, 0])   # class sizes 7, 2, 2
    sup = R.draw(labels, 3, 3, 4, seed=11, offset=5)
    assert sup.shape == (4, 3, 3)
    runs = R.class_runs(labels, 3)
    assert [list(r) for r in runs] == [[1, 3, 4, 6, 8, 9, 10], [2, 7], [0, 5]]
    for e in range(4):
        for c in range(3):
            assert np.array_equal(sup[e, c], runs[c][datafeed_ref.sample_local(len(runs[c]), 3, 11, 5 + e * 3 + c)])
            assert set(sup[e, c]) <= set(runs[c])
        assert len(set(sup[e, 0])) == 3                    # 7 >= 3 rows: without replacement
    assert not np.array_equal(sup, R.draw(labels, 3, 3, 4, seed=11, offset=6))


def test_restatement_summary_against_sklearn():
    from sklearn.metrics import accuracy_score, balanced_accuracy_score, f1_score
    import warnings
    rng = np.random.default_rng(3)
    for C_, absent in ((5, None), (4, 2), (2, None)):
        y = rng.integers(0, C_, 200)
        pred = np.where(rng.random((6, 200)) < 0.7, y[None, :], rng.integers(0, C_, (6, 200)))
        if absent is not None:                             # a class nobody has and nobody predicts: outside both means
            y = np.where(y == absent, 0, y)
            pred = np.where(pred == absent, 1, pred)
        conf, bad, summary = R.tally(pred, y, C_)
        assert not bad.any() and conf.sum() == 6 * 200
        for e in range(6):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want = [100 * accuracy_score(y, pred[e]), 100 * balanced_accuracy_score(y, pred[e]), f1_score(y, pred[e], average="macro")]
            assert np.allclose(summary[e], want, rtol=1e-12, atol=0), (C_, e, summary[e], want)


# ------------------------------------------------------------------ the public face
def test_probe_is_exported_and_checks_its_arguments():
    assert mirror_amd.FewShotProbe is FewShotProbe and "FewShotProbe" in mirror_amd.__all__
    for kw in (dict(num_classes=1), dict(num_classes=65), dict(num_classes=True), dict(num_classes=4, shots=0), dict(num_classes=4, shots=1025),
               dict(num_classes=4, episodes=0), dict(num_classes=4, episodes=(1 << 18) + 1), dict(num_classes=4, metric="l2"),
               dict(num_classes=4, seed=1.5), dict(num_classes=4, offset=-1)):
        with pytest.raises(ValueError):
            FewShotProbe(device="cuda", **kw)
    with pytest.raises(MirrorHipError, match="HIP device"):
        FewShotProbe(4, device="cpu")
    p = FewShotProbe(4, shots=5, episodes=8, metric="cosine", seed=3, offset=9, device="cuda")
    assert (p.num_classes, p.shots, p.episodes, p.center, p.metric, p.seed, p.offset) == (4, 5, 8, True, "cosine", 3, 9)
    assert FewShotProbe(3, device="cuda").shots == 10 and FewShotProbe(3, device="cuda").episodes == 1000
    with pytest.raises(ValueError, match="emb must be"):
        p.fit(torch.zeros((3, 2), dtype=torch.int64), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="labels must be"):
        p.fit(torch.zeros((3, 2)), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="labels must be"):
        p.fit(torch.zeros((3, 2)), torch.zeros(3))
    for call in (p.draw, lambda: p.predict(torch.zeros((3, 2))), lambda: p.evaluate(torch.zeros((3, 2)), torch.zeros(3, dtype=torch.int64)),
                 p.prototypes):
        with pytest.raises(ValueError, match="pool is empty"):
            call()
    with pytest.raises(ValueError, match="query_labels must be"):
        p.evaluate(torch.zeros((3, 2)), torch.zeros(4, dtype=torch.int64))
    for bad in (torch.zeros((1, 4, 5), dtype=torch.int32), torch.zeros((1, 3, 5), dtype=torch.int64), torch.zeros((4, 5), dtype=torch.int64),
                torch.zeros((1, 4, 0), dtype=torch.int64), torch.zeros((1, 4, 1025), dtype=torch.int64), [[0]]):
        with pytest.raises(ValueError, match="support must be"):
            p._support(bad)
    assert p.reset() is p and p.merge_state([]) is p


def test_launchers_check_before_they_launch():
    f = torch.zeros((6, 8))
    rows = torch.zeros((2, 3, 4), dtype=torch.int64)
    assert [K.fewshot_cp(c) for c in (2, 3, 4, 5, 33, 64)] == [2, 4, 4, 8, 64, 64]
    for fn in (K.colmean, lambda t: K.center_l2norm(t, torch.zeros(8)), lambda t: K.fewshot_protos(t, rows, None, "euclidean"),
               lambda t: K.fewshot_predict(t, torch.zeros((2, 4, 8)), None, 3)):
        with pytest.raises(ValueError, match="must be f32"):
            fn(f.double())
        with pytest.raises(ValueError, match="must be f32"):
            fn(f[0])
        with pytest.raises(MirrorHipError, match="HIP device tensors"):       # there is no CPU path
            fn(f)
    pred, y = torch.zeros((2, 5), dtype=torch.int32), torch.zeros(5, dtype=torch.int64)
    with pytest.raises(ValueError, match="pred must be"):
        K.fewshot_tally(pred.long(), y, 3)
    with pytest.raises(ValueError, match="labels must be"):
        K.fewshot_tally(pred, y[:4], 3)
    for bad in (1, 65, 2.0, True):
        with pytest.raises(ValueError, match="C must be"):
            K.fewshot_tally(pred, y, bad)
    with pytest.raises(MirrorHipError, match="HIP device tensors"):
        K.fewshot_tally(pred, y, 3)


# ------------------------------------------------------------------ the declarations and their refusals
NEW = {"mh_colmean": 5, "mh_center_l2norm": 6, "mh_fewshot_protos": 12, "mh_fewshot_predict": 9, "mh_fewshot_tally": 8}


def test_the_entry_points_are_bound_within_the_same_abi_generation():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 123 and lib.mh_version() == 123
    for name, nargs in NEW.items():
        assert name in _lib.EXPORTS and len(_lib._SIGS[name]) == nargs and hasattr(lib, name), name
    assert "mh_colmean_workspace_bytes" in _lib.EXPORTS and "mh_colmean_workspace_bytes" not in _lib._SIGS
    ws = lib.mh_colmean_workspace_bytes
    assert ws.restype is C.c_int64
    # one f64 per column and strip; strips of at least 64 rows, 128 at the most
    assert ws(130, 70) == 3 * 70 * 8 and ws(1, 1) == 8 and ws(64, 512) == 512 * 8 and ws(65, 512) == 2 * 512 * 8
    assert ws(1 << 20, 4096) == 128 * 4096 * 8 and ws(0, 5) == 0 and ws(5, 0) == 0


def _refused(name, match, *args):
    with pytest.raises(MirrorHipError, match=match):
        _lib.call(name, *args)


def test_entry_points_refuse_what_lies_outside_their_limits():
    """Null pointers everywhere: each call must stop in its argument check with MH_EINVAL, and say why, before it launches anything."""
    EU, CO = 0, 1
    # mh_fewshot_protos(y, n, rows, perm, E, C, Cp, K, D, metric, protos, bias)
    pro = lambda E=4, C_=3, Cp=4, K_=5, D=64, n=100, metric=EU: ("mh_fewshot_protos", None, n, None, None, E, C_, Cp, K_, D, metric, None, None)  # noqa: E731
    # mh_fewshot_predict(q, protos, bias, nq, E, C, Cp, D, pred)
    pre = lambda E=4, C_=3, Cp=4, D=64, nq=10: ("mh_fewshot_predict", None, None, None, nq, E, C_, Cp, D, None)  # noqa: E731
    for mk in (pro, pre):
        name = mk()[0]
        _refused(name, r"C = 1 outside \[2, 64\]", *mk(C_=1, Cp=1)[1:])
        _refused(name, r"C = 65 outside \[2, 64\]", *mk(C_=65, Cp=128)[1:])
        _refused(name, "Cp = 6 is not the next power of two", *mk(C_=5, Cp=6)[1:])
        _refused(name, "Cp = 3 is not the next power of two", *mk(C_=3, Cp=3)[1:])
        _refused(name, "Cp = 8 is not the next power of two", *mk(C_=3, Cp=8)[1:])     # a power of two, but not the next one
        _refused(name, "Cp = 2 is not the next power of two", *mk(C_=3, Cp=2)[1:])
        _refused(name, r"D = 4097 outside \[1, 4096\]", *mk(D=4097)[1:])
        _refused(name, r"D = 0 outside \[1, 4096\]", *mk(D=0)[1:])
        _refused(name, "E = 0 episodes", *mk(E=0)[1:])
        _refused(name, r"E = 262145 episodes of Cp = 4 keys outside \[1, 2\^20\]", *mk(E=(1 << 18) + 1)[1:])
        _refused(name, "null pointer", *mk()[1:])                                    # everything in range: the pointers are looked at last
    _refused("mh_fewshot_protos", r"K = 0 outside \[1, 1024\]", *pro(K_=0)[1:])
    _refused("mh_fewshot_protos", r"K = 1025 outside \[1, 1024\]", *pro(K_=1025)[1:])
    _refused("mh_fewshot_protos", r"n = 0 outside", *pro(n=0)[1:])
    _refused("mh_fewshot_protos", "metric = 2", *pro(metric=2)[1:])
    _refused("mh_fewshot_protos", "null pointer", *pro(metric=CO)[1:])
    _refused("mh_fewshot_predict", r"nq = 0 outside", *pre(nq=0)[1:])
    _refused("mh_fewshot_predict", r"nq = 1048577 outside", *pre(nq=(1 << 20) + 1)[1:])
    # mh_fewshot_tally(pred, labels, nq, E, C, conf, bad, summary)
    _refused("mh_fewshot_tally", r"C = 1 outside \[2, 64\]", None, None, 10, 4, 1, None, None, None)
    _refused("mh_fewshot_tally", r"C = 65 outside \[2, 64\]", None, None, 10, 4, 65, None, None, None)
    _refused("mh_fewshot_tally", "E = 0 outside", None, None, 10, 0, 3, None, None, None)
    _refused("mh_fewshot_tally", "nq = 0 outside", None, None, 0, 4, 3, None, None, None)
    _refused("mh_fewshot_tally", "null pointer", None, None, 10, 4, 3, None, None, None)
    # mh_colmean(x, n, D, mu, workspace); mh_center_l2norm(x, mu, y, n, D, eps)
    _refused("mh_colmean", r"D = 4097 outside \[1, 4096\]", None, 10, 4097, None, None)
    _refused("mh_colmean", "n = 0 outside", None, 0, 64, None, None)
    _refused("mh_colmean", "null pointer", None, 10, 64, None, None)
    _refused("mh_center_l2norm", r"D = 4097 outside \[1, 4096\]", None, None, None, 10, 4097, 1e-12)
    _refused("mh_center_l2norm", "n = 0 outside", None, None, None, 0, 64, 1e-12)
    _refused("mh_center_l2norm", "eps = 0 must be positive", None, None, None, 10, 64, 0.0)
    _refused("mh_center_l2norm", "null pointer", None, None, None, 10, 64, 1e-12)
