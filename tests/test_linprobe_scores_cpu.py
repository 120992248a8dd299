"""CPU (no GPU): the float64 restatement of the probe's scores (tests/linprobe_scores_ref.py) against sklearn's roc_auc_score
(multi_class="ovr") and log_loss and against a case worked by hand, the input condition of the end-to-end GPU test from float64 alone,
and the refusals of the new arguments and of the two new entry points (null pointers: nothing is launched)."""
import numpy as np
import pytest
import torch

from mirror_amd import LinearProbe, _lib, kernels as K
from mirror_amd._lib import MirrorHipError
from tests import linprobe_ref as R
from tests import linprobe_scores_ref as SR


def tied_case(n, C, seed, distinct=12):
    """Probability rows drawn (with repetition) from `distinct` softmax rows: every column is full of exact ties."""
    rng = np.random.default_rng(seed)
    base = np.exp(R.log_softmax(rng.integers(-8, 9, (distinct, C)) / 8.0))
    P = base[rng.integers(0, distinct, n)]
    labels = rng.integers(0, C, n).astype(np.int64)
    labels[:C] = np.arange(C)                                                 # every class has a positive
    return P, labels


@pytest.mark.parametrize("n,C", [(40, 2), (200, 3), (150, 5)])
def test_pair_counts_and_averages_against_sklearn(n, C):
    from sklearn.metrics import roc_auc_score
    P, labels = tied_case(n, C, seed=n + C)
    counts = SR.pair_counts(P, labels)
    assert np.array_equal(counts, SR.pair_counts_naive(P, labels))
    assert all(np.intersect1d(P[labels == c, c], P[labels != c, c]).size for c in range(C))      # positives tie with negatives
    auc = SR.auroc(counts)
    onehot = np.eye(C)[labels]
    per_class = np.array([roc_auc_score(onehot[:, c], P[:, c]) for c in range(C)])
    assert np.allclose(auc, per_class, rtol=1e-12, atol=0)
    if C > 2:                                                                 # sklearn's binary path takes one column, not [n, 2]
        assert np.allclose(auc, roc_auc_score(labels, P, multi_class="ovr", average=None), rtol=1e-12, atol=0)
        for average in ("macro", "weighted"):
            want = roc_auc_score(labels, P, multi_class="ovr", average=average)
            assert SR.averaged(auc, counts, average) == pytest.approx(want, rel=1e-12, abs=0)
    else:
        assert auc[1] == pytest.approx(roc_auc_score(labels, P[:, 1]), rel=1e-12, abs=0)


def test_three_rows_by_hand():
    """Rows (label): a (0), b (1), c (0) with class-0 scores 0.5, 0.5, 0.2 and class-1 scores 0.3, 0.1, 0.6; class 2 has no positive."""
    s = np.array([[0.5, 0.3, 0.2], [0.5, 0.1, 0.4], [0.2, 0.6, 0.2]])
    labels = np.array([0, 1, 0])
    counts = SR.pair_counts(s, labels)
    # class 0: positives a, c against the negative b: a ties (1), c loses (0); class 1: b against a, c: loses twice
    assert counts.tolist() == [[1, 2, 1, 0], [0, 1, 2, 0], [0, 0, 3, 0]]
    assert np.array_equal(counts, SR.pair_counts_naive(s, labels))
    auc = SR.auroc(counts)
    assert auc[0] == 0.25 and auc[1] == 0.0 and np.isnan(auc[2])
    assert SR.averaged(auc, counts, "macro") == 0.125                         # class 2 is left out
    assert SR.averaged(auc, counts, "weighted") == pytest.approx(0.5 / 3)     # (2 x 0.25 + 1 x 0) / 3
    # a label outside the classes is a negative of every class; a NaN score takes part in no pair, is counted, and makes the class NaN
    s2, l2 = np.vstack([s, [np.nan, 0.9, 0.0]]), np.array([0, 1, 0, 7])
    c2 = SR.pair_counts(s2, l2)
    assert c2.tolist() == [[1, 2, 2, 1], [0, 1, 3, 0], [0, 0, 4, 0]] and np.array_equal(c2, SR.pair_counts_naive(s2, l2))
    a2 = SR.auroc(c2)
    assert np.isnan(a2[0]) and a2[1] == 0.0 and np.isnan(SR.averaged(a2, c2, "macro"))
    none = SR.pair_counts(s[:2], np.array([5, 5]))                            # no class has a positive: nothing to average
    assert np.isnan(SR.averaged(SR.auroc(none), none, "macro")) and np.isnan(SR.averaged(SR.auroc(none), none, "weighted"))
    # the log-loss by hand: two classes, v = (0, log 3): p = (1 / 4, 3 / 4)
    W, b = np.zeros((2, 1)), np.array([0.0, np.log(3.0)])
    nll, ok = SR.row_nll(W, b, np.zeros((3, 1)), np.array([0, 1, 2]))
    assert ok.tolist() == [True, True, False] and nll[2] == 0.0
    assert nll[:2] == pytest.approx([np.log(4.0), np.log(4.0 / 3.0)], rel=1e-15)
    assert SR.proba(W, b, np.zeros((1, 1)))[0] == pytest.approx([0.25, 0.75], rel=1e-15)


def test_log_loss_against_sklearn():
    from sklearn.metrics import log_loss
    rng = np.random.default_rng(11)
    W, b, y = rng.standard_normal((4, 6)), rng.standard_normal(4), rng.standard_normal((50, 6))
    labels = rng.integers(-1, 5, 50)
    labels[:4] = np.arange(4)
    nll, ok = SR.row_nll(W, b, y, labels)
    assert 0 < (~ok).sum() < 50 and (nll[~ok] == 0).all()
    P = SR.proba(W, b, y)
    assert np.allclose(P.sum(1), 1.0, rtol=0, atol=1e-15)
    assert nll.sum() / ok.sum() == pytest.approx(log_loss(labels[ok], P[ok], labels=np.arange(4)), rel=1e-12)


def test_end_to_end_inputs_overlap_and_are_decided_in_float64():
    """The condition of the GPU end-to-end test, from float64 alone: in every (fold, strength, class) at most 5 % of the (positive,
    negative) pairs of held-out rows have probabilities closer than MARGIN; and the case does what it is there for: the classes
    overlap, no AUROC is near 1."""
    c = SR.E2E
    x, labels, fold = SR.e2e_case()
    assert x.shape == (c["n"], c["D"]) and set(fold) == {0, 1, 2} and set(labels) == {0, 1, 2}
    _, P = SR.e2e_reference()
    worst, aucs = 0.0, []
    for f in range(c["F"]):
        rows = np.flatnonzero(fold == f)
        for s in range(len(c["strengths"])):
            counts = SR.pair_counts(P[f, s, rows], labels[rows])
            auc = SR.auroc(counts)
            for k in range(c["C"]):
                lo, hi, share = SR.auc_interval(P[f, s, rows, k], labels[rows], k, R.MARGIN)
                assert lo <= auc[k] <= hi
                worst = max(worst, share)
                aucs.append(auc[k])
    print(f"held-out AUROC {min(aucs):.4f} .. {max(aucs):.4f}; undecided pairs at most {100 * worst:.2f} %")
    assert 0.72 <= min(aucs) and max(aucs) <= 0.88
    assert worst <= R.MAX_UNDECIDED


# ------------------------------------------------------------------ the public face
def test_new_arguments_are_checked():
    p = LinearProbe(3, device="cuda")
    for kw in (dict(auroc=1), dict(auroc="yes"), dict(auroc=True, average="micro"), dict(auroc=True, average=0), dict(select="f1"),
               dict(select=None), dict(select="auc"), dict(select="nll"), dict(auroc=False, select="auc"),
               dict(auroc=True, average=None, select="auc")):
        with pytest.raises(ValueError, match="auroc must be|average must be|select must be|needs auroc=True|needs average="):
            p.evaluate(**kw)
    for call in (lambda: p.evaluate(auroc=True), p.oof_proba, lambda: p.predict_proba(torch.zeros((3, 2)))):
        with pytest.raises(ValueError, match="nothing is fitted"):
            call()


def test_launchers_check_before_they_launch():
    q = torch.zeros((6, 8))
    W, b = torch.zeros((2, 4, 8)), torch.zeros((2, 4))
    lab = torch.zeros(6, dtype=torch.int64)
    with pytest.raises(ValueError, match="must be f32"):
        K.linprobe_proba(q.double(), W, b, 3)
    with pytest.raises(ValueError, match="C must be"):
        K.linprobe_proba(q, W, b, 1)
    with pytest.raises(ValueError, match=r"weights must be f32 \[J, 4, 8\]"):
        K.linprobe_proba(q, torch.zeros((2, 3, 8)), b, 3)
    with pytest.raises(MirrorHipError, match="HIP device tensors"):           # there is no CPU path; the GPU tests see the later checks
        K.linprobe_proba(q, W, b, 3, labels=lab, want_nll=True)
    s = torch.zeros((2, 6, 3))
    with pytest.raises(ValueError, match=r"scores must be f32 \[E, N, C\]"):
        K.auroc_counts_many(s[0], lab)
    with pytest.raises(ValueError, match=r"scores must be f32 \[E, N, C\]"):
        K.auroc_counts_many(s.double(), lab)
    with pytest.raises(ValueError, match=r"labels must be int64 \[6\]"):
        K.auroc_counts_many(s, lab.int())
    with pytest.raises(ValueError, match=r"counts must be a contiguous int64 \[2, 3, 4\]"):
        K.auroc_counts_many(s, lab, counts=torch.zeros((2, 3, 4)))
    with pytest.raises(MirrorHipError, match="HIP device tensors"):
        K.auroc_counts_many(s, lab)


# ------------------------------------------------------------------ the declarations and their refusals
def test_the_entry_points_are_bound_within_the_same_abi_generation():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 123 and lib.mh_version() == 123
    for name, nargs in {"mh_linprobe_proba": 11, "mh_auroc_counts_many": 8}.items():
        assert name in _lib.EXPORTS and len(_lib._SIGS[name]) == nargs and hasattr(lib, name), name


def _refused(name, match, *args):
    with pytest.raises(MirrorHipError, match=match):
        _lib.call(name, *args)


def test_entry_points_refuse_what_lies_outside_their_limits():
    """Null pointers everywhere: each call must stop in its argument check with MH_EINVAL, and say why, before it launches anything."""
    # mh_linprobe_proba(q, nq, D, W, b, E, C, Cp, labels, P, nll_part)
    proba = lambda n=10, D=64, E=4, C_=3, Cp=4, nll=None: ("mh_linprobe_proba", None, n, D, None, None, E, C_, Cp, None, None, nll)  # noqa: E731
    _refused("mh_linprobe_proba", r"C = 1 outside \[2, 64\]", *proba(C_=1, Cp=1)[1:])
    _refused("mh_linprobe_proba", r"C = 65 outside \[2, 64\]", *proba(C_=65, Cp=128)[1:])
    _refused("mh_linprobe_proba", "Cp = 8 is not the next power of two", *proba(C_=3, Cp=8)[1:])
    _refused("mh_linprobe_proba", r"D = 4097 outside \[1, 4096\]", *proba(D=4097)[1:])
    _refused("mh_linprobe_proba", r"n = 0 outside \[1, 2\^20\]", *proba(n=0)[1:])
    _refused("mh_linprobe_proba", "J = 0 jobs", *proba(E=0)[1:])
    _refused("mh_linprobe_proba", r"n J Cp = 65537 x 1024 x 4 logit gradients", *proba(n=(1 << 16) + 1, E=1024)[1:])
    _refused("mh_linprobe_proba", "nll_part needs labels", *proba(nll=8)[1:])           # a placeholder address, never dereferenced
    _refused("mh_linprobe_proba", "null pointer", *proba()[1:])                          # the pointers are looked at last
    # mh_auroc_counts_many(scores, ld_row, ld_table, labels, N, C, E, counts)
    many = lambda ld=3, ldt=30, N=10, C_=3, E=4: ("mh_auroc_counts_many", None, ld, ldt, None, N, C_, E, None)  # noqa: E731
    _refused("mh_auroc_counts_many", r"N = 0 outside \[1, 2\^20\]", *many(N=0)[1:])
    _refused("mh_auroc_counts_many", r"N = 1048577 outside \[1, 2\^20\]", *many(N=(1 << 20) + 1)[1:])
    _refused("mh_auroc_counts_many", "bad shape C=1", *many(C_=1)[1:])
    _refused("mh_auroc_counts_many", "bad shape C=1025", *many(C_=1025, ld=1025)[1:])
    _refused("mh_auroc_counts_many", "bad shape C=3 ld_row=2", *many(ld=2)[1:])
    _refused("mh_auroc_counts_many", "E = 0 tables", *many(E=0)[1:])
    _refused("mh_auroc_counts_many", r"E = 21846 tables of C = 3 classes, E C <= 65535", *many(E=21846, ldt=30)[1:])
    _refused("mh_auroc_counts_many", r"ld_table = 29 < N ld_row = 10 x 3", *many(ldt=29)[1:])
    _refused("mh_auroc_counts_many", "null pointer", *many(E=21845)[1:])               # E C = 65535 exactly: the pointers come last
    _refused("mh_auroc_counts_many", "null pointer", *many(E=1, ldt=0)[1:])            # one table: ld_table is not looked at
