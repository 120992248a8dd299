"""CPU (no GPU): the subtyping step of train_subtyping.py — numpy restatements of its loss (timm's LabelSmoothingCrossEntropy /
nn.CrossEntropyLoss with label smoothing and ignore_index), of torcheval's MulticlassF1Score and one-vs-rest MulticlassAUROC and
of timm's top-1 accuracy, checked against the golden fixture (tests/golden/golden_cls.npz) and against CPU torch and sklearn;
the loss classes' and metrics' surfaces and the errors they raise before any kernel runs."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import mirror_amd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_cls.npz")
NS, CS = (1, 16, 1000), (2, 5, 33)
SS = ("0", "0.1")
REDUCTIONS = ("mean", "sum", "none")
CASES = [(n, c) for n in NS for c in CS]


def ce_np(x, y, s, ignore_index, reduction, upstream):
    """(loss, dx) in f64: loss_r = (1 - s)(lse_r - x[r, y_r]) + s (lse_r - mean_c x[r, c]), 0 for ignored rows; "mean" divides by
    the non-ignored rows; dx = d(sum(upstream * loss)) / dx."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    N, C = x.shape
    keep = y != ignore_index
    yc = np.where(keep, y, 0)
    m = x.max(1, keepdims=True)
    lse = (m + np.log(np.exp(x - m).sum(1, keepdims=True)))[:, 0]
    rows = np.where(keep, (1 - s) * (lse - x[np.arange(N), yc]) + s * (lse - x.mean(1)), 0.0)
    p = np.exp(x - lse[:, None])
    onehot = np.zeros_like(x)
    onehot[np.arange(N), yc] = 1.0
    G = (p - (1 - s) * onehot - s / C) * keep[:, None]
    n = keep.sum()
    if reduction == "none":
        return rows, G * np.asarray(upstream, dtype=np.float64)[:, None]
    if reduction == "sum":
        return rows.sum(), G * float(upstream)
    return rows.sum() / n, G * float(upstream) / n


def argmax_np(scores):
    """First maximum of each row, or its first NaN (torch.argmax)."""
    s = np.asarray(scores, dtype=np.float32)
    nan = np.isnan(s)
    return np.where(nan.any(1), nan.argmax(1), np.where(nan, -np.inf, s).argmax(1))


def confusion_np(y, pred, C):
    conf = np.zeros((C, C), dtype=np.int64)
    np.add.at(conf, (np.asarray(y), np.asarray(pred)), 1)
    return conf


def f1_np(conf, average):
    tp = np.diag(conf).astype(np.float64)
    n_label, n_pred = conf.sum(1).astype(np.float64), conf.sum(0).astype(np.float64)
    den = n_label + n_pred
    f1 = np.divide(2 * tp, den, out=np.zeros_like(tp), where=den > 0)
    if average == "micro":
        return tp.sum() / conf.sum()
    if average in (None, "none"):
        return f1
    seen = den > 0
    if average == "macro":
        return f1[seen].mean()
    return (f1[seen] * n_label[seen]).sum() / n_label[seen].sum()


def auroc_counts_np(y, scores):
    """[C, 4] int64 {U2, P, Q, NaN}: U2 = 2 #{pos > neg} + #{pos == neg} over (positive of c, any other row) pairs."""
    y = np.asarray(y)
    s = np.asarray(scores, dtype=np.float32)
    C = s.shape[1]
    out = np.zeros((C, 4), dtype=np.int64)
    for c in range(C):
        pos, neg = s[y == c, c], s[y != c, c]
        d = pos[:, None] - neg[None, :]
        out[c] = (2 * (d > 0).sum() + (d == 0).sum(), pos.size, neg.size, np.isnan(s[:, c]).sum())
    return out


def auroc_np(y, scores):
    k = auroc_counts_np(y, scores)
    pq = k[:, 1].astype(np.float64) * k[:, 2]
    auc = np.divide(k[:, 0].astype(np.float64), 2 * pq, out=np.full(pq.shape, 0.5), where=pq > 0)
    auc[(k[:, 3] > 0) & (pq > 0)] = np.nan
    return auc


def metric_cases(z):
    """(key, scores f32 [N, C], labels) of every metric case in the fixture."""
    for N, C in CASES:
        G = f"N{N}_C{C}"
        yield f"met/{G}/f", z[f"cls/{G}/logits"], z[f"met/{G}/f/labels"]
        yield f"met/{G}/i", z[f"met/{G}/i/scores"].astype(np.float32), z[f"met/{G}/i/labels"]
    yield "met/nan", z["met/nan/scores"], z["met/nan/labels"]


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-30)


def test_ce_restatement_matches_golden(z):
    for N, C in CASES:
        G = f"cls/N{N}_C{C}"
        x, y, ii = z[f"{G}/logits"], z[f"{G}/labels"], int(z[f"{G}/ignore_index"])
        for s in SS:
            for red in REDUCTIONS:
                up = z[f"{G}/w"] if red == "none" else z[f"{G}/gs"]
                loss, dx = ce_np(x, y, float(s), ii, red, up)
                assert _rel(loss, z[f"{G}/s{s}/{red}/loss"]) <= 1e-12, (G, s, red)
                if f"{G}/s{s}/{red}/dx" in z:
                    assert _rel(dx, z[f"{G}/s{s}/{red}/dx"]) <= 1e-6, (G, s, red)


def test_golden_fixture_holds_every_case(z):
    ignored, int_dts, ii_class = False, set(), False
    for N, C in CASES:
        G = f"cls/N{N}_C{C}"
        x, y, ii = z[f"{G}/logits"], z[f"{G}/labels"], int(z[f"{G}/ignore_index"])
        assert x.shape == (N, C) and x.dtype == np.float32 and y.shape == (N,)
        int_dts.add(y.dtype.name)
        ignored |= bool((y == ii).any())
        ii_class |= 0 <= ii < C and bool((y == ii).any())
        assert np.all((y == ii) | ((y >= 0) & (y < C)))
        assert N < 5 or np.abs(x).max() > 60                         # rows far from 0: the max shift matters
        for s in SS:
            for red in REDUCTIONS:
                assert z[f"{G}/s{s}/{red}/loss"].shape == ((N,) if red == "none" else ())
                assert red == "sum" or z[f"{G}/s{s}/{red}/dx"].shape == (N, C)
    assert ignored and ii_class and int_dts == {"int32", "int64"}
    degenerate = nan = ties = 0
    for key, sc, y in metric_cases(z):
        a = z[f"{key}/auroc"]
        assert a.shape == (sc.shape[1],) and z[f"{key}/f1_none"].shape == (sc.shape[1],)
        degenerate += int((a == 0.5).sum())
        nan += int(np.isnan(a).sum())
        ties += int(auroc_counts_np(y, sc)[:, 0].sum() % 2)
    assert degenerate > 0 and nan == 1 and ties > 0
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_metric_restatements_match_golden(z):
    for key, sc, y in metric_cases(z):
        C = sc.shape[1]
        pred = argmax_np(sc)
        conf = confusion_np(y, pred, C)
        for avg in ("micro", "macro", "weighted"):
            assert abs(f1_np(conf, avg) - z[f"{key}/f1_{avg}"]) <= 1e-12, (key, avg)
        np.testing.assert_allclose(f1_np(conf, None), z[f"{key}/f1_none"], rtol=0, atol=1e-12)
        assert abs(np.trace(conf) / len(y) - z[f"{key}/acc"]) <= 1e-12
        np.testing.assert_allclose(auroc_np(y, sc), z[f"{key}/auroc"], rtol=0, atol=1e-12, equal_nan=True)


def test_restatements_match_torch_and_sklearn():
    g = np.random.default_rng(5)
    x = (g.normal(size=(64, 7)) * 4).astype(np.float32)
    y = g.integers(0, 7, 64)
    y[::9] = -100
    for s in (0.0, 0.1, 0.3):
        for red in REDUCTIONS:
            up = g.random(64) if red == "none" else 0.7
            xt = torch.from_numpy(x).double().requires_grad_(True)
            ref = nn.functional.cross_entropy(xt, torch.from_numpy(y), reduction=red, label_smoothing=s)
            (ref * (torch.from_numpy(up) if red == "none" else up)).sum().backward()
            loss, dx = ce_np(x, y, s, -100, red, up)
            assert _rel(loss, ref.detach().numpy()) <= 1e-12 and _rel(dx, xt.grad.numpy()) <= 1e-12, (s, red)
    # torch.argmax: first maximum, first NaN
    sc = np.array([[1, 3, 3, 0], [2, np.nan, 5, np.nan], [-np.inf, -np.inf, -np.inf, -np.inf], [0, 0, 0, 0]], dtype=np.float32)
    assert argmax_np(sc).tolist() == torch.argmax(torch.from_numpy(sc), 1).tolist() == [1, 1, 0, 0]
    try:
        from sklearn.metrics import f1_score, roc_auc_score
    except ImportError:                                   # the fixture was recorded with sklearn; nothing more to compare here
        return
    ym = g.integers(0, 5, 300)
    scores = g.integers(-2, 3, (300, 5)).astype(np.float32)
    pred = argmax_np(scores)
    conf = confusion_np(ym, pred, 5)
    for avg in ("micro", "macro", "weighted"):
        assert abs(f1_np(conf, avg) - f1_score(ym, pred, average=avg, zero_division=0)) <= 1e-12
    auc = auroc_np(ym, scores)
    for c in range(5):
        assert abs(auc[c] - roc_auc_score(ym == c, scores[:, c])) <= 1e-12


def test_loss_classes_have_the_reference_signatures():
    from mirror_amd.losses import CrossEntropyLoss, LabelSmoothingCrossEntropy
    ls = LabelSmoothingCrossEntropy()
    assert isinstance(ls, nn.Module) and (ls.smoothing, ls.confidence) == (0.1, 0.9)
    assert LabelSmoothingCrossEntropy(smoothing=0.25).confidence == 0.75
    ce = CrossEntropyLoss()
    assert isinstance(ce, nn.Module)
    assert (ce.weight, ce.ignore_index, ce.reduction, ce.label_smoothing) == (None, -100, "mean", 0.0)
    ce2 = CrossEntropyLoss(ignore_index=3, reduction="none", label_smoothing=0.2)
    assert (ce2.ignore_index, ce2.reduction, ce2.label_smoothing) == (3, "none", 0.2)
    with pytest.warns(UserWarning):                                               # nn.CrossEntropyLoss's positional order
        assert CrossEntropyLoss(None, None, -100, False).reduction == "none"
    with pytest.raises(NotImplementedError):
        CrossEntropyLoss(weight=torch.ones(3))
    with pytest.raises(ValueError):
        CrossEntropyLoss(reduction="avg")
    with pytest.raises(ValueError):
        CrossEntropyLoss(label_smoothing=1.5)
    with pytest.raises(ValueError):
        LabelSmoothingCrossEntropy(smoothing=1.0)
    import mirror_amd.losses as L
    assert sorted(L.__all__) == ["CrossEntropySurvLoss", "InfoNCE", "MIRRORLoss", "NLLSurvLoss"]


def test_loss_inputs_fail_loudly_without_a_kernel():
    from mirror_amd.losses import CrossEntropyLoss, LabelSmoothingCrossEntropy
    x = torch.randn(4, 3)
    y = torch.tensor([0, 1, 2, 1])
    for fn in (LabelSmoothingCrossEntropy(), CrossEntropyLoss(), CrossEntropyLoss(label_smoothing=0.1, reduction="none")):
        with pytest.raises(mirror_amd.MirrorHipError):
            fn(x, y)                                                      # CPU logits: no CPU fallback
        with pytest.raises(NotImplementedError):
            fn(x, torch.softmax(x, 1))                                    # class-probability targets
    with pytest.raises(mirror_amd.MirrorHipError):
        CrossEntropyLoss()(x, y.to(torch.int16))


def test_metric_arguments_are_validated():
    from mirror_amd.metrics import MulticlassAUROC, MulticlassF1Score, accuracy
    for avg in ("macro", None, "none"):
        assert MulticlassAUROC(num_classes=4, average=avg).average == avg
    for avg in ("weighted", "micro", "bogus"):
        with pytest.raises(ValueError):
            MulticlassAUROC(num_classes=4, average=avg)
    with pytest.raises(ValueError):
        MulticlassAUROC(num_classes=1)
    for avg in ("micro", "macro", "weighted", None, "none"):
        assert MulticlassF1Score(num_classes=4, average=avg).average == avg
    assert MulticlassF1Score().average == "micro" and MulticlassF1Score().num_classes is None
    for avg in ("macro", "weighted", None):
        with pytest.raises(ValueError):
            MulticlassF1Score(average=avg)
    with pytest.raises(ValueError):
        MulticlassF1Score(num_classes=4, average="samples")
    with pytest.raises(mirror_amd.MirrorHipError):
        MulticlassF1Score(num_classes=4, device="cpu")
    with pytest.raises(ValueError):
        MulticlassAUROC(num_classes=4).compute()                          # empty state
    with pytest.raises(ValueError):
        MulticlassF1Score(num_classes=4).compute()
    with pytest.raises(NotImplementedError):
        accuracy(torch.randn(4, 6), torch.tensor([0, 1, 2, 3]), topk=(1, 5))


def test_classify_entry_points_are_exported():
    from mirror_amd import _lib
    lib = _lib.load()
    assert lib.mh_version() == _lib.ABI_VERSION == 123
    for name in ("mh_cls_ce_fwd", "mh_cls_ce_bwd", "mh_cls_confusion", "mh_auroc_counts"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
