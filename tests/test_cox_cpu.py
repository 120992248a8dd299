"""Cox partial-likelihood loss and log-rank test without a device: the two f64 restatements of tests/cox_ref.py against each
other, the hand cases, scipy, the stored fixture, and the host-side surface of the feature (exports, aliases, binding
signatures, argument checks)."""
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

from tests import cox_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_cox.npz")


@pytest.mark.parametrize("times", ["distinct", "ties", "equal"])
@pytest.mark.parametrize("N", [1, 2, 3, 17, 120, 300])
def test_pair_form_equals_grouped_form(N, times):
    for k, frac in enumerate((0.0, 0.6, 1.0)):
        r, t, c = R.make_case(N, times, frac, "n3", 100 * N + k)
        up = np.random.RandomState(N + k).uniform(-0.5, 1.5, N)
        for ties in R.TIES:
            for red in R.REDUCTIONS:
                g = up if red == "none" else 0.7
                lp, gp = R.cox_pair(r, t, c, ties, red, g)
                lg, gg = R.cox_grouped(r, t, c, ties, red, g)
                np.testing.assert_allclose(lp, lg, rtol=0, atol=1e-10)
                np.testing.assert_allclose(gp, gg, rtol=0, atol=1e-10)


def test_efron_equals_breslow_when_times_are_distinct():
    r, t, c = R.make_case(200, "distinct", 0.6, "n3", 5)
    for form in (R.cox_pair, R.cox_grouped):
        (le, ge), (lb, gb) = form(r, t, c, "efron", "none"), form(r, t, c, "breslow", "none")
        assert np.array_equal(le, lb) and np.array_equal(ge, gb)
    r, t, c = R.make_case(200, "ties", 0.6, "n3", 5)
    assert np.abs(R.cox_pair(r, t, c, "efron", "sum")[0] - R.cox_pair(r, t, c, "breslow", "sum")[0]) > 1e-3


def test_hand_cases():
    for form in (R.cox_pair, R.cox_grouped):
        # N = 1: the risk set is the row itself
        for c in (0, 1):
            loss, grad = form([0.3], [2.0], [c], "efron", "mean")
            assert abs(loss) < 1e-15 and abs(grad[0]) < 1e-15
        # N = 2, the earlier one an event: loss = log(e^a + e^b) - a; the later event's risk set is itself
        a, b = 0.4, -1.1
        loss, grad = form([a, b], [1.0, 2.0], [1, 1], "efron", "sum")
        p = math.exp(a) / (math.exp(a) + math.exp(b))
        assert loss == pytest.approx(math.log(math.exp(a) + math.exp(b)) - a, abs=1e-14)
        np.testing.assert_allclose(grad, [p - 1.0, 1.0 - p], atol=1e-14)
        # N = 2 tied events: Breslow 2 log(e^a + e^b) - a - b; Efron log(e^a + e^b) + log((e^a + e^b) / 2) - a - b
        s = math.exp(a) + math.exp(b)
        assert form([a, b], [3.0, 3.0], [1, 1], "breslow", "sum")[0] == pytest.approx(2 * math.log(s) - a - b, abs=1e-14)
        assert form([a, b], [3.0, 3.0], [1, 1], "efron", "sum")[0] == pytest.approx(math.log(s) + math.log(s / 2) - a - b, abs=1e-14)
        # reductions: "mean" divides by the events, "batch" by N
        r, t, c = R.make_case(30, "ties", 0.6, "n1", 3)
        total = form(r, t, c, "efron", "sum")[0]
        assert form(r, t, c, "efron", "mean")[0] == pytest.approx(total / int((c == 1).sum()), rel=1e-14)
        assert form(r, t, c, "efron", "batch")[0] == pytest.approx(total / 30, rel=1e-14)
        # all censored: loss 0, gradient 0, for every reduction
        for red in R.REDUCTIONS:
            loss, grad = form(r, t, np.zeros(30, np.int64), "efron", red)
            assert not np.any(loss) and not np.any(grad)
        # anything but 1 is censored
        np.testing.assert_array_equal(form(r, t, np.where(c == 1, 1, 2), "efron", "none")[0], form(r, t, c, "efron", "none")[0])


def test_pair_form_nan_time_and_wide_scores():
    r, t, c = R.make_case(40, "ties", 0.6, "n1", 9)
    t2 = t.copy()
    t2[7] = np.nan
    keep = np.arange(40) != 7
    for ties in R.TIES:
        rows, grad = R.cox_pair(r, t2, c, ties, "none")
        rows_k, grad_k = R.cox_pair(r[keep], t[keep], c[keep], ties, "none")
        assert np.isnan(rows[7]) and np.isnan(grad[7])
        np.testing.assert_allclose(rows[keep], rows_k, atol=1e-12)
        np.testing.assert_allclose(grad[keep], grad_k, atol=1e-12)
    r, t, c = R.make_case(100, "ties", 0.6, "u100", 10)
    loss, grad = R.cox_pair(r, t, c, "efron", "mean")
    assert np.isfinite(loss) and np.isfinite(grad).all()
    assert np.isnan(R.cox_pair(np.where(np.arange(100) == 3, np.nan, r), t, c, "efron", "mean")[0])


def test_logrank_restatement_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    for N, seed in ((2, 0), (30, 1), (65, 2), (400, 3)):
        rng = np.random.RandomState(seed)
        t = rng.randint(0, 12, N).astype(np.float64) if N > 2 else np.array([1.0, 2.0])
        ev = rng.uniform(size=N) < 0.7 if N > 2 else np.array([True, True])
        grp = np.arange(N) % 2 == 1
        if N > 2:
            t = t + 2.0 * grp * (rng.uniform(size=N) < 0.5)       # group 1 lives a little longer
        chi2, p, O1, E1, V, nev = R.logrank(ev, t, grp)
        assert nev == int(ev.sum()) and O1 == int((ev & grp).sum())
        assert p == pytest.approx(float(stats.chi2.sf(chi2, 1)), abs=1e-12)
    assert math.isnan(R.logrank([0, 0, 0], [1.0, 2.0, 3.0], [0, 1, 0])[0])          # no events
    assert math.isnan(R.logrank([1, 1, 1], [1.0, 2.0, 3.0], [0, 0, 0])[0])          # group 1 empty


def test_logrank_restatement_against_scipy_logrank():
    stats = pytest.importorskip("scipy.stats")
    if not hasattr(stats, "logrank") or not hasattr(stats, "CensoredData"):
        pytest.skip("this scipy has no scipy.stats.logrank")
    rng = np.random.RandomState(4)
    N = 120
    t = rng.randint(1, 15, N).astype(np.float64)
    ev = rng.uniform(size=N) < 0.7
    grp = rng.uniform(size=N) < 0.45
    t = t + 3.0 * grp * (rng.uniform(size=N) < 0.5)
    chi2, p = R.logrank(ev, t, grp)[:2]

    def cd(m):
        return stats.CensoredData(uncensored=t[m & ev], right=t[m & ~ev])

    res = stats.logrank(cd(grp), cd(~grp))
    assert float(res.statistic) ** 2 == pytest.approx(chi2, rel=1e-9)
    assert float(res.pvalue) == pytest.approx(p, abs=1e-9)


def test_golden_fixture_is_small_and_rederived():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        make = importlib.import_module("make_golden_cox")
    finally:
        sys.path.pop(0)
    assert os.path.getsize(GOLDEN) < 16 * 1024
    stored = np.load(GOLDEN)
    fresh = make.build()
    assert sorted(stored.files) == sorted(fresh)
    for k in stored.files:
        if k.endswith(("/r", "/t", "/c")) or k == "meta/seed":
            assert np.array_equal(stored[k], fresh[k]), k
        else:       # exp / log of the host's libm: a few ulp
            np.testing.assert_allclose(stored[k], fresh[k], rtol=1e-12, atol=1e-13, err_msg=k)
    # and the other form agrees with what is stored
    for N, times in make.CASES:
        G = f"N{N}_{times}"
        for ties in R.TIES:
            for k, red in enumerate(R.REDUCTIONS):
                loss, grad = R.cox_pair(stored[f"{G}/r"], stored[f"{G}/t"], stored[f"{G}/c"], ties, red)
                want = stored[f"{G}/{ties}/rows"] if red == "none" else stored[f"{G}/{ties}/reduced"][k - 1]
                np.testing.assert_allclose(loss, want, rtol=0, atol=1e-10)
                np.testing.assert_allclose(grad, stored[f"{G}/{ties}/grad"][k], rtol=0, atol=1e-10)


# ----------------------------------------------------------------------------- the feature's host-side surface
def test_cox_loss_and_logrank_are_exported_aliased_and_bound():
    import mirror_amd
    from mirror_amd import _lib, functional, kernels, losses, survival
    assert losses.CoxSurvLoss is importlib.import_module("mirror_amd.losses.cox_surv").CoxSurvLoss
    assert callable(survival.logrank_test) and callable(survival.logrank_by_median)
    assert {"logrank_test", "logrank_by_median"} <= set(survival.__all__)
    assert hasattr(functional, "CoxLossFn")
    for name in ("cox_loss_fwd", "cox_loss_bwd", "logrank_stats"):
        assert callable(getattr(kernels, name))
    for name in ("mh_cox_loss_fwd", "mh_cox_loss_bwd", "mh_logrank_stats"):
        assert name in _lib._SIGS and name in _lib.EXPORTS
    assert "mh_cox_workspace_bytes" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.mh_cox_workspace_bytes(1) == 8 * 6 and lib.mh_cox_workspace_bytes(257) == 8 * (4 * 257 + 2)
    assert lib.mh_cox_workspace_bytes(0) == -1 and lib.mh_cox_workspace_bytes(65537) == -1
    saved = {k: sys.modules.get(k) for k in list(sys.modules) if k == "losses" or k.startswith("losses.") or k == "models"
             or k.startswith("models.")}
    try:
        mirror_amd.install_aliases()
        assert importlib.import_module("losses").CoxSurvLoss is losses.CoxSurvLoss
        assert importlib.import_module("losses.cox_surv").CoxSurvLoss is losses.CoxSurvLoss
    finally:
        for k in [k for k in sys.modules if k == "losses" or k.startswith("losses.") or k == "models" or k.startswith("models.")]:
            del sys.modules[k]
        sys.modules.update({k: v for k, v in saved.items() if v is not None})


def test_cox_loss_argument_checks():
    from mirror_amd import MirrorHipError
    from mirror_amd.losses import CoxSurvLoss
    loss = CoxSurvLoss()
    assert (loss.ties, loss.reduction) == ("efron", "mean")
    with pytest.raises(ValueError):
        CoxSurvLoss(ties="exact")
    with pytest.raises(ValueError):
        CoxSurvLoss(reduction="avg")
    loss.reduction = "avg"
    with pytest.raises(ValueError):
        loss(torch.zeros(4), torch.arange(4.0), torch.ones(4))
    for t in (torch.arange(4.0), torch.arange(4)):           # float and integer times are both times
        with pytest.raises(MirrorHipError, match="no CPU"):
            CoxSurvLoss()(torch.zeros(4, requires_grad=True), t, torch.ones(4))


def test_logrank_argument_checks():
    from mirror_amd import MirrorHipError
    from mirror_amd.survival import logrank_by_median, logrank_test
    ev, t, g = torch.ones(4, dtype=torch.bool), torch.arange(4.0), torch.tensor([0, 1, 0, 1])
    with pytest.raises(MirrorHipError, match="no CPU"):
        logrank_test(ev, t, g)
    with pytest.raises(MirrorHipError, match="no CPU"):
        logrank_by_median(ev, t, torch.arange(4.0))
    with pytest.raises(ValueError):
        logrank_test(ev, t[:3], g)
    with pytest.raises(ValueError):
        logrank_test(ev[:0], t[:0], g[:0])
