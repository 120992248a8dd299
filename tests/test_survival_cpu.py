"""CPU (no GPU): the survival losses of train_survival.py construct as the reference's, the survival golden fixture holds every
case the GPU tests check, the numpy restatement of the censored concordance index gives hand-computed results, and CPU tensors
fail loudly (there is no CPU fallback)."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import mirror_amd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_surv.npz")
NS, MS = (1, 16, 257), (1, 4, 20, 130)
REDUCTIONS = ("mean", "sum", "none")
ALPHAS = {"nll": ("0", "0.4"), "ce": ("0",)}


def cindex_np(event, time, estimate, tied_tol=1e-8):
    """O(n^2) restatement of the censored concordance index (sksurv's documented definition): (cindex, concordant, discordant,
    tied_risk, tied_time).  Pair (i, j) is comparable when event[i] and (time[j] > time[i] or (time[j] == time[i] and not
    event[j])); tied when |est[j] - est[i]| <= tied_tol in f32; concordant when not tied and est[j] < est[i]."""
    event = np.asarray(event, dtype=bool)
    time = np.asarray(time, dtype=np.float64)
    est = np.asarray(estimate, dtype=np.float32)
    tol = np.float32(tied_tol)
    con = dis = tie = ttime = comp = 0
    for i in np.flatnonzero(event):
        same = time == time[i]
        mask = (time > time[i]) | (same & ~event)
        d = np.abs(est[mask] - est[i])
        ties = d <= tol
        c = (est[mask] < est[i]) & ~ties
        comp += int(mask.sum())
        tie += int(ties.sum())
        con += int(c.sum())
        dis += int(mask.sum() - c.sum() - ties.sum())
        ttime += int((same & ~event).sum())
    if not event.any():
        raise ValueError("All samples are censored")
    if comp == 0:
        raise ValueError("Data has no comparable pairs, cannot estimate concordance index.")
    return (con + 0.5 * tie) / comp, con, dis, tie, ttime


def test_survival_losses_construct_with_the_reference_attributes():
    from mirror_amd.losses import CrossEntropySurvLoss, NLLSurvLoss
    nll = NLLSurvLoss(alpha=0.4)
    assert isinstance(nll, nn.Module)
    assert (nll.alpha, nll.eps, nll.reduction) == (0.4, 1e-7, "mean")
    ce = CrossEntropySurvLoss()
    assert isinstance(ce, nn.Module)
    assert (ce.eps, ce.reduction) == (1e-7, "mean")
    ce2 = CrossEntropySurvLoss(eps=1e-6, reduction="none")
    assert (ce2.eps, ce2.reduction) == (1e-6, "none")


def test_survival_submodules_resolve_through_the_alias():
    """train_survival.py:47 imports `from losses import CrossEntropySurvLoss, NLLSurvLoss`; the sub-module paths alias too."""
    import importlib
    import sys
    names = ("models", "models.mirror", "losses", "losses.mirror_loss", "losses.info_nce", "losses.nll_surv",
             "losses.cross_entropy_surv")
    saved = {k: sys.modules.get(k) for k in names}
    try:
        mirror_amd.install_aliases()
        from losses import CrossEntropySurvLoss, NLLSurvLoss
        from losses.cross_entropy_surv import CrossEntropySurvLoss as CE2
        from losses.nll_surv import NLLSurvLoss as N2
        import mirror_amd.losses as L
        assert NLLSurvLoss is N2 is L.NLLSurvLoss and CrossEntropySurvLoss is CE2 is L.CrossEntropySurvLoss
        assert NLLSurvLoss(alpha=0.0, eps=1e-7, reduction="sum").reduction == "sum"
        assert sorted(importlib.import_module("losses").__all__) == ["CrossEntropySurvLoss", "InfoNCE", "MIRRORLoss", "NLLSurvLoss"]
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_golden_fixture_holds_every_case():
    z = np.load(GOLDEN)
    logit_max, sat_seen = 0.0, {"nll": False, "ce": False}
    thr_lo = np.log(1e-7 / (1 - 1e-7))
    thr_hi = -np.log(np.float64(np.float32(1 - 1e-7)) ** -1 - 1)
    tdts, cdts, beyond, c2 = set(), set(), False, False
    for kind in ("nll", "ce"):
        for N in NS:
            for M in MS:
                G = f"{kind}/N{N}_M{M}"
                x, t, c = z[f"{G}/logits"], z[f"{G}/event_times"], z[f"{G}/censoring"]
                assert x.shape == (N, M) and x.dtype == np.float32 and t.shape == (N,) and c.shape == (N,)
                tdts.add(t.dtype.name)
                cdts.add(c.dtype.name)
                ax = np.abs(x)
                logit_max = max(logit_max, float(ax.max()))
                sat = ax >= 20
                sat_seen[kind] |= bool(sat.any())
                # away from the clamp thresholds except in the saturated entries
                reg = x[~sat]
                assert np.all(np.abs(reg - thr_lo) >= 1e-3) and np.all(np.abs(reg - thr_hi) >= 1e-3) and np.all(np.abs(reg) < 20)
                if N >= 16:
                    assert 0 in t and M - 1 in t, G
                    if kind == "nll":
                        assert (t >= M).any(), G
                        c2 |= bool((c == 2).any())
                if kind == "ce":
                    assert t.min() >= 0 and t.max() <= M
                beyond |= kind == "nll" and bool((t >= M).any())
                for a in ALPHAS[kind]:
                    for red in REDUCTIONS:
                        loss, dl = z[f"{G}/a{a}/{red}/loss"], z[f"{G}/a{a}/{red}/dlogits"]
                        want = () if red != "none" else ((N, 1) if kind == "ce" else (N,))
                        assert loss.shape == want, (G, red, loss.shape)
                        assert dl.shape == (N, M) and np.isfinite(dl).all()
                if kind == "nll":
                    assert z[f"risk/N{N}_M{M}"].shape == (N,)
                assert z[f"{G}/w"].shape == ((N, 1) if kind == "ce" else (N,))
    assert 29 <= logit_max <= 30 and all(sat_seen.values())
    assert tdts == {"int32", "int64"} and cdts == {"int64", "float32"} and beyond and c2


def test_cindex_restatement_hand_cases():
    t = np.array([1.0, 2.0, 3.0, 4.0])
    e = np.array([True, True, True, True])
    # higher risk dies earlier: every comparable pair concordant
    assert cindex_np(e, t, [4.0, 3.0, 2.0, 1.0]) == (1.0, 6, 0, 0, 0)
    assert cindex_np(e, t, [1.0, 2.0, 3.0, 4.0]) == (0.0, 0, 6, 0, 0)
    assert cindex_np(e, t, [0.5, 0.5, 0.5, 0.5]) == (0.5, 0, 0, 6, 0)
    # censored at the same time as an event: comparable (tied_time); two events at the same time: not comparable
    e2 = np.array([True, False, True, True, False])
    t2 = np.array([2.0, 2.0, 2.0, 5.0, 1.0])
    est = np.array([3.0, 1.0, 3.0, 0.0, 9.0])
    # events 0 and 2 (t = 2): comparable with 1 (censored, t = 2) and 3 (t = 5) -> 4 pairs, all concordant; event 3: none after it
    assert cindex_np(e2, t2, est) == (1.0, 4, 0, 0, 2)
    est3 = np.array([3.0, 3.0 + 5e-9, 3.0, 3.0, 9.0])   # ties within tol (in f32, 3 + 5e-9 == 3)
    assert cindex_np(e2, t2, est3) == (0.5, 0, 0, 4, 2)
    with pytest.raises(ValueError, match="censored"):
        cindex_np([False, False], [1.0, 2.0], [0.0, 1.0])
    with pytest.raises(ValueError, match="comparable"):
        cindex_np([False, True], [1.0, 2.0], [0.0, 1.0])


def test_cpu_tensors_raise():
    from mirror_amd.losses import CrossEntropySurvLoss, NLLSurvLoss
    from mirror_amd.survival import concordance_index_censored, risk_scores
    x = torch.randn(4, 3)
    t = torch.tensor([0, 1, 2, 3])
    c = torch.tensor([1, 0, 1, 0])
    with pytest.raises(mirror_amd.MirrorHipError):
        NLLSurvLoss()(x, t, c)
    with pytest.raises(mirror_amd.MirrorHipError):
        CrossEntropySurvLoss()(x, t, c)
    with pytest.raises(mirror_amd.MirrorHipError):
        risk_scores(x)
    with pytest.raises(mirror_amd.MirrorHipError):
        concordance_index_censored(c.bool(), t.double(), x[:, 0])


def test_float_event_times_raise_type_error():
    from mirror_amd.losses import CrossEntropySurvLoss, NLLSurvLoss
    for fn in (NLLSurvLoss(), CrossEntropySurvLoss()):
        with pytest.raises(TypeError):
            fn(torch.randn(4, 3), torch.tensor([0.0, 1.0, 2.0, 3.0]), torch.tensor([1, 0, 1, 0]))
