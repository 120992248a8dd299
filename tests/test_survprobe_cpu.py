"""CPU (no GPU): the float64 restatement of the survival linear probe (tests/survprobe_ref.py) against the reference's NLLSurvLoss
restated in f64, against central differences and against scipy's L-BFGS-B within the rate FISTA guarantees; `survival_bins` against
pandas; the input condition of the end-to-end GPU test from float64 alone; SurvivalProbe's argument checks, those of the two launchers,
and the MH_EINVAL refusals of the two entry points (null pointers: nothing is launched)."""
import numpy as np
import pytest
import torch

import mirror_amd
from mirror_amd import SurvivalProbe, _lib, kernels as K, survival
from mirror_amd._lib import MirrorHipError
from tests import survprobe_ref as R


def _f64_nll_rows(logits, t, c, alpha, eps=1e-7):
    """losses/nll_surv.py restated in f64 torch, reduction "none" (the form of tests/test_survival_gpu.py with the alpha mix)."""
    N, M = logits.shape
    h = torch.sigmoid(logits).clamp(min=eps, max=1 - eps)
    tr = torch.arange(M)[None, :]
    tt = t[:, None].long()
    unc, cen = (c == 1)[:, None], (c == 0)[:, None]
    lh, l1 = torch.log(h), torch.log(1 - h)
    u = -((l1 * ((tr < tt) & unc)).sum(1) + (lh * ((tr == tt) & unc)).sum(1))
    ce = -(l1 * ((tr <= tt) & cen)).sum(1)
    nll = torch.where(unc[:, 0], u, torch.where(cen[:, 0], ce, torch.zeros_like(u)))
    return (1 - alpha) * nll + alpha * torch.where(unc[:, 0], u, torch.zeros_like(u))


@pytest.mark.parametrize("alpha", [0.0, 0.4])
def test_row_nll_is_the_reference_loss_without_its_clamp(alpha):
    rng = np.random.default_rng(3)
    n, D, M = 200, 6, 5
    y = rng.standard_normal((n, D))
    W = rng.standard_normal((M, D))
    W *= 10.0 / np.abs(y @ W.T).max()                                         # logits in [-10, 10]
    b = np.zeros(M)
    bins, event = rng.integers(0, M, n), rng.integers(0, 2, n)
    mask = np.ones(n, dtype=bool)
    v = y @ W.T + b
    assert np.abs(v).max() <= 10.0 + 1e-9
    got = R.row_weight(event, alpha) * R.row_nll(W, b, y, bins, event, mask)
    want = _f64_nll_rows(torch.from_numpy(v), torch.from_numpy(bins), torch.from_numpy(event), alpha).numpy()
    print(f"alpha {alpha}: max |row_nll - NLLSurvLoss| = {np.abs(got - want).max():.2e}")
    assert np.abs(got - want).max() <= 1e-12
    assert abs(R.objective(W, b, y, bins, event, mask, 0.0, alpha) - want.mean()) <= 1e-12
    # past log((1 - eps) / eps) = 16.1 the reference clamps the hazard and the two part: the probe optimises the unclamped form
    for big in (16.2, 30.0):
        v1 = np.array([[big, -big]])
        for T, e in ((0, 0), (1, 1)):
            mine = float(np.where(np.arange(2) <= T, R.softplus(v1[0]) - (np.arange(2) == T) * e * v1[0], 0.0).sum())
            ref = float(_f64_nll_rows(torch.from_numpy(v1), torch.tensor([T]), torch.tensor([e]), alpha)[0]) / (1.0 if e else 1 - alpha)
            assert abs(mine - ref) > 1e-3 * big, (big, T, e, mine, ref)


def test_logit_grad_against_central_differences():
    rng = np.random.default_rng(4)
    n, D, M, alpha, lam = 60, 5, 4, 0.4, 1e-2
    y = rng.standard_normal((n, D))
    bins, event, fold = rng.integers(-1, M + 1, n), rng.integers(0, 3, n), rng.integers(-1, 3, n)
    mask = R.train_mask(bins, event, fold, 1, M)
    assert 10 < mask.sum() < n
    W0, b0 = rng.standard_normal((M, D)), rng.standard_normal(M)
    dW, db = R.gradient(W0, b0, y, bins, event, mask, lam, alpha)
    f = lambda W, b: R.objective(W, b, y, bins, event, mask, lam, alpha)  # noqa: E731
    for (t, d) in ((0, 0), (3, 4), (1, 2), (2, 3)):
        E = np.zeros((M, D))
        E[t, d] = 1e-6
        assert abs((f(W0 + E, b0) - f(W0 - E, b0)) / 2e-6 - dW[t, d]) <= 1e-8
    for t in range(M):
        e = np.zeros(M)
        e[t] = 1e-6
        assert abs((f(W0, b0 + e) - f(W0, b0 - e)) / 2e-6 - db[t]) <= 1e-8
    G = R.logit_grad(W0, b0, y, bins, event, mask, alpha)
    assert (G[~mask] == 0).all() and all((G[i, bins[i] + 1:] == 0).all() for i in np.flatnonzero(mask))


@pytest.mark.parametrize("shape", [(300, 16, 4), (200, 40, 5)], ids=lambda s: "n%d-D%d-M%d" % s)
def test_fista_reaches_the_optimum_within_its_guarantee(shape):
    """F(X_k) - F* <= 2 L (|W*|^2 + |b*|^2) / (k + 1)^2 with L = rho / 4 + lambda, against scipy's L-BFGS-B on the same objective."""
    n, D, M = shape
    x, bins, event, time = R.cohort(n, D, M, seed=n + D)
    y, _ = R.prepare(x, x)
    mask = R.train_mask(bins, event, np.zeros(n, dtype=np.int64), -1, M)
    assert mask.all() and 0.15 < 1 - event.mean() < 0.6
    for lam, alpha in ((1e-4, 0.0), (1e-2, 0.4)):
        Ws, bs, Fs = R.optimum(y, bins, event, mask, lam, alpha, M)
        dW, db = R.gradient(Ws, bs, y, bins, event, mask, lam, alpha)
        assert max(np.abs(dW).max(), np.abs(db).max()) <= 1e-6
        L = R.lipschitz(y, lam)
        r2 = float((Ws ** 2).sum() + (bs ** 2).sum())
        for k in (20, 300):
            W, b = R.fista(y, bins, event, mask, lam, alpha, M, k)
            gap = R.objective(W, b, y, bins, event, mask, lam, alpha) - Fs
            bound = 2.0 * L * r2 / (k + 1) ** 2
            print(f"{shape} lambda {lam:g} alpha {alpha}: k = {k}: F - F* = {gap:.3e}, bound {bound:.3e}, max |v*| = {np.abs(y @ Ws.T + bs).max():.1f}")
            assert -1e-10 <= gap <= bound


# ------------------------------------------------------------------ survival_bins
def _edges_close(edges, want, time):
    """pandas interpolates a quantile as a + (b - a) g, numpy as a lerp of its own: each rounds a few times at the size of the two
    neighbouring times, so the edges may differ by a few ulps of the largest time (the bins must not differ at all)."""
    return np.abs(edges.numpy() - want).max() <= 4 * 2.0 ** -52 * max(np.abs(time).max(), 1.0)


def test_survival_bins_against_pandas():
    pytest.importorskip("pandas")
    rng = np.random.default_rng(0)
    for trial in range(60):
        n, M = int(rng.integers(20, 200)), int(rng.integers(2, 7))
        time = rng.exponential(30.0, n)
        if trial % 2:
            time = np.round(time)                                             # whole months: ties, also among the edges
        event = (rng.random(n) < 0.6).astype(np.int64)
        try:
            want, wq = R.bins_ref(time, event, M)
        except ValueError:
            with pytest.raises(ValueError, match="Bin edges must be unique"):
                survival.survival_bins(torch.from_numpy(time), torch.from_numpy(event), M)
            continue
        got, edges = survival.survival_bins(torch.from_numpy(time), torch.from_numpy(event), M)
        assert got.dtype == torch.int64 and edges.dtype == torch.float64 and tuple(edges.shape) == (M + 1,)
        assert np.array_equal(got.numpy(), want) and _edges_close(edges, wq, time), trial
        assert got.min() == 0 and got.max() == M - 1
    # no event at all: equal-width bins; a single distinct time too
    for time in (rng.exponential(30.0, 50), np.full(7, 12.0), np.zeros(3)):
        want, wq = R.bins_ref(time, np.zeros(len(time), dtype=np.int64), 4)
        got, edges = survival.survival_bins(time, np.zeros(len(time), dtype=np.int64), 4)
        assert np.array_equal(got.numpy(), want) and _edges_close(edges, wq, time)
    # the refusal: three of four event-time quantiles coincide
    time, event = np.array([5.0, 5.0, 5.0, 5.0, 9.0, 1.0]), np.array([1, 1, 1, 1, 1, 0])
    with pytest.raises(ValueError):
        R.bins_ref(time, event, 4)
    with pytest.raises(ValueError, match="Bin edges must be unique"):
        survival.survival_bins(time, event, 4)
    for bad in (dict(time=[], event=[]), dict(time=[1.0, float("nan")], event=[1, 0]), dict(time=[1.0, 2.0], event=[1]),
                dict(time=[1.0, 2.0], event=[1, 0], num_bins=0), dict(time=[1.0, 2.0], event=[1, 0], num_bins=2.0)):
        with pytest.raises(ValueError):
            survival.survival_bins(**bad)
    assert "survival_bins" in survival.__all__


# ------------------------------------------------------------------ the end-to-end case
def test_end_to_end_inputs_are_decided_in_float64():
    """The condition of the GPU end-to-end test, from float64 alone: under every held-out job, at most 1 % of the comparable pairs have
    risks closer than 1e-5 (an order above twice the f32 risk tolerance at this shape); in fact none or nearly none do."""
    x, bins, event, time, fold = R.e2e_case()
    c = R.E2E
    assert x.shape == (c["n"], c["D"]) and (fold == -1).sum() == 5 and set(fold) == {-1, 0, 1, 2} and set(bins) == {0, 1, 2, 3, 4}
    y, _ = R.prepare(x, x)
    held, lam = R.jobs(c["F"], c["strengths"])
    for h, l in zip(held[:-len(c["strengths"])], lam):
        mask = R.train_mask(bins, event, fold, h, c["M"])
        W, b = R.fista(y, bins, event, mask, l, 0.0, c["M"], c["steps"])
        rows = np.flatnonzero(fold == h)
        r = R.risk(W, b, y[rows])
        ev, t = event[rows] == 1, time[rows]
        comp = ev[:, None] & (t[None, :] > t[:, None])
        close = comp & (np.abs(r[None, :] - r[:, None]) < 1e-5)
        print(f"fold {h} lambda {l:g}: {close.sum()} of {comp.sum()} comparable pairs under 1e-5, c-index {R.cindex(R.cindex_counts(ev, t, r)):.4f}")
        assert comp.sum() > 500 and close.sum() <= R.MAX_UNDECIDED * comp.sum()


# ------------------------------------------------------------------ the public face
def test_probe_is_exported_and_checks_its_arguments():
    assert mirror_amd.SurvivalProbe is SurvivalProbe and "SurvivalProbe" in mirror_amd.__all__
    for kw in (dict(num_bins=1), dict(num_bins=65), dict(num_bins=True), dict(num_bins=4.0), dict(strengths=()), dict(strengths=0.1),
               dict(strengths=(0.1, 0.0)), dict(strengths=(-1.0,)), dict(strengths=(float("inf"),)), dict(strengths=("a",)),
               dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(alpha=True), dict(alpha="x"), dict(max_iter=0),
               dict(max_iter=2.0), dict(tol=-1e-3), dict(tol=float("nan")), dict(tol="x"), dict(center=1), dict(check_every=0),
               dict(check_every=True)):
        with pytest.raises(ValueError):
            SurvivalProbe(device="cuda", **kw)
    with pytest.raises(MirrorHipError, match="HIP device"):
        SurvivalProbe(device="cpu")
    p = SurvivalProbe(device="cuda")
    assert (p.num_bins, p.strengths, p.alpha, p.max_iter, p.tol, p.center, p.check_every) == (4, (1e-4, 1e-3, 1e-2, 1e-1), 0.0, 2000, 1e-4,
                                                                                             True, 16)
    x, i3, t3 = torch.zeros((3, 2)), torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.float64)
    with pytest.raises(ValueError, match="emb must be"):
        p.fit(torch.zeros((3, 2), dtype=torch.int64), i3, i3, t3)
    with pytest.raises(ValueError, match="emb must be"):
        p.fit(torch.zeros(3), i3, i3, t3)
    with pytest.raises(MirrorHipError, match="D = 4097"):
        p.fit(torch.zeros((3, 4097)), i3, i3, t3)
    with pytest.raises(ValueError, match="bins must be"):
        p.fit(x, torch.zeros(2, dtype=torch.int64), i3, t3)
    with pytest.raises(ValueError, match="bins must be"):
        p.fit(x, torch.zeros(3), i3, t3)
    with pytest.raises(ValueError, match="event must be"):
        p.fit(x, i3, torch.zeros(3), t3)
    with pytest.raises(ValueError, match="event must be"):
        p.fit(x, i3, torch.zeros(4, dtype=torch.bool), t3)
    with pytest.raises(ValueError, match="time must be"):
        p.fit(x, i3, i3, i3)
    with pytest.raises(ValueError, match="time must be"):
        p.fit(x, i3, i3, torch.zeros((3, 1)))
    with pytest.raises(ValueError, match="fold must be"):
        p.fit(x, i3, i3, t3, fold=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="fold must be"):
        p.fit(x, i3, i3, t3, fold=[0, 1, 2])
    with pytest.raises(ValueError, match=r"no row of fold\(s\) \[1\]"):            # an empty fold
        p.fit(x, i3, i3, t3, fold=torch.tensor([0, 2, 0]))
    with pytest.raises(ValueError, match="train_rows must be a 1-D int64"):
        p.fit(x, i3, i3, t3, train_rows=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="train_rows must be a 1-D int64"):
        p.fit(x, i3, i3, t3, train_rows=[0, 1])
    with pytest.raises(ValueError, match="train_rows must index the 3 rows"):
        p.fit(x, i3, i3, t3, train_rows=torch.tensor([0, 3]))
    with pytest.raises(MirrorHipError, match="J \\* Mp <= 2\\^20"):         # 2^18 folds x 4 strengths x 4 slots
        p.fit(x, i3, i3, t3, fold=torch.tensor([0, 1, (1 << 18)]))
    for call in (p.evaluate, p.oof_risk, lambda: p.predict_risk(x)):
        with pytest.raises(ValueError, match="nothing is fitted"):
            call()
    with pytest.raises(ValueError, match="strength must be one of"):           # a strength that is not in the list
        p._strength_index(0.5)
    assert p._strength_index(1e-2) == 2


def test_launchers_check_before_they_launch():
    y = torch.zeros((6, 8))
    W, b = torch.zeros((2, 4, 8)), torch.zeros((2, 4))
    bins, ev, fold = torch.zeros(6, dtype=torch.int64), torch.zeros(6, dtype=torch.uint8), torch.zeros(6, dtype=torch.int32)
    held, r = torch.zeros(2, dtype=torch.int32), torch.zeros(2)
    grad = lambda **kw: K.survprobe_grad(**{**dict(y=y, Wz=W, bz=b, bins=bins, event=ev, fold=fold, heldout=held, rscale=r, w_cens=1.0, M=3), **kw})  # noqa: E731
    with pytest.raises(ValueError, match="must be f32"):
        grad(y=y.double())
    for M in (1, 65, True, 3.0):
        with pytest.raises(ValueError, match="M must be an int in \\[2, 64\\]"):
            grad(M=M)
        with pytest.raises(ValueError, match="M must be an int in \\[2, 64\\]"):
            K.survprobe_risk(y, W, b, M)
    with pytest.raises(ValueError, match=r"bins must be torch.int64 \[6\]"):
        grad(bins=bins.int())
    with pytest.raises(ValueError, match=r"event must be torch.uint8 \[6\]"):
        grad(event=ev.bool())
    with pytest.raises(ValueError, match=r"event must be torch.uint8 \[6\]"):
        grad(event=ev[:5])
    with pytest.raises(ValueError, match=r"fold must be torch.int32 \[6\]"):
        grad(fold=fold.long())
    for w in (-0.1, 1.1, float("nan"), True, "x"):
        with pytest.raises(ValueError, match="w_cens must lie in"):
            grad(w_cens=w)
    with pytest.raises(ValueError, match=r"weights must be f32 \[J, 4, 8\]"):
        grad(Wz=torch.zeros((2, 3, 8)))
    with pytest.raises(ValueError, match=r"bias must be f32 \[2, 4\]"):
        K.survprobe_risk(y, W, torch.zeros((2, 3)), 3)
    with pytest.raises(ValueError, match=r"weights must be f32 \[J, 4, 8\]"):
        K.survprobe_risk(y, torch.zeros((2, 8, 8)), b, 3)
    with pytest.raises(MirrorHipError, match="HIP device tensors"):           # there is no CPU path
        grad()
    with pytest.raises(MirrorHipError, match="HIP device tensors"):
        K.survprobe_risk(y, W, b, 3)


# ------------------------------------------------------------------ the declarations and their refusals
def test_the_entry_points_are_declared_and_exported():
    lib = _lib.load()
    assert lib.mh_version() == _lib.ABI_VERSION
    for name, nargs in {"mh_survprobe_grad": 16, "mh_survprobe_risk": 9}.items():
        assert name in _lib.EXPORTS and len(_lib._SIGS[name]) == nargs and hasattr(lib, name), name


def _refused(name, match, *args):
    with pytest.raises(MirrorHipError, match=match):
        _lib.call(name, *args)


def test_entry_points_refuse_what_lies_outside_their_limits():
    """Null pointers everywhere: each call must stop in its argument check with MH_EINVAL, and say why, before it launches anything."""
    # mh_survprobe_grad(y, n, D, Wz, bz, bins, event, fold, heldout, rscale, w_cens, J, M, Mp, G, loss_part)
    grad = lambda n=10, D=64, J=4, M=3, Mp=4, w=1.0: ("mh_survprobe_grad", None, n, D, None, None, None, None, None, None, None, w, J, M, Mp, None, None)  # noqa: E731
    # mh_survprobe_risk(q, nq, D, W, b, S, M, Mp, risk)
    risk = lambda n=10, D=64, J=4, M=3, Mp=4: ("mh_survprobe_risk", None, n, D, None, None, J, M, Mp, None)  # noqa: E731
    for mk in (grad, risk):
        name = mk()[0]
        _refused(name, r"M = 1 outside \[2, 64\]", *mk(M=1, Mp=1)[1:])
        _refused(name, r"M = 65 outside \[2, 64\]", *mk(M=65, Mp=128)[1:])
        _refused(name, "Mp = 6 is not the next power of two", *mk(M=5, Mp=6)[1:])
        _refused(name, "Mp = 8 is not the next power of two", *mk(M=3, Mp=8)[1:])
        _refused(name, "Mp = 2 is not the next power of two", *mk(M=3, Mp=2)[1:])
        _refused(name, r"D = 4097 outside \[1, 4096\]", *mk(D=4097)[1:])
        _refused(name, r"D = 0 outside \[1, 4096\]", *mk(D=0)[1:])
        _refused(name, r"n = 0 outside \[1, 2\^20\]", *mk(n=0)[1:])
        _refused(name, r"n = 1048577 outside \[1, 2\^20\]", *mk(n=(1 << 20) + 1)[1:])
        _refused(name, "J = 0 jobs", *mk(J=0)[1:])
        _refused(name, r"J = 262145 jobs of Mp = 4 keys outside \[1, 2\^20\]", *mk(n=1, J=(1 << 18) + 1)[1:])
        _refused(name, "null pointer", *mk()[1:])                                    # the pointers are looked at last
    _refused("mh_survprobe_grad", r"n J Mp = 65537 x 1024 x 4 logit gradients", *grad(n=(1 << 16) + 1, J=1024)[1:])
    _refused("mh_survprobe_grad", "null pointer", *grad(n=1 << 16, J=1024)[1:])      # exactly 2^28
    _refused("mh_survprobe_grad", r"w_cens = 1.5 outside \[0, 1\]", *grad(w=1.5)[1:])
    _refused("mh_survprobe_grad", r"w_cens = -0.1 outside \[0, 1\]", *grad(w=-0.1)[1:])
    _refused("mh_survprobe_grad", r"w_cens = nan outside \[0, 1\]", *grad(w=float("nan"))[1:])
