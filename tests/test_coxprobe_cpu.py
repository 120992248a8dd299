"""CPU (no GPU): the float64 scan form of the ridge Cox probe (tests/coxprobe_ref.py) against the all-pairs statement of
tests/cox_ref.py, against central differences, its curvature against the Lipschitz constant the probe steps with, and FISTA against
scipy's L-BFGS-B within the rate it guarantees; the input condition of the end-to-end GPU test from float64 alone; CoxProbe's argument
checks, those of the three launchers, and the MH_EINVAL refusals of the entry points (null pointers: nothing is launched)."""
import numpy as np
import pytest
import torch

import mirror_amd
from mirror_amd import CoxProbe, _lib, kernels as K
from mirror_amd._lib import MirrorHipError
from tests import cox_ref as C
from tests import coxprobe_ref as R


# ------------------------------------------------------------------ the scan form is the pair form
@pytest.mark.parametrize("ties", R.TIES)
@pytest.mark.parametrize("n", [1, 7, 64, 200])
def test_scan_form_is_the_pair_form_on_each_jobs_training_rows(n, ties):
    """Integer times 0 .. 7 (heavy ties), random events and random training masks: on a job's training subset, in sorted order, the
    scan form's loss and score gradient equal cox_pair(..., reduction="sum") to 1e-9 relative, and the gradient is exactly 0 elsewhere."""
    rng = np.random.default_rng(100 + n)
    for trial in range(6):
        time = rng.integers(0, 8, n).astype(np.float64)
        event = rng.integers(0, 2, n)
        mask = rng.random(n) < (0.7 if trial else 1.0)
        v = rng.standard_normal(n) * (3.0 if trial % 2 else 1.0)
        p = R.sort_rows(time)
        time, event, mask, v = time[p], event[p], mask[p], v[p]
        loss, g = R.scan(v, time, event, mask, ties)
        assert (g[~mask] == 0).all()
        if not mask.any():
            assert loss == 0.0
            continue
        want, gw = C.cox_pair(v[mask], time[mask], event[mask], ties, "sum")
        err_l = abs(loss - want) / max(abs(want), 1e-300) if want else abs(loss)
        err_g = np.abs(g[mask] - gw).max() / max(np.abs(gw).max(), 1e-300) if np.abs(gw).max() else np.abs(g[mask]).max()
        print(f"n {n} {ties} trial {trial}: loss rel {err_l:.2e}, grad rel {err_g:.2e}")
        assert err_l <= 1e-9 and err_g <= 1e-9
        assert abs(g.sum()) <= 1e-12 * max(np.abs(g).sum(), 1.0)              # the partial likelihood does not see a shift of the scores


def test_sort_puts_nan_times_last_and_keeps_ties_in_row_order():
    time = np.array([2.0, np.nan, 5.0, 2.0, np.nan, 5.0, 0.5])
    p = R.sort_rows(time)
    assert p.tolist() == [2, 5, 0, 3, 6, 1, 4]
    gid, first, last = R.groups(time[p])
    assert gid.tolist() == [0, 0, 1, 1, 2, 3, 4] and first.tolist() == [0, 2, 4, 5, 6] and last.tolist() == [1, 3, 4, 5, 6]
    # a NaN time trains nowhere and is in no other row's risk set
    ev = np.ones(7, dtype=np.int64)
    fold = np.zeros(7, dtype=np.int64)
    mask = R.train_mask(ev[p], time[p], fold, -1)
    assert mask.tolist() == [True] * 5 + [False] * 2
    v = np.arange(7.0)
    a = R.scan(v, time[p], ev, mask, "efron")
    v[5:] = np.nan                                                            # whatever the score of a row outside the job holds
    b = R.scan(v, time[p], ev, mask, "efron")
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and (a[1][5:] == 0).all()


@pytest.mark.parametrize("ties", R.TIES)
def test_gradient_against_central_differences(ties):
    rng = np.random.default_rng(4)
    n, D, lam = 80, 5, 1e-2
    y = rng.standard_normal((n, D))
    time = np.round(rng.exponential(1.0, n), 1)
    event, fold = rng.integers(0, 3, n), rng.integers(-1, 3, n)
    time[7] = np.nan
    p = R.sort_rows(time)
    y, time, event, fold = y[p], time[p], event[p], fold[p]
    mask = R.train_mask(event, time, fold, 1)
    assert 10 < mask.sum() < n and len(np.unique(time[mask])) < mask.sum()
    w0 = rng.standard_normal(D)
    g = R.gradient(w0, y, time, event, mask, lam, ties)
    for d in range(D):
        e = np.zeros(D)
        e[d] = 1e-6
        num = (R.objective(w0 + e, y, time, event, mask, lam, ties) - R.objective(w0 - e, y, time, event, mask, lam, ties)) / 2e-6
        assert abs(num - g[d]) <= 1e-8, (d, num, g[d])


# ------------------------------------------------------------------ the case: curvature, rate, decided pairs
@pytest.fixture(scope="module")
def case_jobs():
    """Per (ties, job) of the end-to-end case: the mask, lambda, L and the FISTA iterates X_10, X_100, X_300, computed once."""
    y, event, time, fold, _ = R.e2e_sorted()
    held, lam = R.jobs(R.E2E["F"], R.E2E["strengths"])
    out = {}
    for ties in R.TIES:
        for j, (h, l) in enumerate(zip(held, lam)):
            mask = R.train_mask(event, time, fold, h)
            _, kept = R.fista(y, time, event, mask, l, ties, R.E2E["steps"], keep=(10, 100, 300))
            out[ties, j] = dict(mask=mask, lam=l, L=R.lipschitz(y, l, *R.counts_of(event, mask)), X=kept)
    return (y, event, time, fold), out


def test_case_is_what_the_gpu_test_expects():
    x, event, time, fold = R.e2e_case()
    assert x.shape == (240, 16) and np.isnan(time).sum() == 1 and (event == 2).sum() == 1 and (fold == -1).sum() == 5
    assert fold[np.isnan(time)][0] >= 0 and fold[event == 2][0] >= 0 and set(fold) == {-1, 0, 1, 2}
    _, ev0, t0, f0 = R.e2e_case(plain=True)
    assert len(np.unique(t0)) == 44 and (ev0 == 1).sum() == 136 and (f0 >= 0).all() and not np.isnan(t0).any()


@pytest.mark.parametrize("ties", R.TIES)
def test_curvature_at_the_iterate_is_below_the_lipschitz_constant(case_jobs, ties):
    (y, event, time, _), jobs = case_jobs
    for (tj, j), c in jobs.items():
        if tj != ties:
            continue
        top = R.hessian_top(c["X"][300], y, time, event, c["mask"], c["lam"], ties)
        print(f"{ties} job {j} lambda {c['lam']:g}: largest Hessian eigenvalue {top:.4f} = {top / c['L']:.3f} L")
        assert c["lam"] <= top <= c["L"]


@pytest.mark.parametrize("ties", R.TIES)
def test_fista_reaches_the_optimum_within_its_guarantee(case_jobs, ties):
    """F(X_k) - F* <= 2 L |w*|^2 / (k + 1)^2 with L = rho eps + lambda, against scipy's L-BFGS-B on the same objective."""
    (y, event, time, _), jobs = case_jobs
    for (tj, j), c in jobs.items():
        if tj != ties:
            continue
        ws, Fs = R.optimum(y, time, event, c["mask"], c["lam"], ties)
        assert np.abs(R.gradient(ws, y, time, event, c["mask"], c["lam"], ties)).max() <= 1e-6
        for k in (10, 100, 300):
            gap = R.objective(c["X"][k], y, time, event, c["mask"], c["lam"], ties) - Fs
            bound = 2.0 * c["L"] * float(ws @ ws) / (k + 1) ** 2
            print(f"{ties} job {j} lambda {c['lam']:g}: k = {k}: F - F* = {gap:.3e}, bound {bound:.3e}, |w*| = {np.linalg.norm(ws):.2f}")
            assert -1e-10 <= gap <= bound


@pytest.mark.parametrize("ties", R.TIES)
def test_end_to_end_inputs_are_decided_in_float64(ties):
    """The condition of the GPU end-to-end c-index comparison, from float64 alone, on the variant of the case without the added rows:
    under every held-out job, at most 1 % of the comparable pairs have a risk gap under twice the f32 score tolerance
    2 D 2^-24 max|y| |w|; in fact none do."""
    y, event, time, fold, _ = R.e2e_sorted(plain=True)
    c = R.E2E
    held, lam = R.jobs(c["F"], c["strengths"])
    for h, l in zip(held[:-len(c["strengths"])], lam):
        mask = R.train_mask(event, time, fold, h)
        w = R.fista(y, time, event, mask, l, ties, c["steps"])
        rows = np.flatnonzero(fold == h)
        r = y[rows] @ w
        tol = 2.0 * c["D"] * 2.0 ** -24 * np.sqrt((y * y).sum(1).max()) * np.linalg.norm(w)
        ev, t = event[rows] == 1, time[rows]
        comp = ev[:, None] & ((t[None, :] > t[:, None]) | ((t[None, :] == t[:, None]) & ~ev[None, :]))
        close = comp & (np.abs(r[None, :] - r[:, None]) < 2.0 * tol)
        print(f"{ties} fold {h} lambda {l:g}: {close.sum()} of {comp.sum()} comparable pairs under {2 * tol:.2e}, "
              f"c-index {R.cindex(R.cindex_counts(ev, t, r)):.4f}")
        assert comp.sum() > 500 and close.sum() <= R.MAX_UNDECIDED * comp.sum()


# ------------------------------------------------------------------ the public face
def test_probe_is_exported_and_checks_its_arguments():
    assert mirror_amd.CoxProbe is CoxProbe and "CoxProbe" in mirror_amd.__all__
    for kw in (dict(strengths=()), dict(strengths=0.1), dict(strengths=(0.1, 0.0)), dict(strengths=(-1.0,)), dict(strengths=(float("inf"),)),
               dict(strengths=("a",)), dict(ties="exact"), dict(ties=1), dict(ties=None), dict(max_iter=0), dict(max_iter=2.0),
               dict(tol=-1e-3), dict(tol=float("nan")), dict(tol="x"), dict(center=1), dict(check_every=0), dict(check_every=True)):
        with pytest.raises(ValueError):
            CoxProbe(device="cuda", **kw)
    with pytest.raises(MirrorHipError, match="HIP device"):
        CoxProbe(device="cpu")
    p = CoxProbe(device="cuda")
    assert (p.strengths, p.ties, p.max_iter, p.tol, p.center, p.check_every) == ((1e-4, 1e-3, 1e-2, 1e-1), "efron", 2000, 1e-4, True, 16)
    assert CoxProbe(ties="breslow", device="cuda").ties == "breslow"
    x, i3, t3 = torch.zeros((3, 2)), torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.float64)
    with pytest.raises(ValueError, match="emb must be"):
        p.fit(torch.zeros((3, 2), dtype=torch.int64), i3, t3)
    with pytest.raises(ValueError, match="emb must be"):
        p.fit(torch.zeros(3), i3, t3)
    with pytest.raises(MirrorHipError, match="D = 4097"):
        p.fit(torch.zeros((3, 4097)), i3, t3)
    with pytest.raises(ValueError, match="event must be"):
        p.fit(x, torch.zeros(3), t3)
    with pytest.raises(ValueError, match="event must be"):
        p.fit(x, torch.zeros(4, dtype=torch.bool), t3)
    with pytest.raises(ValueError, match="time must be"):
        p.fit(x, i3, i3)
    with pytest.raises(ValueError, match="time must be"):
        p.fit(x, i3, torch.zeros((3, 1)))
    with pytest.raises(ValueError, match="fold must be"):
        p.fit(x, i3, t3, fold=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="fold must be"):
        p.fit(x, i3, t3, fold=[0, 1, 2])
    with pytest.raises(ValueError, match=r"no row of fold\(s\) \[1\]"):            # an empty fold
        p.fit(x, i3, t3, fold=torch.tensor([0, 2, 0]))
    with pytest.raises(ValueError, match="train_rows must be a 1-D int64"):
        p.fit(x, i3, t3, train_rows=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="train_rows must be a 1-D int64"):
        p.fit(x, i3, t3, train_rows=[0, 1])
    with pytest.raises(ValueError, match="train_rows must index the 3 rows"):
        p.fit(x, i3, t3, train_rows=torch.tensor([0, 3]))
    with pytest.raises(MirrorHipError, match="n \\* J <= 2\\^24"):               # 2^21 folds x 4 strengths x 3 rows
        p.fit(x, i3, t3, fold=torch.tensor([0, 1, (1 << 21)]))
    with pytest.raises(MirrorHipError, match="n <= 65536"):
        p.fit(torch.zeros((65537, 2)), torch.zeros(65537, dtype=torch.int64), torch.zeros(65537, dtype=torch.float64))
    for call in (p.evaluate, p.oof_risk, lambda: p.predict_risk(x)):
        with pytest.raises(ValueError, match="nothing is fitted"):
            call()
    with pytest.raises(ValueError, match="strength must be one of"):           # a strength that is not in the list
        p._strength_index(0.5)
    assert p._strength_index(1e-2) == 2


def test_launchers_check_before_they_launch():
    n, D, J = 6, 8, 2
    y, W = torch.zeros((n, D)), torch.zeros((J, D))
    V, G = torch.zeros((J, n)), torch.zeros((n, J))
    tm, ev, fold = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.int32)
    held, r = torch.zeros(J, dtype=torch.int32), torch.zeros(J)
    # coxprobe_scores
    with pytest.raises(ValueError, match="q must be f32"):
        K.coxprobe_scores(y.double(), W)
    with pytest.raises(ValueError, match=r"weights must be f32 \[J, 8\]"):
        K.coxprobe_scores(y, torch.zeros((J, 7)))
    with pytest.raises(ValueError, match=r"weights must be f32 \[J, 8\]"):
        K.coxprobe_scores(y, torch.zeros((J, 1, D)))
    with pytest.raises(ValueError, match=r"V must be a contiguous torch.float32 \[2, 6\]"):
        K.coxprobe_scores(y, W, V=torch.zeros((n, J)))
    with pytest.raises(ValueError, match="V must be a contiguous"):
        K.coxprobe_scores(y, W, V=torch.zeros((n, J)).t())
    with pytest.raises(MirrorHipError, match="HIP device tensors"):           # there is no CPU path
        K.coxprobe_scores(y, W)
    # coxprobe_grad
    grad = lambda **kw: K.coxprobe_grad(**{**dict(V=V, time=tm, event=ev, fold=fold, heldout=held, rscale=r, ties="efron"), **kw})  # noqa: E731
    with pytest.raises(ValueError, match=r"V must be a contiguous f32 \[J, n\]"):
        grad(V=V.double())
    with pytest.raises(ValueError, match=r"V must be a contiguous f32 \[J, n\]"):
        grad(V=G.t())
    with pytest.raises(ValueError, match=r"time must be torch.float64 \[6\]"):
        grad(time=tm.float())
    with pytest.raises(ValueError, match=r"event must be torch.uint8 \[6\]"):
        grad(event=ev.bool())
    with pytest.raises(ValueError, match=r"event must be torch.uint8 \[6\]"):
        grad(event=ev[:5])
    with pytest.raises(ValueError, match=r"fold must be torch.int32 \[6\]"):
        grad(fold=fold.long())
    with pytest.raises(ValueError, match=r"heldout must be torch.int32 \[2\]"):
        grad(heldout=held.long())
    with pytest.raises(ValueError, match=r"rscale must be torch.float32 \[2\]"):
        grad(rscale=torch.zeros(3))
    for ties in ("exact", 1, None):
        with pytest.raises(ValueError, match="ties must be"):
            grad(ties=ties)
    with pytest.raises(ValueError, match=r"G must be a contiguous torch.float32 \[6, 2\]"):
        grad(G=V)
    with pytest.raises(ValueError, match=r"loss must be a contiguous torch.float64 \[2\]"):
        grad(loss=torch.zeros(J))
    with pytest.raises(ValueError, match="workspace must be a contiguous 1-D f64"):
        grad(workspace=torch.zeros(100))
    with pytest.raises(MirrorHipError, match="HIP device tensors"):
        grad()
    # coxprobe_step
    step = lambda **kw: K.coxprobe_step(**{**dict(y=y, G=G, Wx=W, Wz=W.clone(), lam=r, eta=r, beta=0.5), **kw})  # noqa: E731
    with pytest.raises(ValueError, match="y must be f32"):
        step(y=y.double())
    with pytest.raises(ValueError, match=r"Wz must be f32 \[J, 8\]"):
        step(Wz=torch.zeros((J, 2, D)))
    with pytest.raises(ValueError, match=r"Wx must be f32 \[J, 8\]"):
        step(Wx=torch.zeros((J, 9)))
    with pytest.raises(ValueError, match="Wx has 3 jobs, Wz 2"):
        step(Wx=torch.zeros((3, D)))
    with pytest.raises(ValueError, match=r"G must be a contiguous f32 \[6, 2\]"):
        step(G=V)
    with pytest.raises(ValueError, match=r"lam must be torch.float32 \[2\]"):
        step(lam=r.double())
    with pytest.raises(ValueError, match=r"eta must be torch.float32 \[2\]"):
        step(eta=torch.zeros(3))
    for beta in (-0.1, 1.5, float("nan"), True, "x"):
        with pytest.raises(ValueError, match="beta must lie in"):
            step(beta=beta)
    with pytest.raises(ValueError, match=r"gmax_part must be a contiguous torch.float32 \[1, 2\]"):
        step(gmax_part=torch.zeros((2, J)))
    with pytest.raises(MirrorHipError, match="HIP device tensors"):
        step()
    # the workspace's size needs no device
    with pytest.raises(MirrorHipError, match="n \\* J <= 2\\^24"):
        K.coxprobe_workspace(65537, 1, "cpu")
    assert K.coxprobe_workspace(5, 3, "cpu").numel() == (5 * 3 * 28 + 7) // 8


# ------------------------------------------------------------------ the declarations and their refusals
def test_the_entry_points_are_declared_and_exported():
    lib = _lib.load()
    assert lib.mh_version() == _lib.ABI_VERSION == 123
    for name, nargs in {"mh_coxprobe_scores": 6, "mh_coxprobe_grad": 12, "mh_coxprobe_step": 11}.items():
        assert name in _lib.EXPORTS and len(_lib._SIGS[name]) == nargs and hasattr(lib, name), name
    assert "mh_coxprobe_workspace_bytes" in _lib.EXPORTS
    wsb = lib.mh_coxprobe_workspace_bytes
    assert wsb(1, 1) == 32 and wsb(1000, 48) == 1000 * 48 * 28 and wsb(65536, 256) == (1 << 24) * 28
    for n, J in ((0, 1), (65537, 1), (1, 0), (65536, 257), (4097, 4096)):
        assert wsb(n, J) == -1, (n, J)


def _refused(name, match, *args):
    with pytest.raises(MirrorHipError, match=match):
        _lib.call(name, *args)


def test_entry_points_refuse_what_lies_outside_their_limits():
    """Null pointers everywhere: each call must stop in its argument check with MH_EINVAL, and say why, before it launches anything."""
    # mh_coxprobe_scores(q, nq, D, W, J, V)
    sc = lambda nq=10, D=64, J=4: ("mh_coxprobe_scores", None, nq, D, None, J, None)  # noqa: E731
    _refused(*sc(D=0)[:1], r"D = 0 outside \[1, 4096\]", *sc(D=0)[1:])
    _refused(*sc()[:1], r"D = 4097 outside \[1, 4096\]", *sc(D=4097)[1:])
    _refused(*sc()[:1], r"nq = 0 outside \[1, 2\^20\]", *sc(nq=0)[1:])
    _refused(*sc()[:1], r"nq = 1048577 outside \[1, 2\^20\]", *sc(nq=(1 << 20) + 1)[1:])
    _refused(*sc()[:1], r"J = 0 jobs outside", *sc(J=0)[1:])
    _refused(*sc()[:1], r"nq J = 1048576 x 257 scores", *sc(nq=1 << 20, J=257)[1:])
    _refused(*sc()[:1], "null pointer", *sc(nq=1 << 20, J=256)[1:])                # exactly 2^28; the pointers are looked at last
    # mh_coxprobe_grad(V, n, J, time, event, fold, heldout, rscale, ties, G, loss, workspace)
    gr = lambda n=10, J=4, ties=1: ("mh_coxprobe_grad", None, n, J, None, None, None, None, None, ties, None, None, None)  # noqa: E731
    _refused(*gr()[:1], r"n = 0 outside \[1, 65536\]", *gr(n=0)[1:])
    _refused(*gr()[:1], r"n = 65537 outside \[1, 65536\]", *gr(n=65537)[1:])
    _refused(*gr()[:1], r"n J = 10 x 0 scores outside", *gr(J=0)[1:])
    _refused(*gr()[:1], r"n J = 65536 x 257 scores outside \[1, 2\^24\]", *gr(n=65536, J=257)[1:])
    _refused(*gr()[:1], "ties = 2 is neither", *gr(ties=2)[1:])
    _refused(*gr()[:1], "ties = -1 is neither", *gr(ties=-1)[1:])
    _refused(*gr()[:1], "null pointer", *gr(n=65536, J=256)[1:])                   # exactly 2^24
    # mh_coxprobe_step(y, n, D, G, Wx, Wz, lam, eta, beta, J, gmax_part)
    st = lambda n=10, D=64, J=4, beta=0.5: ("mh_coxprobe_step", None, n, D, None, None, None, None, None, beta, J, None)  # noqa: E731
    _refused(*st()[:1], r"D = 0 outside \[1, 4096\]", *st(D=0)[1:])
    _refused(*st()[:1], r"D = 4097 outside \[1, 4096\]", *st(D=4097)[1:])
    _refused(*st()[:1], r"n = 0 outside \[1, 65536\]", *st(n=0)[1:])
    _refused(*st()[:1], r"n = 65537 outside \[1, 65536\]", *st(n=65537)[1:])
    _refused(*st()[:1], r"n J = 10 x 0 score gradients outside", *st(J=0)[1:])
    _refused(*st()[:1], r"n J = 65536 x 257 score gradients outside \[1, 2\^24\]", *st(n=65536, J=257)[1:])
    _refused(*st()[:1], r"beta = 1.5 outside \[0, 1\]", *st(beta=1.5)[1:])
    _refused(*st()[:1], r"beta = nan outside \[0, 1\]", *st(beta=float("nan"))[1:])
    _refused(*st()[:1], "null pointer", *st()[1:])
