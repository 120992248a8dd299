"""MI355X: the survival linear probe (csrc/survprobe.hip, mirror_amd/survprobe.py) against the float64 restatement of
tests/survprobe_ref.py.

Each kernel is compared on what the device itself handed to it (mh_linprobe_step gets the device's own G, the end-to-end checks the
device's own prepared rows and weights), so a kernel's tolerance is that kernel's f32 rounding, derived from the case:

  logits        delta[i, j] = 2 D 2^-24 |y_i| max_t |w_jt|: the k-ordered f32 chain of the tile product (D roundings of partial sums that
                stay below |y_i| |w_jt|, with a factor 2 to spare).  The sigmoid is 1/4-Lipschitz, softplus(v) and softplus(v) - v are
                1-Lipschitz, and at most M bins of a row carry a term.
  expf / log1pf cannot be derived from the number format alone, so it is MEASURED: on inputs whose products and bias adds are exact in
                f32 (small dyadic rationals: the device's logits are float64's), over the shapes of the kernel test, the largest
                |G - G_ref| / (r_j w_i) was 1.34e-07 and the largest mean |w nll - ref| over a job's training rows 5.51e-07 (MI355X,
                2026-10-21, logits up to about 10 in size, up to 64 bins added in f32: the M = 64 case sets the second figure); with a
                margin of 4x: TOL_S = 5.37e-07, TOL_NLL = 2.2e-06 (per training row, summed over a job's rows for its loss).  The
                measurement is repeated on every run and must stay under the constants.
  risk          M (delta / 4 + TOL_S) + M 2^-23 |risk|: every factor sigmoid(-v_t) <= 1 carries the sigmoid's error, the running product
                and the running sum round once per bin.
  weight sums   as tests/test_linprobe_gpu.py derives them (B [k, d] = n 2^-24 sum_i |G[i, k]| |y[i, d]| carried through the update).
"""
import numpy as np
import pytest
import torch

from mirror_amd import SurvivalProbe, kernels as K, survival
from mirror_amd.linprobe import fista_betas
from tests import survprobe_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # half an ulp of a number in [1, 2)
TOL_S = 5.37e-07          # 4 x the measured expf error of a sigmoid, the division and the final roundings (see above)
TOL_NLL = 2.2e-06         # 4 x the measured mean error of w nll over a job's training rows
W_CENS = float(np.float32(0.6))                                               # alpha = 0.4 as the f32 launch scalar the kernel sees
CASES = [(1, 1, 2, 1), (127, 3, 3, 33), (128, 16, 4, 16), (129, 17, 64, 3), (300, 40, 5, 33)]          # n, D, M, J
RISK_CASES = [(1, 1, 2, 1), (129, 17, 64, 2), (300, 40, 4, 5)]                # nq, D, M, S
ids = lambda s: "n%d-D%d-M%d-J%d" % s  # noqa: E731


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()       # a copy: the shared inputs are read-only


def host(t):
    return t.detach().cpu().numpy()


def make_case(n, D, M, J, dyadic=False):
    """Unit rows, weight rows of norm up to 10, bins in [-1, M], events in {0, 1, 2}, folds in [-1, 2]; the pad slots of the weights and
    of the bias hold NaN: whoever looked at one would show it.  dyadic=True: every product and bias add is exact."""
    rng = np.random.default_rng(1000 * n + 10 * D + M)
    Mp = R.cp_of(M)
    W = np.full((J, Mp, D), np.nan, dtype=np.float32)
    b = np.full((J, Mp), np.nan, dtype=np.float32)
    if dyadic:
        p2 = 1 << int(np.ceil(np.log2(np.sqrt(D))))
        y = (rng.integers(-4, 5, (n, D)) / (4.0 * p2)).astype(np.float32)
        W[:, :M] = rng.integers(-8, 9, (J, M, D)) / (1.0 if D <= 3 else 2.0)      # logits up to about 10, as below
        b[:, :M] = rng.integers(-8, 9, (J, M)) / 4.0
    else:
        y = rng.standard_normal((n, D))
        y = (y / np.linalg.norm(y, axis=1, keepdims=True)).astype(np.float32)
        w = rng.standard_normal((J, M, D))
        W[:, :M] = w / np.linalg.norm(w, axis=2, keepdims=True) * rng.uniform(0, 10, (J, M, 1))
        b[:, :M] = rng.standard_normal((J, M))
    bins = rng.integers(-1, M + 1, n).astype(np.int64)
    event = rng.integers(0, 3, n).astype(np.uint8)
    fold = rng.integers(-1, 3, n).astype(np.int32)
    held = rng.integers(-1, 3, J).astype(np.int32)
    bins[0], event[0], fold[0], held[0] = M - 1, 1, 0, -1                     # (row 0, job 0) trains on every bin, also at n = 1
    ntrain = np.array([R.train_mask(bins, event, fold, h, M).sum() for h in held])
    r = (1.0 / np.maximum(ntrain, 1)).astype(np.float32)
    return dict(n=n, D=D, M=M, J=J, Mp=Mp, y=y, W=W, b=b, bins=bins, event=event, fold=fold, held=held, r=r)


def run_grad(c, want_loss=True):
    return K.survprobe_grad(dev(c["y"]), dev(c["W"]), dev(c["b"]), dev(c["bins"]), dev(c["event"]), dev(c["fold"]), dev(c["held"]),
                            dev(c["r"]), W_CENS, c["M"], want_loss=want_loss)


def grad_reference(c):
    """(G_ref / (r w) [n, J, M], w nll_ref [n, J], mask [n, J], delta [n, J], active [n, M]) in float64 from the f32 inputs."""
    y = c["y"].astype(np.float64)
    n, J, M = c["n"], c["J"], c["M"]
    S, nll, mask, delta = np.zeros((n, J, M)), np.zeros((n, J)), np.zeros((n, J), dtype=bool), np.zeros((n, J))
    w = R.row_weight(c["event"], 1.0 - W_CENS)
    for j in range(J):
        W, b = c["W"][j, :M].astype(np.float64), c["b"][j, :M].astype(np.float64)
        mask[:, j] = R.train_mask(c["bins"], c["event"], c["fold"], c["held"][j], M)
        # logit_grad with alpha = 0 and the division by the count undone: sigmoid - target on the active bins
        S[:, j] = R.logit_grad(W, b, y, c["bins"], c["event"], mask[:, j], 0.0) * max(int(mask[:, j].sum()), 1)
        nll[:, j] = w * R.row_nll(W, b, y, c["bins"], c["event"], mask[:, j])
        delta[:, j] = 2 * c["D"] * U * np.linalg.norm(y, axis=1) * np.linalg.norm(W, axis=1).max()
    active = np.arange(M)[None, :] <= c["bins"][:, None]
    return S, nll, mask, delta, active, w


# ------------------------------------------------------------------ 1. mh_survprobe_grad
def test_transcendental_error_is_what_the_constants_say():
    """The measurement behind TOL_S and TOL_NLL: with exact logits the whole error of G / (r w) and of the loss is expf / log1pf's, the
    division's and the final roundings'.  Printed on every run; asserted against the constants, which carry the margin of 4x over the
    figures in the docstring."""
    worst_s = worst_nll = 0.0
    for shape in CASES:
        c = make_case(*shape, dyadic=True)
        G, part = run_grad(c)
        S, nll, mask, _, _, w = grad_reference(c)
        got = host(G).astype(np.float64).reshape(c["n"], c["J"], c["Mp"])[:, :, :c["M"]]
        r = c["r"].astype(np.float64)
        e_s = (np.abs(got / (r[None, :, None] * w[:, None, None]) - S) * mask[:, :, None]).max()
        # the loss is a sum of the rows' terms: compare per training row on average (the f64 sum adds no error of its own)
        nt = np.maximum(mask.sum(0), 1)
        e_nll = (np.abs(host(part).sum(0) - r * nll.sum(0)) / (r * nt)).max()
        print(f"{shape}: |G - G_ref| / (r w) <= {e_s:.3e}, mean |w nll - ref| per row <= {e_nll:.3e}")
        worst_s, worst_nll = max(worst_s, e_s), max(worst_nll, e_nll)
    print(f"measured: sigmoid {worst_s:.3e} (TOL_S {TOL_S:.2e}), nll {worst_nll:.3e} (TOL_NLL {TOL_NLL:.2e})")
    assert worst_s <= TOL_S and worst_nll <= TOL_NLL


@pytest.mark.parametrize("shape", CASES, ids=ids)
def test_grad_against_float64(shape):
    c = make_case(*shape)
    n, J, M, Mp = c["n"], c["J"], c["M"], c["Mp"]
    G, part = run_grad(c)
    assert G.dtype == torch.float32 and tuple(G.shape) == (n, J * Mp) and tuple(part.shape) == ((n + 127) // 128, J)
    got = host(G).astype(np.float64).reshape(n, J, Mp)
    S, nll, mask, delta, active, w = grad_reference(c)
    r = c["r"].astype(np.float64)
    assert mask[0, 0] and (n == 1 or not mask.all())
    assert not np.isnan(got).any()                                            # the pads hold NaN: nobody looked
    assert (got[:, :, M:] == 0).all()                                         # pad columns: exactly 0
    assert (got[~mask] == 0).all()                                            # rows outside train_j: exactly 0
    assert (got[:, :, :M][np.broadcast_to(~active[:, None, :], (n, J, M))] == 0).all()          # bins past T_i: exactly 0
    scale = r[None, :, None] * w[:, None, None]
    err = np.abs(got[:, :, :M] - scale * S)
    tol = scale * (delta[:, :, None] / 4 + TOL_S)
    print(f"{shape}: max |G - G_ref| / (r w) = {(err / scale).max():.3e}, max delta = {delta.max():.3e}, "
          f"worst err / tol = {(err / tol).max():.3f}")
    assert (err <= tol).all()
    loss = host(part).sum(0)
    want = r * nll.sum(0)
    ltol = r * ((M * delta + TOL_NLL) * mask).sum(0)
    print(f"{shape}: max |loss - loss_ref| = {np.abs(loss - want).max():.3e}, worst err / tol = {(np.abs(loss - want) / np.maximum(ltol, 1e-300)).max():.3f}")
    assert (np.abs(loss - want) <= ltol).all()
    G2, part2 = run_grad(c)
    assert torch.equal(G, G2) and torch.equal(part, part2)
    G3, none = run_grad(c, want_loss=False)                                   # without the loss table the gradient is the same
    assert none is None and torch.equal(G, G3)


# ------------------------------------------------------------------ 2. mh_linprobe_step with M in the role of C
def chain_bound(G, y):
    """B [J Mp, D + 1] = n 2^-24 sum_i |G[i, k]| |(y, 1)[i, d]|."""
    y1 = np.concatenate([np.abs(y), np.ones((len(y), 1))], axis=1)
    return len(y) * U * (np.abs(G).T @ y1)


def test_step_against_float64_from_the_device_gradient():
    """mh_linprobe_step, unchanged, on the hazard gradient at a non-power-of-two M: the pads (3 of 8 slots) keep what they held."""
    shape = (129, 17, 5, 3)
    c = make_case(*shape)
    n, D, J, M, Mp = c["n"], c["D"], c["J"], c["M"], c["Mp"]
    rng = np.random.default_rng(7 + n)
    yd = dev(c["y"])
    Gd, _ = run_grad(c)
    G, y = host(Gd).astype(np.float64), c["y"].astype(np.float64)
    full = G.T @ np.concatenate([y, np.ones((n, 1))], axis=1)                 # [J Mp, D + 1]: dW without the penalty, and db
    B = chain_bound(G, y)
    real = np.tile(np.arange(Mp) < M, J)                                      # the slots that are not pads
    lam = rng.uniform(1e-3, 0.1, J).astype(np.float32)
    pad_b = np.where(np.arange(Mp) < M, 0.0, 7.0).astype(np.float32)          # a mark in the pads of the bias

    # (a) Wz = 0, eta = 1, beta = 0: Wx becomes minus the chain, exactly
    ones = torch.ones((J,), device="cuda")
    Wx, Wz = torch.zeros((J, Mp, D), device="cuda"), torch.zeros((J, Mp, D), device="cuda")
    bx, bz = dev(np.tile(pad_b, (J, 1))), dev(np.tile(pad_b, (J, 1)))
    gm = K.linprobe_step(yd, Gd, Wx, bx, Wz, bz, dev(lam), ones, 0.0, M, want_gmax=True)
    assert tuple(gm.shape) == ((D + 1 + 127) // 128, J)
    gotW, gotb = -host(Wx).astype(np.float64).reshape(J * Mp, D), -host(bx).astype(np.float64).reshape(J * Mp)
    eW, eb = np.abs(gotW - full[:, :D])[real], np.abs(gotb - full[:, D])[real]
    print(f"{shape}: dW err / bound <= {(eW / np.maximum(B[real, :D], 1e-300)).max():.3f}, db err / bound <= "
          f"{(eb / np.maximum(B[real, D], 1e-300)).max():.3f} (bound up to {B.max():.2e})")
    assert (eW <= B[real, :D]).all() and (eb <= B[real, D]).all()
    assert torch.equal(Wx, Wz) and torch.equal(bx, bz)                        # beta = 0: Z' = X'
    assert (host(Wx).reshape(J * Mp, D)[~real] == 0).all() and (host(bx).reshape(-1)[~real] == 7.0).all()
    gmax = host(gm.amax(0)).astype(np.float64)
    want = np.abs(np.where(real[:, None], full, 0.0)).reshape(J, Mp * (D + 1)).max(1)
    assert (np.abs(gmax - want) <= np.where(real[:, None], B, 0.0).reshape(J, -1).max(1)).all()

    # (b) a general state, beta = 0.5
    beta = 0.5
    eta = rng.uniform(0.5, 1.0, J).astype(np.float32)
    X0 = np.where(real[:, None], rng.standard_normal((J * Mp, D)), 0.0).astype(np.float32)
    bX0 = np.where(real, rng.standard_normal(J * Mp), 7.0).astype(np.float32)
    Z0 = np.where(real[:, None], c["W"].reshape(J * Mp, D), 0.0).astype(np.float32)
    bZ0 = np.where(real, c["b"].reshape(J * Mp), 7.0).astype(np.float32)
    state = lambda: (dev(X0.reshape(J, Mp, D)), dev(bX0.reshape(J, Mp)), dev(Z0.reshape(J, Mp, D)), dev(bZ0.reshape(J, Mp)))  # noqa: E731
    Wx, bx, Wz, bz = state()
    gm = K.linprobe_step(yd, Gd, Wx, bx, Wz, bz, dev(lam), dev(eta), beta, M, want_gmax=True)
    lamk, etak = np.repeat(lam.astype(np.float64), Mp)[:, None], np.repeat(eta.astype(np.float64), Mp)[:, None]
    Zf = np.concatenate([Z0, bZ0[:, None]], axis=1).astype(np.float64)[real]
    Xf = np.concatenate([X0, bX0[:, None]], axis=1).astype(np.float64)[real]
    pen = np.concatenate([np.ones(D), [0.0]])                                 # the bias is not penalised
    g = full[real] + lamk[real] * pen * Zf
    Xn = Zf - etak[real] * g
    Zn = Xn + beta * (Xn - Xf)
    tg = B[real] + U * (np.abs(g) + B[real])                                  # each rounding is of the DEVICE's value: |ref| + its error
    tX = etak[real] * tg + U * (np.abs(Xn) + etak[real] * tg)
    td = tX + U * (np.abs(Xn - Xf) + tX)                                      # X' - X, X exact
    tZ = tX + beta * td + U * (np.abs(Zn) + tX + beta * td)
    gotX = np.concatenate([host(Wx).reshape(J * Mp, D), host(bx).reshape(J * Mp, 1)], axis=1).astype(np.float64)
    gotZ = np.concatenate([host(Wz).reshape(J * Mp, D), host(bz).reshape(J * Mp, 1)], axis=1).astype(np.float64)
    assert not np.isnan(gotX).any() and not np.isnan(gotZ).any()
    print(f"{shape}: X' err / tol <= {(np.abs(gotX[real] - Xn) / tX).max():.3f}, Z' err / tol <= {(np.abs(gotZ[real] - Zn) / tZ).max():.3f}")
    assert (np.abs(gotX[real] - Xn) <= tX).all() and (np.abs(gotZ[real] - Zn) <= tZ).all()
    for got in (gotX, gotZ):                                                  # pad slots: still exactly 0 and the mark
        assert (got[~real, :D] == 0).all() and (got[~real, D] == 7.0).all()
    again = state()
    gm2 = K.linprobe_step(yd, Gd, *again, dev(lam), dev(eta), beta, M, want_gmax=True)
    assert all(torch.equal(a, b_) for a, b_ in zip(again, (Wx, bx, Wz, bz))) and torch.equal(gm, gm2)


# ------------------------------------------------------------------ 3. mh_survprobe_risk
def risk_tolerance(W, b, y, D, ref):
    """[n'] for one job: M (delta / 4 + TOL_S) + M 2^-23 |ref|."""
    M = W.shape[0]
    delta = 2 * D * U * np.linalg.norm(y, axis=1) * np.linalg.norm(W, axis=1).max()
    return M * (delta / 4 + TOL_S) + M * 2 * U * np.abs(ref)


@pytest.mark.parametrize("shape", RISK_CASES, ids=lambda s: "n%d-D%d-M%d-S%d" % s)
def test_risk_against_float64(shape):
    c = make_case(*shape)
    n, D, M, S = c["n"], c["D"], c["M"], c["J"]
    q, Wd, bd = dev(c["y"]), dev(c["W"]), dev(c["b"])
    risk = K.survprobe_risk(q, Wd, bd, M)
    assert risk.dtype == torch.float32 and tuple(risk.shape) == (S, n)
    got = host(risk).astype(np.float64)
    assert not np.isnan(got).any()                                            # the pads hold NaN: nobody looked
    y = c["y"].astype(np.float64)
    worst = worst_other = 0.0
    for s in range(S):
        W, b = c["W"][s, :M].astype(np.float64), c["b"][s, :M].astype(np.float64)
        ref = R.risk(W, b, y)
        tol = risk_tolerance(W, b, y, D, ref)
        # the definition of survival.risk_scores, on logits formed in float64 and rounded once: within the same bound
        other = host(survival.risk_scores(dev((y @ W.T + b).astype(np.float32)))).astype(np.float64)
        worst, worst_other = max(worst, (np.abs(got[s] - ref) / tol).max()), max(worst_other, (np.abs(got[s] - other) / tol).max())
    print(f"{shape}: worst |risk - ref| / tol = {worst:.3f}, worst |risk - risk_scores| / tol = {worst_other:.3f}")
    assert worst <= 1.0 and worst_other <= 1.0
    assert -M <= got.min() and got.max() <= 0
    assert torch.equal(risk, K.survprobe_risk(q, Wd, bd, M))
    if S > 1:                                                                 # a job's risk does not depend on the jobs beside it
        assert torch.equal(risk[1:2], K.survprobe_risk(q, Wd[1:2], bd[1:2], M))


# ------------------------------------------------------------------ 4. end to end
def pair_tables(ev, t, r):
    """(comparable [i, j], r_j - r_i) in float64: i has the event and j outlives it."""
    same = t[None, :] == t[:, None]
    comp = ev[:, None] & ((t[None, :] > t[:, None]) | (same & ~ev[None, :]))
    return comp, r[None, :] - r[:, None]


@pytest.fixture(scope="module")
def case():
    x, bins, event, time, fold = R.e2e_case()
    return dict(x=x, bins=bins, event=event, time=time, fold=fold)


def fit(case, alpha, **kw):
    c = R.E2E
    p = SurvivalProbe(c["M"], strengths=c["strengths"], alpha=alpha, max_iter=c["steps"], tol=0.0, device="cuda")
    return p.fit(dev(case["x"]), dev(case["bins"]), dev(case["event"]), dev(case["time"]), dev(case["fold"]), **kw)


@pytest.mark.parametrize("alpha", [0.0, 0.4])
def test_fit_end_to_end(case, alpha):
    """The input condition (essentially no comparable pair with a float64 risk gap near the f32 tolerance) is checked for this seed on
    the CPU from float64 alone: tests/test_survprobe_cpu.py::test_end_to_end_inputs_are_decided_in_float64."""
    c, bins, event, time, fold = R.E2E, case["bins"], case["event"], case["time"], case["fold"]
    M, F, S, D, k = c["M"], c["F"], len(c["strengths"]), c["D"], c["steps"]
    J = (F + 1) * S
    p = fit(case, alpha)
    assert p.n_iter_ == k and tuple(p.coef_.shape) == (J, M, D) and tuple(p.intercept_.shape) == (J, M)
    assert p.loss_.dtype == torch.float64 and tuple(p.loss_.shape) == (J,) and tuple(p.grad_inf_.shape) == (J,)
    y = host(p._y).astype(np.float64)                                         # the device's own prepared rows
    y_ref, _ = R.prepare(case["x"], case["x"])
    assert np.abs(y - y_ref).max() <= 1e-6
    W, b = host(p.coef_).astype(np.float64), host(p.intercept_).astype(np.float64)
    held, lam = R.jobs(F, c["strengths"])
    a_eff = 1.0 - float(np.float32(1.0 - alpha))                              # the launch scalar is f32
    masks = [R.train_mask(bins, event, fold, h, M) for h in held]
    assert np.array_equal(host(p.n_train_), [m.sum() for m in masks]) and p.n_train_.dtype == torch.int64
    assert masks[-1].sum() == int(((fold >= 0) & (bins < M) & (event <= 1)).sum()) < int((fold >= 0).sum())
    for j in range(J):
        Ws, bs, Fs = R.optimum(y, bins, event, masks[j], lam[j], a_eff, M)
        L = R.lipschitz(y, lam[j])
        bound = 2.0 * L * float((Ws ** 2).sum() + (bs ** 2).sum()) / (k + 1) ** 2
        delta = 2 * D * U * np.linalg.norm(y, axis=1) * np.linalg.norm(W[j], axis=1).max()
        ltol = float(((M * delta + TOL_NLL) * masks[j]).sum()) / masks[j].sum()
        Fj = R.objective(W[j], b[j], y, bins, event, masks[j], lam[j], a_eff)
        got = float(p.loss_[j])
        print(f"alpha {alpha} job {j} (lambda {lam[j]:g}, holds out {held[j]}): loss_ = {got:.9f}, F64 = {Fj:.9f}, F* = {Fs:.9f}, "
              f"bound {bound:.2e}, f32 tolerance {ltol:.2e}, max |v| = {np.abs(y @ W[j].T + b[j]).max():.1f}")
        assert abs(got - Fj) <= ltol + 1e-12 * abs(Fj)                        # 1e-12: the regulariser's own f64 sums
        assert Fs - ltol <= got <= Fs + bound + ltol

    out = p.evaluate()
    counts, per_job = host(out["counts"]), host(out["per_job"])
    assert counts.shape == (F, S, 5) and counts.dtype == np.int64 and per_job.shape == (F, S) and per_job.dtype == np.float64
    assert out["survprobe_folds"] == F and out["survprobe_n"] == int((fold >= 0).sum()) and out["survprobe_strengths"] == c["strengths"]
    for f in range(F):
        rows = np.flatnonzero(fold == f)
        ev, t = event[rows] == 1, time[rows]
        risks = host(K.survprobe_risk(p._y.index_select(0, dev(rows)), p._Wx[f * S:(f + 1) * S], p._bx[f * S:(f + 1) * S], M))
        for s in range(S):
            j = f * S + s
            # the counts are those of the device's own risks, exactly: integers
            want = R.cindex_counts(ev, t, risks[s])
            assert np.array_equal(counts[f, s], want), (f, s, counts[f, s], want)
            assert per_job[f, s] == (want[0] + 0.5 * want[2]) / want[4]
            # and the float64 c-index of the device's weights differs by the undecided pairs at the most
            r64 = R.risk(W[j], b[j], y[rows])
            rtol = risk_tolerance(W[j], b[j], y[rows], D, r64).max()
            comp, diff = pair_tables(ev, t, r64)
            undecided = int((comp & (np.abs(diff) < 2 * rtol)).sum())
            c64 = float((comp & (diff < 0)).sum() + 0.5 * (comp & (diff == 0)).sum()) / comp.sum()
            print(f"alpha {alpha} fold {f} lambda {lam[j]:g}: c-index {per_job[f, s]:.6f}, float64 {c64:.6f}, {undecided} of "
                  f"{comp.sum()} comparable pairs undecided (risk tolerance {rtol:.2e})")
            assert comp.sum() == want[4] and undecided <= R.MAX_UNDECIDED * comp.sum()
            assert abs(per_job[f, s] - c64) <= undecided / comp.sum() + 1e-15
    mean = per_job.mean(0)
    best = max(range(S), key=lambda s: (mean[s], c["strengths"][s]))
    assert out["survprobe_best_strength"] == c["strengths"][best] and out["survprobe_cindex"] == pytest.approx(mean[best], rel=1e-14)
    assert out["survprobe_cindex_mean"] == pytest.approx(tuple(mean), rel=1e-14)              # three f64 additions and a division
    assert np.allclose(out["survprobe_cindex_std"], per_job.std(0, ddof=1), rtol=1e-12, atol=0)
    assert 0.55 < out["survprobe_cindex"] <= 1.0                              # the synthetic hazard is linear in x: there is signal


def test_train_rows_keep_the_other_rows_out_of_training_and_in_the_scores(case):
    c, bins, event, time, fold = R.E2E, case["bins"], case["event"], case["time"], case["fold"]
    M, F, S = c["M"], c["F"], len(c["strengths"])
    rng = np.random.default_rng(5)
    shots = np.sort(rng.choice(c["n"], 60, replace=False)).astype(np.int64)
    p = fit(case, 0.0, train_rows=dev(shots))
    inside = np.zeros(c["n"], dtype=bool)
    inside[shots] = True
    held, _ = R.jobs(F, c["strengths"])
    masks = np.stack([R.train_mask(bins, event, fold, h, M) & inside for h in held])
    assert np.array_equal(host(p.n_train_), masks.sum(1)) and 0 < masks.sum(1).min() and masks.sum(1).max() <= 60
    bd, ev, fd, heldout, rscale, w_cens = p._train
    assert np.array_equal(host(fd), np.where(inside, np.maximum(fold, -1), -1)) and w_cens == 1.0
    G, _ = K.survprobe_grad(p._y, p._Wx, p._bx, bd, ev, fd, heldout, rscale, w_cens, M)
    G = host(G).reshape(c["n"], len(held), R.cp_of(M))
    assert (G[~inside] == 0).all()                                            # exactly zero gradient outside train_rows
    assert all((G[masks[j], j, 0] != 0).all() for j in range(len(held)))      # bin 0 of a training row always carries a term
    out = p.evaluate()
    counts = host(out["counts"])
    for f in range(F):                                                        # every row of the fold is scored, few-shot or not
        rows = np.flatnonzero(fold == f)
        comp, _ = pair_tables(event[rows] == 1, time[rows], np.zeros(len(rows)))
        assert (counts[f, :, 4] == comp.sum()).all() and (~inside[rows]).sum() > 0
    assert out["survprobe_n"] == int((fold >= 0).sum())


# ------------------------------------------------------------------ 5. behaviour
def test_predict_risk_and_oof_risk(case):
    c, fold = R.E2E, case["fold"]
    M, F, S, D = c["M"], c["F"], len(c["strengths"]), c["D"]
    p = fit(case, 0.0)
    best = p.evaluate()["survprobe_best_strength"]
    rng = np.random.default_rng(3)                                            # 50 fresh rows: rows of the pool under new noise
    fresh = (case["x"][rng.choice(c["n"], 50, replace=False)] + rng.standard_normal((50, D))).astype(np.float32)
    got = host(p.predict_risk(dev(fresh)))
    assert got.dtype == np.float32 and got.shape == (50,)
    q, _ = R.prepare(case["x"], fresh)                                        # with the POOL's mean
    W, b = host(p.coef_).astype(np.float64), host(p.intercept_).astype(np.float64)
    for strength, res in ((best, got), (c["strengths"][0], host(p.predict_risk(dev(fresh), strength=c["strengths"][0])))):
        j = F * S + c["strengths"].index(strength)                            # the all-rows job of that strength
        ref = R.risk(W[j], b[j], q)
        tol = risk_tolerance(W[j], b[j], q, D, ref) + M * np.abs(W[j]).sum(1).max() * 1e-6 / 4      # q itself is f32 on the device
        assert (np.abs(res - ref) <= tol).all(), (strength, (np.abs(res - ref) / tol).max())
    with pytest.raises(ValueError, match="strength must be one of"):
        p.predict_risk(dev(fresh), strength=0.5)
    s = c["strengths"].index(best)
    oof = p.oof_risk()
    assert oof.dtype == torch.float32 and tuple(oof.shape) == (c["n"],)
    assert np.array_equal(np.isnan(host(oof)), fold < 0)                      # NaN outside every fold, and only there
    for f in range(F):
        rows = dev(np.flatnonzero(fold == f))
        want = K.survprobe_risk(p._y.index_select(0, rows), p._Wx[f * S:(f + 1) * S], p._bx[f * S:(f + 1) * S], M)[s]
        assert torch.equal(oof.index_select(0, rows), want)                   # the job that held the row's fold out
    other = c["strengths"][1 - s]
    assert not torch.equal(p.oof_risk(strength=other)[dev(np.flatnonzero(fold >= 0))], oof[dev(np.flatnonzero(fold >= 0))])


def test_fit_stops_at_a_check_below_the_tolerance(case):
    x, bins, event, time, fold = (dev(case[k]) for k in ("x", "bins", "event", "time", "fold"))
    p = SurvivalProbe(4, strengths=(1e-2, 1e-1), max_iter=2000, tol=1e-3, check_every=16, device="cuda").fit(x, bins, event, time, fold)
    g = host(p.grad_inf_)
    print(f"stopped after {p.n_iter_} iterations, grad_inf_ {g.max():.2e}")
    assert p.n_iter_ % 16 == 0 and 16 <= p.n_iter_ < 2000 and g.shape == (8,) and (g <= 1e-3).all()
    q = SurvivalProbe(4, strengths=(1e-2, 1e-1), max_iter=40, tol=1e-3, check_every=16, device="cuda").fit(x, bins, event.bool(), time)
    assert q.n_folds_ == 0 and tuple(q.coef_.shape) == (2, 4, case["x"].shape[1]) and q.n_iter_ <= 40
    assert np.array_equal(host(q.n_train_), [239, 239])                       # fold=None: every row with a valid bin (a bool event is 0 / 1)
    with pytest.raises(ValueError, match="needs folds"):
        q.evaluate()
    with pytest.raises(ValueError, match="needs folds"):
        q.oof_risk(strength=1e-2)
    with pytest.raises(ValueError, match="no best strength"):
        q.predict_risk(x)
    assert tuple(q.predict_risk(x, strength=1e-1).shape) == (240,)


def test_a_fold_without_comparable_pairs_is_left_out_of_the_means(case):
    c, fold, time = R.E2E, case["fold"], case["time"]
    F, S = c["F"], len(c["strengths"])

    def run(event):
        p = SurvivalProbe(c["M"], strengths=c["strengths"], max_iter=16, tol=0.0, device="cuda")
        return p.fit(dev(case["x"]), dev(case["bins"]), dev(event), dev(time), dev(fold)).evaluate()

    event = case["event"].copy()
    event[fold == 1] = 0                                                      # fold 1: everybody censored, no comparable pair
    out = run(event)
    per_job, counts = host(out["per_job"]), host(out["counts"])
    assert np.isnan(per_job[1]).all() and not np.isnan(per_job[[0, 2]]).any() and (counts[1] == 0).all()
    mean = per_job[[0, 2]].mean(0)
    assert out["survprobe_cindex_mean"] == pytest.approx(tuple(mean), rel=1e-14)
    assert np.allclose(out["survprobe_cindex_std"], per_job[[0, 2]].std(0, ddof=1), rtol=1e-12, atol=0)
    best = max(range(S), key=lambda s: (mean[s], c["strengths"][s]))
    assert out["survprobe_best_strength"] == c["strengths"][best] and out["survprobe_folds"] == F
    with pytest.raises(ValueError, match="All samples are censored"):
        run(np.zeros_like(event))
    last = np.zeros_like(event)                                               # one event per fold, at the fold's largest time: nobody outlives it
    for f in range(F):
        rows = np.flatnonzero(fold == f)
        last[rows[np.argmax(time[rows])]] = 1
    with pytest.raises(ValueError, match="no comparable pairs"):
        run(last)


def test_a_nan_row_poisons_exactly_the_jobs_that_train_on_it(case):
    c, fold = R.E2E, case["fold"]
    F, S = c["F"], len(c["strengths"])
    x = case["x"].copy()
    row = int(np.flatnonzero(fold == 1)[0])
    x[row, 3] = np.nan
    p = SurvivalProbe(c["M"], strengths=c["strengths"], max_iter=32, tol=0.0, center=False, device="cuda")
    p.fit(dev(x), dev(case["bins"]), dev(case["event"]), dev(case["time"]), dev(case["fold"]))
    held, _ = R.jobs(F, c["strengths"])
    trains = held != 1                                                        # the row lies in fold 1 and is valid
    assert R.train_mask(case["bins"], case["event"], fold, -1, c["M"])[row] and trains.sum() == (F + 1) * S - S
    bad_w = host(torch.isnan(p.coef_).flatten(1).any(1))
    bad_l, bad_g = host(torch.isnan(p.loss_)), host(torch.isnan(p.grad_inf_))
    assert np.array_equal(bad_w, trains)                                      # the bins up to the row's own turn NaN, the later ones stay finite
    assert np.array_equal(bad_l, trains) and np.array_equal(bad_g, trains)
    clean = SurvivalProbe(c["M"], strengths=c["strengths"], max_iter=32, tol=0.0, center=False, device="cuda")
    keep = np.arange(c["n"]) != row                                           # the jobs that hold fold 1 out never saw the row
    clean.fit(dev(x[keep]), dev(case["bins"][keep]), dev(case["event"][keep]), dev(case["time"][keep]), dev(case["fold"][keep]))
    assert np.array_equal(host(p.n_train_)[~trains], host(clean.n_train_)[~trains])
    # the same sums with one zero term less: 1e-5 is far above any re-association of f32 sums over 32 steps and far below what a
    # changed training set or step size would do to weights of size 1
    assert np.abs(host(p.coef_)[~trains] - host(clean.coef_)[~trains]).max() <= 1e-5


def test_sixteen_iterations_replay_bit_for_bit_from_a_graph():
    c = make_case(300, 40, 5, 33)
    M, J, Mp, D, n = c["M"], c["J"], c["Mp"], c["D"], c["n"]
    yd, bins, ev, fold, held, r = dev(c["y"]), dev(c["bins"]), dev(c["event"]), dev(c["fold"]), dev(c["held"]), dev(c["r"])
    lam = dev(np.linspace(1e-3, 0.1, J).astype(np.float32))
    eta = 1.0 / (0.5 + lam)
    betas = fista_betas(16)

    def start():
        return [torch.zeros((J, Mp, D), device="cuda"), torch.zeros((J, Mp), device="cuda"), torch.zeros((J, Mp, D), device="cuda"),
                torch.zeros((J, Mp), device="cuda")]

    G = torch.empty((n, J * Mp), device="cuda")
    gm = torch.empty(((D + 1 + 127) // 128, J), device="cuda")

    def run(st):
        for beta in betas:                                                    # one linear chain: grad, step, grad, step, ..
            K.survprobe_grad(yd, st[2], st[3], bins, ev, fold, held, r, W_CENS, M, G=G)
            K.linprobe_step(yd, G, st[0], st[1], st[2], st[3], lam, eta, beta, M, gmax_part=gm)

    eager = start()
    run(eager)
    eager_gm = gm.clone()
    torch.cuda.synchronize()
    st = start()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(st)
    for t, s0 in zip(st, start()):                                            # the same start again: capture ran nothing
        t.copy_(s0)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b_) for a, b_ in zip(st, eager)) and torch.equal(gm, eager_gm)
    assert float(eager[0].abs().max()) > 0 and not torch.isnan(eager[0]).any()
