"""MI355X: the linear probe (csrc/linprobe.hip, mirror_amd/linprobe.py) against the float64 restatement of tests/linprobe_ref.py.

Each kernel is compared on what the device itself handed to it (mh_linprobe_step gets the device's own G), so a kernel's tolerance is
that kernel's f32 rounding, derived from the case:

  logits       delta[i, j] = 2 D 2^-24 max_c |y_i| |w_jc|: the k-ordered f32 chain of the tile product (D roundings of partial sums that
               stay below |y_i| |w_jc|, with a factor 2 to spare).  The softmax is 1-Lipschitz from the max norm of the logits to that of
               the probabilities, CE 2-Lipschitz.
  expf / logf  cannot be derived from the number format alone, so it is MEASURED: on inputs whose products and bias adds are exact in f32
               (small dyadic rationals: the device's logits are float64's), over the shapes of the kernel test, the largest
               |G - G_ref| / r_j was 4.81e-07 and the largest mean |CE - CE_ref| over a job's training rows 9.20e-08 (MI355X,
               2026-10-21, logits up to about 10 in size); with a margin of 4x: TOL_P = 1.93e-06, TOL_CE = 3.7e-07 (per training row,
               summed over a job's rows for its loss).  The measurement is repeated on every run and must stay under the constants.
  weight sums  B[k, d] = n 2^-24 sum_i |G[i, k]| |y[i, d]|: one row-ordered f32 chain of n terms.  With Wz = 0, eta = 1, beta = 0 the
               updated Wx is minus the chain itself, exactly, so dW and db are recovered without a further rounding.  The update from a
               general state rounds once in each of g = fmaf(lam, Z, sum), X' = fmaf(-eta, g, Z), X' - X and Z' = fmaf(beta, X' - X, X'):
               its tolerance is B carried through the update plus 2^-24 of each of those results.
"""
import numpy as np
import pytest
import torch

from mirror_amd import LinearProbe, kernels as K
from mirror_amd.linprobe import fista_betas
from tests import linprobe_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # half an ulp of a number in [1, 2)
TOL_P = 1.93e-06          # 4 x the measured expf / logf error of a probability (see above)
TOL_CE = 3.7e-07          # 4 x the measured mean error of lse - v_label over a job's training rows
CASES = [(1, 1, 2, 1), (127, 3, 3, 33), (128, 16, 5, 16), (129, 17, 64, 3), (300, 40, 3, 33)]          # n, D, C, J


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()       # a copy: the shared inputs are read-only


def host(t):
    return t.detach().cpu().numpy()


def make_case(n, D, C, J, dyadic=False):
    """Unit rows, weight rows of norm up to 10, labels in [-1, C], folds in [-1, 2]; dyadic=True: every product and bias add is exact."""
    rng = np.random.default_rng(1000 * n + 10 * D + C)
    Cp = R.cp_of(C)
    W = np.zeros((J, Cp, D), dtype=np.float32)
    b = np.full((J, Cp), -np.inf, dtype=np.float32)
    if dyadic:
        p2 = 1 << int(np.ceil(np.log2(np.sqrt(D))))
        y = (rng.integers(-4, 5, (n, D)) / (4.0 * p2)).astype(np.float32)
        W[:, :C] = rng.integers(-8, 9, (J, C, D)) / (1.0 if D <= 3 else 2.0)      # logits up to about 10, as below
        b[:, :C] = rng.integers(-8, 9, (J, C)) / 4.0
    else:
        y = rng.standard_normal((n, D))
        y = (y / np.linalg.norm(y, axis=1, keepdims=True)).astype(np.float32)
        w = rng.standard_normal((J, C, D))
        W[:, :C] = w / np.linalg.norm(w, axis=2, keepdims=True) * rng.uniform(0, 10, (J, C, 1))
        b[:, :C] = rng.standard_normal((J, C))
    labels = rng.integers(-1, C + 1, n).astype(np.int64)
    fold = rng.integers(-1, 3, n).astype(np.int32)
    held = rng.integers(-1, 3, J).astype(np.int32)
    labels[0], fold[0], held[0] = C - 1, 0, -1                                # (row 0, job 0) trains whatever the draw, also at n = 1
    ntrain = np.array([R.train_mask(labels, fold, h, C).sum() for h in held])
    r = (1.0 / np.maximum(ntrain, 1)).astype(np.float32)
    return dict(n=n, D=D, C=C, J=J, Cp=Cp, y=y, W=W, b=b, labels=labels, fold=fold, held=held, r=r)


def run_grad(c):
    G, part = K.linprobe_grad(dev(c["y"]), dev(c["W"]), dev(c["b"]), dev(c["labels"]), dev(c["fold"]), dev(c["held"]), dev(c["r"]), c["C"],
                              want_loss=True)
    return G, part


def grad_reference(c):
    """(G_ref [n, J, C], CE_ref [n, J], mask [n, J], delta [n, J]) in float64 from the f32 inputs."""
    y = c["y"].astype(np.float64)
    n, J, C = c["n"], c["J"], c["C"]
    G, ce, mask, delta = np.zeros((n, J, C)), np.zeros((n, J)), np.zeros((n, J), dtype=bool), np.zeros((n, J))
    for j in range(J):
        W, b = c["W"][j, :C].astype(np.float64), c["b"][j, :C].astype(np.float64)
        mask[:, j] = R.train_mask(c["labels"], c["fold"], c["held"][j], C)
        G[:, j] = R.logit_grad(W, b, y, c["labels"], mask[:, j]) * max(int(mask[:, j].sum()), 1) * float(c["r"][j])
        ce[:, j] = R.row_ce(W, b, y, c["labels"], mask[:, j])
        delta[:, j] = 2 * c["D"] * U * np.linalg.norm(y, axis=1) * np.linalg.norm(W, axis=1).max()
    return G, ce, mask, delta


# ------------------------------------------------------------------ 1. mh_linprobe_grad
def test_transcendental_error_is_what_the_constants_say():
    """The measurement behind TOL_P and TOL_CE: with exact logits the whole error of G / r and of the loss is expf / logf's and the final
    roundings'.  Printed on every run; asserted against the constants, which carry the margin of 4x over the figures in the docstring."""
    worst_p = worst_ce = 0.0
    for shape in CASES:
        c = make_case(*shape, dyadic=True)
        G, part = run_grad(c)
        Gr, ce, mask, _ = grad_reference(c)
        got = host(G).astype(np.float64).reshape(c["n"], c["J"], c["Cp"])[:, :, :c["C"]]
        r = c["r"].astype(np.float64)
        e_p = (np.abs(got - Gr) / r[None, :, None]).max()
        # the loss is a sum of the rows' CE: compare per training row on average (the f64 sum adds no error of its own)
        nt = np.maximum(mask.sum(0), 1)
        e_ce = (np.abs(host(part).sum(0) - r * ce.sum(0)) / (r * nt)).max()
        print(f"{shape}: |G - G_ref| / r <= {e_p:.3e}, mean |CE - CE_ref| per row <= {e_ce:.3e}")
        worst_p, worst_ce = max(worst_p, e_p), max(worst_ce, e_ce)
    print(f"measured: probabilities {worst_p:.3e} (TOL_P {TOL_P:.1e}), CE {worst_ce:.3e} (TOL_CE {TOL_CE:.1e})")
    assert worst_p <= TOL_P and worst_ce <= TOL_CE


@pytest.mark.parametrize("shape", CASES, ids=lambda s: "n%d-D%d-C%d-J%d" % s)
def test_grad_against_float64(shape):
    c = make_case(*shape)
    n, J, C, Cp = c["n"], c["J"], c["C"], c["Cp"]
    G, part = run_grad(c)
    assert G.dtype == torch.float32 and tuple(G.shape) == (n, J * Cp) and tuple(part.shape) == ((n + 127) // 128, J)
    got = host(G).astype(np.float64).reshape(n, J, Cp)
    Gr, ce, mask, delta = grad_reference(c)
    r = c["r"].astype(np.float64)
    assert mask[0, 0] and (n == 1 or not mask.all())
    assert not np.isnan(got).any()
    assert (got[:, :, C:] == 0).all()                                         # pad columns: exactly 0
    assert (got[~mask] == 0).all()                                            # rows outside train_j: exactly 0
    err = np.abs(got[:, :, :C] - Gr)
    tol = r[None, :, None] * (delta[:, :, None] + TOL_P)
    print(f"{shape}: max |G - G_ref| / r = {(err / r[None, :, None]).max():.3e}, max delta = {delta.max():.3e}, "
          f"worst err / tol = {(err / tol).max():.3f}")
    assert (err <= tol).all()
    # every (row, job) sums to zero: the logit error does not enter (any softmax sums to 1), expf's C roundings and lse's do
    rowsum = np.abs(got.sum(2))
    assert (rowsum <= r[None, :] * (TOL_P + C * 2 * U)).all(), (rowsum / r[None, :]).max()
    loss = host(part).sum(0)
    want = r * ce.sum(0)
    ltol = r * ((2 * delta + TOL_CE) * mask).sum(0)
    print(f"{shape}: max |loss - loss_ref| = {np.abs(loss - want).max():.3e}, worst err / tol = {(np.abs(loss - want) / np.maximum(ltol, 1e-300)).max():.3f}")
    assert (np.abs(loss - want) <= ltol).all()
    G2, part2 = run_grad(c)
    assert torch.equal(G, G2) and torch.equal(part, part2)
    # without the loss table the gradient is the same
    G3, none = K.linprobe_grad(dev(c["y"]), dev(c["W"]), dev(c["b"]), dev(c["labels"]), dev(c["fold"]), dev(c["held"]), dev(c["r"]), C)
    assert none is None and torch.equal(G, G3)


# ------------------------------------------------------------------ 2. mh_linprobe_step
def chain_bound(G, y):
    """B [J Cp, D + 1] = n 2^-24 sum_i |G[i, k]| |(y, 1)[i, d]|."""
    y1 = np.concatenate([np.abs(y), np.ones((len(y), 1))], axis=1)
    return len(y) * U * (np.abs(G).T @ y1)


@pytest.mark.parametrize("shape", CASES, ids=lambda s: "n%d-D%d-C%d-J%d" % s)
def test_step_against_float64_from_the_device_gradient(shape):
    c = make_case(*shape)
    n, D, J, C, Cp = c["n"], c["D"], c["J"], c["C"], c["Cp"]
    rng = np.random.default_rng(7 + n)
    yd = dev(c["y"])
    Gd, _ = run_grad(c)
    G, y = host(Gd).astype(np.float64), c["y"].astype(np.float64)
    full = G.T @ np.concatenate([y, np.ones((n, 1))], axis=1)                 # [J Cp, D + 1]: dW without the penalty, and db
    B = chain_bound(G, y)
    real = np.tile(np.arange(Cp) < C, J)                                      # the slots that are not pads
    lam = rng.uniform(1e-3, 0.1, J).astype(np.float32)
    pad_b = np.where(np.arange(Cp) < C, 0.0, -np.inf).astype(np.float32)

    # (a) Wz = 0, eta = 1, beta = 0: Wx becomes minus the chain, exactly
    ones = torch.ones((J,), device="cuda")
    Wx, Wz = torch.zeros((J, Cp, D), device="cuda"), torch.zeros((J, Cp, D), device="cuda")
    bx, bz = dev(np.tile(pad_b, (J, 1))), dev(np.tile(pad_b, (J, 1)))
    gm = K.linprobe_step(yd, Gd, Wx, bx, Wz, bz, dev(lam), ones, 0.0, C, want_gmax=True)
    assert tuple(gm.shape) == ((D + 1 + 127) // 128, J)
    gotW, gotb = -host(Wx).astype(np.float64).reshape(J * Cp, D), -host(bx).astype(np.float64).reshape(J * Cp)
    eW, eb = np.abs(gotW - full[:, :D])[real], np.abs(gotb - full[:, D])[real]
    print(f"{shape}: dW err / bound <= {(eW / np.maximum(B[real, :D], 1e-300)).max():.3f}, db err / bound <= "
          f"{(eb / np.maximum(B[real, D], 1e-300)).max():.3f} (bound up to {B.max():.2e})")
    assert (eW <= B[real, :D]).all() and (eb <= B[real, D]).all()
    assert torch.equal(Wx, Wz) and torch.equal(bx, bz)                        # beta = 0: Z' = X'
    assert (host(Wx).reshape(J * Cp, D)[~real] == 0).all() and np.isneginf(host(bx).reshape(-1)[~real]).all()
    gmax = host(gm.amax(0)).astype(np.float64)
    want = np.abs(np.where(real[:, None], full, 0.0)).reshape(J, Cp * (D + 1)).max(1)
    assert (np.abs(gmax - want) <= np.where(real[:, None], B, 0.0).reshape(J, -1).max(1)).all()

    # (b) a general state, beta = 0.5
    beta = 0.5
    eta = rng.uniform(0.5, 1.0, J).astype(np.float32)
    X0 = np.where(real[:, None], rng.standard_normal((J * Cp, D)), 0.0).astype(np.float32)
    bX0 = np.where(real, rng.standard_normal(J * Cp), -np.inf).astype(np.float32)
    Z0, bZ0 = c["W"].reshape(J * Cp, D), c["b"].reshape(J * Cp)
    state = lambda: (dev(X0.reshape(J, Cp, D)), dev(bX0.reshape(J, Cp)), dev(Z0.reshape(J, Cp, D)), dev(bZ0.reshape(J, Cp)))  # noqa: E731
    Wx, bx, Wz, bz = state()
    gm = K.linprobe_step(yd, Gd, Wx, bx, Wz, bz, dev(lam), dev(eta), beta, C, want_gmax=True)
    lamk, etak = np.repeat(lam.astype(np.float64), Cp)[:, None], np.repeat(eta.astype(np.float64), Cp)[:, None]
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
    gotX = np.concatenate([host(Wx).reshape(J * Cp, D), host(bx).reshape(J * Cp, 1)], axis=1).astype(np.float64)
    gotZ = np.concatenate([host(Wz).reshape(J * Cp, D), host(bz).reshape(J * Cp, 1)], axis=1).astype(np.float64)
    assert not np.isnan(gotX).any() and not np.isnan(gotZ).any()
    print(f"{shape}: X' err / tol <= {(np.abs(gotX[real] - Xn) / tX).max():.3f}, Z' err / tol <= {(np.abs(gotZ[real] - Zn) / tZ).max():.3f}")
    assert (np.abs(gotX[real] - Xn) <= tX).all() and (np.abs(gotZ[real] - Zn) <= tZ).all()
    for got in (gotX, gotZ):                                                  # pad slots: still exactly 0 and -inf
        assert (got[~real, :D] == 0).all() and np.isneginf(got[~real, D]).all()
    gj = np.zeros((J * Cp, D + 1))
    gj[real] = np.abs(g)
    tj = np.zeros((J * Cp, D + 1))
    tj[real] = tg
    assert (np.abs(host(gm.amax(0)) - gj.reshape(J, -1).max(1)) <= tj.reshape(J, -1).max(1)).all()
    again = state()
    gm2 = K.linprobe_step(yd, Gd, *again, dev(lam), dev(eta), beta, C, want_gmax=True)
    assert all(torch.equal(a, b_) for a, b_ in zip(again, (Wx, bx, Wz, bz))) and torch.equal(gm, gm2)


# ------------------------------------------------------------------ 3. end to end
@pytest.fixture(scope="module")
def e2e():
    x, labels, fold = R.e2e_case()
    c = R.E2E
    p = LinearProbe(c["C"], strengths=c["strengths"], max_iter=c["steps"], tol=0.0, device="cuda")
    p.fit(dev(x), dev(labels), dev(fold))
    y, ref = R.e2e_reference(x, labels, fold)
    return dict(x=x, labels=labels, fold=fold, p=p, y=y, ref=ref)


def test_fit_end_to_end_reaches_the_guaranteed_objective(e2e):
    c, p, y, labels = R.E2E, e2e["p"], e2e["y"], e2e["labels"]
    J = (c["F"] + 1) * len(c["strengths"])
    assert p.n_iter_ == c["steps"] and tuple(p.coef_.shape) == (J, c["C"], c["D"]) and tuple(p.intercept_.shape) == (J, c["C"])
    assert p.loss_.dtype == torch.float64 and tuple(p.loss_.shape) == (J,) and tuple(p.grad_inf_.shape) == (J,)
    assert np.array_equal(host(p.n_train_), [job["mask"].sum() for job in e2e["ref"]]) and p.n_train_.dtype == torch.int64
    W, b = host(p.coef_).astype(np.float64), host(p.intercept_).astype(np.float64)
    for j, job in enumerate(e2e["ref"]):
        Ws, bs, Fs = R.sklearn_optimum(y, labels, job["mask"], job["lam"], c["C"])
        L = R.lipschitz(y, job["lam"])
        bound = 2.0 * L * float((Ws ** 2).sum() + (bs ** 2).sum()) / (c["steps"] + 1) ** 2
        W32, b32 = R.fista(y, labels, job["mask"], job["lam"], c["C"], c["steps"], round_grad=True)
        F64 = R.objective(job["W"], job["b"], y, labels, job["mask"], job["lam"])
        slack = 4.0 * abs(F64 - R.objective(W32, b32, y, labels, job["mask"], job["lam"]))
        F = R.objective(W[j], b[j], y, labels, job["mask"], job["lam"])
        print(f"job {j} (lambda {job['lam']:g}, holds out {job['heldout']}): F = {F:.9f}, F* = {Fs:.9f}, F64 = {F64:.9f}, "
              f"bound {bound:.2e}, slack {slack:.2e}, loss_ {float(p.loss_[j]):.9f}")
        assert F <= Fs + bound + slack


def test_fit_end_to_end_predictions_and_scores(e2e):
    c, p, y, labels, fold = R.E2E, e2e["p"], e2e["y"], e2e["labels"], e2e["fold"]
    S = len(c["strengths"])
    out = p.evaluate()
    per_job = host(out["per_job"])
    assert per_job.shape == (c["F"], S, 3) and out["linprobe_folds"] == c["F"] and out["linprobe_n"] == int((fold >= 0).sum())
    skipped = total = 0
    for f in range(c["F"]):
        rows = np.flatnonzero(fold == f)
        got = host(K.fewshot_predict(p._y.index_select(0, dev(rows)), p._Wx[f * S:(f + 1) * S], p._bx[f * S:(f + 1) * S], c["C"]))
        for s in range(S):
            job = e2e["ref"][f * S + s]
            want, margin = R.predict(job["W"], job["b"], y[rows])
            decided = margin >= R.MARGIN
            assert np.array_equal(got[s][decided], want[decided]), (f, s)
            skipped += int((~decided).sum())
            total += len(rows)
        # evaluate()'s figures are those of the device's own predictions, exactly: they come from integer counts
        assert np.array_equal(per_job[f], R.tally(got, labels[rows], c["C"])[2])
    print(f"{skipped} of {total} held-out (row, job) pairs undecided in float64")
    assert skipped <= R.MAX_UNDECIDED * total
    mean = per_job.mean(0)
    best = max(range(S), key=lambda s: (mean[s, 0], c["strengths"][s]))
    assert out["linprobe_best_strength"] == c["strengths"][best] and out["linprobe_acc"] == mean[best, 0]
    assert out["linprobe_acc_mean"] == tuple(mean[:, 0]) and out["linprobe_f1_mean"] == tuple(mean[:, 2])
    assert np.allclose(out["linprobe_bacc_std"], per_job[:, :, 1].std(0, ddof=1), rtol=1e-12, atol=0)


def test_predict_uses_the_all_rows_job_of_the_best_strength(e2e):
    c, p = R.E2E, e2e["p"]
    S = len(c["strengths"])
    rng = np.random.default_rng(3)                                            # 50 fresh rows: rows of the pool under new noise
    fresh = (e2e["x"][rng.choice(c["n"], 50, replace=False)] + rng.standard_normal((50, c["D"]))).astype(np.float32)
    best = p.evaluate()["linprobe_best_strength"]
    got = host(p.predict(dev(fresh)))
    assert got.dtype == np.int32 and got.shape == (50,)
    q, _ = R.prepare(e2e["x"], fresh)                                         # with the POOL's mean
    job = e2e["ref"][c["F"] * S + c["strengths"].index(best)]
    assert job["heldout"] == -1
    want, margin = R.predict(job["W"], job["b"], q)
    decided = margin >= R.MARGIN
    assert decided.sum() >= 45 and np.array_equal(got[decided], want[decided])
    other = c["strengths"][0] if best != c["strengths"][0] else c["strengths"][-1]
    job = e2e["ref"][c["F"] * S + c["strengths"].index(other)]
    want, margin = R.predict(job["W"], job["b"], q)
    assert np.array_equal(host(p.predict(dev(fresh), strength=other))[margin >= R.MARGIN], want[margin >= R.MARGIN])
    with pytest.raises(ValueError, match="strength must be one of"):
        p.predict(dev(fresh), strength=0.5)


# ------------------------------------------------------------------ 4. stopping
def test_fit_stops_at_a_check_below_the_tolerance():
    x, labels, fold = R.e2e_case()
    p = LinearProbe(3, strengths=(1e-2, 1e-1), max_iter=2000, tol=1e-3, check_every=16, device="cuda").fit(dev(x), dev(labels), dev(fold))
    g = host(p.grad_inf_)
    print(f"stopped after {p.n_iter_} iterations, grad_inf_ {g.max():.2e}")
    assert p.n_iter_ % 16 == 0 and 16 <= p.n_iter_ < 2000 and g.shape == (8,) and (g <= 1e-3).all()
    q = LinearProbe(3, strengths=(1e-2, 1e-1), max_iter=40, tol=1e-3, check_every=16, device="cuda").fit(dev(x), dev(labels))
    assert q.n_folds_ == 0 and tuple(q.coef_.shape) == (2, 3, x.shape[1]) and q.n_iter_ <= 40
    assert np.array_equal(host(q.n_train_), [298, 298])                       # fold=None: every row with a valid label
    with pytest.raises(ValueError, match="needs folds"):
        q.evaluate()
    with pytest.raises(ValueError, match="no best strength"):
        q.predict(dev(x))


# ------------------------------------------------------------------ 5. graph replay
def test_sixteen_iterations_replay_bit_for_bit_from_a_graph():
    c = make_case(300, 40, 3, 33)
    C, J, Cp, D, n = c["C"], c["J"], c["Cp"], c["D"], c["n"]
    yd, lab, fold, held, r = dev(c["y"]), dev(c["labels"]), dev(c["fold"]), dev(c["held"]), dev(c["r"])
    lam = dev(np.linspace(1e-3, 0.1, J).astype(np.float32))
    eta = 1.0 / (1.0 + lam)
    betas = fista_betas(16)
    pad_b = dev(np.tile(np.where(np.arange(Cp) < C, 0.0, -np.inf).astype(np.float32), (J, 1)))

    def start():
        return [torch.zeros((J, Cp, D), device="cuda"), pad_b.clone(), torch.zeros((J, Cp, D), device="cuda"), pad_b.clone()]

    G = torch.empty((n, J * Cp), device="cuda")
    gm = torch.empty(((D + 1 + 127) // 128, J), device="cuda")

    def run(st):
        for beta in betas:                                                    # one linear chain: grad, step, grad, step, ..
            K.linprobe_grad(yd, st[2], st[3], lab, fold, held, r, C, G=G)
            K.linprobe_step(yd, G, st[0], st[1], st[2], st[3], lam, eta, beta, C, gmax_part=gm)

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
