"""float64 numpy restatement of mirror_amd/geneselect.py (GeneSelect): the objective, the FISTA round, the elimination, the choice of
the subset size and the closing report, with the jobs in lockstep and the iteration count of every round as an argument, so that a test
can replay the device's own counts.  Nothing here touches a device; the tests of test_geneselect_cpu.py hold it against sklearn."""
from __future__ import annotations

import math

import numpy as np


def fista_betas(steps: int) -> list:
    out, t = [], 1.0
    for _ in range(steps):
        t1 = (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0
        out.append((t - 1.0) / t1)
        t = t1
    return out


def planted(seed: int = 0, n: int = 96, D: int = 40, C: int = 3, informative: int = 6, folds: int = 4):
    """The planted set of the issue: (x f64 [n, D], labels int64 [n], fold int64 [n]); only the first `informative` columns carry the
    class.  The draws are made in this order and no other."""
    r = np.random.default_rng(seed)
    lab = r.integers(0, C, n)
    x = r.normal(size=(n, D))
    mu = 1.5 * r.normal(size=(C, informative))
    x[:, :informative] += mu[lab]
    x = x * r.uniform(0.5, 3, D) + 2 * r.normal(size=D)
    return x, lab.astype(np.int64), (np.arange(n) % folds).astype(np.int64)


def planted_more(seed: int, n: int, D: int = 40, C: int = 3, informative: int = 6, extra_seed: int = 1000):
    """n further rows of planted(seed)'s recipe: the same class means, scales and shifts, fresh labels and noise."""
    r = np.random.default_rng(seed)
    n0 = 96
    r.integers(0, C, n0)
    r.normal(size=(n0, D))
    mu = 1.5 * r.normal(size=(C, informative))
    scale = r.uniform(0.5, 3, D)
    shift = 2 * r.normal(size=D)
    q = np.random.default_rng(extra_seed + seed)
    lab = q.integers(0, C, n)
    x = q.normal(size=(n, D))
    x[:, :informative] += mu[lab]
    return x * scale + shift, lab.astype(np.int64)


def schedule(D: int, step, min_features: int = 1) -> list:
    """The subset sizes of the rounds, D first: sklearn's `step` (a float in (0, 1): int(max(1, step D)); an int >= 1 as it is)."""
    k = int(max(1, step * D)) if 0.0 < step < 1.0 else int(step)
    sizes = [D]
    while sizes[-1] > min_features:
        sizes.append(sizes[-1] - min(k, sizes[-1] - min_features))
    return sizes


def standardize(x: np.ndarray):
    """(y, mu, rstd): population standard deviation, rstd = 0 for a constant column."""
    mu = x.mean(0)
    sd = np.sqrt(((x - mu) ** 2).mean(0))
    rstd = np.where(sd > 0, 1.0 / np.where(sd > 0, sd, 1.0), 0.0)
    return (x - mu) * rstd, mu, rstd


def targets(lab: np.ndarray, C: int) -> np.ndarray:
    """t [n, C]: +1 at the row's class, -1 elsewhere (rows with a label outside [0, C) are never in train)."""
    t = -np.ones((lab.shape[0], C))
    ok = (lab >= 0) & (lab < C)
    t[np.nonzero(ok)[0], lab[ok]] = 1.0
    return t


def jobs(lab: np.ndarray, fold, C: int):
    """(train bool [J, n], heldout int [J], F): job f < F holds out fold f, job F trains on every valid row."""
    n = lab.shape[0]
    fd = np.zeros(n, np.int64) if fold is None else np.maximum(np.asarray(fold, np.int64), -1)
    F = 0 if fold is None else max(int(fd.max()) + 1, 0)
    heldout = np.array(list(range(F)) + [-1], np.int64)
    valid = (lab >= 0) & (lab < C) & (fd >= 0)
    return valid[None, :] & (fd[None, :] != heldout[:, None]), heldout, F, fd, valid


def objective(W, b, y, T, train, r, lam, mask):
    """F_j [J] at weights W [J, C, D], bias b [J, C]."""
    V = np.einsum("jcd,nd->jnc", W, y) + b[:, None, :]
    H = np.maximum(0.0, 1.0 - T[None] * V) * train[:, :, None]
    return r * (H ** 2).sum((1, 2)) + 0.5 * lam * ((W * mask[:, None, :]) ** 2).sum((1, 2))


def logit_grad(W, b, y, T, train, r):
    """G [J, n, C] = -2 r_j t max(0, 1 - t v) on the training rows, 0 elsewhere; and the logits V."""
    V = np.einsum("jcd,nd->jnc", W, y) + b[:, None, :]
    H = np.maximum(0.0, 1.0 - T[None] * V) * train[:, :, None]
    return -2.0 * r[:, None, None] * T[None] * H, V


def gradient(W, b, y, T, train, r, lam, mask, fit_intercept=True):
    """(dW [J, C, D], db [J, C]) of F_j; masked columns and a pinned bias have gradient 0."""
    G, _ = logit_grad(W, b, y, T, train, r)
    dW = (np.einsum("jnc,nd->jcd", G, y) + lam[:, None, None] * W) * mask[:, None, :]
    db = G.sum(1) if fit_intercept else np.zeros_like(b)
    return dW, db


def step_sizes(y, mask, lam):
    """eta_j = 1 / (2 rho_j + lambda_j), rho_j = 1 + max_i sum_{d active in j} y_id^2."""
    rho = 1.0 + ((y ** 2)[None, :, :] * mask[:, None, :]).sum(2).max(1)
    return 1.0 / (2.0 * rho + lam)


def fista_round(Wx, bx, y, T, train, r, lam, mask, fit_intercept, iters=None, tol=1e-4, max_iter=2000, check_every=16):
    """One round, restarted at t = 1 from (Wx, bx), all jobs in lockstep.  iters: run exactly that many iterations; None: stop as the
    device does, at the first multiple of check_every (below max_iter) where every job's max-norm gradient is <= tol, or at max_iter.
    Returns (Wx, bx, iterations done, the max-norm gradient [J] of the last step)."""
    eta = step_sizes(y, mask, lam)
    Wz, bz = Wx.copy(), bx.copy()
    total = max_iter if iters is None else iters
    done, gmax = 0, np.zeros(Wx.shape[0])
    for beta in fista_betas(total):
        dW, db = gradient(Wz, bz, y, T, train, r, lam, mask, fit_intercept)
        gmax = np.maximum(np.abs(dW).max((1, 2)), np.abs(db).max(1))
        Xn, bn = Wz - eta[:, None, None] * dW, bz - eta[:, None] * db
        Wz, bz = Xn + beta * (Xn - Wx), bn + beta * (bn - bx)
        Wx, bx = Xn, bn
        done += 1
        if iters is None and done % check_every == 0 and done < max_iter and bool((gmax <= tol).all()):
            break
    return Wx, bx, done, gmax


def predict_classes(W, b, y):
    """[J, n]: the first largest v_c."""
    return (np.einsum("jcd,nd->jnc", W, y) + b[:, None, :]).argmax(2)


def eliminate(Wx, mask, elim_round, k: int, rnd: int):
    """Drop every job's k least important active features in place (stable: equal importances by the smaller index).  Returns the
    smallest relative gap (first kept - last dropped) / first kept over the jobs (inf when a job keeps nothing or k = 0)."""
    gap = math.inf
    imp = (Wx ** 2).sum(1)
    for j in range(Wx.shape[0]):
        act = np.nonzero(mask[j])[0]
        order = act[np.argsort(imp[j, act], kind="stable")]
        kk = min(k, act.shape[0])
        drop = order[:kk]
        if 0 < kk < act.shape[0]:
            last, first = imp[j, order[kk - 1]], imp[j, order[kk]]
            gap = min(gap, (first - last) / first if first > 0 else 0.0)
        mask[j, drop] = 0
        elim_round[j, drop] = rnd
        Wx[j][:, drop] = 0.0
    return gap


def choose(correct: np.ndarray, total: np.ndarray, sizes: list):
    """RFECV.fit of sklearn 1.7 on integer counts: correct int [F, R], total int [F].  Returns (the round m whose size has the highest
    score summed over the folds in fold order, ties to the fewest features; the scores f64 [F, R])."""
    scores = correct.astype(np.float64) / total.astype(np.float64)[:, None]
    F, R = scores.shape
    sums = [sum(float(scores[f, e]) for f in range(F)) for e in range(R)]
    best = max(range(R), key=lambda e: (sums[e], -sizes[e]))
    return best, scores


def ranking(elim_round_all: np.ndarray, m: int):
    """(support bool [D], ranking int64 [D]) of the all-rows job's elimination order cut at round m (sklearn's meaning: 1 = selected,
    2 = dropped by the last elimination before m, ..)."""
    e = elim_round_all
    support = (e < 0) | (e >= m)
    return support, np.where(support, 1, m - e + 1).astype(np.int64)


def rfecv(x, lab, fold, C, step=0.05, min_features=1, svm_c=1.0, standardize_rows=True, fit_intercept=True, iters=None, final_iters=None,
          tol=1e-4, max_iter=2000, check_every=16):
    """The whole of GeneSelect.fit.  iters: a list with the iteration count of every round (None: the device's stopping rule);
    final_iters: that of the final fit.  Returns a dict with sklearn's names, `elim_round` [J, D], `n_iter` per round, `gap` (the
    smallest relative importance gap over all jobs and rounds), `correct` / `total` (the integer counts behind the scores)."""
    x = np.asarray(x, np.float64)
    lab = np.asarray(lab, np.int64)
    n, D = x.shape
    if standardize_rows:
        y, mu, rstd = standardize(x)
    else:
        y, mu, rstd = x, np.zeros(D), np.ones(D)
    train, heldout, F, fd, valid = jobs(lab, fold, C)
    J = F + 1
    T = targets(lab, C)
    ntr = train.sum(1)
    r = np.where(ntr > 0, 1.0 / np.maximum(ntr, 1), 0.0)
    lam = np.where(ntr > 0, 1.0 / (svm_c * np.maximum(ntr, 1)), 1.0 / svm_c)
    sizes = schedule(D, step, min_features)
    R = len(sizes)
    Wx, bx = np.zeros((J, C, D)), np.zeros((J, C))
    mask = np.ones((J, D), np.uint8)
    elim_round = -np.ones((J, D), np.int64)
    correct, total = np.zeros((F, R), np.int64), np.zeros(F, np.int64)
    n_iter, gap = [], math.inf
    for e in range(R):
        Wx, bx, done, _ = fista_round(Wx, bx, y, T, train, r, lam, mask, fit_intercept, None if iters is None else iters[e], tol,
                                      max_iter, check_every)
        n_iter.append(done)
        pred = predict_classes(Wx, bx, y)
        for f in range(F):
            rows = valid & (fd == f)
            correct[f, e] = int((pred[f, rows] == lab[rows]).sum())
            total[f] = int(rows.sum())
        if e + 1 < R:
            gap = min(gap, eliminate(Wx, mask, elim_round, sizes[e] - sizes[e + 1], e))
    out = {"sizes": sizes, "elim_round": elim_round, "n_iter": n_iter, "gap": gap, "correct": correct, "total": total, "mu": mu,
           "rstd": rstd}
    if F > 0:
        m, scores = choose(correct, total, sizes)
        out["cv_results"] = {"n_features": sizes[::-1], "mean_test_score": scores.mean(0)[::-1], "std_test_score": scores.std(0)[::-1]}
        for f in range(F):
            out["cv_results"][f"split{f}_test_score"] = scores[f][::-1]
    else:
        m = R - 1
    support, rank = ranking(elim_round[J - 1], m)
    out["support"], out["ranking"], out["n_features"] = support, rank, int(support.sum())
    W1, b1, done, _ = fista_round(np.zeros((1, C, D)), np.zeros((1, C)), y, T, train[J - 1:], r[J - 1:], lam[J - 1:],
                                  support[None, :].astype(np.uint8), fit_intercept, final_iters, tol, max_iter, check_every)
    out["coef"], out["intercept"], out["final_iter"] = W1[0], b1[0], done
    return out


def report(conf: np.ndarray):
    """accuracy and weighted precision / recall / F1 of a confusion table conf[label, prediction] (sklearn's zero_division=0)."""
    conf = conf.astype(np.float64)
    tp, sup, prd = np.diag(conf), conf.sum(1), conf.sum(0)
    prec = np.where(prd > 0, tp / np.where(prd > 0, prd, 1), 0.0)
    rec = np.where(sup > 0, tp / np.where(sup > 0, sup, 1), 0.0)
    f1 = np.where(sup + prd > 0, 2 * tp / np.where(sup + prd > 0, sup + prd, 1), 0.0)
    w = sup / sup.sum()
    return {"accuracy": tp.sum() / sup.sum(), "precision": (w * prec).sum(), "recall": (w * rec).sum(), "f1": (w * f1).sum()}
