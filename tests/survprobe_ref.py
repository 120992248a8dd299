"""The survival linear probe (csrc/survprobe.hip, mirror_amd/survprobe.py) restated in float64 numpy from the header text: the
objective of one job, its logit gradient, the FISTA iteration, the risk, the concordance pair counts and the time bins.  Shared by
tests/test_survprobe_{cpu,gpu}.py; the preparation of the rows is tests/fewshot_ref.py's.

    nll_i   = sum_{t < T_i} softplus(v_t) + softplus(v_T) - e_i v_T,      v = W y_i + b
    F(W, b) = r sum_{i in train} w_i nll_i + (lam / 2) |W|^2,             r = 1 / |train|,  w_i = 1 if e_i == 1 else 1 - alpha
"""
import numpy as np

from tests.fewshot_ref import cp_of, prepare  # noqa: F401  (re-exported)
from tests.linprobe_ref import betas, jobs  # noqa: F401  (re-exported)


def train_mask(bins, event, fold, heldout, M):
    bins, event, fold = np.asarray(bins), np.asarray(event), np.asarray(fold)
    return (bins >= 0) & (bins < M) & ((event == 0) | (event == 1)) & (fold >= 0) & (fold != heldout)


def softplus(v):
    return np.maximum(v, 0.0) + np.log1p(np.exp(-np.abs(v)))


def sigmoid(v):
    e = np.exp(-np.abs(v))
    return np.where(v >= 0, 1.0, e) / (1.0 + e)


def _terms(bins, event, mask, M):
    """(active [n, M]: t <= T_i on the training rows, target [n, M]: e_i at t = T_i)."""
    t = np.arange(M)[None, :]
    T = np.asarray(bins)[:, None]
    active = (t <= T) & np.asarray(mask)[:, None]
    target = ((t == T) & (np.asarray(event)[:, None] == 1) & active).astype(np.float64)
    return active, target


def row_weight(event, alpha):
    return np.where(np.asarray(event) == 1, 1.0, 1.0 - alpha)


def row_nll(W, b, y, bins, event, mask):
    """nll_i of the training rows (0 elsewhere) WITHOUT the weight w_i, float64 [n]."""
    v = y @ W.T + b
    active, target = _terms(bins, event, mask, W.shape[0])
    return np.where(active, softplus(v) - target * v, 0.0).sum(1)


def logit_grad(W, b, y, bins, event, mask, alpha):
    """r w_i (sigmoid(v_t) - [t = T_i] e_i) over t <= T_i of the training rows, 0 elsewhere: float64 [n, M]."""
    v = y @ W.T + b
    active, target = _terms(bins, event, mask, W.shape[0])
    m = max(int(np.asarray(mask).sum()), 1)
    return np.where(active, row_weight(event, alpha)[:, None] * (sigmoid(v) - target), 0.0) / m


def objective(W, b, y, bins, event, mask, lam, alpha):
    m = int(np.asarray(mask).sum())
    data = float((row_weight(event, alpha) * row_nll(W, b, y, bins, event, mask)).sum()) / m if m else 0.0
    return data + 0.5 * lam * float((W * W).sum())


def gradient(W, b, y, bins, event, mask, lam, alpha):
    G = logit_grad(W, b, y, bins, event, mask, alpha)
    return G.T @ y + lam * W, G.sum(0)


def lipschitz(y, lam):
    """L = rho / 4 + lam, rho = 1 + max_i |y_i|^2: sigmoid' <= 1 / 4, w_i <= 1, and the bias is a feature of value 1."""
    return 0.25 * (1.0 + float((y * y).sum(1).max())) + lam


def fista(y, bins, event, mask, lam, alpha, M, steps):
    """(W, b) = X_steps of plain FISTA from zero with step 1 / L."""
    n, D = y.shape
    eta = 1.0 / lipschitz(y, lam)
    Wx, bx = np.zeros((M, D)), np.zeros(M)
    Wz, bz = Wx.copy(), bx.copy()
    for beta in betas(steps):
        dW, db = gradient(Wz, bz, y, bins, event, mask, lam, alpha)
        Wn, bn = Wz - eta * dW, bz - eta * db
        Wz, bz = Wn + beta * (Wn - Wx), bn + beta * (bn - bx)
        Wx, bx = Wn, bn
    return Wx, bx


def optimum(y, bins, event, mask, lam, alpha, M):
    """(W*, b*, F*) from scipy's L-BFGS-B on the same objective with its analytic gradient."""
    from scipy.optimize import minimize
    D = y.shape[1]

    def fg(x):
        W, b = x[:M * D].reshape(M, D), x[M * D:]
        dW, db = gradient(W, b, y, bins, event, mask, lam, alpha)
        return objective(W, b, y, bins, event, mask, lam, alpha), np.concatenate([dW.ravel(), db])

    res = minimize(fg, np.zeros(M * D + M), jac=True, method="L-BFGS-B", options=dict(maxiter=20000, maxfun=40000, ftol=1e-15, gtol=1e-10))
    W, b = res.x[:M * D].reshape(M, D), res.x[M * D:]
    return W, b, float(res.fun)


def risk(W, b, q):
    """-sum_t prod_{u <= t} sigmoid(-v_u), float64 [n']."""
    return -np.cumprod(sigmoid(-(q @ W.T + b)), axis=1).sum(1)


def cindex_counts(event, time, est, tol=1e-8):
    """int64 [5] {concordant, discordant, tied_risk, tied_time, comparable} of survival.concordance_index_censored's definition; `est`
    is compared as the f32 numbers the device compares (|e_j - e_i| formed in f32)."""
    ev = np.asarray(event) != 0
    t = np.asarray(time, dtype=np.float64)
    e = np.asarray(est, dtype=np.float32)
    same = t[None, :] == t[:, None]
    comp = ev[:, None] & ((t[None, :] > t[:, None]) | (same & ~ev[None, :]))           # [i, j]: i has the event, j outlives it
    diff = e[None, :] - e[:, None]                                                      # f32
    tie = comp & (np.abs(diff) <= np.float32(tol))
    con = comp & ~tie & (diff < 0)
    dis = comp & ~tie & ~(diff < 0)
    return np.array([con.sum(), dis.sum(), tie.sum(), (comp & same).sum(), comp.sum()], dtype=np.int64)


def cindex(counts):
    return (counts[0] + 0.5 * counts[2]) / counts[4] if counts[4] else np.nan


def bins_ref(time, event, num_bins=4, eps=1e-6):
    """(bins, edges) through pandas, as datasets/dataset_survival.py:_gen_disc_label forms them (needs pandas)."""
    import pandas as pd
    t = pd.Series(np.asarray(time, dtype=np.float64))
    ev = t[np.asarray(event) == 1]
    if len(ev) > 0:
        _, q = pd.qcut(ev, q=num_bins, retbins=True, labels=False)
        q[-1] = t.max() + eps
        q[0] = t.min() - eps
        lab, q = pd.cut(t, bins=q, retbins=True, labels=False, right=False, include_lowest=True)
    else:
        lab, q = pd.cut(t, bins=num_bins, retbins=True, labels=False, right=False, include_lowest=True)
    return lab.values.astype(np.int64), np.asarray(q, dtype=np.float64)


# ------------------------------------------------------------------ cohorts
def cohort(n, D, M, seed, censor=0.35):
    """(x f32 [n, D], bins int64 [n], event int64 [n], time f64 [n]): exponential times from a linear log-hazard of x, independent
    exponential censoring (about `censor` of the rows), bins from the event-time quantiles (searchsorted restated here: the cohort must
    not depend on the code under test)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, D)) + 0.5 * rng.standard_normal(D)
    beta = rng.standard_normal(D) / np.sqrt(D)
    t_event = rng.exponential(1.0, n) * np.exp(-1.5 * (x @ beta))
    t_cens = rng.exponential(np.quantile(t_event, 1.0 - censor) * 1.5, n)
    event = (t_event <= t_cens).astype(np.int64)
    time = np.minimum(t_event, t_cens)
    edges = np.quantile(time[event == 1], np.linspace(0, 1, M + 1))
    edges[0], edges[-1] = time.min() - 1e-6, time.max() + 1e-6
    bins = (np.searchsorted(edges, time, side="right") - 1).astype(np.int64)
    return x.astype(np.float32), bins, event, time


# the end-to-end case of tests/test_survprobe_gpu.py; tests/test_survprobe_cpu.py checks its input condition from float64 alone
E2E = dict(n=240, D=16, M=4, F=3, strengths=(1e-3, 1e-1), steps=300, seed=77)
MAX_UNDECIDED = 0.01      # at most this share of a job's comparable pairs may have a float64 risk gap under twice the risk tolerance


def e2e_case():
    """(x, bins, event, time, fold): 5 rows in no fold, one row with a bin outside the bins and one with an event of 2 (both in a fold:
    they train nowhere and are scored)."""
    c = E2E
    x, bins, event, time = cohort(c["n"], c["D"], c["M"], c["seed"])
    rng = np.random.default_rng(c["seed"] + 1)
    fold = rng.integers(0, c["F"], c["n"]).astype(np.int64)
    fold[rng.choice(c["n"], 5, replace=False)] = -1
    bins, event = bins.copy(), event.copy()
    bins[11], event[100] = c["M"], 2
    return x, bins, event, time, fold
