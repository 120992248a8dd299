"""The ridge Cox probe (csrc/coxprobe.hip, mirror_amd/coxprobe.py) restated in float64 numpy from the header text, in the SCAN form the
kernel uses: on rows in non-increasing time order the risk set of a row is a prefix and a tie group is a run, so

    S_i = P[last row of i's group],  P = the inclusive prefix sum of w = a exp(v - m)
    sum_i q_i ([t_k > t_i] + [t_k = t_i]) = Qs[first row of k's group],  Qs = the inclusive suffix sum of q = a e / den

and D, d, l, sum q f are sums over runs.  tests/test_coxprobe_cpu.py checks it against the all-pairs statement of tests/cox_ref.py;
the preparation of the rows is tests/fewshot_ref.py's, the job order and the FISTA momenta are tests/linprobe_ref.py's.

    F(w) = r sum_i a_i e_i (log den_i + m - v_i) + (lam / 2) |w|^2,   v = y w,   r = 1 / |train|   (no intercept)
"""
import numpy as np

from tests.fewshot_ref import prepare  # noqa: F401  (re-exported)
from tests.linprobe_ref import betas, jobs  # noqa: F401  (re-exported)
from tests.survprobe_ref import MAX_UNDECIDED, cindex, cindex_counts, cohort  # noqa: F401  (re-exported)

TIES = ("breslow", "efron")


def train_mask(event, time, fold, heldout):
    event, time, fold = np.asarray(event), np.asarray(time, dtype=np.float64), np.asarray(fold)
    return ((event == 0) | (event == 1)) & ~np.isnan(time) & (fold >= 0) & (fold != heldout)


def sort_rows(time):
    """The permutation of CoxProbe.fit: time descending and stable, NaN times last (in row order)."""
    time = np.asarray(time, dtype=np.float64)
    nan = np.isnan(time)
    p1 = np.argsort(-np.where(nan, 0.0, time), kind="stable")
    return p1[np.argsort(nan[p1], kind="stable")]


def groups(time):
    """(gid [n], first [n_groups], last [n_groups]) of the runs of equal times; a NaN time is a run of its own."""
    time = np.asarray(time, dtype=np.float64)
    n = len(time)
    start = np.ones(n, dtype=bool)
    start[1:] = time[1:] != time[:-1]
    gid = np.cumsum(start) - 1
    first = np.flatnonzero(start)
    last = np.append(first[1:] - 1, n - 1)
    return gid, first, last


def scan(v, time, event, mask, ties="efron", r=1.0, full=False):
    """(data term r sum_i ..., g [n] = its gradient in the scores) of ONE job in float64; the rows must be in non-increasing time order.
    g is exactly 0 off the training rows; a NaN among the training scores makes the loss and g on the training rows NaN.
    full=True: a dict with `loss`, `g`, `abs_loss` = r sum_i |term_i| and `wq` [n] = r w_k sum_{t_i <= t_k} q_i (what a change of the
    ratios w_k / den_i scales)."""
    if ties not in TIES:
        raise ValueError(ties)
    v = np.asarray(v, dtype=np.float64)
    time = np.asarray(time, dtype=np.float64)
    a = np.asarray(mask, dtype=bool)
    e = a & (np.asarray(event) == 1)
    n = len(v)
    assert not (time[1:] > time[:-1]).any(), "rows must be sorted by time, non-increasing"
    if not a.any():
        return dict(loss=0.0, g=np.zeros(n), abs_loss=0.0, wq=np.zeros(n)) if full else (0.0, np.zeros(n))
    m = np.nan if np.isnan(v[a]).any() else v[a].max()
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.zeros(n)
        w[a] = np.exp(v[a] - m)
    gid, first, last = groups(time)
    S = np.cumsum(w)[last][gid]
    D = np.bincount(gid, np.where(e, w, 0.0), minlength=len(first))[gid]
    d = np.bincount(gid, e, minlength=len(first)).astype(np.int64)[gid]
    before = np.cumsum(e) - e                                                    # training events in the rows before i
    l = before - before[first][gid]
    f = np.where(e, l / np.maximum(d, 1), 0.0) if ties == "efron" else np.zeros(n)
    den = S - f * D
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.zeros(n)
        q[e] = 1.0 / den[e]
        loss = r * float((np.log(den[e]) + m - v[e]).sum())
    Qs = np.cumsum(q[::-1])[::-1][first][gid]
    B = np.bincount(gid, q * f, minlength=len(first))[gid]
    g = np.zeros(n)
    with np.errstate(invalid="ignore"):
        g[a] = r * (w[a] * (Qs[a] - np.where(e[a], B[a], 0.0)) - e[a])
        if full:
            return dict(loss=loss, g=g, abs_loss=r * float(np.abs(np.log(den[e]) + m - v[e]).sum()), wq=r * w * Qs)
    return loss, g


def objective(w, y, time, event, mask, lam, ties="efron"):
    nt = int(np.asarray(mask).sum())
    data = scan(y @ w, time, event, mask, ties, 1.0 / nt)[0] if nt else 0.0
    return data + 0.5 * lam * float(w @ w)


def gradient(w, y, time, event, mask, lam, ties="efron"):
    nt = int(np.asarray(mask).sum())
    g = scan(y @ w, time, event, mask, ties, 1.0 / nt)[1] if nt else np.zeros(len(y))
    return g @ y + lam * w


def counts_of(event, mask):
    """(n_events, n_train) of a job."""
    mask = np.asarray(mask, dtype=bool)
    return int((mask & (np.asarray(event) == 1)).sum()), int(mask.sum())


def lipschitz(y, lam, n_events, n_train):
    """L = rho eps + lam, rho = max_i |y_i|^2 over the finite rows, eps = n_events / n_train: each event's term is a log-sum-exp with
    non-negative coefficients, its Hessian a covariance of y under a weighted softmax over the risk set (largest eigenvalue <= rho);
    there are n_events of them, each scaled by 1 / n_train."""
    ss = (np.asarray(y, dtype=np.float64) ** 2).sum(1)
    rho = float(ss[np.isfinite(ss)].max())
    return rho * n_events / max(n_train, 1) + lam


def fista(y, time, event, mask, lam, ties, steps, keep=()):
    """w = X_steps of plain FISTA from zero with step 1 / L; `keep`: iteration counts k whose X_k are returned as a dict too."""
    eta = 1.0 / lipschitz(y, lam, *counts_of(event, mask))
    wx = np.zeros(y.shape[1])
    wz = wx.copy()
    kept = {}
    for k, beta in enumerate(betas(steps), 1):
        wn = wz - eta * gradient(wz, y, time, event, mask, lam, ties)
        wz = wn + beta * (wn - wx)
        wx = wn
        if k in keep:
            kept[k] = wx.copy()
    return (wx, kept) if keep else wx


def optimum(y, time, event, mask, lam, ties):
    """(w*, F*) from scipy's L-BFGS-B on the same objective with its analytic gradient."""
    from scipy.optimize import minimize

    def fg(w):
        return objective(w, y, time, event, mask, lam, ties), gradient(w, y, time, event, mask, lam, ties)

    res = minimize(fg, np.zeros(y.shape[1]), jac=True, method="L-BFGS-B", options=dict(maxiter=20000, maxfun=40000, ftol=1e-15, gtol=1e-10))
    return res.x, float(res.fun)


def hessian_top(w, y, time, event, mask, lam, ties, h=1e-5):
    """The largest eigenvalue of the numerical Hessian of F at w (central differences of the analytic gradient, symmetrised)."""
    D = len(w)
    H = np.empty((D, D))
    for k in range(D):
        e = np.zeros(D)
        e[k] = h
        H[k] = (gradient(w + e, y, time, event, mask, lam, ties) - gradient(w - e, y, time, event, mask, lam, ties)) / (2 * h)
    return float(np.linalg.eigvalsh(0.5 * (H + H.T)).max())


# ------------------------------------------------------------------ the end-to-end case
# shared by tests/test_coxprobe_gpu.py (the fit) and tests/test_coxprobe_cpu.py (its input condition, curvature and rate from float64)
E2E = dict(n=240, D=16, F=3, strengths=(1e-3, 1e-1), steps=300, seed=77)


def e2e_case(plain=False):
    """(x f32 [n, D], event, time, fold) in the CALLER's order (unsorted): survprobe_ref.cohort(240, 16, 4, 77) with the times rounded to
    multiples of 0.05 (44 distinct times, 136 events: heavy ties), 3 folds, 5 rows in no fold, one event of 2 and one NaN time (both in
    a fold: they train nowhere and are scored).  plain=True leaves the added rows out: every row is in a fold and valid."""
    c = E2E
    x, _, event, time = cohort(c["n"], c["D"], 4, c["seed"])
    time = np.round(time / 0.05) * 0.05
    rng = np.random.default_rng(c["seed"] + 1)
    fold = rng.integers(0, c["F"], c["n"]).astype(np.int64)
    out = rng.choice(c["n"], 5, replace=False)
    event, time = event.copy(), time.copy()
    if not plain:
        fold[out] = -1
        inside = np.flatnonzero(fold >= 0)
        event[inside[100]], time[inside[11]] = 2, np.nan
    return x, event, time, fold


def e2e_sorted(plain=False):
    """(y f64 [n, D] prepared and sorted, event, time, fold sorted, perm) of the case."""
    x, event, time, fold = e2e_case(plain)
    y, _ = prepare(x, x)
    perm = sort_rows(time)
    return y[perm], event[perm], time[perm], fold[perm], perm
