"""f64 restatements of the Cox partial-likelihood loss and the two-group log-rank test, in two independent forms.

* `cox_pair`: the all-pairs statement of include/mirror_hip.h (what csrc/cox.hip computes), numpy, with the closed-form gradient.
* `cox_grouped_rows` / `cox_grouped`: the textbook statement per distinct event time (risk set, tied events, Efron's k / d
  shares), torch f64, its gradient by autograd.

The event flag is `censoring == 1`, as the other survival losses read it.  Reductions: "none", "sum", "mean" (sum /
max(n_events, 1)), "batch" (sum / N).
"""
from __future__ import annotations

import math

import numpy as np
import torch

TIES = ("breslow", "efron")
REDUCTIONS = ("none", "sum", "mean", "batch")


def events(censoring) -> np.ndarray:
    return np.asarray(censoring).astype(np.float64).reshape(-1) == 1.0


def _coef(reduction: str, e: np.ndarray) -> float:
    return {"none": 1.0, "sum": 1.0, "mean": 1.0 / max(int(e.sum()), 1), "batch": 1.0 / len(e)}[reduction]


# ----------------------------------------------------------------------------- pair form
def cox_pair(r, t, censoring, ties: str = "efron", reduction: str = "mean", g=None):
    """(loss, dloss/dr) in f64.  g: upstream gradient, [N] for "none" (default ones), a scalar otherwise (default 1).
    A NaN time gives NaN in that row's loss and gradient; the row is in no other row's risk set."""
    r = np.asarray(r, np.float64).reshape(-1)
    t = np.asarray(t, np.float64).reshape(-1)
    e = events(censoring)
    N = len(r)
    m = np.nan if np.isnan(r).any() else r.max()
    w = np.exp(r - m)
    with np.errstate(invalid="ignore"):
        ge = t[None, :] >= t[:, None]                       # [i, j]: t_j >= t_i
        eq = t[None, :] == t[:, None]
    S = (ge * w[None, :]).sum(1) if not np.isnan(m) else np.full(N, np.nan)
    eqe = eq & e[None, :]
    D = np.where(eqe, w[None, :], 0.0).sum(1)
    d = eqe.sum(1)
    l = (eqe & (np.arange(N)[None, :] < np.arange(N)[:, None])).sum(1)
    f = np.zeros(N)
    if ties == "efron":
        f = np.where(e & (d > 0), l / np.maximum(d, 1), 0.0)
    elif ties != "breslow":
        raise ValueError(ties)
    den = S - f * D
    nan_t = np.isnan(t)
    with np.errstate(divide="ignore", invalid="ignore"):
        rows = np.where(e, np.log(den) + m - r, 0.0)
    rows[nan_t] = np.nan
    coef = _coef(reduction, e)
    gi = (np.ones(N) if g is None else np.asarray(g, np.float64).reshape(-1)) if reduction == "none" else \
        np.full(N, coef * (1.0 if g is None else float(g)))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(e & ~nan_t, gi / den, 0.0)
        gt = t[:, None] > t[None, :]                        # [k, i]: t_k > t_i
        eqk = t[:, None] == t[None, :]
    A = np.where(gt, q[None, :], 0.0).sum(1)
    B = np.where(eqk, q[None, :], 0.0).sum(1)
    C = np.where(eqk, (q * f)[None, :], 0.0).sum(1)
    grad = w * (A + B - np.where(e, C, 0.0)) - np.where(e, gi, 0.0)
    grad[nan_t] = np.nan
    loss = rows if reduction == "none" else coef * rows.sum()
    return loss, grad


# ----------------------------------------------------------------------------- grouped form (per distinct event time)
def cox_grouped_rows(r: torch.Tensor, t, censoring, ties: str = "efron") -> torch.Tensor:
    """Per-row losses [N] (f64, differentiable in r): for every distinct event time tau with risk set R = {t_j >= tau} and tied events
    H (in index order, d = |H|), the k-th of them carries log(sum_R exp r - (k / d) sum_H exp r) - r_h  (k = 0 for Breslow)."""
    if ties not in TIES:
        raise ValueError(ties)
    t = np.asarray(t, np.float64).reshape(-1)
    e = events(censoring)
    r = r.reshape(-1)
    rows = [None] * len(t)
    for tau in np.unique(t[e & ~np.isnan(t)]):
        R = torch.from_numpy(np.nonzero(t >= tau)[0])
        H = np.nonzero((t == tau) & e)[0]
        m = r[R].max().detach()
        sR = torch.exp(r[R] - m).sum()
        sH = torch.exp(r[torch.from_numpy(H)] - m).sum()
        for k, h in enumerate(H):
            share = k / len(H) if ties == "efron" else 0.0
            rows[h] = torch.log(sR - share * sH) + m - r[h]
    zero = r.sum() * 0.0
    return torch.stack([zero if x is None else x for x in rows])


def cox_grouped(r, t, censoring, ties: str = "efron", reduction: str = "mean", g=None):
    """(loss, dloss/dr) as numpy f64 by autograd of the grouped form (no NaN times here)."""
    if reduction not in REDUCTIONS:
        raise ValueError(reduction)
    rt = torch.tensor(np.asarray(r, np.float64).reshape(-1), dtype=torch.float64, requires_grad=True)
    rows = cox_grouped_rows(rt, t, censoring, ties)
    e = events(censoring)
    if reduction == "none":
        up = torch.ones_like(rows) if g is None else torch.tensor(np.asarray(g, np.float64).reshape(-1))
        (rows * up).sum().backward()
        return rows.detach().numpy(), rt.grad.numpy()
    loss = rows.sum() * _coef(reduction, e)
    (loss * (1.0 if g is None else float(g))).backward()
    return float(loss.detach()), rt.grad.numpy()


# ----------------------------------------------------------------------------- log-rank
def logrank(event, t, group):
    """(chi2, p, O1, E1, V, n_events) of the two-group log-rank test, per distinct event time; chi2 = p = NaN when V == 0."""
    ev = np.asarray(event).reshape(-1) != 0
    t = np.asarray(t, np.float64).reshape(-1)
    g1 = np.asarray(group).reshape(-1) != 0
    ev = ev & ~np.isnan(t)
    O1 = E1 = V = 0.0
    for tau in np.unique(t[ev]):
        at = t >= tau
        n, n1 = int(at.sum()), int((at & g1).sum())
        dm = (t == tau) & ev
        d, d1 = int(dm.sum()), int((dm & g1).sum())
        O1 += d1
        E1 += d * n1 / n
        if n > 1:
            V += n1 * (n - n1) * d * (n - d) / (n * n * (n - 1.0))
    if V > 0:
        chi2 = (O1 - E1) ** 2 / V
        return chi2, math.erfc(math.sqrt(chi2 / 2.0)), O1, E1, V, int(ev.sum())
    return float("nan"), float("nan"), O1, E1, V, int(ev.sum())


def cindex(event, t, est, tied_tol: float = 1e-8) -> float:
    """Harrell's concordance index for right-censored data (sksurv's definition), all pairs."""
    ev = np.asarray(event).reshape(-1) != 0
    t = np.asarray(t, np.float64).reshape(-1)
    est = np.asarray(est, np.float64).reshape(-1)
    comp = ev[:, None] & ((t[None, :] > t[:, None]) | ((t[None, :] == t[:, None]) & ~ev[None, :]))
    diff = est[None, :] - est[:, None]
    tie = comp & (np.abs(diff) <= tied_tol)
    con = comp & ~tie & (diff < 0)
    return float((con.sum() + 0.5 * tie.sum()) / comp.sum())


# ----------------------------------------------------------------------------- shared inputs
def make_case(N: int, times: str, frac: float, scores: str, seed: int):
    """(r f32 [N], t f64 [N], censoring int64 [N]).  times: "distinct" floats, "ties" (integers 0..7), "equal"; frac: event fraction
    (0 and 1 exactly); scores: "n1" ~ N(0, 1), "n3" ~ N(0, 3), "u100" ~ U(-100, 100)."""
    rng = np.random.RandomState(seed)
    t = {"distinct": lambda: rng.permutation(N).astype(np.float64) * 0.37 + rng.uniform(0.0, 0.3, N),
         "ties": lambda: rng.randint(0, 8, N).astype(np.float64),
         "equal": lambda: np.full(N, 2.5)}[times]()
    c = (rng.uniform(size=N) < frac).astype(np.int64) if 0.0 < frac < 1.0 else np.full(N, int(frac), np.int64)
    r = {"n1": lambda: rng.normal(0.0, 1.0, N), "n3": lambda: rng.normal(0.0, 3.0, N),
         "u100": lambda: rng.uniform(-100.0, 100.0, N)}[scores]().astype(np.float32)
    return r, t, c


# ----------------------------------------------------------------------------- Cox linear probe (f64 restatement of the GPU loop)
PROBE = dict(N=512, D=64, steps=30, lr=0.05, seed=11)


def probe_problem():
    """Synthetic embeddings x f32 [N, D], exponential times from a planted beta, about 30 % censoring, and the head's initial
    weight / bias."""
    rng = np.random.RandomState(PROBE["seed"])
    N, D = PROBE["N"], PROBE["D"]
    x = rng.normal(0.0, 1.0, (N, D)).astype(np.float32)
    beta = rng.normal(0.0, 1.0, D) / math.sqrt(D)
    t_event = rng.exponential(1.0, N) / np.exp(x.astype(np.float64) @ beta)
    t_cens = rng.exponential(2.3, N)
    event = (t_event <= t_cens).astype(np.int64)
    t = np.minimum(t_event, t_cens)
    w0 = (rng.uniform(-1.0, 1.0, (1, D)) / math.sqrt(D)).astype(np.float32)
    b0 = np.zeros(1, np.float32)
    return x, t, event, w0, b0


def probe_loop_f64():
    """The probe in f64 on the host: torch.optim.Adam on a Linear(D, 1) head under the grouped-form loss (Efron, "mean").
    Returns (the loss at the final weights, the concordance index of the final scores)."""
    x, t, event, w0, b0 = probe_problem()
    X = torch.tensor(x, dtype=torch.float64)
    W = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(b0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([W, b], lr=PROBE["lr"])
    coef = _coef("mean", events(event))

    def loss_of():
        return cox_grouped_rows((X @ W.t() + b).reshape(-1), t, event, "efron").sum() * coef

    for _ in range(PROBE["steps"]):
        opt.zero_grad()
        loss_of().backward()
        opt.step()
    with torch.no_grad():
        return float(loss_of()), cindex(event, t, (X @ W.t() + b).reshape(-1).numpy())
