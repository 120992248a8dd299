"""Ridge Cox probe of frozen embeddings: the survival protocol slide-encoder benchmarks report.

An L2-penalised Cox proportional-hazards model on the frozen slide embedding, the strength chosen over folds and every fold scored by
the censored concordance index.  Unlike the hazard probe of `survprobe.py` (the reference's `train_survival.py --linear_probe`, which
bins the follow-up into `num_bins` intervals) it uses the follow-up time itself.  With F folds and S strengths there are
J = (F + 1) S independent regressions over the SAME prepared rows, as in `linprobe.py` / `survprobe.py`; job f S + s holds out fold f
at strength s, the last S jobs hold out nothing and are the models `predict_risk` uses.  A job has one weight vector w in R^D and NO
intercept: the partial likelihood does not see one.  Row i trains in job j (a_ij = 1) iff its event is 0 or 1, its time is not NaN,
fold_i >= 0 and fold_i != heldout_j.  With scores v_i = y_i . w_j and the definitions of include/mirror_hip.h's Cox block restricted
to a job's training rows,

    m = max_train v,  w_k = a_k exp(v_k - m),  S_i = sum_{t_k >= t_i} w_k,  D_i, d_i: the sum of w_k / the count over the training
    events tied with t_i,  l_i: i's rank among them in row order,  f_i = 0 (Breslow) or l_i / d_i (Efron),  den_i = S_i - f_i D_i
    F_j(w) = r_j sum_i a_ij e_i (log den_i + m - v_i) + (lambda_j / 2) |w|^2,      r_j = 1 / |train_j|

which has the minimiser of sksurv's `CoxPHSurvivalAnalysis(alpha = lambda |train_j|, ties=...)`.  Every job runs `linprobe.py`'s
plain FISTA iteration from zero (`fista_betas`) with step 1 / L_j,

    L_j = rho eps_j + lambda_j,    rho = max_i |y_i|^2 over the finite rows,    eps_j = n_events_j / n_train_j.

Why L_j bounds the curvature: each event's term log den_i - v_i is a log-sum-exp of the scores of its risk set with NON-NEGATIVE
coefficients (1 for Breslow, 1 - f_i >= 0 on the tied events for Efron) minus a linear term, so its Hessian in w is the covariance of
y under a weighted softmax over the risk set; the largest eigenvalue of a covariance is at most E[(y . u)^2] <= max |y|^2 = rho.
There are n_events_j such terms, each scaled by r_j.  FISTA's guarantee is F_j(X_k) - F_j* <= 2 L_j |w*|^2 / (k + 1)^2.

`fit` sorts the rows ONCE by time, descending and stable, NaN times last (torch plumbing); on rows in that order a risk set is a
prefix and a tie group is a run, so the gradient of every job is two scans, not the all-pairs pass of `csrc/cox.hip`.  One iteration
is three launches and nothing else: `mh_coxprobe_scores` (the J weight rows are the keys of the retrieval kernels' exact-f32 tile
product; scores job-major), `mh_coxprobe_grad` (one workgroup per job: f64 block scans, the score gradient and the data term) and
`mh_coxprobe_step` (`mh_linprobe_step`'s kernel with one key per job and no bias column).  All are deterministic: no float atomics,
two fits agree bit for bit.  A held-out fold is scored through `mh_coxprobe_scores` on its rows and `mh_cindex_counts` once per
strength; all counts are stacked on the device and read back in one copy.

Not built: the baseline hazard and survival curves, the Brier score and time-dependent AUC, stratified Cox, a pool gathered over DDP
ranks, the log-rank test of the out-of-fold split (`survival.logrank_test` takes any split).
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Optional, Sequence

import torch

from . import kernels as K
from ._lib import MirrorHipError
from .linprobe import LinearProbe, _int_in, fista_betas
from .survprobe import _INT, _vec

__all__ = ["CoxProbe"]


class CoxProbe:
    """`fit(emb, event, time, fold=None, train_rows=None)` trains every job; `evaluate()` scores the held-out folds with the censored
    concordance index; `predict_risk(emb, strength=None)` gives new rows their risk y . w under the all-rows job of the best (or the
    given) strength; `oof_risk(strength=None)` gives every row of the pool its risk under the job that held its fold out.

    The rows are prepared as LinearProbe prepares them: center=True, y = (x - mu) / max(|x - mu|, 1e-12) with mu the pool's column mean
    (mh_colmean, mh_center_l2norm, over the rows in the caller's order); center=False, normalised only.  Later queries use the POOL's
    mean.

    event: bool / uint8 / int32 / int64 [n], 1 = death observed; time: floating point [n].  A row whose event is neither 0 nor 1 or
    whose time is NaN trains nowhere but is still scored if it lies in a fold (as censored unless its event is 1).  fold: as
    LinearProbe's (values in [0, F), negative: in no job; every fold in [0, F) needs a row; None: F = 0, every valid row trains).
    train_rows: an int64 index tensor into the caller's rows; rows outside it are kept out of training in EVERY job but are still scored
    in their fold.  ties: "efron" or "breslow".

    After `fit`, on the device: `coef_` f32 [J, D], `loss_` f64 [J] (F_j at coef_: the data term from mh_coxprobe_grad, the
    regulariser added here), `grad_inf_` f32 [J] (the max norm of the gradient the LAST step used, at its look-ahead point),
    `n_train_` and `n_events_` int64 [J]; `n_iter_` an int.  The sort is kept: `_perm` int64 [n] (sorted position -> the caller's row)
    and `_y`, `_event`, `_time` in sorted order.  `fit` waits on the host once per `check_every` iterations, for `grad_inf_` alone, and
    stops when every job is <= tol (a NaN job never is) or at max_iter.  A job without training events keeps zero weights, loss 0 and
    gradient 0.  A NaN embedding row makes every job that trains on it NaN, and no other.  Limits: n <= 65536, n J <= 2^24, and the
    spread of a job's training scores <= 700 (|y| <= 1: |w| <= 350)."""

    def __init__(self, strengths: Sequence[float] = (1e-4, 1e-3, 1e-2, 1e-1), ties: str = "efron", max_iter: int = 2000,
                 tol: float = 1e-4, center: bool = True, check_every: int = 16, device=None):
        if isinstance(strengths, (str, bytes)) or not isinstance(strengths, (tuple, list)) or not (1 <= len(strengths) <= 1024):
            raise ValueError(f"strengths must be a tuple of 1..1024 positive floats, got {strengths!r}")
        for s in strengths:
            if isinstance(s, bool) or not isinstance(s, (int, float)) or not (0.0 < float(s) < math.inf):
                raise ValueError(f"strengths must be positive finite floats, got {s!r}")
        if not isinstance(ties, str) or ties not in K.COX_TIES:
            raise ValueError(f'ties must be "efron" or "breslow", got {ties!r}')
        _int_in(max_iter, 1, 1 << 20, "max_iter")
        if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not (0.0 <= float(tol) < math.inf):
            raise ValueError(f"tol must be a non-negative finite float, got {tol!r}")
        if not isinstance(center, bool):
            raise ValueError(f"center must be a bool, got {center!r}")
        _int_in(check_every, 1, 1 << 16, "check_every")
        d = torch.device("cuda") if device is None else torch.device(device)
        if d.type != "cuda":
            raise MirrorHipError(f"mirror_amd metrics keep their state on a HIP device, got {d}")
        self.strengths = tuple(float(s) for s in strengths)
        self.ties = ties
        self.max_iter = max_iter
        self.tol = float(tol)
        self.center = center
        self.check_every = check_every
        self.device = d
        self._clear()

    def _clear(self) -> None:
        self.mu_ = self._perm = self._y = self._event = self._time = self._fold_rows = self._fold_pos = self._train = None
        self._Wx = None
        self.coef_ = self.loss_ = self.grad_inf_ = self.n_train_ = self.n_events_ = None
        self.n_iter_ = 0
        self.n_folds_ = 0
        self.per_job = self.counts = self.best_strength_ = None

    _rows = staticmethod(LinearProbe._rows)

    def _prepare(self, x: torch.Tensor) -> torch.Tensor:
        mu = self.mu_ if self.center else torch.zeros((x.shape[1],), device=self.device, dtype=torch.float32)
        return K.center_l2norm(x, mu)

    @staticmethod
    def _limits(n: int, F: int, S: int) -> None:
        if n > K.COXPROBE_MAX_N or n * (F + 1) * S > (1 << 24):
            raise MirrorHipError(f"CoxProbe: ({F} folds + 1) x {S} strengths over n = {n} rows (n <= {K.COXPROBE_MAX_N}, n * J <= 2^24)")

    # ------------------------------------------------------------------ fit
    def fit(self, emb: torch.Tensor, event: torch.Tensor, time: torch.Tensor, fold: Optional[torch.Tensor] = None,
            train_rows: Optional[torch.Tensor] = None) -> "CoxProbe":
        self._rows(emb, "emb")
        n, D = emb.shape
        _vec(event, n, (torch.bool, torch.uint8) + _INT, "event", "a bool / uint8 / int32 / int64")
        _vec(time, n, None, "time", "a floating point")
        if fold is not None:
            _vec(fold, n, _INT, "fold", "an int32 / int64")
        if train_rows is not None and (not isinstance(train_rows, torch.Tensor) or train_rows.dim() != 1 or train_rows.dtype != torch.int64):
            got = f"{train_rows.dtype} {tuple(train_rows.shape)}" if isinstance(train_rows, torch.Tensor) else type(train_rows).__name__
            raise ValueError(f"train_rows must be a 1-D int64 index tensor, got {got}")
        S = len(self.strengths)
        fold_rows = []
        if fold is not None:
            fh = fold.detach().cpu()                                          # the one host copy: F and every fold's rows
            F = max(int(fh.max()) + 1, 0)
            self._limits(n, F, S)
            fold_rows = [torch.nonzero(fh == f).view(-1) for f in range(F)]
            empty = [f for f, r in enumerate(fold_rows) if r.numel() == 0]
            if empty:
                raise ValueError(f"CoxProbe: no row of fold(s) {empty} (fold values must cover [0, {F}))")
            train_fold = fh.clamp(min=-1).to(torch.int32)
        else:
            F = 0
            self._limits(n, F, S)
            train_fold = torch.zeros((n,), dtype=torch.int32)
        J = (F + 1) * S
        if train_rows is not None:                                            # few-shot: the gradient kernel sees fold -1 outside train_rows
            tr = train_rows.detach().cpu()
            if tr.numel() and (int(tr.min()) < 0 or int(tr.max()) >= n):
                raise ValueError(f"train_rows must index the {n} rows, got values in [{int(tr.min())}, {int(tr.max())}]")
            keep = torch.zeros((n,), dtype=torch.bool)
            keep[tr] = True
            train_fold = torch.where(keep, train_fold, torch.full_like(train_fold, -1))
        self._clear()
        dev = self.device
        x = emb.detach().to(device=dev, dtype=torch.float32, non_blocking=True, copy=True).contiguous()
        self.mu_ = K.colmean(x) if self.center else None
        y0 = self._prepare(x)
        # the sort: time descending and stable, NaN times last as rows of their own (they train nowhere)
        t0 = time.detach().to(device=dev, dtype=torch.float64, non_blocking=True, copy=True).contiguous()
        nan_t = torch.isnan(t0)
        p1 = torch.sort(torch.where(nan_t, torch.zeros((), device=dev, dtype=torch.float64), t0), descending=True, stable=True).indices
        perm = self._perm = p1.index_select(0, torch.sort(nan_t.index_select(0, p1).to(torch.uint8), stable=True).indices)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(n, device=dev)
        y = self._y = y0.index_select(0, perm).contiguous()
        self._time = t0.index_select(0, perm).contiguous()
        ev = event.detach().to(device=dev, non_blocking=True)
        if ev.dtype == torch.bool:
            ev = ev.contiguous().view(torch.uint8).clone()
        else:                                                                 # 2: neither 0 nor 1, whatever the value was
            ev = torch.where((ev == 0) | (ev == 1), ev, torch.full_like(ev, 2)).to(torch.uint8)
        ev = ev.index_select(0, perm).contiguous()
        self._event = (ev == 1).view(torch.uint8)                             # the indicator the concordance index sees
        fd = train_fold.to(dev, non_blocking=True).index_select(0, perm).contiguous()
        self._fold_rows = [r.to(device=dev, non_blocking=True) for r in fold_rows]              # the caller's rows
        self._fold_pos = [inv.index_select(0, r) for r in self._fold_rows]                      # their sorted positions
        self.n_folds_ = F
        heldout = torch.tensor([f for f in range(F) for _ in range(S)] + [-1] * S, dtype=torch.int32).to(dev, non_blocking=True)
        lam = torch.tensor(list(self.strengths) * (F + 1), dtype=torch.float32).to(dev, non_blocking=True)
        valid = (ev <= 1) & ~torch.isnan(self._time) & (fd >= 0)
        member = valid[None, :] & (fd[None, :] != heldout[:, None])
        self.n_train_ = member.sum(1)
        self.n_events_ = (member & (ev == 1)[None, :]).sum(1)
        rscale = torch.where(self.n_train_ > 0, 1.0 / self.n_train_.clamp(min=1).to(torch.float32), torch.zeros((), device=dev))
        # A row with a NaN must poison the jobs that train on it and no other.  mh_coxprobe_grad does that by itself (G is NaN where the
        # row trains, exactly 0 where it does not), but the step's product would form 0 * NaN for the other jobs: it reads such a row
        # as zeros (NaN * 0 is still NaN where the row trains), and the row stays out of rho.
        ss = (y * y).sum(1)
        finite = torch.isfinite(ss)
        ys = torch.where(finite[:, None], y, torch.zeros((), device=dev))
        rho = torch.where(finite, ss, torch.zeros((), device=dev)).max()
        eps = self.n_events_.to(torch.float32) / self.n_train_.clamp(min=1).to(torch.float32)
        eta = (1.0 / (rho * eps + lam)).to(torch.float32)
        self._train = (ev, fd, heldout, rscale)                               # what mh_coxprobe_grad was given beside the scores

        Wx = torch.zeros((J, D), device=dev, dtype=torch.float32)
        Wz = torch.zeros_like(Wx)
        V = torch.empty((J, n), device=dev, dtype=torch.float32)
        G = torch.empty((n, J), device=dev, dtype=torch.float32)
        part = torch.empty((J,), device=dev, dtype=torch.float64)
        ws = K.coxprobe_workspace(n, J, dev)
        gmax = torch.empty(((D + 1 + 127) // 128, J), device=dev, dtype=torch.float32)
        done = 0
        for beta in fista_betas(self.max_iter):
            K.coxprobe_scores(y, Wz, V=V)
            K.coxprobe_grad(V, self._time, ev, fd, heldout, rscale, self.ties, G=G, loss=part, workspace=ws)
            K.coxprobe_step(ys, G, Wx, Wz, lam, eta, beta, gmax_part=gmax)
            done += 1
            if done % self.check_every == 0 and done < self.max_iter:
                if bool((gmax.amax(0) <= self.tol).all()):                    # the one host wait of these iterations
                    break
        self.n_iter_ = done
        self.grad_inf_ = gmax.amax(0)
        K.coxprobe_scores(y, Wx, V=V)
        K.coxprobe_grad(V, self._time, ev, fd, heldout, rscale, self.ties, G=G, loss=part, workspace=ws)
        self._Wx = self.coef_ = Wx
        self.loss_ = part + 0.5 * lam.double() * Wx.double().square().sum(1)
        return self

    def _fitted(self) -> None:
        if self._Wx is None:
            raise ValueError("CoxProbe: nothing is fitted (call fit() first)")

    # ------------------------------------------------------------------ scores of the held-out folds
    def evaluate(self, tied_tol: float = 1e-8):
        """Every fold's rows under the S jobs that held it out: an OrderedDict of `coxprobe_cindex` (the censored concordance index of
        `survival.concordance_index_censored` at the best strength, the mean over the folds), `coxprobe_cindex_mean` and
        `coxprobe_cindex_std` (sample standard deviation over the folds, 0 for fewer than two) as tuples over the strengths in the
        constructor's order, `coxprobe_best_strength` (the highest mean, ties to the larger lambda), `coxprobe_strengths`,
        `coxprobe_folds`, `coxprobe_n` (the rows that lie in a fold), `per_job` f64 [F, S] and `counts` int64 [F, S, 5]
        {concordant, discordant, tied_risk, tied_time, comparable} on the device.  A fold whose held-out rows have no comparable pair
        gives NaN for its jobs and is left out of the means; when every fold is such, ValueError as sksurv words it.  One host copy."""
        self._fitted()
        F, S = self.n_folds_, len(self.strengths)
        if F < 1:
            raise ValueError("CoxProbe: evaluate() needs folds (fit(emb, event, time, fold=...))")
        counts = []
        for f, pos in enumerate(self._fold_pos):
            risk = K.coxprobe_scores(self._y.index_select(0, pos), self._Wx[f * S:(f + 1) * S])
            ev, tm = self._event.index_select(0, pos), self._time.index_select(0, pos)
            counts.extend(K.cindex_counts(ev, tm, risk[s], tied_tol) for s in range(S))
        self.counts = torch.stack(counts).view(F, S, 5)
        c = self.counts.double()
        self.per_job = torch.where(c[:, :, 4] > 0, (c[:, :, 0] + 0.5 * c[:, :, 2]) / c[:, :, 4].clamp(min=1.0),
                                   torch.full((), math.nan, device=self.device, dtype=torch.float64))
        t = self.per_job.cpu()                                                # the one host wait
        ok = ~torch.isnan(t)
        if not bool(ok.any()):
            if not bool(torch.cat([self._event.index_select(0, r) for r in self._fold_pos]).any()):
                raise ValueError("All samples are censored")
            raise ValueError("Data has no comparable pairs, cannot estimate concordance index.")
        cnt = ok.sum(0)
        mean = torch.where(ok, t, torch.zeros_like(t)).sum(0) / cnt.clamp(min=1)
        dev2 = torch.where(ok, (t - mean[None, :]) ** 2, torch.zeros_like(t)).sum(0)
        std = torch.where(cnt > 1, (dev2 / (cnt - 1).clamp(min=1)).sqrt(), torch.zeros_like(mean))
        mean = torch.where(cnt > 0, mean, torch.full_like(mean, math.nan))
        key = [float(a) if a == a else -math.inf for a in mean]
        best = max(range(S), key=lambda s: (key[s], self.strengths[s]))
        self.best_strength_ = self.strengths[best]
        out: "OrderedDict[str, object]" = OrderedDict()
        out["coxprobe_cindex"] = float(mean[best])
        out["coxprobe_cindex_mean"] = tuple(float(v) for v in mean)
        out["coxprobe_cindex_std"] = tuple(float(v) for v in std)
        out["coxprobe_best_strength"] = self.best_strength_
        out["coxprobe_strengths"] = self.strengths
        out["coxprobe_folds"] = F
        out["coxprobe_n"] = int(sum(r.numel() for r in self._fold_rows))
        out["per_job"] = self.per_job
        out["counts"] = self.counts
        return out

    # ------------------------------------------------------------------ risks
    def _strength_index(self, strength) -> int:
        S = len(self.strengths)
        if strength is None:
            if S == 1:
                strength = self.strengths[0]
            elif self.best_strength_ is None and self.n_folds_ < 1:
                raise ValueError("CoxProbe: without folds there is no best strength (name one: strength=...)")
            else:
                if self.best_strength_ is None:
                    self.evaluate()
                strength = self.best_strength_
        if isinstance(strength, bool) or not isinstance(strength, (int, float)) or float(strength) not in self.strengths:
            raise ValueError(f"strength must be one of {self.strengths}, got {strength!r}")
        return self.strengths.index(float(strength))

    def predict_risk(self, emb: torch.Tensor, strength: Optional[float] = None) -> torch.Tensor:
        """f32 [n'] on the device: the risks y . w of emb's rows, prepared with the pool's mean, under the all-rows job of `strength` (one
        of the constructor's) or, for None, of `coxprobe_best_strength` (evaluate() is run when it has not been; without folds and with
        more than one strength, name the strength).  A larger risk means an earlier expected event."""
        self._fitted()
        self._rows(emb, "emb", self._Wx.shape[1])
        j = self.n_folds_ * len(self.strengths) + self._strength_index(strength)
        q = self._prepare(emb.detach().to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous())
        return K.coxprobe_scores(q, self._Wx[j:j + 1])[0]

    def oof_risk(self, strength: Optional[float] = None) -> torch.Tensor:
        """f32 [n] on the device, in the CALLER's row order: every pool row's risk under the job that held its fold out at `strength`
        (None: as predict_risk), NaN for the rows that lie in no fold."""
        self._fitted()
        if self.n_folds_ < 1:
            raise ValueError("CoxProbe: oof_risk() needs folds (fit(emb, event, time, fold=...))")
        S, s = len(self.strengths), self._strength_index(strength)
        out = torch.full((self._y.shape[0],), math.nan, device=self.device, dtype=torch.float32)
        for f, (rows, pos) in enumerate(zip(self._fold_rows, self._fold_pos)):
            j = f * S + s
            out.index_copy_(0, rows, K.coxprobe_scores(self._y.index_select(0, pos), self._Wx[j:j + 1])[0])
        return out
