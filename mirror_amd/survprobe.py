"""Survival linear probe of frozen embeddings: the survival half of the MIRROR paper's downstream tables.

The reference trains it with `train_survival.py --linear_probe` (freeze the encoder, train one linear layer of `num_bins` hazard
logits under `NLLSurvLoss`) over the folds of `tools/gen_splits.py` and scores every fold with the censored concordance index of the
risk of `train_survival.py:1431-1433`; its "10-shot" figure is the same run on the few-shot file of `tools/gen_few_shot_files.py`.
On cached embeddings [n, D] the figure is small and regular, exactly as the subtyping probe of `linprobe.py` is: with F folds and S
L2 strengths there are J = (F + 1) S independent regressions over the SAME prepared rows.  Row i has a discrete bin T_i in [0, M), an
event indicator e_i (1 = death observed, the reference's `censorship == 1`) and a fold; with hazard logits v = W y_i + b in R^M,

    nll_i   = sum_{t < T_i} softplus(v_t)  +  softplus(v_T) - e_i v_T            (t = T_i: target e_i;  t > T_i: no term)
    w_i     = 1 if e_i == 1 else 1 - alpha
    F_j     = r_j sum_{i in train_j} w_i nll_i + (lambda_j / 2) |W|^2,      r_j = 1 / |train_j|,   the bias is not penalised
    train_j = { i : T_i in [0, M), e_i in {0, 1}, fold_i >= 0, fold_i != heldout_j }

This is `losses/nll_surv.py` with `reduction="mean"` WITHOUT its clamp of the hazards to [eps, 1 - eps]: -log(sigmoid(v)) =
softplus(-v) and -log(1 - sigmoid(v)) = softplus(v), so the two agree wherever every |v_t| <= log((1 - eps) / eps), about 16.1 at
eps = 1e-7, and differ beyond (a weakly regularised job does reach such logits).  The probe optimises the unclamped form, which is
smooth and convex: masked binary cross-entropy per bin.  Job f S + s holds out fold f at strength s; the last S jobs hold out nothing
and are the models `predict_risk` uses.  Every job runs `linprobe.py`'s plain FISTA iteration from zero (`fista_betas`) with

    eta_j = 1 / L_j,  L_j = rho / 4 + lambda_j,  rho = 1 + max_i |y_i|^2

(sigmoid' <= 1 / 4, w_i <= 1, r_j sum_i |(y_i, 1)|^2 <= rho, and the Hessian is block-diagonal over the bins), whose guarantee is
F_j(X_k) - F_j* <= 2 L_j |(W*, b*)|^2 / (k + 1)^2.  One iteration is two launches and nothing else: `mh_survprobe_grad` (every job's
logits, hazard NLL and logit gradient: the J Mp weight rows are the keys of the retrieval kernels' exact-f32 tile product) and
`mh_linprobe_step`, unchanged, with M in the role of C.  Both are deterministic: no float atomics, two fits agree bit for bit.  A
held-out fold is scored by `mh_survprobe_risk` (its S jobs as keys, the logits never stored) and `mh_cindex_counts` once per strength;
all counts are stacked on the device and read back in one copy.

Not built: time-dependent AUC, the Brier score, a pool gathered over DDP ranks, a batched concordance kernel (a fold is a few hundred
rows).  A Cox objective inside a probe, on the follow-up time itself, is `coxprobe.py`'s `CoxProbe`.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Optional, Sequence

import torch

from . import kernels as K
from ._lib import MirrorHipError
from .linprobe import LinearProbe, _int_in, fista_betas

__all__ = ["SurvivalProbe"]

_INT = (torch.int32, torch.int64)


def _vec(t, n: int, dtypes, name: str, kinds: str) -> None:
    ok = isinstance(t, torch.Tensor) and t.dim() == 1 and t.numel() == n
    if not (ok and (t.is_floating_point() if dtypes is None else t.dtype in dtypes)):
        got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{name} must be {kinds} [{n}] tensor, got {got}")


class SurvivalProbe:
    """`fit(emb, bins, event, time, fold=None, train_rows=None)` trains every job; `evaluate()` scores the held-out folds with the
    censored concordance index; `predict_risk(emb, strength=None)` gives new rows their risk under the all-rows job of the best (or the
    given) strength; `oof_risk(strength=None)` gives every row of the pool its risk under the job that held its fold out.

    The rows are prepared as LinearProbe prepares them: center=True, y = (x - mu) / max(|x - mu|, 1e-12) with mu the pool's column mean
    (mh_colmean, mh_center_l2norm); center=False, normalised only.  Later queries use the POOL's mean.

    bins: int32 / int64 [n], the discrete bin of `survival.survival_bins`; event: bool / uint8 / int32 / int64 [n], 1 = death observed;
    time: floating point [n], the continuous time the concordance index compares.  A row whose bin lies outside [0, num_bins) or whose
    event is neither 0 nor 1 trains nowhere but is still scored if it lies in a fold (as censored unless its event is 1).
    fold: as LinearProbe's (values in [0, F), negative: in no job; every fold in [0, F) needs a row; None: F = 0, every valid row
    trains).  train_rows: an int64 index tensor; rows outside it are kept out of training in EVERY job but are still scored in their
    fold: the reference's few-shot survival run over the same folds.  It is a remap of the fold values the gradient kernel sees
    (`train_fold`: -1 outside train_rows); scoring uses the original folds.

    After `fit`, on the device: `coef_` f32 [J, M, D], `intercept_` f32 [J, M], `loss_` f64 [J] (F_j at coef_ / intercept_: the data
    term from mh_survprobe_grad in f64 sums of f32 terms, the regulariser added here), `grad_inf_` f32 [J] (the max norm of the gradient
    the LAST step used, at its look-ahead point), `n_train_` int64 [J]; `n_iter_` an int.  `fit` waits on the host once per
    `check_every` iterations, for `grad_inf_` alone, and stops when every job is <= tol (a NaN job never is) or at max_iter.  A job
    without training rows keeps zero weights.  A NaN row makes every job that trains on it NaN, and no other."""

    def __init__(self, num_bins: int = 4, strengths: Sequence[float] = (1e-4, 1e-3, 1e-2, 1e-1), alpha: float = 0.0,
                 max_iter: int = 2000, tol: float = 1e-4, center: bool = True, check_every: int = 16, device=None):
        _int_in(num_bins, 2, 64, "num_bins")
        if isinstance(strengths, (str, bytes)) or not isinstance(strengths, (tuple, list)) or not (1 <= len(strengths) <= 1024):
            raise ValueError(f"strengths must be a tuple of 1..1024 positive floats, got {strengths!r}")
        for s in strengths:
            if isinstance(s, bool) or not isinstance(s, (int, float)) or not (0.0 < float(s) < math.inf):
                raise ValueError(f"strengths must be positive finite floats, got {s!r}")
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not (0.0 <= float(alpha) <= 1.0):
            raise ValueError(f"alpha must be a float in [0, 1], got {alpha!r}")
        _int_in(max_iter, 1, 1 << 20, "max_iter")
        if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not (0.0 <= float(tol) < math.inf):
            raise ValueError(f"tol must be a non-negative finite float, got {tol!r}")
        if not isinstance(center, bool):
            raise ValueError(f"center must be a bool, got {center!r}")
        _int_in(check_every, 1, 1 << 16, "check_every")
        d = torch.device("cuda") if device is None else torch.device(device)
        if d.type != "cuda":
            raise MirrorHipError(f"mirror_amd metrics keep their state on a HIP device, got {d}")
        self.num_bins = num_bins
        self.strengths = tuple(float(s) for s in strengths)
        self.alpha = float(alpha)
        self.max_iter = max_iter
        self.tol = float(tol)
        self.center = center
        self.check_every = check_every
        self.device = d
        self._clear()

    def _clear(self) -> None:
        self.mu_ = self._y = self._event = self._time = self._fold_rows = self._train = None
        self._Wx = self._bx = None
        self.coef_ = self.intercept_ = self.loss_ = self.grad_inf_ = self.n_train_ = None
        self.n_iter_ = 0
        self.n_folds_ = 0
        self.per_job = self.counts = self.best_strength_ = None

    _rows = staticmethod(LinearProbe._rows)

    def _prepare(self, x: torch.Tensor) -> torch.Tensor:
        mu = self.mu_ if self.center else torch.zeros((x.shape[1],), device=self.device, dtype=torch.float32)
        return K.center_l2norm(x, mu)

    # ------------------------------------------------------------------ fit
    def fit(self, emb: torch.Tensor, bins: torch.Tensor, event: torch.Tensor, time: torch.Tensor, fold: Optional[torch.Tensor] = None,
            train_rows: Optional[torch.Tensor] = None) -> "SurvivalProbe":
        self._rows(emb, "emb")
        n, D = emb.shape
        _vec(bins, n, _INT, "bins", "an int32 / int64")
        _vec(event, n, (torch.bool, torch.uint8) + _INT, "event", "a bool / uint8 / int32 / int64")
        _vec(time, n, None, "time", "a floating point")
        if fold is not None:
            _vec(fold, n, _INT, "fold", "an int32 / int64")
        if train_rows is not None and (not isinstance(train_rows, torch.Tensor) or train_rows.dim() != 1 or train_rows.dtype != torch.int64):
            got = f"{train_rows.dtype} {tuple(train_rows.shape)}" if isinstance(train_rows, torch.Tensor) else type(train_rows).__name__
            raise ValueError(f"train_rows must be a 1-D int64 index tensor, got {got}")
        M, S = self.num_bins, len(self.strengths)
        Mp = K.fewshot_cp(M)
        fold_rows = []
        if fold is not None:
            fh = fold.detach().cpu()                                          # the one host copy: F and every fold's rows
            F = max(int(fh.max()) + 1, 0)
            if (F + 1) * S * Mp > (1 << 20) or n * (F + 1) * S * Mp > (1 << 28):
                raise MirrorHipError(f"SurvivalProbe: ({F} folds + 1) x {S} strengths x {Mp} bin slots over n = {n} rows "
                                     "(J * Mp <= 2^20, n * J * Mp <= 2^28)")
            fold_rows = [torch.nonzero(fh == f).view(-1) for f in range(F)]
            empty = [f for f, r in enumerate(fold_rows) if r.numel() == 0]
            if empty:
                raise ValueError(f"SurvivalProbe: no row of fold(s) {empty} (fold values must cover [0, {F}))")
            train_fold = fh.clamp(min=-1).to(torch.int32)
        else:
            F = 0
            if S * Mp > (1 << 20) or n * S * Mp > (1 << 28):
                raise MirrorHipError(f"SurvivalProbe: {S} strengths x {Mp} bin slots over n = {n} rows (J * Mp <= 2^20, n * J * Mp <= 2^28)")
            train_fold = torch.zeros((n,), dtype=torch.int32)
        if train_rows is not None:                                            # few-shot: the gradient kernel sees fold -1 outside train_rows
            tr = train_rows.detach().cpu()
            if tr.numel() and (int(tr.min()) < 0 or int(tr.max()) >= n):
                raise ValueError(f"train_rows must index the {n} rows, got values in [{int(tr.min())}, {int(tr.max())}]")
            keep = torch.zeros((n,), dtype=torch.bool)
            keep[tr] = True
            train_fold = torch.where(keep, train_fold, torch.full_like(train_fold, -1))
        J = (F + 1) * S
        self._clear()
        dev = self.device
        x = emb.detach().to(device=dev, dtype=torch.float32, non_blocking=True, copy=True).contiguous()
        self.mu_ = K.colmean(x) if self.center else None
        y = self._y = self._prepare(x)
        bd = bins.detach().to(device=dev, dtype=torch.int64, non_blocking=True, copy=True).contiguous()
        ev = event.detach().to(device=dev, non_blocking=True)
        if ev.dtype == torch.bool:
            ev = ev.contiguous().view(torch.uint8).clone()
        else:                                                                 # 2: neither 0 nor 1, whatever the value was
            ev = torch.where((ev == 0) | (ev == 1), ev, torch.full_like(ev, 2)).to(torch.uint8).contiguous()
        self._event = (ev == 1).view(torch.uint8)                             # the indicator the concordance index sees
        self._time = time.detach().to(device=dev, dtype=torch.float64, non_blocking=True, copy=True).contiguous()
        fd = train_fold.to(dev, non_blocking=True)
        self._fold_rows = [r.to(device=dev, non_blocking=True) for r in fold_rows]
        self.n_folds_ = F
        heldout = torch.tensor([f for f in range(F) for _ in range(S)] + [-1] * S, dtype=torch.int32).to(dev, non_blocking=True)
        lam = torch.tensor(list(self.strengths) * (F + 1), dtype=torch.float32).to(dev, non_blocking=True)
        valid = (bd >= 0) & (bd < M) & (ev <= 1) & (fd >= 0)
        self.n_train_ = (valid[None, :] & (fd[None, :] != heldout[:, None])).sum(1)
        rscale = torch.where(self.n_train_ > 0, 1.0 / self.n_train_.clamp(min=1).to(torch.float32), torch.zeros((), device=dev))
        # A row with a NaN must poison the jobs that train on it and no other.  mh_survprobe_grad does that by itself (G is NaN where
        # the row trains, exactly 0 where it does not), but the step's product would form 0 * NaN for the other jobs: it reads such a
        # row as zeros (NaN * 0 is still NaN where the row trains), and the row stays out of rho.
        ss = (y * y).sum(1)
        finite = torch.isfinite(ss)
        ys = torch.where(finite[:, None], y, torch.zeros((), device=dev))
        rho = 1.0 + torch.where(finite, ss, torch.zeros((), device=dev)).max()
        eta = (1.0 / (0.25 * rho + lam)).to(torch.float32)
        w_cens = 1.0 - self.alpha
        self._train = (bd, ev, fd, heldout, rscale, w_cens)                   # what mh_survprobe_grad was given beside the weights

        Wx = torch.zeros((J, Mp, D), device=dev, dtype=torch.float32)
        Wz = torch.zeros_like(Wx)
        bx = torch.zeros((J, Mp), device=dev, dtype=torch.float32)            # pad slots stay 0: no kernel reads or writes them
        bz = bx.clone()
        G = torch.empty((n, J * Mp), device=dev, dtype=torch.float32)
        gmax = torch.empty(((D + 1 + 127) // 128, J), device=dev, dtype=torch.float32)
        done = 0
        for beta in fista_betas(self.max_iter):
            K.survprobe_grad(y, Wz, bz, bd, ev, fd, heldout, rscale, w_cens, M, G=G)
            K.linprobe_step(ys, G, Wx, bx, Wz, bz, lam, eta, beta, M, gmax_part=gmax)
            done += 1
            if done % self.check_every == 0 and done < self.max_iter:
                if bool((gmax.amax(0) <= self.tol).all()):                    # the one host wait of these iterations
                    break
        self.n_iter_ = done
        self.grad_inf_ = gmax.amax(0)
        _, part = K.survprobe_grad(y, Wx, bx, bd, ev, fd, heldout, rscale, w_cens, M, G=G, want_loss=True)
        self._Wx, self._bx = Wx, bx
        self.coef_, self.intercept_ = Wx[:, :M, :], bx[:, :M]
        self.loss_ = part.sum(0) + 0.5 * lam.double() * self.coef_.double().square().sum((1, 2))
        return self

    def _fitted(self) -> None:
        if self._Wx is None:
            raise ValueError("SurvivalProbe: nothing is fitted (call fit() first)")

    # ------------------------------------------------------------------ scores of the held-out folds
    def evaluate(self, tied_tol: float = 1e-8):
        """Every fold's rows under the S jobs that held it out: an OrderedDict of `survprobe_cindex` (the censored concordance index of
        `survival.concordance_index_censored` at the best strength, the mean over the folds), `survprobe_cindex_mean` and
        `survprobe_cindex_std` (sample standard deviation over the folds, 0 for fewer than two) as tuples over the strengths in the
        constructor's order, `survprobe_best_strength` (the highest mean, ties to the larger lambda), `survprobe_strengths`,
        `survprobe_folds`, `survprobe_n` (the rows that lie in a fold), `per_job` f64 [F, S] and `counts` int64 [F, S, 5]
        {concordant, discordant, tied_risk, tied_time, comparable} on the device.  A fold whose held-out rows have no comparable pair
        gives NaN for its jobs and is left out of the means; when every fold is such, ValueError as sksurv words it.  One host copy."""
        self._fitted()
        F, S, M = self.n_folds_, len(self.strengths), self.num_bins
        if F < 1:
            raise ValueError("SurvivalProbe: evaluate() needs folds (fit(emb, bins, event, time, fold=...))")
        counts = []
        for f, rows in enumerate(self._fold_rows):
            risk = K.survprobe_risk(self._y.index_select(0, rows), self._Wx[f * S:(f + 1) * S], self._bx[f * S:(f + 1) * S], M)
            ev, tm = self._event.index_select(0, rows), self._time.index_select(0, rows)
            counts.extend(K.cindex_counts(ev, tm, risk[s], tied_tol) for s in range(S))
        self.counts = torch.stack(counts).view(F, S, 5)
        c = self.counts.double()
        self.per_job = torch.where(c[:, :, 4] > 0, (c[:, :, 0] + 0.5 * c[:, :, 2]) / c[:, :, 4].clamp(min=1.0),
                                   torch.full((), math.nan, device=self.device, dtype=torch.float64))
        t = self.per_job.cpu()                                                # the one host wait
        ok = ~torch.isnan(t)
        if not bool(ok.any()):
            if not bool(torch.cat([self._event.index_select(0, r) for r in self._fold_rows]).any()):
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
        out["survprobe_cindex"] = float(mean[best])
        out["survprobe_cindex_mean"] = tuple(float(v) for v in mean)
        out["survprobe_cindex_std"] = tuple(float(v) for v in std)
        out["survprobe_best_strength"] = self.best_strength_
        out["survprobe_strengths"] = self.strengths
        out["survprobe_folds"] = F
        out["survprobe_n"] = int(sum(r.numel() for r in self._fold_rows))
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
                raise ValueError("SurvivalProbe: without folds there is no best strength (name one: strength=...)")
            else:
                if self.best_strength_ is None:
                    self.evaluate()
                strength = self.best_strength_
        if isinstance(strength, bool) or not isinstance(strength, (int, float)) or float(strength) not in self.strengths:
            raise ValueError(f"strength must be one of {self.strengths}, got {strength!r}")
        return self.strengths.index(float(strength))

    def predict_risk(self, emb: torch.Tensor, strength: Optional[float] = None) -> torch.Tensor:
        """f32 [n'] on the device: the risks of emb's rows, prepared with the pool's mean, under the all-rows job of `strength` (one of
        the constructor's) or, for None, of `survprobe_best_strength` (evaluate() is run when it has not been; without folds and with
        more than one strength, name the strength).  A larger risk means an earlier expected event."""
        self._fitted()
        self._rows(emb, "emb", self._Wx.shape[2])
        j = self.n_folds_ * len(self.strengths) + self._strength_index(strength)
        q = self._prepare(emb.detach().to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous())
        return K.survprobe_risk(q, self._Wx[j:j + 1], self._bx[j:j + 1], self.num_bins)[0]

    def oof_risk(self, strength: Optional[float] = None) -> torch.Tensor:
        """f32 [n] on the device: every pool row's risk under the job that held its fold out at `strength` (None: as predict_risk),
        NaN for the rows that lie in no fold."""
        self._fitted()
        if self.n_folds_ < 1:
            raise ValueError("SurvivalProbe: oof_risk() needs folds (fit(emb, bins, event, time, fold=...))")
        S, s = len(self.strengths), self._strength_index(strength)
        out = torch.full((self._y.shape[0],), math.nan, device=self.device, dtype=torch.float32)
        for f, rows in enumerate(self._fold_rows):
            j = f * S + s
            out.index_copy_(0, rows, K.survprobe_risk(self._y.index_select(0, rows), self._Wx[j:j + 1], self._bx[j:j + 1], self.num_bins)[0])
        return out
