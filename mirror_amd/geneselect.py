"""Cross-validated recursive gene elimination: which transcripts the RNA encoder ever sees.

The reference picks them offline with `tools/distill_rna_feature.py`: `RFECV(LinearSVC(), step=0.05, cv=StratifiedKFold(5),
scoring="accuracy", min_features_to_select=1)` over the cohort's transcripts against the subtype labels, the union of the selected
transcripts with the COSMIC ones, and a closing report of accuracy and weighted precision / recall / F1.  On ~1000 samples x ~2e5
isoforms that is ~21 elimination rounds x 6 liblinear fits on CPU cores.  Here an elimination round is a batch of linear models over
the SAME prepared rows, the folds side by side as jobs: the shape of `linprobe.py`, with LinearSVC's default loss, the squared hinge,
which is smooth, so that file's plain FISTA iteration applies with another constant.

Rows are prepared once: y = (x - mu_d) rstd_d per column with the population standard deviation (ddof = 0) and rstd = 0 where it is
0 (`mh_colstats`, `mh_standardize`); standardize=False: y = x.  Jobs: J = F + 1; job f < F holds out fold f, job F trains on every
valid row; lambda_j = 1 / (svm_c n_train_j).  There are always C one-vs-rest machines per job, also for C = 2: the two are then mirror
images, and sum_c w_cd^2 ranks the features as sklearn's single machine does.

    F_j(W, b) = r_j sum_{i in train_j} sum_{c < C} max(0, 1 - t_ic v_ic)^2 + (lambda_j / 2) |W o mask_j|^2
    t_ic      = +1 if label_i = c else -1,   v = W y_i + b,   r_j = 1 / n_train_j
    train_j   = { i : label_i in [0, C), fold_i >= 0, fold_i != heldout_j }

This has the minimiser of `LinearSVC(C=svm_c)` up to the intercept: the bias is NOT penalised here (the other probes' convention),
liblinear penalises it as one more weight.  fit_intercept=False pins the bias to 0 and is the setting under which sklearn is an exact
yardstick.  Weights of eliminated features are exactly 0 and stay 0.

One round is the FISTA of `linprobe.py`, restarted at t = 1 (beta from `fista_betas`) and warm-started from the previous round's
weights, with eta_j = 1 / (2 rho_j + lambda_j), rho_j = 1 + max_i sum_{d active in j} y_id^2 (`mh_gsel_rowsq`; the hinge's second
derivative is <= 2, r_j sum y y^T <= rho, the bias is a feature of value 1).  All jobs run in lockstep; an iteration is
`mh_gsel_grad` (two launches: the tile product split over D, then the hinge) and `mh_gsel_step` (one launch); the host waits once per
`check_every` iterations, for the max-norm gradient alone, and a round stops when every job is <= tol or at max_iter.  After the round
every fold job's held-out rows are scored (the classes from `mh_gsel_grad`, accuracy from integer counts) and, unless the active
count has reached min_features, every job drops the k = min(step, active - min_features) features of smallest sum_c Wx[j, c, d]^2
(`mh_gsel_eliminate`: exact, ties to the smaller index).  step is sklearn's: a float in (0, 1) means int(max(1, step D)), an int >= 1
is taken as it is.  All jobs share the schedule of subset sizes.

The subset size is chosen as sklearn 1.7's `RFECV.fit` does: the size with the highest score summed over the folds, ties to the
fewest features.  The all-rows job's elimination order, cut at that size, is the support: the order is deterministic, so no second
elimination run is needed.  One more single-job fit on the support, from zero, gives `coef_` / `intercept_`.

Not built: compaction of the active columns in late rounds (the products walk all D columns, eliminated ones as zeros); `scoring`
other than accuracy; L1 / hinge loss; a pool gathered over DDP ranks.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Optional

import torch

from . import kernels as K
from ._lib import MirrorHipError
from .linprobe import _int_in, fista_betas

__all__ = ["GeneSelect", "size_schedule"]


def size_schedule(D: int, step, min_features: int = 1) -> list:
    """The subset sizes of the rounds, D first, min_features last (sklearn's RFE: k = int(max(1, step D)) for a float step in (0, 1))."""
    k = int(max(1, step * D)) if isinstance(step, float) else step
    sizes = [D]
    while sizes[-1] > min_features:
        sizes.append(sizes[-1] - min(k, sizes[-1] - min_features))
    return sizes


class GeneSelect:
    """`fit(x, labels, fold=None)` runs the elimination; `predict` / `score` use the final fit on the support; `selected(keep=)` is the
    support united with further indices (the COSMIC union); `transform(x)` keeps those columns.

    fold: an integer [n] tensor with values in [0, F), F = max + 1 (found in the one host copy `fit` makes of it); a negative value
    keeps the row out of every job; every fold in [0, F) needs a row.  fold=None: plain RFE of the one all-rows job down to
    min_features, with no choice of size.

    After `fit`, on the device: `support_` bool [D], `ranking_` int64 [D] (sklearn's meaning: 1 = selected, 2 = dropped by the last
    elimination before the chosen size, ..), `elim_round_` int32 [J, D] (the round that dropped the feature from job j, -1: never),
    `coef_` f32 [C, D] and `intercept_` f32 [C] of the final fit (in the standardised space; 0 outside the support), `mu_` / `rstd_`
    f32 [D] (None for standardize=False).  On the host: `n_features_`, `n_iter_` (a list, one count per round), `n_iter_final_`, and
    `cv_results_` (None without folds): a dict in ASCENDING size as sklearn's, `n_features` a list, `mean_test_score`, `std_test_score`
    (over the folds, ddof = 0) and `split{f}_test_score` f64 host tensors."""

    def __init__(self, num_classes: int, step=0.05, min_features: int = 1, svm_c: float = 1.0, max_iter: int = 2000, tol: float = 1e-4,
                 standardize: bool = True, fit_intercept: bool = True, check_every: int = 16, device=None):
        _int_in(num_classes, 2, 64, "num_classes")
        if isinstance(step, bool) or not ((isinstance(step, float) and 0.0 < step < 1.0) or (isinstance(step, int) and 1 <= step <= (1 << 18))):
            raise ValueError(f"step must be a float in (0, 1) or an int in [1, 2^18], got {step!r}")
        _int_in(min_features, 1, 1 << 18, "min_features")
        if isinstance(svm_c, bool) or not isinstance(svm_c, (int, float)) or not (0.0 < float(svm_c) < math.inf):
            raise ValueError(f"svm_c must be a positive finite float, got {svm_c!r}")
        _int_in(max_iter, 1, 1 << 20, "max_iter")
        if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not (0.0 <= float(tol) < math.inf):
            raise ValueError(f"tol must be a non-negative finite float, got {tol!r}")
        if not isinstance(standardize, bool):
            raise ValueError(f"standardize must be a bool, got {standardize!r}")
        if not isinstance(fit_intercept, bool):
            raise ValueError(f"fit_intercept must be a bool, got {fit_intercept!r}")
        _int_in(check_every, 1, 1 << 16, "check_every")
        d = torch.device("cuda") if device is None else torch.device(device)
        if d.type != "cuda":
            raise MirrorHipError(f"mirror_amd metrics keep their state on a HIP device, got {d}")
        self.num_classes = num_classes
        self.step = step
        self.min_features = min_features
        self.svm_c = float(svm_c)
        self.max_iter = max_iter
        self.tol = float(tol)
        self.standardize = standardize
        self.fit_intercept = fit_intercept
        self.check_every = check_every
        self.device = d
        self._clear()

    def _clear(self) -> None:
        self.mu_ = self.rstd_ = None
        self.support_ = self.ranking_ = self.elim_round_ = self.coef_ = self.intercept_ = None
        self._W = self._b = None
        self.n_features_ = 0
        self.n_iter_ = []
        self.n_iter_final_ = 0
        self.n_folds_ = 0
        self.cv_results_ = None

    # ------------------------------------------------------------------ preparation
    @staticmethod
    def _rows(x, what: str, D: Optional[int] = None) -> None:
        ok = isinstance(x, torch.Tensor) and x.dim() == 2 and x.is_floating_point() and (D is None or x.shape[1] == D)
        if not ok:
            got = f"{x.dtype} {tuple(x.shape)}" if isinstance(x, torch.Tensor) else type(x).__name__
            raise ValueError(f"{what} must be floating point [n, {'D' if D is None else D}], got {got}")
        n, d = x.shape
        if not (1 <= n <= (1 << 20)) or not (1 <= d <= (1 << 18)):
            raise MirrorHipError(f"{what}: n = {n} (1..2^20), D = {d} (1..2^18)")

    def _prepare(self, x: torch.Tensor) -> torch.Tensor:
        """A fresh f32 device copy of x, standardised in place with the pool's mu / rstd."""
        y = x.detach().to(device=self.device, dtype=torch.float32, non_blocking=True, copy=True).contiguous()
        return K.standardize(y, self.mu_, self.rstd_, out=y) if self.standardize else y

    # ------------------------------------------------------------------ one round
    def _round(self, y, lab, fd, heldout, rscale, lam, Wx, bx, Wz, bz, mask, G, ws, gmax) -> int:
        """FISTA from (Wx, bx), restarted at t = 1, every job in lockstep; returns the iterations done."""
        C = self.num_classes
        Wz.copy_(Wx)
        bz.copy_(bx)
        rho = 1.0 + K.gsel_rowsq(y, mask).amax(1)
        eta = (1.0 / (2.0 * rho + lam)).to(torch.float32)
        done = 0
        for beta in fista_betas(self.max_iter):
            K.gsel_grad(y, Wz, bz, lab, fd, heldout, rscale, C, G=G, workspace=ws)
            K.gsel_step(y, G, Wx, bx, Wz, bz, lam, eta, beta, mask, self.fit_intercept, C, gmax_part=gmax)
            done += 1
            if done % self.check_every == 0 and done < self.max_iter:
                if bool((gmax.amax(0) <= self.tol).all()):                    # the one host wait of these iterations
                    break
        return done

    # ------------------------------------------------------------------ fit
    def fit(self, x: torch.Tensor, labels: torch.Tensor, fold: Optional[torch.Tensor] = None) -> "GeneSelect":
        self._rows(x, "x")
        n, D = x.shape
        for t, name in ((labels, "labels"),) + (((fold, "fold"),) if fold is not None else ()):
            if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.numel() != n or t.dtype not in (torch.int32, torch.int64):
                got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"{name} must be an int32 / int64 [{n}] tensor, got {got}")
        if self.min_features > D:
            raise ValueError(f"GeneSelect: min_features = {self.min_features} exceeds D = {D}")
        C = self.num_classes
        Cp = K.fewshot_cp(C)
        F = 0
        if fold is not None:
            fh = fold.detach().cpu()                                          # the one host copy: F and that every fold has a row
            F = max(int(fh.max()) + 1, 0)
            if F < 1:
                raise ValueError("GeneSelect: no row lies in a fold (every fold value is negative)")
            empty = [f for f in range(F) if not bool((fh == f).any())]
            if empty:
                raise ValueError(f"GeneSelect: no row of fold(s) {empty} (fold values must cover [0, {F}))")
        J = F + 1
        if J * Cp > (1 << 20) or n * J * Cp > (1 << 28):
            raise MirrorHipError(f"GeneSelect: ({F} folds + 1) x {Cp} class slots over n = {n} rows (J * Cp <= 2^20, n * J * Cp <= 2^28)")
        self._clear()
        dev = self.device
        y = x.detach().to(device=dev, dtype=torch.float32, non_blocking=True, copy=True).contiguous()
        if self.standardize:
            self.mu_, self.rstd_ = K.colstats(y)
            K.standardize(y, self.mu_, self.rstd_, out=y)
        lab = labels.detach().to(device=dev, dtype=torch.int64, non_blocking=True, copy=True).contiguous()
        if fold is not None:
            fd = fold.detach().to(device=dev, non_blocking=True).clamp(min=-1).to(torch.int32).contiguous()
        else:
            fd = torch.zeros((n,), device=dev, dtype=torch.int32)
        self.n_folds_ = F
        heldout = torch.tensor(list(range(F)) + [-1], dtype=torch.int32).to(dev, non_blocking=True)
        valid = (lab >= 0) & (lab < C) & (fd >= 0)
        n_train = (valid[None, :] & (fd[None, :] != heldout[:, None])).sum(1)
        rscale = torch.where(n_train > 0, 1.0 / n_train.clamp(min=1).to(torch.float32), torch.zeros((), device=dev))
        lam = (1.0 / (self.svm_c * n_train.clamp(min=1).to(torch.float64))).to(torch.float32)
        sizes = size_schedule(D, self.step, self.min_features)
        R = len(sizes)

        Wx = torch.zeros((J, Cp, D), device=dev, dtype=torch.float32)
        Wz = torch.zeros_like(Wx)
        bx = torch.zeros((J, Cp), device=dev, dtype=torch.float32)
        bz = torch.zeros_like(bx)
        mask = torch.ones((J, D), device=dev, dtype=torch.uint8)
        elim = torch.full((J, D), -1, device=dev, dtype=torch.int32)
        G = torch.empty((n, J * Cp), device=dev, dtype=torch.float32)
        ws = K.gsel_workspace(n, J, Cp, D, dev)
        gmax = torch.empty(((D + 1 + 127) // 128, J), device=dev, dtype=torch.float32)
        if F:
            in_fold = valid[None, :] & (fd[None, :] == heldout[:F, None])     # [F, n]: the rows job f is scored on
        correct = []
        for e in range(R):
            self.n_iter_.append(self._round(y, lab, fd, heldout, rscale, lam, Wx, bx, Wz, bz, mask, G, ws, gmax))
            if F:
                pred = K.gsel_grad(y, Wx, bx, lab, fd, heldout, rscale, C, G=G, want_pred=True, workspace=ws)[2]
                correct.append(((pred[:F].to(torch.int64) == lab[None, :]) & in_fold).sum(1))
            if e + 1 < R:
                K.gsel_eliminate(Wx, Wz, mask, elim, sizes[e] - sizes[e + 1], e, C)
        self.elim_round_ = elim

        if F:
            counts = torch.cat([torch.stack(correct, 1), in_fold.sum(1, keepdim=True)], 1).cpu()     # [F, R + 1]: one host wait
            unscored = [f for f in range(F) if int(counts[f, R]) == 0]
            if unscored:
                raise ValueError(f"GeneSelect: no row of fold(s) {unscored} has a label in [0, {C}): nothing to score them on")
            scores = [[int(counts[f, e]) / int(counts[f, R]) for e in range(R)] for f in range(F)]
            sums = [sum(scores[f][e] for f in range(F)) for e in range(R)]    # in fold order
            m = max(range(R), key=lambda e: (sums[e], -sizes[e]))
            st = torch.tensor(scores, dtype=torch.float64)
            res = OrderedDict()
            res["n_features"] = sizes[::-1]
            res["mean_test_score"] = st.mean(0).flip(0)
            res["std_test_score"] = st.std(0, unbiased=False).flip(0)
            for f in range(F):
                res[f"split{f}_test_score"] = st[f].flip(0)
            self.cv_results_ = res
        else:
            m = R - 1
        e_all = elim[J - 1].to(torch.int64)
        self.support_ = (e_all < 0) | (e_all >= m)
        self.ranking_ = torch.where(self.support_, 1, m - e_all + 1)
        self.n_features_ = sizes[m]

        W = torch.zeros((1, Cp, D), device=dev, dtype=torch.float32)
        b = torch.zeros((1, Cp), device=dev, dtype=torch.float32)
        m1 = self.support_.to(torch.uint8).view(1, D).contiguous()
        self.n_iter_final_ = self._round(y, lab, fd, heldout[J - 1:], rscale[J - 1:].contiguous(), lam[J - 1:].contiguous(), W, b,
                                         torch.zeros_like(W), torch.zeros_like(b), m1, torch.empty((n, Cp), device=dev, dtype=torch.float32),
                                         ws, torch.empty(((D + 1 + 127) // 128, 1), device=dev, dtype=torch.float32))
        self._W, self._b = W, b
        self.coef_, self.intercept_ = W[0, :C, :], b[0, :C]
        return self

    def _fitted(self) -> None:
        if self._W is None:
            raise ValueError("GeneSelect: nothing is fitted (call fit() first)")

    # ------------------------------------------------------------------ new rows
    def predict(self, x: torch.Tensor) -> torch.Tensor:
        """int32 [n'] on the device: the classes of x's rows, prepared with the pool's mu / rstd, under the final fit (mh_gsel_grad's
        class rule: the largest v_c, ties to the smaller class, -1 for a NaN row)."""
        self._fitted()
        self._rows(x, "x", self._W.shape[2])
        q = self._prepare(x)
        n = q.shape[0]
        none = torch.full((n,), -1, device=self.device, dtype=torch.int32)    # no row trains: G is zeros, only the classes matter
        return K.gsel_grad(q, self._W, self._b, torch.zeros((n,), device=self.device, dtype=torch.int64), none,
                           torch.full((1,), -1, device=self.device, dtype=torch.int32),
                           torch.zeros((1,), device=self.device, dtype=torch.float32), self.num_classes, want_pred=True)[2][0]

    def score(self, x: torch.Tensor, labels: torch.Tensor):
        """The reference's closing report on (x, labels): an OrderedDict of `accuracy` and support-weighted `precision`, `recall`, `f1`
        (sklearn's average="weighted", zero_division=0), formed in f64 from mh_fewshot_tally's integer confusion counts; then
        `confusion` int32 [C, C] ([label, prediction]) on the device.  One host copy."""
        pred = self.predict(x)
        if not isinstance(labels, torch.Tensor) or labels.dim() != 1 or labels.numel() != pred.numel() or labels.dtype not in (torch.int32, torch.int64):
            got = f"{labels.dtype} {tuple(labels.shape)}" if isinstance(labels, torch.Tensor) else type(labels).__name__
            raise ValueError(f"labels must be an int32 / int64 [{pred.numel()}] tensor, got {got}")
        lab = labels.detach().to(device=self.device, dtype=torch.int64, non_blocking=True).contiguous()
        conf = K.fewshot_tally(pred.view(1, -1), lab, self.num_classes)[0][0]
        c = conf.double()
        tp, sup, prd = c.diagonal(), c.sum(1), c.sum(0)
        zero = torch.zeros((), device=self.device, dtype=torch.float64)
        prec = torch.where(prd > 0, tp / prd.clamp(min=1), zero)
        rec = torch.where(sup > 0, tp / sup.clamp(min=1), zero)
        f1 = torch.where(sup + prd > 0, 2 * tp / (sup + prd).clamp(min=1), zero)
        w = sup / sup.sum()
        vals = torch.stack([tp.sum() / sup.sum(), (w * prec).sum(), (w * rec).sum(), (w * f1).sum()]).cpu()       # the one host wait
        out: "OrderedDict[str, object]" = OrderedDict(zip(("accuracy", "precision", "recall", "f1"), (float(v) for v in vals)))
        out["confusion"] = conf
        return out

    def selected(self, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int64 on the device, ascending: the indices of `support_`, united with the index tensor `keep` (int32 / int64, values in
        [0, D): the transcripts kept whatever the elimination says)."""
        self._fitted()
        s = self.support_
        if keep is not None:
            D = s.numel()
            if not isinstance(keep, torch.Tensor) or keep.dim() != 1 or keep.dtype not in (torch.int32, torch.int64):
                got = f"{keep.dtype} {tuple(keep.shape)}" if isinstance(keep, torch.Tensor) else type(keep).__name__
                raise ValueError(f"keep must be a 1-D int32 / int64 tensor, got {got}")
            kh = keep.detach().to(torch.int64)
            if kh.numel() and not bool(((kh >= 0) & (kh < D)).all()):
                raise ValueError(f"keep holds indices outside [0, {D})")
            s = s.clone()
            s[kh.to(self.device)] = True
        return torch.nonzero(s).view(-1)

    def transform(self, x: torch.Tensor, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x's columns `selected(keep)`, as they are (not standardised), on the device."""
        self._fitted()
        self._rows(x, "x", self.support_.numel())
        return x.detach().to(self.device, non_blocking=True).index_select(1, self.selected(keep))
