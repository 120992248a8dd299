"""Linear probe of frozen embeddings: the figure the MIRROR paper reports first for subtyping.

The reference trains it with `train_subtyping.py --linear_probe` (freeze the encoder, train one linear layer) over the folds of
`tools/gen_splits.py`, pushing the slides through the frozen encoder every epoch.  On cached embeddings [n, D] the same figure is small
and regular: with F folds and S L2 strengths there are J = (F + 1) S independent softmax regressions over the SAME prepared rows,

    F_j(W, b) = r_j sum_{i in train_j} CE(softmax(W y_i + b), label_i) + (lambda_j / 2) |W|^2,      r_j = 1 / |train_j|
    train_j   = { i : label_i in [0, C), fold_i >= 0, fold_i != heldout_j }

(the bias is not penalised: sklearn's convention; `LogisticRegression(C=1 / (lambda n_train))` has the same minimiser).  Job f S + s
holds out fold f at strength s; the last S jobs hold out nothing and are the models `predict` uses.  Every job runs the same plain
FISTA iteration from zero for the same number of steps,

    g = grad F_j(Z_k),   X_{k+1} = Z_k - eta_j g,   Z_{k+1} = X_{k+1} + beta_k (X_{k+1} - X_k)
    t_0 = 1,  t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2,  beta_k = (t_k - 1) / t_{k+1}          (host, f64; passed as an f32 scalar)
    eta_j = 1 / L_j,  L_j = rho / 2 + lambda_j,  rho = 1 + max_i |y_i|^2                    (the softmax Hessian is <= 1 / 2 and
                                                                                             the bias is a feature of value 1)

whose guarantee is F_j(X_k) - F_j* <= 2 L_j |(W*, b*)|^2 / (k + 1)^2.  One iteration is two launches and nothing else:
`mh_linprobe_grad` (every job's logits, softmax and logit gradient: the J Cp weight rows are the keys of the retrieval kernels'
exact-f32 tile product) and `mh_linprobe_step` (every weight gradient as one product contracted over the rows, and the update in
place).  Both are deterministic: no float atomics, two fits agree bit for bit.  Scoring the held-out folds reuses
`mh_fewshot_predict` / `mh_fewshot_tally` with a fold's S jobs in the role of the episodes.

The figures that need a score (the reference's validation pass prints Acc, AUC and F1: train_subtyping.py:1355-1432) come from two
more launches per fold: `mh_linprobe_proba` (the tile product and the softmax of `mh_linprobe_grad`, bit for bit, with the
probabilities [S, n_f, C] and the held-out log-loss as its outputs) and `mh_auroc_counts_many` (the exact integer pair counts of
`mh_auroc_counts` for the S tables at once).  `evaluate(auroc=True)` forms the one-vs-rest AUROC in f64 from those counts, ON THE
SOFTMAX PROBABILITIES as sklearn's `roc_auc_score(multi_class="ovr")` does on `predict_proba`; the reference feeds raw logits to
torcheval's MulticlassAUROC, which ranks the same for C = 2 and differently for C > 2.  `predict_proba` / `oof_proba` hand the
probabilities out.

Not built: class weights, calibration figures (ECE, Brier score), momentum restart or line search, bf16 embeddings, a pool gathered
over DDP ranks, a split of the step kernel over n (at J Cp = 160, D = 512 it runs on a handful of workgroups).
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Optional, Sequence

import torch

from . import kernels as K
from ._lib import MirrorHipError

__all__ = ["LinearProbe", "fista_betas"]


def _int_in(v, lo: int, hi: int, what: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not (lo <= v <= hi):
        raise ValueError(f"{what} must be an int in [{lo}, {hi}], got {v!r}")
    return v


def _floats(t: torch.Tensor):
    """A host tensor as floats: a float for a scalar, nested tuples otherwise."""
    return tuple(_floats(x) for x in t) if t.dim() else float(t)


def fista_betas(steps: int) -> list:
    """beta_0 .. beta_{steps - 1} of the iteration above, in f64 on the host (beta_0 = 0)."""
    out, t = [], 1.0
    for _ in range(steps):
        t1 = (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0
        out.append((t - 1.0) / t1)
        t = t1
    return out


class LinearProbe:
    """`fit(emb, labels, fold=None)` trains every job; `evaluate()` scores the held-out folds (`auroc=True`: with AUROC and log-loss);
    `predict(emb, strength=None)` classifies new rows under the all-rows job of the best (or the given) strength and `predict_proba`
    gives their class probabilities; `oof_proba(strength=None)` gives every pool row's under the job that held its fold out.

    The rows are prepared as FewShotProbe / ClusterProbe prepare them: center=True, y = (x - mu) / max(|x - mu|, 1e-12) with mu the
    pool's column mean (mh_colmean, mh_center_l2norm); center=False, normalised only.  Later queries use the POOL's mean.

    fold: an integer [n] tensor with values in [0, F), F = max + 1 (found in the one host copy `fit` makes of it); a negative value
    keeps the row out of every job; every fold in [0, F) needs a row.  fold=None: F = 0, J = S, every valid row trains.

    After `fit`, on the device: `coef_` f32 [J, C, D] (a view of the padded weights, in the prepared space), `intercept_` f32 [J, C],
    `loss_` f64 [J] (F_j at coef_ / intercept_: the data term from mh_linprobe_grad in f64 sums of f32 terms, the regulariser
    added here), `grad_inf_` f32 [J] (the max norm of the gradient the LAST step used, i.e. at its look-ahead point), `n_train_`
    int64 [J]; `n_iter_` an int.  `fit` waits on the host once per `check_every` iterations, for `grad_inf_` alone, and stops when every
    job is <= tol (a NaN job never is) or at max_iter.  A job without training rows keeps zero weights.  A NaN row makes every job
    that trains on it NaN."""

    def __init__(self, num_classes: int, strengths: Sequence[float] = (1e-4, 1e-3, 1e-2, 1e-1), max_iter: int = 2000,
                 tol: float = 1e-4, center: bool = True, check_every: int = 16, device=None):
        _int_in(num_classes, 2, 64, "num_classes")
        if isinstance(strengths, (str, bytes)) or not isinstance(strengths, (tuple, list)) or not (1 <= len(strengths) <= 1024):
            raise ValueError(f"strengths must be a tuple of 1..1024 positive floats, got {strengths!r}")
        for s in strengths:
            if isinstance(s, bool) or not isinstance(s, (int, float)) or not (0.0 < float(s) < math.inf):
                raise ValueError(f"strengths must be positive finite floats, got {s!r}")
        _int_in(max_iter, 1, 1 << 20, "max_iter")
        if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not (0.0 <= float(tol) < math.inf):
            raise ValueError(f"tol must be a non-negative finite float, got {tol!r}")
        if not isinstance(center, bool):
            raise ValueError(f"center must be a bool, got {center!r}")
        _int_in(check_every, 1, 1 << 16, "check_every")
        d = torch.device("cuda") if device is None else torch.device(device)
        if d.type != "cuda":
            raise MirrorHipError(f"mirror_amd metrics keep their state on a HIP device, got {d}")
        self.num_classes = num_classes
        self.strengths = tuple(float(s) for s in strengths)
        self.max_iter = max_iter
        self.tol = float(tol)
        self.center = center
        self.check_every = check_every
        self.device = d
        self._clear()

    def _clear(self) -> None:
        self.mu_ = self._y = self._labels = self._fold_rows = None
        self._Wx = self._bx = None
        self.coef_ = self.intercept_ = self.loss_ = self.grad_inf_ = self.n_train_ = None
        self.n_iter_ = 0
        self.n_folds_ = 0
        self.per_job = self.per_job_auc = self.per_job_nll = self.best_strength_ = None

    # ------------------------------------------------------------------ preparation
    @staticmethod
    def _rows(emb, what: str, D: Optional[int] = None) -> None:
        ok = isinstance(emb, torch.Tensor) and emb.dim() == 2 and emb.is_floating_point() and (D is None or emb.shape[1] == D)
        if not ok:
            got = f"{emb.dtype} {tuple(emb.shape)}" if isinstance(emb, torch.Tensor) else type(emb).__name__
            raise ValueError(f"{what} must be floating point [n, {'D' if D is None else D}], got {got}")
        n, d = emb.shape
        if not (1 <= n <= (1 << 20)) or not (1 <= d <= 4096):
            raise MirrorHipError(f"{what}: n = {n} (1..2^20), D = {d} (1..4096)")

    def _prepare(self, x: torch.Tensor) -> torch.Tensor:
        mu = self.mu_ if self.center else torch.zeros((x.shape[1],), device=self.device, dtype=torch.float32)
        return K.center_l2norm(x, mu)

    # ------------------------------------------------------------------ fit
    def fit(self, emb: torch.Tensor, labels: torch.Tensor, fold: Optional[torch.Tensor] = None) -> "LinearProbe":
        self._rows(emb, "emb")
        n, D = emb.shape
        for t, name in ((labels, "labels"),) + (((fold, "fold"),) if fold is not None else ()):
            if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.numel() != n or t.dtype not in (torch.int32, torch.int64):
                got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"{name} must be an int32 / int64 [{n}] tensor, got {got}")
        C, S = self.num_classes, len(self.strengths)
        Cp = K.fewshot_cp(C)
        fold_rows = []
        if fold is not None:
            fh = fold.detach().cpu()                                          # the one host copy: F and every fold's rows
            F = max(int(fh.max()) + 1, 0)
            if (F + 1) * S * Cp > (1 << 20) or n * (F + 1) * S * Cp > (1 << 28):
                raise MirrorHipError(f"LinearProbe: ({F} folds + 1) x {S} strengths x {Cp} class slots over n = {n} rows "
                                     "(J * Cp <= 2^20, n * J * Cp <= 2^28)")
            fold_rows = [torch.nonzero(fh == f).view(-1) for f in range(F)]
            empty = [f for f, r in enumerate(fold_rows) if r.numel() == 0]
            if empty:
                raise ValueError(f"LinearProbe: no row of fold(s) {empty} (fold values must cover [0, {F}))")
        else:
            F = 0
            if S * Cp > (1 << 20) or n * S * Cp > (1 << 28):
                raise MirrorHipError(f"LinearProbe: {S} strengths x {Cp} class slots over n = {n} rows (J * Cp <= 2^20, n * J * Cp <= 2^28)")
        J = (F + 1) * S
        self._clear()
        dev = self.device
        x = emb.detach().to(device=dev, dtype=torch.float32, non_blocking=True, copy=True).contiguous()
        self.mu_ = K.colmean(x) if self.center else None
        y = self._y = self._prepare(x)
        lab = self._labels = labels.detach().to(device=dev, dtype=torch.int64, non_blocking=True, copy=True).contiguous()
        if fold is not None:
            fd = fold.detach().to(device=dev, non_blocking=True).clamp(min=-1).to(torch.int32).contiguous()
        else:
            fd = torch.zeros((n,), device=dev, dtype=torch.int32)
        self._fold_rows = [r.to(device=dev, non_blocking=True) for r in fold_rows]
        self.n_folds_ = F
        heldout = torch.tensor([f for f in range(F) for _ in range(S)] + [-1] * S, dtype=torch.int32).to(dev, non_blocking=True)
        lam = torch.tensor(list(self.strengths) * (F + 1), dtype=torch.float32).to(dev, non_blocking=True)
        valid = (lab >= 0) & (lab < C) & (fd >= 0)
        self.n_train_ = (valid[None, :] & (fd[None, :] != heldout[:, None])).sum(1)
        rscale = torch.where(self.n_train_ > 0, 1.0 / self.n_train_.clamp(min=1).to(torch.float32), torch.zeros((), device=dev))
        rho = 1.0 + (y * y).sum(1).max()
        eta = (1.0 / (0.5 * rho + lam)).to(torch.float32)

        Wx = torch.zeros((J, Cp, D), device=dev, dtype=torch.float32)
        Wz = torch.zeros_like(Wx)
        bx = torch.zeros((J, Cp), device=dev, dtype=torch.float32)
        bx[:, C:] = -math.inf
        bz = bx.clone()
        G = torch.empty((n, J * Cp), device=dev, dtype=torch.float32)
        gmax = torch.empty(((D + 1 + 127) // 128, J), device=dev, dtype=torch.float32)
        done = 0
        for beta in fista_betas(self.max_iter):
            K.linprobe_grad(y, Wz, bz, lab, fd, heldout, rscale, C, G=G)
            K.linprobe_step(y, G, Wx, bx, Wz, bz, lam, eta, beta, C, gmax_part=gmax)
            done += 1
            if done % self.check_every == 0 and done < self.max_iter:
                if bool((gmax.amax(0) <= self.tol).all()):                    # the one host wait of these iterations
                    break
        self.n_iter_ = done
        self.grad_inf_ = gmax.amax(0)
        _, part = K.linprobe_grad(y, Wx, bx, lab, fd, heldout, rscale, C, G=G, want_loss=True)
        self._Wx, self._bx = Wx, bx
        self.coef_, self.intercept_ = Wx[:, :C, :], bx[:, :C]
        self.loss_ = part.sum(0) + 0.5 * lam.double() * self.coef_.double().square().sum((1, 2))
        return self

    def _fitted(self) -> None:
        if self._Wx is None:
            raise ValueError("LinearProbe: nothing is fitted (call fit() first)")

    # ------------------------------------------------------------------ scores of the held-out folds
    def evaluate(self, auroc: bool = False, average: Optional[str] = "macro", select: str = "acc"):
        """Every fold's rows under the S jobs that held it out: an OrderedDict of `linprobe_acc` (per cent), `linprobe_bacc` (balanced
        accuracy, per cent) and `linprobe_f1` (macro F1) at the best strength, each the mean over the folds, with `_mean` and `_std`
        (sample standard deviation over the folds, 0 for one fold) as tuples over the strengths in the constructor's order; then
        `linprobe_best_strength` (the highest mean accuracy, ties to the larger lambda), `linprobe_strengths`, `linprobe_folds`,
        `linprobe_n` (the rows that lie in a fold) and `per_job` f64 [F, S, 3] on the device.  One host copy.

        auroc=True adds the two figures that need a score, per fold from one `mh_linprobe_proba` over the fold's rows under its S
        jobs and one `mh_auroc_counts_many` on the result: `linprobe_auc` and `linprobe_nll` with `_mean` / `_std` as above,
        `per_job_auc` f64 [F, S, C] and `per_job_nll` f64 [F, S] on the device; still one host copy.  The AUROC is one-vs-rest ON THE
        SOFTMAX PROBABILITIES, class c's column against the rows of every other label, U2_c / (2 P_c Q_c) in f64 from the exact
        integer pair counts: sklearn's `roc_auc_score(predict_proba, multi_class="ovr")`.  The reference hands torcheval's
        MulticlassAUROC the raw logits (train_subtyping.py:1391); the two rankings agree for C = 2 and differ for C > 2, where a row's
        lse moves its probability of c but not its logit.  A class without a positive or without a negative in the fold (P_c Q_c = 0)
        is NaN in `per_job_auc` and left out of the average; a NaN probability in a column makes that job's AUROC NaN; a fold where no
        class has both gives NaN.  average: "macro" (the mean over the classes with P_c Q_c > 0), "weighted" (weights P_c) or None
        (per class only: `linprobe_auc` is a tuple over the classes, `_mean` / `_std` tuples over the strengths of such tuples).
        `linprobe_nll` is the mean held-out log-loss: the sum of lse - v_label over the fold's rows with a label in [0, C), divided by
        their number.  select: "acc", "auc" (the highest mean AUROC; needs an average) or "nll" (the lowest mean log-loss) chooses
        `linprobe_best_strength`, ties to the larger lambda; "auc" and "nll" need auroc=True."""
        if not isinstance(auroc, bool):
            raise ValueError(f"auroc must be a bool, got {auroc!r}")
        if average is not None and average not in ("macro", "weighted"):
            raise ValueError(f"average must be 'macro', 'weighted' or None, got {average!r}")
        if select not in ("acc", "auc", "nll"):
            raise ValueError(f"select must be 'acc', 'auc' or 'nll', got {select!r}")
        if select != "acc" and not auroc:
            raise ValueError(f"select={select!r} needs auroc=True")
        if select == "auc" and average is None:
            raise ValueError("select='auc' needs average='macro' or 'weighted'")
        self._fitted()
        F, S, C = self.n_folds_, len(self.strengths), self.num_classes
        if F < 1:
            raise ValueError("LinearProbe: evaluate() needs folds (fit(emb, labels, fold=...))")
        tables, aucs, pos, nlls = [], [], [], []
        for f, rows in enumerate(self._fold_rows):
            q = self._y.index_select(0, rows)
            lab = self._labels.index_select(0, rows)
            W, b = self._Wx[f * S:(f + 1) * S], self._bx[f * S:(f + 1) * S]
            pred = K.fewshot_predict(q, W, b, C)
            tables.append(K.fewshot_tally(pred, lab, C)[2])
            if auroc:
                P, part = K.linprobe_proba(q, W, b, C, labels=lab, want_nll=True)
                cnt = K.auroc_counts_many(P, lab).double()                    # [S, C, 4]: every count is below 2^53, exact in f64
                a = cnt[:, :, 0] / (2.0 * cnt[:, :, 1] * cnt[:, :, 2])        # 0 / 0 = NaN where P_c Q_c = 0
                aucs.append(torch.where(cnt[:, :, 3] > 0, math.nan, a))
                pos.append(cnt[0, :, 1] * (cnt[0, :, 2] > 0))                 # P_c of the classes that count, 0 for the others
                nlls.append(part.sum(0) / ((lab >= 0) & (lab < C)).sum())
        self.per_job = torch.stack(tables)
        if auroc:
            self.per_job_auc, self.per_job_nll = torch.stack(aucs), torch.stack(nlls)
            packed = torch.cat([self.per_job.reshape(-1), self.per_job_auc.reshape(-1), self.per_job_nll.reshape(-1),
                                torch.stack(pos).reshape(-1)]).cpu()          # the one host wait
            t, auc_t, nll_t, w = (x.reshape(sh) for x, sh in zip(packed.split([F * S * 3, F * S * C, F * S, F * C]),
                                                                  ((F, S, 3), (F, S, C), (F, S), (F, C))))
        else:
            self.per_job_auc = self.per_job_nll = None
            t = self.per_job.cpu()                                            # the one host wait
        mean = t.mean(0)
        std = t.std(0, unbiased=True) if F > 1 else torch.zeros_like(mean)
        score = [float(a) for a in mean[:, 0]]
        if auroc:
            if average is None:
                job_auc = auc_t                                               # [F, S, C]
            else:
                wt = (w > 0).double() if average == "macro" else w            # [F, C]
                job_auc = torch.where(wt[:, None, :] > 0, auc_t, 0.0).mul(wt[:, None, :]).sum(2) / wt.sum(1)[:, None]
            auc_mean, nll_mean = job_auc.mean(0), nll_t.mean(0)
            auc_std = job_auc.std(0, unbiased=True) if F > 1 else torch.zeros_like(auc_mean)
            nll_std = nll_t.std(0, unbiased=True) if F > 1 else torch.zeros_like(nll_mean)
            if select == "auc":
                score = [float(a) for a in auc_mean]
            elif select == "nll":
                score = [-float(a) for a in nll_mean]
        score = [a if a == a else -math.inf for a in score]
        best = max(range(S), key=lambda s: (score[s], self.strengths[s]))
        self.best_strength_ = self.strengths[best]
        out: "OrderedDict[str, object]" = OrderedDict()
        for k, name in enumerate(("linprobe_acc", "linprobe_bacc", "linprobe_f1")):
            out[name] = float(mean[best, k])
            out[name + "_mean"] = tuple(float(v) for v in mean[:, k])
            out[name + "_std"] = tuple(float(v) for v in std[:, k])
        out["linprobe_best_strength"] = self.best_strength_
        out["linprobe_strengths"] = self.strengths
        out["linprobe_folds"] = F
        out["linprobe_n"] = int(sum(r.numel() for r in self._fold_rows))
        out["per_job"] = self.per_job
        if auroc:
            for name, m, sd in (("linprobe_auc", auc_mean, auc_std), ("linprobe_nll", nll_mean, nll_std)):
                out[name], out[name + "_mean"], out[name + "_std"] = _floats(m[best]), _floats(m), _floats(sd)
            out["per_job_auc"], out["per_job_nll"] = self.per_job_auc, self.per_job_nll
        return out

    def _strength_index(self, strength: Optional[float]) -> int:
        """The position of `strength` among the constructor's, or for None of `linprobe_best_strength` (evaluate() is run when it has
        not been; without folds and with more than one strength, name the strength)."""
        S = len(self.strengths)
        if strength is None:
            if S == 1:
                strength = self.strengths[0]
            elif self.best_strength_ is None and self.n_folds_ < 1:
                raise ValueError("LinearProbe: without folds there is no best strength (predict(emb, strength=...))")
            else:
                if self.best_strength_ is None:
                    self.evaluate()
                strength = self.best_strength_
        if isinstance(strength, bool) or not isinstance(strength, (int, float)) or float(strength) not in self.strengths:
            raise ValueError(f"strength must be one of {self.strengths}, got {strength!r}")
        return self.strengths.index(float(strength))

    def oof_proba(self, strength: Optional[float] = None) -> torch.Tensor:
        """f32 [n, C] on the device: every pool row's class probabilities under the job that held its fold out at `strength` (None: as
        predict), NaN for the rows that lie in no fold."""
        self._fitted()
        if self.n_folds_ < 1:
            raise ValueError("LinearProbe: oof_proba() needs folds (fit(emb, labels, fold=...))")
        S, s, C = len(self.strengths), self._strength_index(strength), self.num_classes
        out = torch.full((self._y.shape[0], C), math.nan, device=self.device, dtype=torch.float32)
        for f, rows in enumerate(self._fold_rows):
            j = f * S + s
            out.index_copy_(0, rows, K.linprobe_proba(self._y.index_select(0, rows), self._Wx[j:j + 1], self._bx[j:j + 1], C)[0][0])
        return out

    # ------------------------------------------------------------------ new rows
    def predict(self, emb: torch.Tensor, strength: Optional[float] = None) -> torch.Tensor:
        """int32 [n'] on the device: the classes of emb's rows, prepared with the pool's mean, under the all-rows job of `strength`
        (one of the constructor's) or, for None, of `linprobe_best_strength` (evaluate() is run when it has not been; without folds
        and with more than one strength, name the strength)."""
        j, q = self._all_rows_job(emb, strength)
        return K.fewshot_predict(q, self._Wx[j:j + 1], self._bx[j:j + 1], self.num_classes)[0]

    def predict_proba(self, emb: torch.Tensor, strength: Optional[float] = None) -> torch.Tensor:
        """f32 [n', C] on the device: the class probabilities of emb's rows under the same job and the same preparation as `predict`
        (mh_linprobe_proba).  Its argmax is `predict`'s class wherever the two largest probabilities differ; where they are equal,
        `predict` answers the smaller class."""
        j, q = self._all_rows_job(emb, strength)
        return K.linprobe_proba(q, self._Wx[j:j + 1], self._bx[j:j + 1], self.num_classes)[0][0]

    def _all_rows_job(self, emb: torch.Tensor, strength: Optional[float]):
        """(the all-rows job of `strength`, emb's rows prepared with the pool's mean)."""
        self._fitted()
        self._rows(emb, "emb", self._Wx.shape[2])
        j = self.n_folds_ * len(self.strengths) + self._strength_index(strength)
        return j, self._prepare(emb.detach().to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous())
