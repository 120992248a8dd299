"""The scores of the linear probe (mh_linprobe_proba, mh_auroc_counts_many, LinearProbe.evaluate(auroc=True)) restated in float64 numpy
from the header text.  Shared by tests/test_linprobe_scores_{cpu,gpu}.py; the fit itself is tests/linprobe_ref.py's.

    p[i, c]   = exp(v_c - lse_i),  v = W y_i + b,  lse = m + log(sum_c exp(v_c - m))
    counts[c] = {U2, P, Q, NaN}: positives are the rows with label c, negatives ALL others (labels outside [0, C) included),
                U2 = 2 #{(i pos, j neg): s_i > s_j} + #{s_i == s_j}; a NaN score takes part in no pair and is counted in NaN
    AUROC_c   = U2 / (2 P Q); NaN when P Q = 0 (left out of an average) or when column c holds a NaN (kept: the average is NaN)
    nll       = mean over the rows with a label in [0, C) of lse - v_label
"""
import numpy as np

from tests import linprobe_ref as R


def proba(W, b, y):
    """float64 [n, C]: softmax(W y_i + b)."""
    with np.errstate(invalid="ignore"):
        return np.exp(R.log_softmax(np.asarray(y, dtype=np.float64) @ W.T + b))


def row_nll(W, b, y, labels):
    """(lse - v_label float64 [n], 0 for the rows whose label lies outside [0, C); the mask of the counted rows)."""
    labels = np.asarray(labels)
    C = W.shape[0]
    ok = (labels >= 0) & (labels < C)
    out = np.zeros(len(labels))
    idx = np.flatnonzero(ok)
    out[idx] = -R.log_softmax(np.asarray(y, dtype=np.float64)[idx] @ W.T + b)[np.arange(len(idx)), labels[idx]]
    return out, ok


def pair_counts_naive(scores, labels):
    """int64 [C, 4] by the definition, every pair looked at: for small N."""
    scores, labels = np.asarray(scores), np.asarray(labels)
    N, C = scores.shape
    out = np.zeros((C, 4), dtype=np.int64)
    for c in range(C):
        for i in range(N):
            out[c, 1] += labels[i] == c
            out[c, 2] += labels[i] != c
            out[c, 3] += np.isnan(scores[i, c])
            if labels[i] != c:
                continue
            for j in range(N):
                if labels[j] != c:                       # a comparison with a NaN is false both times
                    out[c, 0] += int(scores[i, c] > scores[j, c]) + int(scores[i, c] >= scores[j, c])
    return out


def pair_counts(scores, labels):
    """int64 [C, 4], the same integers through a sort of the negatives: #{neg < s} + #{neg <= s} per positive s."""
    scores, labels = np.asarray(scores), np.asarray(labels)
    N, C = scores.shape
    out = np.zeros((C, 4), dtype=np.int64)
    for c in range(C):
        s = scores[:, c]
        pos = labels == c
        nan = np.isnan(s)
        neg = np.sort(s[~pos & ~nan])
        sp = s[pos & ~nan]
        u2 = np.searchsorted(neg, sp, side="left").sum() + np.searchsorted(neg, sp, side="right").sum()
        out[c] = (u2, pos.sum(), N - pos.sum(), nan.sum())
    return out


def auroc(counts):
    """float64 [.., C] from int64 [.., C, 4]."""
    counts = np.asarray(counts)
    pq = counts[..., 1].astype(np.float64) * counts[..., 2].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = counts[..., 0].astype(np.float64) / (2.0 * pq)
    return np.where(counts[..., 3] > 0, np.nan, a)


def averaged(auc, counts, average):
    """float64 [..]: "macro" the mean over the classes with P Q > 0, "weighted" with weights P over the same classes; NaN when none."""
    counts = np.asarray(counts)
    use = (counts[..., 1] * counts[..., 2]) > 0
    w = use.astype(np.float64) if average == "macro" else np.where(use, counts[..., 1], 0).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.where(use, auc, 0.0) * w).sum(-1) / w.sum(-1)


def auc_interval(p, labels, c, margin):
    """(lo, hi, share): the AUROC of class c when every (positive, negative) pair whose float64 scores p lie at least `margin` apart is
    ranked as float64 ranks it and every other pair is counted against (lo) or for (hi) the positive; share = those pairs / all."""
    p, labels = np.asarray(p, dtype=np.float64), np.asarray(labels)
    d = p[labels == c][:, None] - p[labels != c][None, :]
    und = int((np.abs(d) < margin).sum())
    won = int((d >= margin).sum())
    return won / d.size, (won + und) / d.size, und / d.size


# the end-to-end case of tests/test_linprobe_scores_gpu.py: classes that overlap (tests/linprobe_ref.py's E2E is separable: AUROC 1)
E2E = dict(n=300, D=24, C=3, F=3, strengths=(1e-4, 1e-1), steps=300, sep=1.0, seed=43)


def e2e_case():
    """(x f32 [n, D], labels int64 [n], fold int64 [n]): every row in a fold, every label valid."""
    c = E2E
    x, labels = R.blobs(c["n"], c["D"], c["C"], c["sep"], c["seed"])
    fold = np.random.default_rng(c["seed"] + 1).integers(0, c["F"], c["n"]).astype(np.int64)
    return x, labels, fold


_cache = {}


def e2e_reference():
    """(y float64 [n, D], P float64 [F, S, n, C]: under job f S + s, the float64 iterate after E2E["steps"] steps; only the rows of fold f
    are held out there).  Computed once per process."""
    if "ref" not in _cache:
        c = E2E
        x, labels, fold = e2e_case()
        y, _ = R.prepare(x, x)
        held, lam = R.jobs(c["F"], c["strengths"])
        S = len(c["strengths"])
        P = np.zeros((c["F"], S, c["n"], c["C"]))
        for j in range(c["F"] * S):
            W, b = R.fista(y, labels, R.train_mask(labels, fold, held[j], c["C"]), lam[j], c["C"], c["steps"])
            P[j // S, j % S] = proba(W, b, y)
        P.setflags(write=False)
        _cache["ref"] = (y, P)
    return _cache["ref"]
