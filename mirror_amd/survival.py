"""Survival validation metrics of train_survival.py on HIP kernels: the risk score of :1431-1433 and the censored concordance
index of :1460-1465 (`sksurv.metrics.concordance_index_censored`, restated from its documented definition; sksurv is not a
dependency), and the two-group log-rank test of a high / low risk split that sits beside it in a results table.  All take
device tensors."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import kernels as K

__all__ = ["concordance_index_censored", "logrank_by_median", "logrank_test", "risk_scores", "survival_bins"]


def survival_bins(time, event, num_bins: int = 4, eps: float = 1e-6):
    """(bins int64 [n], edges f64 [num_bins + 1]) as CPU tensors: the discrete time bins of `datasets/dataset_survival.py:_gen_disc_label`,
    restated in f64 on the host (numpy; pandas is not a dependency).  The cohort is binned once, as the reference bins it.

    With at least one event (`event == 1`): the edges are the linear-interpolation quantiles of the EVENT times at k / num_bins
    (`pd.qcut`), the first then overwritten by min(time) - eps and the last by max(time) + eps over ALL rows.  With no event: num_bins
    equal-width bins over [min, max] with the last edge moved up by 0.1 % of the range (min == max: 0.1 % of |min| to either side, 0.001
    at 0), as `pd.cut(bins=num_bins, right=False)` forms them.  Either way bin = searchsorted(edges, time, side="right") - 1: the bins
    are closed on the left.  Raises ValueError where the edges are not strictly increasing (where `pd.qcut` refuses duplicate edges),
    for an empty or non-finite `time`, and for num_bins < 1."""
    if isinstance(num_bins, bool) or not isinstance(num_bins, int) or num_bins < 1:
        raise ValueError(f"num_bins must be a positive int, got {num_bins!r}")
    t = np.asarray(time.detach().cpu() if isinstance(time, torch.Tensor) else time, dtype=np.float64).reshape(-1)
    e = np.asarray(event.detach().cpu() if isinstance(event, torch.Tensor) else event).reshape(-1)
    if t.size == 0 or e.size != t.size:
        raise ValueError(f"time and event must be non-empty and of one length, got {t.size} and {e.size}")
    if not np.isfinite(t).all():
        raise ValueError("survival_bins: time must be finite")
    te = t[e == 1]
    if te.size:
        edges = np.quantile(te, np.linspace(0.0, 1.0, num_bins + 1))
        if not (np.diff(edges) > 0).all():
            raise ValueError(f"Bin edges must be unique: the event-time quantiles are {edges.tolist()}")
        edges[-1] = t.max() + eps
        edges[0] = t.min() - eps
    else:
        mn, mx = float(t.min()), float(t.max())
        if mn == mx:
            mn -= 0.001 * abs(mn) if mn != 0 else 0.001
            mx += 0.001 * abs(mx) if mx != 0 else 0.001
            edges = np.linspace(mn, mx, num_bins + 1)
        else:
            edges = np.linspace(mn, mx, num_bins + 1)
            edges[-1] += (mx - mn) * 0.001
    if not (np.diff(edges) > 0).all():
        raise ValueError(f"Bin edges must increase strictly, got {edges.tolist()}")
    bins = np.searchsorted(edges, t, side="right") - 1
    return torch.from_numpy(bins.astype(np.int64)), torch.from_numpy(edges)


def risk_scores(logits: torch.Tensor) -> torch.Tensor:
    """-sum(cumprod(1 - sigmoid(logits), dim=1), dim=1) of f32 logits [N, M] as f32 [N] (train_survival.py:1431-1433)."""
    return K.surv_risk(logits)


def concordance_index_censored(event_indicator: torch.Tensor, event_time: torch.Tensor, estimate: torch.Tensor, tied_tol: float = 1e-8):
    """Harrell's concordance index for right-censored data, sksurv's 5-tuple (cindex, concordant, discordant, tied_risk, tied_time).

    Pair (i, j) is comparable when sample i has an event and j outlives it (time[j] > time[i], or the same time with j censored);
    it is tied when |estimate[j] - estimate[i]| <= tied_tol (in f32), concordant when not tied and estimate[i] > estimate[j],
    discordant otherwise.  cindex = (concordant + 0.5 * tied_risk) / comparable.  The counts are computed on the device (one
    launch, integer atomics) and read back with one sync; `event_time` is converted to f64 and `estimate` to f32 on the device.
    Raises ValueError when every sample is censored or when no pair is comparable (where sksurv raises, and also where it would
    return 0 / 0)."""
    n = event_indicator.numel()
    if event_time.numel() != n or estimate.numel() != n:
        raise ValueError(f"event_indicator, event_time and estimate differ in length: {n}, {event_time.numel()}, {estimate.numel()}")
    if n == 0:
        raise ValueError("concordance_index_censored: empty input")
    if estimate.is_complex() or not (estimate.is_floating_point() or estimate.dtype in (torch.int32, torch.int64)):
        raise ValueError(f"estimate must be real-valued, got {estimate.dtype}")
    K._chk(event_indicator, event_time, estimate)
    ev = event_indicator.reshape(-1)
    ev = (ev if ev.dtype == torch.bool else ev != 0).contiguous().view(torch.uint8)
    counts = K.cindex_counts(ev, event_time.reshape(-1).to(torch.float64).contiguous(),
                             estimate.reshape(-1).to(torch.float32).contiguous(), tied_tol)
    con, dis, tie, ttime, comp = (np.int64(v) for v in counts.cpu().numpy())
    if comp == 0:
        if not bool(ev.any()):
            raise ValueError("All samples are censored")
        raise ValueError("Data has no comparable pairs, cannot estimate concordance index.")
    cindex = np.float64((con + 0.5 * tie) / comp)
    return cindex, con, dis, tie, ttime


def logrank_test(event_indicator: torch.Tensor, event_time: torch.Tensor, group: torch.Tensor):
    """Two-group log-rank test: (chi2, p, observed1, expected1, variance) as Python floats.

    For every distinct event time tau: n = #{t_j >= tau}, n1 the same within group 1 (`group != 0`), d = #{t_j == tau, event_j},
    d1.  observed1 = sum d1, expected1 = sum d n1 / n, variance = sum n1 (n - n1) d (n - d) / (n^2 (n - 1)) over n > 1,
    chi2 = (observed1 - expected1)^2 / variance and p = erfc(sqrt(chi2 / 2)), the survival function of chi-square with one degree
    of freedom.  The sums are one launch on the device (integer counts, f64 terms in a fixed order), read back with one sync;
    `event_time` is converted to f64 on the device and samples with a NaN time are ignored.  Raises ValueError when the variance
    is 0: no events, or one group empty at every event time.  At most 65536 samples."""
    n = event_indicator.numel()
    if event_time.numel() != n or group.numel() != n:
        raise ValueError(f"event_indicator, event_time and group differ in length: {n}, {event_time.numel()}, {group.numel()}")
    if n == 0:
        raise ValueError("logrank_test: empty input")
    K._chk(event_indicator, event_time, group)

    def as_u8(x):
        x = x.reshape(-1)
        return (x if x.dtype == torch.bool else x != 0).contiguous().view(torch.uint8)

    stats = K.logrank_stats(as_u8(event_indicator), event_time.reshape(-1).to(torch.float64).contiguous(), as_u8(group))
    o1, e1, var, n_events = (float(v) for v in stats.cpu().numpy())
    if n_events == 0:
        raise ValueError("All samples are censored")
    if not var > 0.0:
        raise ValueError("log-rank variance is 0: one group is empty at every event time")
    chi2 = (o1 - e1) ** 2 / var
    return chi2, math.erfc(math.sqrt(chi2 / 2.0)), o1, e1, var


def logrank_by_median(event_indicator: torch.Tensor, event_time: torch.Tensor, risk: torch.Tensor):
    """logrank_test of the split `risk > median(risk)` (torch.median: the lower of the two middle values for an even count)."""
    risk = risk.reshape(-1)
    return logrank_test(event_indicator, event_time, risk > risk.median())
