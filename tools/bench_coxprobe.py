"""Time the ridge Cox probe: this build (A: mh_coxprobe_scores + mh_coxprobe_grad + mh_coxprobe_step, three launches per iteration for
all J jobs) against what the repository offered before (B: one job at a time, `CoxSurvLoss` under autograd on a torch product,
full-batch gradient steps with the same step size, a host loop over the jobs).

GPU only (fails without a device), one process.  n = 1000 rows, D = 512, F = 5 folds, S = 8 strengths (J = 48 jobs), Efron ties.  Two
figures, each the median with the min..max spread of `--rounds` alternations A, B, A, B, ... in the same call, every window between two
device events:

  * one iteration: A's three launches for the 48 jobs, in a window of `--iters` iterations; B's forward, backward and update for the
    48 jobs in turn, in a window of `--iters-b` sweeps (B is a plain gradient step: its iterates are not A's, only its work per
    iteration is comparable);
  * a whole fit: `CoxProbe.fit` with max_iter = `--iters`, tol = 0 (the sort, the preparation, one host wait per 16 iterations) against
    B's `--iters` sweeps scaled from the window above.

Prints the launches per iteration of A (counted, not assumed) and one JSON line.

    python tools/bench_coxprobe.py [--rounds 5] [--iters 200] [--iters-b 4] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mirror_amd import CoxProbe, _lib, kernels as K  # noqa: E402
from mirror_amd.linprobe import fista_betas  # noqa: E402
from mirror_amd.losses import CoxSurvLoss  # noqa: E402

N, D, F, S = 1000, 512, 5, 8


def stats(xs):
    xs = sorted(xs)
    return {"median_us": xs[len(xs) // 2], "min_us": xs[0], "max_us": xs[-1]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--iters-b", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_coxprobe.py needs a GPU")
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(N + D)
    J = (F + 1) * S
    x = torch.randn(N, D, device=dev, generator=g) + 0.5 * torch.randn(D, device=dev, generator=g)
    beta_true = torch.randn(D, device=dev, generator=g) / D ** 0.5
    t_event = torch.empty(N, device=dev).exponential_(1.0, generator=g) * torch.exp(-1.5 * (x @ beta_true))
    t_cens = torch.empty(N, device=dev).exponential_(1.0, generator=g) * float(t_event.median()) * 2.0
    event = (t_event <= t_cens).to(torch.uint8)
    time = torch.round(torch.minimum(t_event, t_cens).double() * 20.0) / 20.0                  # ties, as months of follow-up give
    fold = torch.randint(0, F, (N,), device=dev, generator=g).to(torch.int32)
    strengths = tuple(float(v) for v in torch.logspace(-5, -1, S))

    # ---- the rows as fit() leaves them: prepared, sorted by time descending
    y0 = K.center_l2norm(x, K.colmean(x))
    perm = torch.sort(time, descending=True, stable=True).indices
    y, tm, ev, fd = y0[perm].contiguous(), time[perm].contiguous(), event[perm].contiguous(), fold[perm].contiguous()
    heldout = torch.tensor([f for f in range(F) for _ in range(S)] + [-1] * S, dtype=torch.int32, device=dev)
    lam = torch.tensor(list(strengths) * (F + 1), dtype=torch.float32, device=dev)
    member = fd[None, :] != heldout[:, None]                                                   # [J, n]
    ntrain = member.sum(1)
    rscale = (1.0 / ntrain).float()
    eps = (member & (ev == 1)[None, :]).sum(1).float() / ntrain.float()
    eta = (1.0 / ((y * y).sum(1).max() * eps + lam)).float()
    betas = fista_betas(args.iters)

    # ---- A: the build
    Wx, Wz = torch.zeros((J, D), device=dev), torch.zeros((J, D), device=dev)
    V, G = torch.empty((J, N), device=dev), torch.empty((N, J), device=dev)
    part = torch.empty((J,), device=dev, dtype=torch.float64)
    ws = K.coxprobe_workspace(N, J, dev)
    launches = []
    real_call = _lib.call

    def counting_call(name, *a, **kw):
        launches.append(name)
        return real_call(name, *a, **kw)

    def iteration(beta):
        K.coxprobe_scores(y, Wz, V=V)
        K.coxprobe_grad(V, tm, ev, fd, heldout, rscale, "efron", G=G, loss=part, workspace=ws)
        K.coxprobe_step(y, G, Wx, Wz, lam, eta, beta)

    _lib.call = K._lib.call = counting_call
    iteration(0.0)
    _lib.call = K._lib.call = real_call
    per_iteration = list(launches)

    def run_a():
        Wx.zero_(), Wz.zero_()
        for beta in betas:
            iteration(beta)

    def fit_a():
        CoxProbe(strengths=strengths, max_iter=args.iters, tol=0.0, device=dev).fit(x, event, time, fold)

    # ---- B: job by job, CoxSurvLoss under autograd on a torch product, a plain gradient step
    loss_fn = CoxSurvLoss(ties="efron", reduction="batch")
    rows = [torch.nonzero(member[j]).view(-1) for j in range(J)]
    yj = [y.index_select(0, r) for r in rows]
    tj = [tm.index_select(0, r) for r in rows]
    cj = [ev.index_select(0, r).long() for r in rows]
    Wb = [torch.zeros((D, 1), device=dev, requires_grad=True) for _ in range(J)]
    lam_h, eta_h = [float(v) for v in lam], [float(v) for v in eta]

    def run_b():
        for _ in range(args.iters_b):
            for j in range(J):
                w = Wb[j]
                loss = loss_fn(yj[j] @ w, tj[j], cj[j]) + 0.5 * lam_h[j] * (w * w).sum()
                (gw,) = torch.autograd.grad(loss, w)
                with torch.no_grad():
                    w.sub_(eta_h[j] * gw)

    def timed(fn, per):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / per

    for f in (run_a, run_b, fit_a, run_a, run_b, fit_a):
        f()                                                                                    # warm-up, every side
    torch.cuda.synchronize()
    ta, tb, tf = [], [], []
    for _ in range(args.rounds):
        ta.append(timed(run_a, args.iters))
        tb.append(timed(run_b, args.iters_b))
        tf.append(timed(fit_a, 1))
    a, b, f = stats(ta), stats(tb), stats(tf)
    rec = {"n": N, "D": D, "folds": F, "strengths": S, "jobs": J, "ties": "efron", "iters": args.iters, "iters_b": args.iters_b,
           "rounds": args.rounds, "launches_per_iteration": per_iteration, "build_iteration": a, "baseline_iteration": b,
           "build_fit": f, "baseline_fit_us_scaled": b["median_us"] * args.iters}
    print(f"n={N} D={D} J={J} ({F} folds + 1) x {S} strengths, Efron; {args.rounds} alternations")
    print(f"launches per iteration of the build: {len(per_iteration)} ({', '.join(per_iteration)})")
    print(f"one iteration, all {J} jobs: build {a['median_us']:9.1f} us [{a['min_us']:.1f}..{a['max_us']:.1f}]   "
          f"CoxSurvLoss job by job {b['median_us']:11.1f} us [{b['min_us']:.1f}..{b['max_us']:.1f}]")
    print(f"a fit of {args.iters} iterations: build {f['median_us'] / 1e3:9.2f} ms [{f['min_us'] / 1e3:.2f}..{f['max_us'] / 1e3:.2f}]   "
          f"job by job, scaled from its window: {b['median_us'] * args.iters / 1e3:.1f} ms")
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
