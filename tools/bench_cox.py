"""Time the Cox partial-likelihood loss, forward + backward: this build (A) against the same definition (Efron ties, "mean") written
with torch ops on the same device (B), whose risk-set and tie matrices are N x N f32 temporaries.

GPU only (fails without a device), one process.  Per N: warm-up of both, then `--rounds` alternations A, B, A, B, ... in the same
call, each round the mean of `--iters` forward + backward passes between two device events.  Prints the median and the min..max
spread of the rounds in microseconds and the bytes of ONE N x N f32 temporary of the torch form (it makes several per pass).

    python tools/bench_cox.py [--rounds 5] [--iters 5] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mirror_amd.losses import CoxSurvLoss  # noqa: E402

NS = (1024, 8192)


def torch_loss(r, t, c):
    """Efron partial likelihood, "mean", in f32 torch ops: the max-shifted form of `exp(theta) * R_mat` with the tie terms."""
    e = (c == 1).float()
    w = torch.exp(r - r.max().detach())
    ge = (t[None, :] >= t[:, None]).float()                 # [i, j]
    eqe = (t[None, :] == t[:, None]).float() * e[None, :]
    S = ge @ w
    D = eqe @ w
    d = eqe.sum(1)
    l = torch.tril(eqe, -1).sum(1)
    den = S - e * l / d.clamp(min=1.0) * D
    rows = e * (torch.log(den) + r.max().detach() - r)
    return rows.sum() / e.sum().clamp(min=1.0)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def stats(xs):
    xs = sorted(xs)
    return {"median_us": xs[len(xs) // 2], "min_us": xs[0], "max_us": xs[-1]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cox.py needs a GPU")
    crit = CoxSurvLoss(ties="efron", reduction="mean")
    results = []
    for N in NS:
        g = torch.Generator(device="cuda").manual_seed(N)
        r = torch.randn(N, device="cuda", generator=g, requires_grad=True)
        t = torch.randint(0, max(N // 4, 1), (N,), device="cuda", generator=g).double()
        c = (torch.rand(N, device="cuda", generator=g) < 0.7).long()
        t32 = t.float()

        def both_a():
            r.grad = None
            crit(r, t, c).backward()

        def both_b():
            r.grad = None
            torch_loss(r, t32, c).backward()

        la, lb = float(crit(r, t, c).detach()), float(torch_loss(r, t32, c).detach())
        for f in (both_a, both_b, both_a, both_b):
            f()                                           # warm-up, both sides
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(both_a, args.iters))
            tb.append(timed(both_b, args.iters))
        a, b = stats(ta), stats(tb)
        rec = {"N": N, "loss_build": la, "loss_torch": lb, "fwd_bwd": {"build": a, "torch": b}, "nxn_f32_bytes": 4 * N * N}
        print(f"cox efron mean N={N:<5d} fwd+bwd  build {a['median_us']:9.1f} us [{a['min_us']:.1f}..{a['max_us']:.1f}]  torch "
              f"{b['median_us']:9.1f} us [{b['min_us']:.1f}..{b['max_us']:.1f}]  one N x N f32 temporary {4 * N * N / 2**20:6.1f} MiB  "
              f"loss {la:.6f} / {lb:.6f}", flush=True)
        results.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
