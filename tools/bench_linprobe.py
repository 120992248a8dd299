"""Time the linear probe's FISTA iteration: this build (A: mh_linprobe_grad + mh_linprobe_step, two launches) against the same iteration
written with torch ops on the same device (B: one matmul for every job's logits, log_softmax, one matmul for every weight gradient,
elementwise updates).

GPU only (fails without a device), one process.  n = 1024 rows, D = 512, C = 4 classes, F = 5 folds, S = 8 strengths (J = 48 jobs,
J Cp = 192 keys), `--iters` = 200 iterations per timed window.  Warm-up of both, then `--rounds` alternations A, B, A, B, ... in the same
call, each round one window of `--iters` iterations from the same start between two device events.  Prints the median and the min..max
spread of the rounds in microseconds per iteration, the bytes one iteration of A moves from the shapes, and how far the two final
iterates lie apart (they sum in different orders).

    python tools/bench_linprobe.py [--rounds 5] [--iters 200] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mirror_amd import kernels as K  # noqa: E402
from mirror_amd.linprobe import fista_betas  # noqa: E402

N, D, C, F, S = 1024, 512, 4, 5, 8


def stats(xs):
    xs = sorted(xs)
    return {"median_us": xs[len(xs) // 2], "min_us": xs[0], "max_us": xs[-1]}


def bytes_per_iteration(n, D, J, C, Cp):
    """What one iteration of A reads and writes, from the shapes (tiles re-read their operands; L2 may serve the repeats)."""
    nk = J * Cp
    rt, kt, ct = math.ceil(n / 128), math.ceil(nk / 128), math.ceil((D + 1) / 128)
    grad = 4 * (kt * n * D + rt * nk * D + n * nk)                  # y per key tile, Wz per row tile, G written
    step = 4 * (ct * n * nk + kt * n * D + 4 * J * C * (D + 1))     # G per column tile, y per key tile, X and Z read and written
    return grad, step


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linprobe.py needs a GPU")
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(N + D)
    Cp = K.fewshot_cp(C)
    J = (F + 1) * S
    labels = torch.randint(0, C, (N,), device=dev, generator=g)
    cent = 0.5 * torch.randn(C, D, device=dev, generator=g)
    x = cent[labels] + torch.randn(N, D, device=dev, generator=g)
    y = K.center_l2norm(x, K.colmean(x))
    fold = torch.randint(0, F, (N,), device=dev, generator=g).to(torch.int32)
    heldout = torch.tensor([f for f in range(F) for _ in range(S)] + [-1] * S, dtype=torch.int32, device=dev)
    lam = torch.logspace(-5, -1, S, device=dev).repeat(F + 1).float()
    mask = fold[:, None] != heldout[None, :]                                      # [n, J]
    rscale = (1.0 / mask.sum(0)).float()
    eta = (1.0 / (0.5 * (1.0 + (y * y).sum(1).max()) + lam)).float()
    betas = fista_betas(args.iters)

    # ---- A: the build
    G = torch.empty((N, J * Cp), device=dev)
    pad_b = torch.zeros((J, Cp), device=dev)
    pad_b[:, C:] = -math.inf
    sa = [torch.zeros((J, Cp, D), device=dev), pad_b.clone(), torch.zeros((J, Cp, D), device=dev), pad_b.clone()]

    def run_a():
        sa[0].zero_(), sa[2].zero_(), sa[1].copy_(pad_b), sa[3].copy_(pad_b)
        for beta in betas:
            K.linprobe_grad(y, sa[2], sa[3], labels, fold, heldout, rscale, C, G=G)
            K.linprobe_step(y, G, sa[0], sa[1], sa[2], sa[3], lam, eta, beta, C)

    # ---- B: the same iteration in torch ops (no pads: [J, C, D] weights as one [J C, D] matrix)
    sb = [torch.zeros((J * C, D), device=dev), torch.zeros((J, C), device=dev), torch.zeros((J * C, D), device=dev),
          torch.zeros((J, C), device=dev)]
    onehot = torch.nn.functional.one_hot(labels, C).float()[:, None, :]           # [n, 1, C]
    scale = (mask.float() * rscale[None, :])[:, :, None]                          # [n, J, 1]
    lam_k, eta_k = lam.repeat_interleave(C)[:, None], eta.repeat_interleave(C)[:, None]

    def run_b():
        for t in sb:
            t.zero_()
        Wx, bx, Wz, bz = sb
        for beta in betas:
            v = (y @ Wz.t()).view(N, J, C) + bz
            Gt = (torch.softmax(v, dim=2) - onehot) * scale
            dW = torch.addmm(lam_k * Wz, Gt.view(N, J * C).t(), y)
            db = Gt.sum(0)
            Xn, bn = Wz - eta_k * dW, bz - eta[:, None] * db
            Wz.copy_(Xn + beta * (Xn - Wx))
            bz.copy_(bn + beta * (bn - bx))
            Wx.copy_(Xn)
            bx.copy_(bn)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters

    for f in (run_a, run_b, run_a, run_b):
        f()                                                                       # warm-up, both sides
    torch.cuda.synchronize()
    diff = float((sa[0][:, :C, :].reshape(J * C, D) - sb[0]).abs().max())
    size = float(sb[0].abs().max())
    ta, tb = [], []
    for _ in range(args.rounds):
        ta.append(timed(run_a))
        tb.append(timed(run_b))
    a, b = stats(ta), stats(tb)
    gb, sbytes = bytes_per_iteration(N, D, J, C, Cp)
    rec = {"n": N, "D": D, "C": C, "folds": F, "strengths": S, "jobs": J, "iters": args.iters, "rounds": args.rounds, "build": a, "torch": b,
           "bytes_grad": gb, "bytes_step": sbytes, "max_abs_diff_Wx": diff, "max_abs_Wx": size}
    print(f"n={N} D={D} C={C} J={J} ({F} folds + 1) x {S} strengths, {args.iters} iterations per window, {args.rounds} alternations")
    print(f"build {a['median_us']:8.1f} us / iteration [{a['min_us']:.1f}..{a['max_us']:.1f}]   "
          f"torch {b['median_us']:8.1f} us / iteration [{b['min_us']:.1f}..{b['max_us']:.1f}]")
    print(f"bytes per iteration of the build: grad {gb / 2**20:.2f} MiB, step {sbytes / 2**20:.2f} MiB;  "
          f"final iterates differ by {diff:.2e} at |W| <= {size:.2e}")
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
