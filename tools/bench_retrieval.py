"""Time the retrieval ranks: this build's fused kernel (A, `retrieval.retrieval_ranks`) against the same definition composed from
torch ops on the same device (B: `S = q @ k.T`, compare with the diagonal, count), which materialises the [n, n] f32 matrix.

GPU only (fails without a device), one process.  Per shape: the two results are compared, both are warmed up, then `--rounds`
alternations A, B, A, B, ... in the same call, each round the mean of `--iters` calls between two device events.  Prints the median
and the min..max spread of the rounds in microseconds, the f32-MFMA share of A (2 n^2 D flops against the f32 matrix peak, 1/16 of
the bf16 peak) and the peak device memory either form allocates on top of its inputs (torch.cuda.max_memory_allocated).

    python tools/bench_retrieval.py [--rounds 5] [--iters 5] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mirror_amd.retrieval import retrieval_ranks  # noqa: E402

F32_MFMA_PEAK = 2516.6e12 / 16      # flop / s: v_mfma_f32_32x32x2_f32 runs at 1/16 of the bf16 MFMA peak

CASES = [(2048, 512), (8192, 512), (16384, 512), (8192, 768)]      # n, D


def torch_ranks(q, k):
    """ranks[i] = 1 + #{j != i: not (S[i, j] < S[i, i])}: the diagonal itself is the 1 (a NaN-free positive never beats itself)."""
    S = q @ k.T
    return (~(S < S.diagonal().unsqueeze(1))).sum(1, dtype=torch.int32)


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


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_retrieval.py needs a GPU")
    results = []
    for n, D in CASES:
        g = torch.Generator(device="cuda").manual_seed(n + D)
        q = torch.randn(n, D, device="cuda", generator=g)
        k = 0.1 * q + torch.randn(n, D, device="cuda", generator=g)

        def fa():
            return retrieval_ranks(q, k)

        def fb():
            return torch_ranks(q, k)

        ra, rb = fa(), fb()
        differ = int((ra != rb).sum())        # torch's product sums in another order: near-ties may land on either side
        mem_a, mem_b = peak_bytes(fa), peak_bytes(fb)
        for f in (fa, fb, fa, fb):
            f()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(fa, args.iters))
            tb.append(timed(fb, args.iters))
        a, b = stats(ta), stats(tb)
        flops = 2.0 * n * n * D
        share = flops / (a["median_us"] * 1e-6) / F32_MFMA_PEAK
        results.append({"n": n, "D": D, "build": a, "torch": b, "flops": flops, "build_f32_mfma_share": share,
                        "build_peak_bytes": mem_a, "torch_peak_bytes": mem_b, "ranks_differing": differ,
                        "mean_rank": float(ra.float().mean())})
        print(f"n={n:<6d} D={D:<4d} build {a['median_us']:9.1f} us [{a['min_us']:.1f}..{a['max_us']:.1f}]  torch {b['median_us']:9.1f} us "
              f"[{b['min_us']:.1f}..{b['max_us']:.1f}]  {flops / (a['median_us'] * 1e-6) / 1e12:6.1f} TF = {100 * share:5.1f} % of f32 MFMA  "
              f"peak memory build {mem_a / 2**20:8.2f} MiB, torch {mem_b / 2**20:8.2f} MiB  ranks differing {differ}", flush=True)
        del q, k, ra, rb
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
