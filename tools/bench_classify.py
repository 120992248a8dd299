"""Time the subtyping step's kernels (csrc/classify.hip) on one GPU: the exact one-vs-rest AUROC pair count (mh_auroc_counts,
O(N^2 C)) at N in {10^3, 10^4, 10^5}, C = 4, and, for scale, the loss forward + backward and the confusion update at the same N.
Prints one JSON line per case (median of HIP-event-timed repeats after a warm-up).  Figures only: nothing is asserted.

    python tools/bench_classify.py [--ns 1000 10000 100000] [--classes 4] [--reps 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mirror_amd import kernels as K  # noqa: E402


def _time(fn, reps: int) -> float:
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ns", type=int, nargs="+", default=[1000, 10000, 100000])
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    C = args.classes
    g = torch.Generator(device="cuda").manual_seed(0)
    for N in args.ns:
        x = torch.randn(N, C, device="cuda", generator=g)
        y = torch.randint(0, C, (N,), device="cuda", generator=g)
        out = torch.empty(1, device="cuda")
        one = torch.ones((), device="cuda")
        conf = torch.zeros((C, C), dtype=torch.int64, device="cuda")
        bad = torch.zeros(1, dtype=torch.int64, device="cuda")
        rec = {"N": N, "C": C,
               "auroc_counts_us": _time(lambda: K.auroc_counts(x, y), args.reps),
               "ce_fwd_us": _time(lambda: K.cls_ce_fwd(x, y, 0.1, -100, K.CLS_RED["mean"], None, out), args.reps),
               "ce_bwd_us": _time(lambda: K.cls_ce_bwd(x, y, 0.1, -100, one, K.CLS_RED["mean"]), args.reps),
               "confusion_us": _time(lambda: K.cls_confusion(x, y, conf, bad), args.reps)}
        rec["auroc_pairs_per_s"] = N * N * C / (rec["auroc_counts_us"] * 1e-6)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
