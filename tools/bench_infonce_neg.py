"""Time InfoNCE with explicit negative keys: this build (A) against the same definition written with torch ops on the same device (B).

GPU only (fails without a device), one process.  Per shape: warm-up of both, then `--rounds` alternations A, B, A, B, ... in the same
call, each round the mean of `--iters` forward (+ backward) passes between two device events.  Prints the median and the min..max
spread of the rounds in microseconds, the compulsory bytes of the negatives from the shapes (paired forward N M D s, backward
2 N M D s with a gradient for them, N M D s without; unpaired: M D s per pass over the bank) and the GB/s they amount to at A's time.

    python tools/bench_infonce_neg.py [--rounds 5] [--iters 5] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mirror_amd.losses import InfoNCE  # noqa: E402

HBM_ACHIEVABLE = 6.3e12      # bytes / s

CASES = [
    # mode, N, M, D, dtype, negatives require grad
    ("paired", 256, 1024, 512, torch.float32, True),
    ("paired", 256, 1024, 512, torch.float32, False),
    ("paired", 16, 4096, 768, torch.float32, True),
    ("paired", 16, 4096, 768, torch.float32, False),
    ("unpaired", 256, 65536, 512, torch.float32, True),
    ("unpaired", 256, 65536, 512, torch.float32, False),
    ("unpaired", 256, 65536, 512, torch.bfloat16, True),
    ("unpaired", 256, 65536, 512, torch.bfloat16, False),
]


def torch_loss(q, k, n, temperature, mode):
    """The reference's formulation (losses/info_nce.py:122-143) plus the cross-entropy it forgets, in torch ops."""
    q, k, n = F.normalize(q, dim=-1), F.normalize(k, dim=-1), F.normalize(n.float(), dim=-1)
    pos = torch.sum(q * k, dim=1, keepdim=True)
    if mode == "unpaired":
        neg = q @ n.transpose(-2, -1)
    else:
        neg = (q.unsqueeze(1) @ n.transpose(-2, -1)).squeeze(1)
    logits = torch.cat([pos, neg], dim=1)
    labels = torch.zeros(len(logits), dtype=torch.long, device=q.device)
    return F.cross_entropy(logits / temperature, labels)


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
        raise SystemExit("bench_infonce_neg.py needs a GPU")
    crit = {m: InfoNCE(temperature=0.07, negative_mode=m) for m in ("paired", "unpaired")}
    results = []
    for mode, N, M, D, dtype, ngrad in CASES:
        g = torch.Generator(device="cuda").manual_seed(N + M)
        q = torch.randn(N, D, device="cuda", generator=g, requires_grad=True)
        k = torch.randn(N, D, device="cuda", generator=g, requires_grad=True)
        n = torch.randn(*((M, D) if mode == "unpaired" else (N, M, D)), device="cuda", generator=g).to(dtype).requires_grad_(ngrad)

        def fwd_a():
            with torch.no_grad():
                crit[mode](q, k, n)

        def fwd_b():
            with torch.no_grad():
                torch_loss(q, k, n, 0.07, mode)

        def both_a():
            q.grad = k.grad = n.grad = None
            crit[mode](q, k, n).backward()

        def both_b():
            q.grad = k.grad = n.grad = None
            torch_loss(q, k, n, 0.07, mode).backward()

        la, lb = float(crit[mode](q, k, n)), float(torch_loss(q, k, n, 0.07, mode))
        rec = {"mode": mode, "N": N, "M": M, "D": D, "dtype": str(dtype).replace("torch.", ""), "negatives_grad": ngrad,
               "loss_build": la, "loss_torch": lb}
        nbytes = n.numel() * n.element_size()
        passes = {"fwd": 1, "fwd_bwd": 1 + (2 if ngrad else 1) if mode == "paired" else 1 + (2 if ngrad else 0)}
        for what, fa, fb in (("fwd", fwd_a, fwd_b), ("fwd_bwd", both_a, both_b)):
            for f in (fa, fb, fa, fb):
                f()                                           # warm-up, both sides
            torch.cuda.synchronize()
            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(timed(fa, args.iters))
                tb.append(timed(fb, args.iters))
            a, b = stats(ta), stats(tb)
            comp = passes[what] * nbytes
            gbs = comp / (a["median_us"] * 1e-6) / 1e9
            rec[what] = {"build": a, "torch": b, "compulsory_bytes": comp, "build_GBps": gbs, "hbm_share": gbs * 1e9 / HBM_ACHIEVABLE}
            print(f"{mode:8s} N={N:<4d} M={M:<6d} D={D:<4d} {rec['dtype']:8s} neg.grad={int(ngrad)} {what:7s} "
                  f"build {a['median_us']:9.1f} us [{a['min_us']:.1f}..{a['max_us']:.1f}]  torch {b['median_us']:9.1f} us "
                  f"[{b['min_us']:.1f}..{b['max_us']:.1f}]  {comp / 2**20:7.1f} MiB  {gbs:7.1f} GB/s  {100 * rec[what]['hbm_share']:5.1f} % of HBM",
                  flush=True)
        results.append(rec)
        del q, k, n
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
