"""Time the cluster probe at a cohort's size: `ClusterProbe.fit` as a whole (a host clock around the call, which ends in a device
synchronise: the read-backs of the change table are part of it), and each of its kernels alone on the fitted state between two device
events: `mh_kmeans_assign` (with the f32 flops 2 n R K D of its tile product), `mh_kmeans_update`, `mh_kmeans_inertia`,
`mh_kmeans_tally`.

GPU only (fails without a device), one process.  Warm-up of everything, then `--rounds` rounds in the same call; a round times
`--fits` fits in a row (some tenths of a second) and, per kernel, `--iters` launches between two events (the same).  Prints the median
and the min..max spread of the rounds in microseconds.  The kernel figures are event timings of back-to-back launches, not a kernel
trace: they include the launch gaps.

    python tools/bench_cluster.py [--rounds 5] [--fits 20] [--iters 1000] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mirror_amd import kernels as K  # noqa: E402
from mirror_amd.cluster import ClusterProbe  # noqa: E402

N, D, KK, R, CLASSES, NOISE = 8192, 512, 32, 16, 32, 4.0


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
    ap.add_argument("--fits", type=int, default=20)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cluster.py needs a GPU")
    g = torch.Generator(device="cuda").manual_seed(1)
    centres = torch.randn(CLASSES, D, device="cuda", generator=g)
    yl = torch.arange(N, device="cuda") % CLASSES
    pool = centres[yl] + NOISE * torch.randn(N, D, device="cuda", generator=g) + 3.0
    out = {"n": N, "D": D, "K": KK, "R": R, "rounds": args.rounds, "fits_per_round": args.fits, "launches_per_round": args.iters}
    for metric in ("cosine", "euclidean"):
        probe = ClusterProbe(KK, restarts=R, metric=metric, seed=1, device="cuda")

        def fit(times=1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(times):
                probe.fit(pool)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / times

        fit(2)                                                # warm-up
        y, cent, bias, assign = probe._y, probe.centroids_.clone(), None if probe.bias_ is None else probe.bias_.clone(), probe.assign_
        stages = {"assign": lambda: K.kmeans_assign(y, cent, bias, out=assign), "update": lambda: K.kmeans_update(y, assign, cent, bias, metric),
                  "inertia": lambda: K.kmeans_inertia(y, cent, assign), "tally": lambda: K.kmeans_tally(assign, yl, KK, CLASSES)}
        for f in stages.values():
            f()
        torch.cuda.synchronize()
        tf, ts = [], {k: [] for k in stages}
        for _ in range(args.rounds):
            tf.append(fit(args.fits))
            for k, f in stages.items():
                ts[k].append(timed(f, args.iters))
        sf, ss = stats(tf), {k: stats(v) for k, v in ts.items()}
        steps = int(probe.changed_.shape[0])
        flops = 2.0 * N * R * KK * D
        scores = probe.evaluate(yl, CLASSES)
        rec = {"metric": metric, "fit": sf, "steps_run": steps, "n_iter": probe.n_iter_.tolist(), "stages_alone": ss, "assign_flops": flops,
               "assign_tflops": flops / (ss["assign"]["median_us"] * 1e-6) / 1e12, "nmi": scores["cluster_nmi"], "ari": scores["cluster_ari"]}
        out[metric] = rec
        print(f"{metric:9s} n={N} D={D} K={KK} R={R}: fit {sf['median_us']:9.1f} us [{sf['min_us']:.1f}..{sf['max_us']:.1f}] over {steps} steps "
              f"(n_iter {min(rec['n_iter'])}..{max(rec['n_iter'])});  alone: " +
              ", ".join(f"{k} {v['median_us']:.1f} [{v['min_us']:.1f}..{v['max_us']:.1f}]" for k, v in ss.items()) +
              f" us;  assign = {rec['assign_tflops']:.2f} Tflop/s f32 of {flops / 1e9:.2f} Gflop;  NMI {rec['nmi']:.3f} ARI {rec['ari']:.3f}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
