"""Measurements for the cluster probe's seeding and silhouette.

    silhouette   `mh_silhouette` at n = 8192, D = 512, K = 8, one label row, against `mh_retrieval_ranks` on the same rows as queries and
                 keys: the same n x n exact-f32 product with a comparing epilogue.  The two alternate in one process; a run is
                 `--iters` back-to-back calls between two device events (launch gaps and the wrappers' allocations included, not kernel
                 times from a trace); the median of `--rounds` runs with min and max, and the ratio of the medians.
    seeding      for the three end-to-end inputs of tests/kmeans_ref.py: mean NMI and mean n_iter_ over 16 restarts with
                 seeding="random" and with "kmeans++", both metrics.  Observations, not claims.

GPU only.  Each step runs in a child process of its own under its own time limit, and a step that fails ends the run: nothing more
is started on the device.  Reads nothing outside the repository.

    python tools/bench_cluster_ext.py [--rounds 7] [--iters 10] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, KK = 8192, 512, 8
STEPS = {"silhouette": 240, "seeding": 240}                  # seconds


def stats(xs):
    xs = sorted(xs)
    return {"median_us": xs[len(xs) // 2], "min_us": xs[0], "max_us": xs[-1]}


def step_silhouette(args) -> dict:
    import torch
    from mirror_amd import kernels as K

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters

    g = torch.Generator(device="cuda").manual_seed(1)
    centres = torch.randn(KK, D, device="cuda", generator=g)
    yl = (torch.arange(N, device="cuda") * 7919) % KK           # unsorted ids
    x = centres[yl] + 2.0 * torch.randn(N, D, device="cuda", generator=g) + 3.0
    y = K.center_l2norm(x, K.colmean(x))
    lab = yl.to(torch.int32).view(1, N).contiguous()
    out = {"n": N, "D": D, "K": KK, "rounds": args.rounds, "calls_per_run": args.iters, "product_flops": 2.0 * N * N * D}
    for metric in ("euclidean", "cosine"):
        sil = lambda: K.silhouette(y, lab, KK, metric)          # noqa: E731
        ranks = lambda: K.retrieval_ranks(y, y)                 # noqa: E731
        for f in (sil, ranks, sil, ranks):
            f()
        torch.cuda.synchronize()
        ts, tr = [], []
        for _ in range(args.rounds):                            # alternate
            ts.append(timed(sil))
            tr.append(timed(ranks))
        s, r = stats(ts), stats(tr)
        mean = float(K.silhouette(y, lab, KK, metric)[0][0])
        out[metric] = {"silhouette": s, "retrieval_ranks": r, "ratio": s["median_us"] / r["median_us"], "mean_silhouette": mean,
                       "silhouette_tflops": out["product_flops"] / (s["median_us"] * 1e-6) / 1e12}
        print(f"{metric:9s} n={N} D={D} K={KK}: mh_silhouette {s['median_us']:.1f} us [{s['min_us']:.1f}..{s['max_us']:.1f}], "
              f"mh_retrieval_ranks {r['median_us']:.1f} us [{r['min_us']:.1f}..{r['max_us']:.1f}], ratio {out[metric]['ratio']:.3f}, "
              f"{out[metric]['silhouette_tflops']:.1f} Tflop/s of the product; silhouette {mean:.4f}", flush=True)
    return out


def step_seeding(args) -> dict:
    import numpy as np
    import torch
    from mirror_amd.cluster import ClusterProbe
    from tests import kmeans_ref as R

    out = {}
    for shape in R.E2E:
        C, Dd, per, noise, Kk = shape
        pool, yl = R.clusters(C, Dd, per, noise, seed=C * 1000 + Dd)
        xd, ld = torch.from_numpy(pool).cuda(), torch.from_numpy(yl).cuda()
        for metric in ("cosine", "euclidean"):
            for seeding in ("random", "kmeans++"):
                p = ClusterProbe(Kk, restarts=16, metric=metric, seed=1, seeding=seeding, device="cuda").fit(xd)
                res = p.evaluate(ld, C, matched=True)
                rec = {"nmi_mean": res["cluster_nmi_mean"], "nmi_best": res["cluster_nmi"], "acc_mean": res["cluster_acc_mean"],
                       "n_iter_mean": float(p.n_iter_.double().mean()), "inertia_mean": float(p.inertia_.mean()),
                       "inertia_best": res["cluster_inertia"]}
                out[f"{shape}/{metric}/{seeding}"] = rec
                print(f"{str(shape):28s} {metric:9s} {seeding:8s}: mean NMI {rec['nmi_mean']:.4f} (best restart {rec['nmi_best']:.4f}), "
                      f"mean matched accuracy {rec['acc_mean']:.2f} %, mean n_iter {rec['n_iter_mean']:.2f}, mean inertia "
                      f"{rec['inertia_mean']:.4f}", flush=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run one step in this process (what the parent starts)")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("at least five rounds")
    if args.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_cluster_ext.py needs a GPU")
        rec = {"silhouette": step_silhouette, "seeding": step_seeding}[args.step](args)
        print("RESULT " + json.dumps(rec), flush=True)
        return
    result = {}
    for step, limit in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--rounds", str(args.rounds), "--iters", str(args.iters)]
        try:
            done = subprocess.run(cmd, cwd=ROOT, timeout=limit, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step {step} did not end within {limit} s: nothing more is started")
        lines = done.stdout.splitlines()
        print("\n".join(ln for ln in lines if not ln.startswith("RESULT ")), flush=True)
        if done.returncode != 0:
            raise SystemExit(f"step {step} ended with status {done.returncode}: nothing more is started")
        result[step] = json.loads([ln for ln in lines if ln.startswith("RESULT ")][-1][len("RESULT "):])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
