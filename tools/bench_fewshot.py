"""Time the few-shot prototype probe: this build (A, `FewShotProbe.run`: query preparation, the draw, prototypes, prediction and the
per-episode tally, five launches) against the same definition in batched torch ops on the same device (B: the [E, C, K, D] gather, its
mean, one [nq, D] x [D, E C] product, argmax and the per-episode accuracy; it is handed A's support rows, since torch has no
counterpart of the draw, and it forms neither the confusion counts nor balanced accuracy / F1).  Both sides reuse the prepared pool.

GPU only (fails without a device), one process.  Per case: warm-up of both, then `--rounds` alternations A, B, A, B, ... in the same
call, each round the mean of `--iters` passes between two device events.  Prints the median and the min..max spread of the rounds in
microseconds, the same for `mh_fewshot_predict` alone, and the f32 flops 2 E nq Cp D of the tile product (pads included: they are
multiplied) that this amounts to; then A replayed from a captured graph (no host work between its launches) and each of A's other
stages alone, timed in the same rounds.

    python tools/bench_fewshot.py [--rounds 5] [--iters 3] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mirror_amd import kernels as K  # noqa: E402
from mirror_amd.fewshot import FewShotProbe  # noqa: E402

E, SHOTS, D, POOL, NQ = 1000, 10, 512, 4000, 1000
CASES = [2, 10]              # classes


def torch_probe(y, mu, q, labels, support):
    """SimpleShot on the prepared pool y [n, D] with the support rows [E, C, K]: per-episode accuracy in percent, f64 [E]."""
    qn = F.normalize(q - mu, dim=1, eps=1e-12)
    p = y[support].mean(2)                                  # [E, C, D]
    e, c, d = p.shape
    s = (qn @ p.reshape(e * c, d).t()).view(-1, e, c) - 0.5 * (p * p).sum(2)
    pred = s.argmax(2)                                      # [nq, E]
    return 100.0 * (pred == labels[:, None]).double().mean(0), pred.t()


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
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fewshot.py needs a GPU")
    results = []
    for C in CASES:
        g = torch.Generator(device="cuda").manual_seed(C)
        centres = torch.randn(C, D, device="cuda", generator=g)
        yl = torch.arange(POOL, device="cuda") % C
        ql = torch.arange(NQ, device="cuda") % C
        pool = centres[yl] + 5.5 * torch.randn(POOL, D, device="cuda", generator=g) + 3.0
        q = centres[ql] + 5.5 * torch.randn(NQ, D, device="cuda", generator=g) + 3.0
        probe = FewShotProbe(C, shots=SHOTS, episodes=E, seed=1, device="cuda").fit(pool, yl)
        P = probe._pool()
        support = probe.draw()
        qn = K.center_l2norm(q, P["mu"])
        protos, bias = probe.prototypes()

        def a():
            probe.run(q, ql)

        def b():
            torch_probe(P["y"], P["mu"], q, ql, support)

        def a_predict():
            K.fewshot_predict(qn, protos, bias, C)

        rows = probe._draw_sorted(P)
        pred = K.fewshot_predict(qn, protos, bias, C)
        stages = {"query_prep": lambda: K.center_l2norm(q, P["mu"]), "draw": lambda: probe._draw_sorted(P),
                  "protos": lambda: K.fewshot_protos(P["y"], rows, P["perm"], "euclidean"), "tally": lambda: K.fewshot_tally(pred, ql, C)}

        acc_a = probe.run(q, ql)[:, 0].clone()
        acc_b, pred_b = torch_probe(P["y"], P["mu"], q, ql, support)
        differ = int((probe.pred.long() != pred_b).sum())
        for f in (a, b, a_predict, a, b, a_predict):
            f()                                               # warm-up, both sides
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()                        # A as a caller that repeats the evaluation would run it: no host work between launches
        with torch.cuda.graph(graph):
            probe.run(q, ql)
        graph.replay()
        torch.cuda.synchronize()
        ta, tb, tp, tg = [], [], [], []
        ts = {k: [] for k in stages}
        for _ in range(args.rounds):
            ta.append(timed(a, args.iters))
            tb.append(timed(b, args.iters))
            tg.append(timed(graph.replay, args.iters))
            tp.append(timed(a_predict, args.iters))
            for k, f in stages.items():
                ts[k].append(timed(f, args.iters))
        sa, sb, sp, sg = stats(ta), stats(tb), stats(tp), stats(tg)
        ss = {k: stats(v) for k, v in ts.items()}
        Cp = K.fewshot_cp(C)
        flops = 2.0 * E * NQ * Cp * D
        rec = {"C": C, "Cp": Cp, "E": E, "shots": SHOTS, "D": D, "pool": POOL, "nq": NQ, "build": sa, "torch": sb, "build_graph_replay": sg, "predict_alone": sp, "stages_alone": ss,
               "flops": flops, "predict_tflops": flops / (sp["median_us"] * 1e-6) / 1e12,
               "acc_build": float(acc_a.mean()), "acc_torch": float(acc_b.mean()), "predictions_differ": differ}
        print(f"C={C:<3d} Cp={Cp:<3d} E={E} K={SHOTS} D={D} pool={POOL} nq={NQ}  build {sa['median_us']:9.1f} us "
              f"[{sa['min_us']:.1f}..{sa['max_us']:.1f}]  torch {sb['median_us']:9.1f} us [{sb['min_us']:.1f}..{sb['max_us']:.1f}]  "
              f"predict alone {sp['median_us']:8.1f} us [{sp['min_us']:.1f}..{sp['max_us']:.1f}] = {rec['predict_tflops']:.2f} Tflop/s f32 "
              f"of {flops / 1e9:.1f} Gflop;  accuracy {rec['acc_build']:.3f} / {rec['acc_torch']:.3f} %, {differ} of {E * NQ} predictions differ",
              flush=True)
        print(f"      build as a graph replay {sg['median_us']:9.1f} us [{sg['min_us']:.1f}..{sg['max_us']:.1f}];  alone: " +
              ", ".join(f"{k} {v['median_us']:.1f}" for k, v in ss.items()) + " us", flush=True)
        results.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
