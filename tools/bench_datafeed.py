"""Time the device batch draw of DeviceSlideBank on one GPU: `bank.batch(ids, generator=gen)` (a host loop of torch.randperm /
randint per slide, then mh_gather_rows) against `bank.batch_sampled(ids, seed=, offset=)` (one mh_sample_rows launch, then the same
gathers), on the same bank and ids.

Shapes: B = 16 slots over 16 slides whose lengths are uniform in [2048, 60000] (seeded), bf16 features; (N, F) = (4096, 1024) and
(2048, 768).  After a warm-up the two paths are timed in interleaved pairs (old, new, old, new, ...), device events around each call
and a synchronise behind it, so drift of the box hits both alike; also timed the same way: K.sample_rows alone, and batch_sampled
replayed from a captured graph (device ids, the draw id bumped through dev_base).  Prints one JSON line per shape: median and
quartiles in microseconds.  Figures only: nothing is asserted.

    python tools/bench_datafeed.py [--pairs 50] [--warmup 10] [--batch 16]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mirror_amd import kernels as K  # noqa: E402
from mirror_amd.data import DeviceSlideBank  # noqa: E402

SHAPES = ((4096, 1024), (2048, 768))


def _timed(fn) -> float:
    """Device time of one fn() in microseconds (HIP events; the call is complete when this returns)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def _quartiles(ts) -> dict:
    ts = sorted(ts)
    q = lambda f: round(ts[min(len(ts) - 1, int(f * len(ts)))], 1)  # noqa: E731
    return {"median_us": q(0.5), "q1_us": q(0.25), "q3_us": q(0.75)}


def run(N: int, F: int, batch: int, pairs: int, warmup: int) -> dict:
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2048 + N)
    lengths = torch.randint(2048, 60001, (batch,), generator=g).tolist()
    gd = torch.Generator(device=dev).manual_seed(7)
    slides = [torch.randn(n, F, device=dev, generator=gd).to(torch.bfloat16) for n in lengths]
    bank = DeviceSlideBank(slides, torch.randn(batch, 2048, generator=g), N, device=dev)
    del slides
    ids = torch.randperm(batch, generator=g).tolist()
    dids = torch.as_tensor(ids, device=dev)
    base = torch.zeros(1, dtype=torch.int64, device=dev)
    step = [0]

    def old():
        return bank.batch(ids, generator=gd)

    def new():
        step[0] += batch
        return bank.batch_sampled(ids, seed=7, offset=step[0])

    def draw_only():
        step[0] += batch
        return K.sample_rows(dids, bank.lengths_dev, bank.offsets_dev, N, 7, step[0])

    for _ in range(warmup):
        old(), new(), draw_only()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = bank.batch_sampled(dids, seed=7, offset=1 << 40, dev_base=base)

    def replay():
        base.add_(batch)
        graph.replay()
        return held

    for _ in range(warmup):
        replay()
    torch.cuda.synchronize()
    ts = {"batch_generator": [], "batch_sampled": [], "sample_rows_alone": [], "batch_sampled_graph_replay": []}
    for _ in range(pairs):
        ts["batch_generator"].append(_timed(old))
        ts["batch_sampled"].append(_timed(new))
        ts["sample_rows_alone"].append(_timed(draw_only))
        ts["batch_sampled_graph_replay"].append(_timed(replay))
    return {"B": batch, "N": N, "F": F, "dtype": "bf16", "lengths_min": min(lengths), "lengths_max": max(lengths), "pairs": pairs,
            "gather_bytes": batch * N * F * 2 * 2, **{k: _quartiles(v) for k, v in ts.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_datafeed.py times an MI355X: no device here")
    for N, F in SHAPES:
        print(json.dumps(run(N, F, args.batch, args.pairs, args.warmup)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
