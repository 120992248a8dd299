"""Time the retrieval ranks: this build's fused kernel (A, `retrieval.retrieval_ranks`) against the same definition composed from
torch ops on the same device (B: `S = q @ k.T`, compare with the diagonal, count), which materialises the [n, n] f32 matrix.

GPU only (fails without a device), one process.  Per shape: the two results are compared, both are warmed up, then `--rounds`
alternations A, B, A, B, ... in the same call, each round the mean of `--iters` calls between two device events.  Prints the median
and the min..max spread of the rounds in microseconds, the f32-MFMA share of A (2 n^2 D flops against the f32 matrix peak, 1/16 of
the bf16 peak) and the peak device memory either form allocates on top of its inputs (torch.cuda.max_memory_allocated).

The grouped leg (`--grouped`, n = 8192, D = 512, groups of 1..3 rows): the ungrouped `mh_retrieval_ranks` (U) alternated with the
grouped call on the same embeddings, as the whole `retrieval_ranks(query_group=, key_group=, key_count=)` (G: the device sort of the ids
and the two launches) and with the sort handed over (K: the two launches alone).  `--ungrouped-lib FILE.so` takes U from another build
of csrc/retrieval.hip (e.g. the commit before the grouped entry point) through ctypes instead of from this one.

    python tools/bench_retrieval.py [--rounds 5] [--iters 5] [--grouped] [--ungrouped-lib FILE.so] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mirror_amd import kernels as K  # noqa: E402
from mirror_amd.retrieval import first_of_group, retrieval_ranks  # noqa: E402

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


def foreign_ungrouped(path):
    """mh_retrieval_ranks of another build of the library, on the current stream, with the workspace allocated as kernels does."""
    lib = ctypes.CDLL(os.path.abspath(path))
    P, L, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.mh_retrieval_ranks.argtypes = [P, P, L, L, I, P, P, P, P]
    lib.mh_retrieval_ranks.restype = I
    lib.mh_retrieval_workspace_bytes.argtypes = [L, L, I]
    lib.mh_retrieval_workspace_bytes.restype = L

    def run(q, k):
        n, D = q.shape
        ranks = torch.empty((n,), device=q.device, dtype=torch.int32)
        ws = torch.empty(((int(lib.mh_retrieval_workspace_bytes(n, n, D)) + 3) // 4,), device=q.device, dtype=torch.float32)
        rc = lib.mh_retrieval_ranks(q.data_ptr(), k.data_ptr(), n, n, D, None, ranks.data_ptr(), ws.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
        if rc:
            raise SystemExit(f"{path}: mh_retrieval_ranks returned {rc}")
        return ranks
    return run


def grouped_leg(args, n=8192, D=512):
    g = torch.Generator(device="cuda").manual_seed(n + D + 1)
    q = torch.randn(n, D, device="cuda", generator=g)
    k = 0.1 * q + torch.randn(n, D, device="cuda", generator=g)
    cpu = torch.Generator().manual_seed(7)
    sizes = torch.randint(1, 4, (n,), generator=cpu)
    ids = torch.repeat_interleave(torch.arange(n), sizes)[:n][torch.randperm(n, generator=cpu)].cuda()
    order = torch.sort(ids, stable=True)
    first = first_of_group(*order)
    foreign = foreign_ungrouped(args.ungrouped_lib) if args.ungrouped_lib else None

    def fu():
        return foreign(q, k) if foreign else retrieval_ranks(q, k)

    def fg():
        return retrieval_ranks(q, k, query_group=ids, key_group=ids, key_count=first)

    def fk():
        return K.retrieval_ranks_grouped(q, k, ids, ids, first, key_order=order)

    assert torch.equal(fg(), fk())
    if foreign:
        assert torch.equal(fu(), retrieval_ranks(q, k)), "the two builds' ungrouped ranks differ"
    distinct = torch.arange(n, device="cuda")
    assert torch.equal(retrieval_ranks(q, k, query_group=distinct, key_group=distinct), retrieval_ranks(q, k))
    for f in (fu, fg, fk, fu, fg, fk):
        f()
    torch.cuda.synchronize()
    tu, tg, tk = [], [], []
    for _ in range(args.rounds):
        tu.append(timed(fu, args.iters))
        tg.append(timed(fg, args.iters))
        tk.append(timed(fk, args.iters))
    u, gr, kk = stats(tu), stats(tg), stats(tk)
    res = {"leg": "grouped", "n": n, "D": D, "groups": int(first.sum()), "ungrouped": u, "grouped_call": gr, "grouped_launches": kk,
           "ungrouped_from": args.ungrouped_lib or "this build", "mean_rank_grouped": float(fg().float().mean())}
    print(f"grouped leg n={n} D={D} groups={res['groups']}: ungrouped ({res['ungrouped_from']}) {u['median_us']:.1f} us "
          f"[{u['min_us']:.1f}..{u['max_us']:.1f}]  grouped call {gr['median_us']:.1f} us [{gr['min_us']:.1f}..{gr['max_us']:.1f}]  "
          f"its two launches {kk['median_us']:.1f} us [{kk['min_us']:.1f}..{kk['max_us']:.1f}]", flush=True)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--grouped", action="store_true", help="the grouped leg alone")
    ap.add_argument("--ungrouped-lib", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_retrieval.py needs a GPU")
    results = []
    for n, D in ([] if args.grouped else CASES):
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
    results.append(grouped_leg(args))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
