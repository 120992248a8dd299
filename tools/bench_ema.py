"""Time the model EMA (timm ModelEmaV3, --model-ema) on one GPU.

(a) The c2 training step (bench.py's headline shapes, bf16, whole-step graph) with and without `TrainEngine(model_ema=...)`,
    two engines on identical models, timed in alternating blocks of steps so that drift of the box hits both alike: the per-step
    difference is what the fused EMA lerp inside mh_adam_ema costs.
(b) mh_ema_update_many (the standalone path) at 1e6, 1e7 and 3.5e7 parameters, as one tensor split into table rows: GB/s counted
    as 12 B per element (EMA read + write, source read).
Prints one JSON line per measurement (medians).  Figures only: nothing is asserted.

    python tools/bench_ema.py [--steps 20] [--rounds 5] [--batch 16] [--sizes 1e6 1e7 3.5e7]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mirror_amd import functional as Fn  # noqa: E402
from mirror_amd import kernels as K  # noqa: E402


def _time(fn, reps: int) -> float:
    """Median wall time of fn() in microseconds (HIP events)."""
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


def step_delta(steps: int, rounds: int, batch: int) -> dict:
    import mirror_amd.models as M
    from mirror_amd.ema import ModelEmaV3
    from mirror_amd.engine import TrainEngine
    from mirror_amd.losses import MIRRORLoss
    dev = torch.device("cuda:0")
    engines = {}
    for name in ("plain", "ema"):
        torch.manual_seed(42)
        model = M.mirror(wsi_embed_dim=1024, rna_embed_dim=2048, embed_dim=512, wsi_num_tokens=4096, rna_encoder_depth=6,
                         rna_mlp_ratio=4.0, rna_norm_layer="layernorm", rna_act_layer="gelu", rna_num_heads=8).to(dev).train()
        loss_fn = MIRRORLoss(alignment_loss_weight=0.5, wsi_retention_loss_weight=0.15, rna_retention_loss_weight=0.15,
                             style_loss_weight=0.1, cluster_loss_weight=0.1)
        ema = ModelEmaV3(model, decay=0.9998, use_warmup=True) if name == "ema" else None
        engines[name] = TrainEngine(model, loss_fn, lr=2e-5, precision="bf16", model_ema=ema)
    Fn.manual_seed(1234)
    g = torch.Generator(device=dev).manual_seed(1234)
    wsi = torch.randn(batch, 4096, 1024, device=dev, generator=g).to(torch.bfloat16)
    rna = torch.randn(batch, 2048, device=dev, generator=g)
    for eng in engines.values():           # eager warm-up, capture, a few replays
        for _ in range(5):
            eng.step(wsi, rna)
    torch.cuda.synchronize()
    per = {k: [] for k in engines}
    for _ in range(rounds):
        for name, eng in engines.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                eng.step(wsi, rna)
            b.record()
            b.synchronize()
            per[name].append(a.elapsed_time(b) / steps)
    med = {k: sorted(v)[len(v) // 2] for k, v in per.items()}
    n = engines["ema"].numel
    return {"bench": "c2_step_ema", "batch": batch, "params": n, "steps_per_block": steps, "rounds": rounds,
            "ms_per_step_plain": round(med["plain"], 4), "ms_per_step_ema": round(med["ema"], 4),
            "delta_us_per_step": round((med["ema"] - med["plain"]) * 1e3, 1),
            "ms_plain_blocks": [round(x, 4) for x in per["plain"]], "ms_ema_blocks": [round(x, 4) for x in per["ema"]],
            "ema_extra_bytes_per_step": 8 * n}


def update_many(n: int, reps: int) -> dict:
    from mirror_amd.ema import _rows
    dev = torch.device("cuda:0")
    src = torch.randn(n, device=dev)
    ema = torch.randn(n, device=dev)
    rows = _rows(0, src)
    table = torch.tensor(rows, dtype=torch.int64, device=dev)
    us = _time(lambda: K.ema_update_many(ema, table, len(rows) // 3, 2e-4), reps)
    return {"bench": "mh_ema_update_many", "n": n, "rows": len(rows) // 3, "us": round(us, 2), "GBps": round(12 * n / us / 1e3, 1)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--sizes", type=float, nargs="+", default=[1e6, 1e7, 3.5e7])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--skip-step", action="store_true", help="(b) only")
    a = ap.parse_args()
    for n in a.sizes:
        print(json.dumps(update_many(int(n), a.reps)), flush=True)
    if not a.skip_step:
        print(json.dumps(step_delta(a.steps, a.rounds, a.batch)), flush=True)


if __name__ == "__main__":
    main()
