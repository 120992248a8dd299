"""Time the arena optimizer behind torch.optim's interface (mirror_amd.optim.ArenaOptimizer) on one GPU.

(a) `zero_grad()` + `step()` over the parameters of `mirror_classifier` at the subtyping template geometry (D = 768, 10234 genes, 4
    classes), fine-tune (every parameter) and linear probe (the head alone), for ArenaOptimizer, torch.optim.Adam with its defaults
    and torch.optim.Adam(fused=True).  Each optimizer gets its own copy of the model; the gradients are resident and filled once (the
    update does not depend on their values), and zero_grad runs with each optimizer's own default.
(b) mh_optim_groups against mh_optim_step on one arena of 40 M elements (rule Adam, a group map with three groups, one learning rate),
    in alternating blocks, with the run-to-run spread of each: the medians of `--rounds` blocks and their min .. max.
HIP events around `--reps` calls per block after a warm-up; medians over the blocks.  One JSON line per measurement.  Figures only:
nothing is asserted.

    python tools/bench_arena_optim.py [--reps 50] [--rounds 7] [--n 40000000]
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mirror_amd import kernels as K  # noqa: E402


def _block_us(fn, reps: int) -> float:
    """Mean time of fn() over one block of `reps` back-to-back calls, in microseconds (HIP events, one synchronise)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def _alternate(fns: dict, reps: int, rounds: int) -> dict:
    """Blocks of every candidate in turn, `rounds` times, so that drift of the machine hits all alike."""
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            per[k].append(_block_us(fn, reps))
    return {k: sorted(v) for k, v in per.items()}


def _stats(v):
    return {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "max_us": round(v[-1], 2)}


def optimizers(mode: str, reps: int, rounds: int) -> dict:
    import mirror_amd.models as M
    from mirror_amd.optim import create_optimizer_v2
    torch.manual_seed(0)
    base = M.create_model("mirror_classifier", wsi_embed_dim=768, rna_embed_dim=10234, embed_dim=768, num_classes=4,
                          rna_encoder_depth=2, rna_mlp_ratio=4.0, rna_norm_layer="layernorm", rna_act_layer="gelu", fusion="concat")
    if mode == "linear_probe":
        for p in base.parameters():
            p.requires_grad_(False)
        for p in base.head.parameters():
            p.requires_grad_(True)
    base = base.cuda()
    base.precision = "bf16"
    models = {k: copy.deepcopy(base) for k in ("arena", "torch_adam", "torch_adam_fused")}
    train = {k: [p for p in m.parameters() if p.requires_grad] for k, m in models.items()}
    opts = {"arena": create_optimizer_v2(models["arena"], opt="adam", lr=1e-4),
            "torch_adam": torch.optim.Adam(train["torch_adam"], lr=1e-4),
            "torch_adam_fused": torch.optim.Adam(train["torch_adam_fused"], lr=1e-4, fused=True)}

    def fill(k):
        for p in train[k]:
            if p.grad is None:
                p.grad = torch.empty_like(p)
            p.grad.normal_(std=1e-3)

    def runner(k):
        o = opts[k]
        if k == "arena":
            def run():
                o.zero_grad()
                o.step()
        else:
            def run():               # set_to_none would leave nothing to step on: the gradients stay resident, as the arena's do
                o.zero_grad(set_to_none=False)
                o.step()
        return run
    for k in opts:
        fill(k)
    per = _alternate({k: runner(k) for k in opts}, reps, rounds)
    n = sum(p.numel() for p in train["arena"])
    out = {"bench": "zero_grad_step", "mode": mode, "params": n, "tensors": len(train["arena"]), "reps": reps, "rounds": rounds}
    out.update({k: _stats(v) for k, v in per.items()})
    return out


def kernels(n: int, reps: int, rounds: int) -> dict:
    from mirror_amd._lib import OptimCfg
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    bufs = {}
    for k in ("step", "groups"):
        bufs[k] = [torch.randn(n, device=dev, generator=g) * s for s in (1.0, 1e-3, 0.0, 0.0)] + [torch.zeros(n, device=dev, dtype=torch.bfloat16)]
        bufs[k][3] = bufs[k][3].abs()
    gmap = (torch.arange((n + 7) // 8, device=dev) // 4099 % 3).to(torch.uint8)
    wd = torch.tensor([0.0, 0.05, 0.1], device=dev)
    lrs = torch.full((3,), 1e-4, device=dev)
    cfg = OptimCfg(0, 0.9, 0.999, 1e-8, 0.0, 0)
    states = {k: torch.tensor([0.0, 0.0, 0.0, 1e-4, 1.0, 0.0], device=dev) for k in bufs}

    def step():
        p, gr, m, v, sh = bufs["step"]
        K.optim_step(p, gr, m, v, sh, cfg, states["step"], group_map=gmap, group_wd=wd)

    def groups():
        p, gr, m, v, sh = bufs["groups"]
        K.optim_groups(p, gr, m, v, sh, cfg, states["groups"], gmap, wd, lrs)
    per = _alternate({"mh_optim_step": step, "mh_optim_groups": groups}, reps, rounds)
    out = {"bench": "optim_kernels", "n": n, "reps": reps, "rounds": rounds, "bytes_per_param": 30.125,
           "note": "each figure includes the one-thread tick launch in front of the update"}
    out.update({k: _stats(v) for k, v in per.items()})
    a, b = per["mh_optim_step"], per["mh_optim_groups"]
    spread = a[-1] - a[0]
    diff = b[len(b) // 2] - a[len(a) // 2]
    out.update(spread_of_optim_step_us=round(spread, 2), groups_minus_step_us=round(diff, 2),
               difference_in_spreads=round(diff / spread, 2) if spread > 0 else None,
               GBps_groups=round(30.125 * n / b[len(b) // 2] / 1e3, 1))
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--n", type=int, default=40_000_000)
    ap.add_argument("--skip-optimizers", action="store_true", help="(b) only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_arena_optim.py measures on an MI355X: no GPU found")
    print(json.dumps(kernels(a.n, a.reps, a.rounds)), flush=True)
    if not a.skip_optimizers:
        for mode in ("fine_tune", "linear_probe"):
            print(json.dumps(optimizers(mode, a.reps, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
