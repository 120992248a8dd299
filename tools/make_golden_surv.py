"""Generate tests/golden/golden_surv.npz by running the REFERENCE survival losses themselves (CPU, f32).

`losses/nll_surv.py` and `losses/cross_entropy_surv.py` of a reference MIRROR checkout are pure torch: they are imported by path,
unmodified, and run on seeded inputs.  The risk score is the reference trainer's own expression (train_survival.py:1431-1433).
Nothing from the reference is copied: the fixture holds inputs, seeds and expected outputs.

    python tools/make_golden_surv.py --reference /path/to/MIRROR

Layout (K = "nll" / "ce", G = "N{N}_M{M}"; A = "a0" / "a0.4" for NLL, "a0" for CE; R = "mean" / "sum" / "none"):
  {K}/{G}/logits, /event_times, /censoring   inputs (dtypes as fed: event_times int32 or int64, censoring int64 or f32)
  {K}/{G}/w, /gs                             upstream: per-row weight ("none", the loss's own shape) / scalar ("mean", "sum")
  {K}/{G}/{A}/{R}/loss, /dlogits             reference outputs: loss (0-d or per-row) and d(upstream . loss)/d logits
  risk/{G}                                   risk scores of {nll}/{G}/logits
"""
from __future__ import annotations

import argparse
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "golden_surv.npz")

NS = (1, 16, 257)
MS = (1, 4, 20, 130)
ALPHAS = {"nll": (0.0, 0.4), "ce": (0.0,)}
REDUCTIONS = ("mean", "sum", "none")
SAT = 20.0          # saturated entries: 20 <= |x| <= 30 (both hazard clamps fire there)
REG = 12.0          # every other entry: |x| <= 12, far from the clamp thresholds (logit(1e-7) = -16.1, logit(1 - 1e-7) = 15.9)
SEED = 20260


def load_reference_losses(ref: str):
    mods = {}
    for name in ("nll_surv", "cross_entropy_surv"):
        spec = importlib.util.spec_from_file_location(f"ref_losses_{name}", os.path.join(ref, "losses", f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods["nll_surv"].NLLSurvLoss, mods["cross_entropy_surv"].CrossEntropySurvLoss


def make_inputs(kind: str, N: int, M: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(N, M, generator=g) * 2 - 1) * REG
    # saturated rows (every third row from row 1) and single saturated entries (every fifth row)
    sat = (SAT + torch.rand(N, M, generator=g) * (30.0 - SAT)) * torch.where(torch.rand(N, M, generator=g) < 0.5, -1.0, 1.0)
    rows = torch.arange(N)
    full = (rows % 3 == 1)[:, None].expand(N, M)
    one = ((rows % 5 == 2)[:, None] & (torch.arange(M)[None, :] == (rows[:, None] % M)))
    x = torch.where(full | one, sat, x).contiguous()
    if kind == "nll":
        t = torch.randint(-1, M + 3, (N,), generator=g)            # T < 0 and T >= M are valid for NLL
        special = [0, M - 1, M, M + 1, -1]
        c = torch.randint(0, 2, (N,), generator=g)
        c[rows % 11 == 4] = 2                                      # neither censored nor uncensored: row loss 0
    else:
        t = torch.randint(0, M + 1, (N,), generator=g)             # an uncensored T = M selects the no-event class
        special = [0, M - 1, M]
        c = torch.randint(0, 2, (N,), generator=g)
    for i, v in enumerate(special):
        if 2 * i < N:
            t[2 * i] = v
    k = NS.index(N) * len(MS) + MS.index(M)
    t = t.to(torch.int32 if k % 2 else torch.int64)
    c = c.to(torch.float32 if (k // 2) % 2 else torch.int64)
    w = torch.rand((N, 1) if kind == "ce" else (N,), generator=g) * 2 - 0.5
    gs = torch.rand((), generator=g) + 0.5
    return x, t, c, w, gs


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of a reference MIRROR checkout (losses/ is imported from it)")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    NLL, CE = load_reference_losses(args.reference)
    torch.set_num_threads(1)
    rec = {"meta/seed": np.int64(SEED), "meta/ns": np.array(NS), "meta/ms": np.array(MS)}
    for kind in ("nll", "ce"):
        for N in NS:
            for M in MS:
                G = f"N{N}_M{M}"
                x, t, c, w, gs = make_inputs(kind, N, M, SEED + 1000 * NS.index(N) + 10 * MS.index(M) + (kind == "ce"))
                rec[f"{kind}/{G}/logits"], rec[f"{kind}/{G}/event_times"] = x.numpy(), t.numpy()
                rec[f"{kind}/{G}/censoring"], rec[f"{kind}/{G}/w"], rec[f"{kind}/{G}/gs"] = c.numpy(), w.numpy(), gs.numpy()
                for alpha in ALPHAS[kind]:
                    for red in REDUCTIONS:
                        fn = NLL(alpha=alpha, reduction=red) if kind == "nll" else CE(reduction=red)
                        xl = x.clone().requires_grad_(True)
                        loss = fn(xl, t, c)
                        (loss * (w if red == "none" else gs)).sum().backward()
                        key = f"{kind}/{G}/a{alpha:g}/{red}"
                        rec[key + "/loss"] = loss.detach().numpy()
                        rec[key + "/dlogits"] = xl.grad.numpy()
                        assert np.isfinite(rec[key + "/loss"]).all() and np.isfinite(rec[key + "/dlogits"]).all(), key
                if kind == "nll":
                    hazards = torch.sigmoid(x)
                    rec[f"risk/{G}"] = (-torch.sum(torch.cumprod(1 - hazards, dim=1), dim=1)).numpy()
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {len(rec)} arrays, {os.path.getsize(args.out) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
