"""Generate tests/golden/golden_infonce_neg.npz: InfoNCE with explicit negative keys, in f64.

The reference's explicit-negatives branch (losses/info_nce.py:126-143) builds `logits = cat([pos, neg], 1)` and `labels = 0` and
never assigns `loss`.  This fixture is the reference's logits with the missing line supplied:
`F.cross_entropy(logits / temperature, labels, reduction=reduction)`, stated here from the definition (no reference code is copied):

    q^, k^, n^ = x / max(|x|_2, 1e-12) along the last dim
    pos[i] = q^[i].k^[i];  neg[i, j] = q^[i].n^[j] (unpaired, negatives [M, D]) or q^[i].n^[i, j] (paired, negatives [N, M, D])
    row[i] = logsumexp([pos[i] | neg[i, :]] / t) - pos[i] / t;  "mean" -> mean, "sum" -> sum, "none" -> [N]

The tool also checks against a reference MIRROR checkout that (a) its InfoNCE still raises UnboundLocalError on this branch and (b) its
`normalize()` agrees with the one above on the fixture's inputs, so the statement in this header stays true.

    python tools/make_golden_infonce_neg.py --reference /path/to/MIRROR

Layout (MODE = "paired" / "unpaired", T = "t0.07" / "t0.5", R = "mean" / "sum" / "none"):
  {MODE}/query, /positive_key, /negative_keys     f64 inputs (exactly representable in f32)
  {MODE}/w                                        per-row upstream weights for R = "none" (the differentiated scalar is sum(w * loss))
  {MODE}/{T}/{R}/loss, /dquery, /dpositive_key, /dnegative_keys     f64 loss (0-d or [N]) and gradients
"""
from __future__ import annotations

import argparse
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "golden_infonce_neg.npz")

N, M, D = 8, 12, 32
MODES = ("paired", "unpaired")
TEMPERATURES = (0.07, 0.5)
REDUCTIONS = ("mean", "sum", "none")
SEED = 20261


def normalize(x: torch.Tensor) -> torch.Tensor:
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def info_nce_neg(query, positive_key, negative_keys, temperature, reduction, mode):
    q, k, n = normalize(query), normalize(positive_key), normalize(negative_keys)
    pos = (q * k).sum(-1, keepdim=True)
    neg = q @ n.t() if mode == "unpaired" else torch.einsum("id,ijd->ij", q, n)
    logits = torch.cat([pos, neg], 1) / temperature
    rows = torch.logsumexp(logits, 1) - logits[:, 0]
    return rows.mean() if reduction == "mean" else rows.sum() if reduction == "sum" else rows


def make_inputs(mode: str):
    g = torch.Generator().manual_seed(SEED + MODES.index(mode))
    f = lambda *shape: torch.randn(*shape, generator=g).double()      # f32 draws: the fixture's inputs are exact in f32
    q, k = f(N, D), f(N, D) * 3.0
    n = f(M, D) if mode == "unpaired" else f(N, M, D)
    n = (n * (torch.rand(n.shape[:-1] + (1,), generator=g).double() * 4.0 + 0.1)).float().double()      # rows of mixed length
    k = (0.6 * k + 0.8 * q).float().double()                          # positives correlate with their queries
    w = (torch.rand(N, generator=g) * 2 - 0.5).double()
    return q, k, n, w


def check_reference(ref: str, cases) -> None:
    spec = importlib.util.spec_from_file_location("ref_info_nce", os.path.join(ref, "losses", "info_nce.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for mode, (q, k, n, _) in cases.items():
        crit = mod.InfoNCE(temperature=0.07, negative_mode=mode)
        try:
            crit(q, k, n)
        except UnboundLocalError:
            pass
        else:
            raise SystemExit(f"the reference's explicit-negatives branch ({mode}) now returns a loss: regenerate this fixture from it")
        for a, b in zip(crit.normalize(q, k, n), (normalize(q), normalize(k), normalize(n))):
            assert torch.allclose(a, b, rtol=1e-14, atol=0), (mode, float((a - b).abs().max()))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="path of a reference MIRROR checkout")
    args = ap.parse_args()
    cases = {mode: make_inputs(mode) for mode in MODES}
    check_reference(args.reference, cases)
    out = {}
    for mode, (q, k, n, w) in cases.items():
        out[f"{mode}/query"], out[f"{mode}/positive_key"], out[f"{mode}/negative_keys"], out[f"{mode}/w"] = (
            x.numpy() for x in (q, k, n, w))
        for t in TEMPERATURES:
            for red in REDUCTIONS:
                qq, kk, nn = (x.clone().requires_grad_(True) for x in (q, k, n))
                loss = info_nce_neg(qq, kk, nn, t, red, mode)
                ((loss * w).sum() if red == "none" else loss).backward()
                key = f"{mode}/t{t}/{red}"
                out[f"{key}/loss"] = loss.detach().numpy()
                out[f"{key}/dquery"], out[f"{key}/dpositive_key"], out[f"{key}/dnegative_keys"] = (
                    x.grad.numpy() for x in (qq, kk, nn))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
