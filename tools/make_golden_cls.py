"""Generate tests/golden/golden_cls.npz: expected values of the subtyping step's loss and validation metrics (train_subtyping.py).

The loss and its logit gradient come from CPU torch in f64 (`torch.nn.functional.cross_entropy(..., label_smoothing=s,
ignore_index=...)` and autograd), which restates timm's LabelSmoothingCrossEntropy (train_subtyping.py:984) and is
nn.CrossEntropyLoss (:986, :990).  F1 and the per-class one-vs-rest AUROC come from sklearn (`f1_score(..., zero_division=0)`,
`roc_auc_score` on y == c against the raw column), with torcheval's rule of 0.5 for a class without positives or negatives;
predictions are CPU `torch.argmax` of the f32 scores.  Needs torch and sklearn; GPU tests read only the fixture.

    python tools/make_golden_cls.py

Layout (G = "N{N}_C{C}", S = "s0" / "s0.1", R = "mean" / "sum" / "none"):
  cls/{G}/logits f32 [N, C], /labels int32 or int64 [N], /ignore_index, /w f32 [N] (upstream of "none"), /gs f32 (of mean / sum)
  cls/{G}/{S}/{R}/loss f64 (0-d or [N]), /dx f32 [N, C] (not for R = "sum" when N * C > DX_SUM_MAX)
  met/{G}/{V}/...   V = "f": scores are cls/{G}/logits; V = "i": integer-valued scores /scores int8 [N, C] (dense ties)
      /labels int64 [N], /auroc f64 [C], /f1_micro, /f1_macro, /f1_weighted f64, /f1_none f64 [C], /acc f64 (correct / N)
  met/nan/...       one NaN score (row 3, class 2) and one class without positives: /scores f32 [16, 5] plus the keys above
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch
import torch.nn.functional as F
from sklearn.metrics import f1_score, roc_auc_score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "golden_cls.npz")

NS = (1, 16, 1000)
CS = (2, 5, 33)
SS = (0.0, 0.1)
REDUCTIONS = ("mean", "sum", "none")
SEED = 20261
DX_SUM_MAX = 10000  # above N * C = 10^4 the "sum" gradient (the "mean" one times a scalar) is not stored: the file stays < 1 MiB


def auroc_ref(y: np.ndarray, scores: np.ndarray) -> np.ndarray:
    C = scores.shape[1]
    out = np.empty(C)
    for c in range(C):
        pos = y == c
        if pos.all() or not pos.any():
            out[c] = 0.5
        elif np.isnan(scores[:, c]).any():
            out[c] = np.nan
        else:
            out[c] = roc_auc_score(pos.astype(np.int64), scores[:, c].astype(np.float64))
    return out


def metrics_ref(rec: dict, key: str, scores: np.ndarray, y: np.ndarray) -> None:
    C = scores.shape[1]
    pred = torch.argmax(torch.from_numpy(scores.astype(np.float32)), dim=1).numpy()
    rec[key + "/labels"] = y.astype(np.int64)
    rec[key + "/auroc"] = auroc_ref(y, scores)
    for avg in ("micro", "macro", "weighted"):
        rec[f"{key}/f1_{avg}"] = np.float64(f1_score(y, pred, average=avg, zero_division=0))
    rec[key + "/f1_none"] = f1_score(y, pred, labels=np.arange(C), average=None, zero_division=0).astype(np.float64)
    rec[key + "/acc"] = np.float64((pred == y).mean())


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    torch.set_num_threads(1)
    rec = {"meta/seed": np.int64(SEED), "meta/ns": np.array(NS), "meta/cs": np.array(CS)}
    k = 0
    for N in NS:
        for C in CS:
            G = f"N{N}_C{C}"
            g = torch.Generator().manual_seed(SEED + 100 * k)
            x = torch.randn(N, C, generator=g) * 3
            x[torch.arange(N) % 9 == 4] *= 12                      # a few rows with logits near +-100: the max shift matters
            y = torch.randint(0, C, (N,), generator=g)
            ii = 1 if k % 3 == 2 else -100                         # ignore_index of a real class, or torch's default
            if ii == -100:
                y[torch.arange(N) % 7 == 3] = -100
            elif N == 1:
                y[0] = 0
            y = y.to(torch.int32 if k % 2 else torch.int64)
            w = torch.rand(N, generator=g) * 2 - 0.5
            gs = torch.rand((), generator=g) + 0.5
            rec.update({f"cls/{G}/logits": x.numpy(), f"cls/{G}/labels": y.numpy(), f"cls/{G}/ignore_index": np.int64(ii),
                        f"cls/{G}/w": w.numpy(), f"cls/{G}/gs": gs.numpy()})
            for s in SS:
                for red in REDUCTIONS:
                    xd = x.double().requires_grad_(True)
                    loss = F.cross_entropy(xd, y.long(), ignore_index=ii, reduction=red, label_smoothing=s)
                    (loss * (w.double() if red == "none" else gs.double())).sum().backward()
                    key = f"cls/{G}/s{s:g}/{red}"
                    rec[key + "/loss"] = loss.detach().numpy()
                    if red != "sum" or N * C <= DX_SUM_MAX:
                        rec[key + "/dx"] = xd.grad.numpy().astype(np.float32)
                    assert np.isfinite(rec[key + "/loss"]).all(), key
            # metrics: the same logits with labels in range, and integer-valued scores (class C - 1 absent when C = 5)
            ym = torch.randint(0, C, (N,), generator=g).numpy()
            metrics_ref(rec, f"met/{G}/f", x.numpy(), ym)
            si = torch.randint(-3, 4, (N, C), generator=g).to(torch.int8).numpy()
            yi = torch.randint(0, C - 1 if C == 5 else C, (N,), generator=g).numpy()
            rec[f"met/{G}/i/scores"] = si
            metrics_ref(rec, f"met/{G}/i", si.astype(np.float32), yi)
            k += 1
    g = torch.Generator().manual_seed(SEED - 1)
    sn = torch.randint(-2, 3, (16, 5), generator=g).float().numpy()
    sn[3, 2] = np.nan
    yn = torch.randint(0, 4, (16,), generator=g).numpy()
    yn[3], yn[5] = 2, 0
    rec["met/nan/scores"] = sn
    metrics_ref(rec, "met/nan", sn, yn)
    assert np.isnan(rec["met/nan/auroc"][2]) and rec["met/nan/auroc"][4] == 0.5
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {len(rec)} arrays, {os.path.getsize(args.out) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
