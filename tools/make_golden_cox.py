"""Generate tests/golden/golden_cox.npz from the grouped (per distinct event time) f64 statement of the Cox partial likelihood in
tests/cox_ref.py, and the log-rank statistics of the same inputs split at the median score.

    python tools/make_golden_cox.py

Layout (G = "N{N}_{times}"; T = "breslow" / "efron"; R = "none" / "sum" / "mean" / "batch"):
  {G}/r, /t, /c            inputs: scores f32, times f64, censoring int64 (1 = event)
  {G}/{T}/rows             f64 [N]: the per-row losses ("none")
  {G}/{T}/reduced          f64 [3]: the "sum", "mean" and "batch" losses
  {G}/{T}/grad             f64 [4, N]: d loss / d r for "none", "sum", "mean", "batch" and an upstream gradient of ones
  {G}/logrank              f64 [6] = {chi2, p, O1, E1, V, n_events} for group = r > median(r)
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import cox_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "golden_cox.npz")
CASES = ((1, "distinct"), (2, "ties"), (7, "equal"), (12, "distinct"), (24, "ties"))
SEED = 4100


def build() -> dict:
    rec = {"meta/seed": np.int64(SEED)}
    for k, (N, times) in enumerate(CASES):
        G = f"N{N}_{times}"
        r, t, c = R.make_case(N, times, 0.6, "n1", SEED + k)
        rec[f"{G}/r"], rec[f"{G}/t"], rec[f"{G}/c"] = r, t, c
        for ties in R.TIES:
            res = [R.cox_grouped(r, t, c, ties, red) for red in R.REDUCTIONS]
            rec[f"{G}/{ties}/rows"] = res[0][0]
            rec[f"{G}/{ties}/reduced"] = np.array([x[0] for x in res[1:]], np.float64)
            rec[f"{G}/{ties}/grad"] = np.stack([x[1] for x in res])
        rec[f"{G}/logrank"] = np.array(R.logrank(c == 1, t, r > np.median(r)), np.float64)
    return rec


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    rec = build()
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {len(rec)} arrays, {os.path.getsize(args.out) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
