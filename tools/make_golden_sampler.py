"""Generate tests/golden/golden_sampler.npz by running the REFERENCE class-balanced sampler itself.

`utils/loader.py` of a reference MIRROR checkout is pure torch: it is imported by path, unmodified, and handed a tiny dataset that
offers what `class_balanced_sampler` reads (`slide_cls_ids`, `get_label`, `__len__`; dataset_survival.py:81-84, :276).  Nothing from the
reference is copied: the fixture holds the labels fed in and the weights its WeightedRandomSampler was built with.

    python tools/make_golden_sampler.py --reference /path/to/MIRROR

Layout:  labels int64 [80] (class sizes 50 / 7 / 20 / 3, class after class), weights float64 [80], num_samples int64.
"""
from __future__ import annotations

import argparse
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "golden_sampler.npz")
CLASS_SIZES = (50, 7, 20, 3)


class TinyDataset:
    def __init__(self, labels):
        self.labels = labels
        self.slide_cls_ids = [np.where(labels == c)[0] for c in range(len(CLASS_SIZES))]

    def __len__(self):
        return len(self.labels)

    def get_label(self, idx):
        return int(self.labels[idx])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_utils_loader", os.path.join(args.reference, "utils", "loader.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    labels = np.repeat(np.arange(len(CLASS_SIZES)), CLASS_SIZES).astype(np.int64)
    sampler = mod.class_balanced_sampler(TinyDataset(labels))
    assert sampler.replacement
    np.savez(OUT, labels=labels, weights=sampler.weights.numpy().astype(np.float64), num_samples=np.int64(sampler.num_samples))
    print(f"wrote {OUT}: {len(labels)} labels, weights {sorted(set(sampler.weights.tolist()))}")


if __name__ == "__main__":
    main()
