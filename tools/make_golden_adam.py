"""Record tests/golden/golden_adam_bits.npz: what mh_adam and mh_adam_ema compute, bit for bit.

Run it on an MI355X against the library whose bits are to be pinned.  The committed fixture was recorded from the build of the last
commit that kept mh_adam in a device body of its own (loss.hip), selected with MIRROR_HIP_LIB:

    MIRROR_HIP_LIB=/path/to/that/libmirror_hip.so python tools/make_golden_adam.py

tests/test_adam_bits_gpu.py replays the same launches (`replay` below) on the tree's own library and asks for torch.equal.

N = 2051 elements: live quads on both sides of the hole [512, 1024) and a 3-element scalar tail.  Three updates per case: one launch,
then a two-launch step (tick="early" over the hole's range, then tick=False around the hole), then one launch.
  a    mh_adam with the device step state: grad_scale 0.5, clip factor 0.5 in state[4], the counter, the shadow,
       the clamped element in a live quad (index 8)
  b    mh_adam_ema: the same, plus the EMA (warm-up decay schedule)
  c    mh_adam with host-side lr / bias corrections (dev_state NULL), no shadow, the clamped element in the tail (index 2049)
Layout: p0, g (3 x N), e0, ema_cfg (the six EmaCfg fields as f64): the inputs, shared by the cases;
{case}/p, /m, /v, /counter, and where the case has them /shadow (the bf16 bits as int16), /state, /ema: the results.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "golden_adam_bits.npz")

N = 2051
HOLE = (512, 1024)
CASES = {"a": 8, "b": 8, "c": 2049}          # case -> index of the clamped element
LR, B1, B2, EPS, GS, CLIP = 1e-2, 0.9, 0.999, 1e-8, 0.5, 0.5
CLAMP_LO, CLAMP_HI = 0.0, math.log(100.0)
EMA_CFG = (0.999, 0.0, 1.0, 2.0 / 3.0, 0, 1)


def inputs() -> dict:
    gen = torch.Generator().manual_seed(2051)
    p0 = torch.randn(N, generator=gen)
    g = torch.randn(3, N, generator=gen)
    p0[[8, 2049]] = 7.0                      # above ln 100, and a negative gradient keeps pushing up: the clamp bites at every step
    g[:, [8, 2049]] = -1.0
    return {"p0": p0.numpy(), "g": g.numpy(), "e0": torch.randn(N, generator=gen).numpy(),
            "ema_cfg": np.array(EMA_CFG, dtype=np.float64)}


def replay(z, case: str) -> dict:
    """The case's three updates on the loaded library, from the inputs in `z`; the results as CPU tensors."""
    from mirror_amd import kernels as K
    from mirror_amd._lib import EmaCfg
    dev = "cuda"
    p = torch.from_numpy(np.array(z["p0"])).to(dev)
    gs = [torch.from_numpy(np.array(r)).to(dev) for r in z["g"]]      # one allocation each: rows of [3, N] are not 16-byte aligned
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    host = case == "c"
    sh = None if host else torch.zeros(N, device=dev, dtype=torch.bfloat16)
    st = None if host else torch.tensor([0.0, 0.0, 0.0, LR, CLIP, 0.0], device=dev)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    if case == "b":
        c = z["ema_cfg"]
        e = torch.from_numpy(np.array(z["e0"])).to(dev)
        ecfg = EmaCfg(float(c[0]), float(c[1]), float(c[2]), float(c[3]), int(c[4]), int(c[5]))
    clamp = (CASES[case], CLAMP_LO, CLAMP_HI)
    lo, hi = HOLE

    def launch(t, a, b, **more):
        if case == "b":
            more.update(ema=e[a:b], ema_cfg=ecfg)
        bc1, bc2 = (1.0 - B1 ** t, 1.0 - B2 ** t) if host else (1.0, 1.0)
        K.adam(p[a:b], gs[t - 1][a:b], m[a:b], v[a:b], None if sh is None else sh[a:b], LR if host else 0.0, B1, B2, EPS, bc1, bc2,
               grad_scale=GS, dev_state=st, **more)
    launch(1, 0, N, clamp=clamp, counter=ctr, counter_add=5)
    launch(2, lo, hi, tick="early")
    launch(2, 0, N, clamp=clamp, counter=ctr, counter_add=5, tick=False, hole=HOLE)
    launch(3, 0, N, clamp=clamp, counter=ctr, counter_add=5)
    torch.cuda.synchronize()
    out = {"p": p, "m": m, "v": v, "counter": ctr}
    if not host:
        out.update(shadow=sh.view(torch.int16), state=st)
    if case == "b":
        out["ema"] = e
    return {k: t.cpu() for k, t in out.items()}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    from mirror_amd import _lib
    z = inputs()
    for case in CASES:
        for k, t in replay(z, case).items():
            z[f"{case}/{k}"] = t.numpy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **z)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes) from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
