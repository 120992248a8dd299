"""MI355X: mh_mse_masked_fwd_ordered (csrc/loss.hip) behind kernels.mse_masked_fwd: the masked-MSE accumulator of the retention
losses with its blocks' partial sums added in block order.  The same inputs give the same bits on every launch (the float atomics
of mh_mse_masked_fwd do not: a validation loss moved by an ulp between two validate() calls), and the sums agree with float64 to
the f32 summation error: rows / 256 * 2^-24 relative is the bound of adding up to 1024 partial sums of like sign in f32, with the
in-block sums (256 threads, a few rows each) inside the same bound."""
import numpy as np
import pytest
import torch

from mirror_amd import kernels as K

pytestmark = pytest.mark.gpu

# rows x D: more rows than 16 * 1024 (every one of the 1024 blocks works), a ragged small case, and the flat D = 1 kernel
CASES = [(20000, 64, torch.float32), (20000, 64, torch.bfloat16), (243, 40, torch.float32), (50000, 1, torch.float32)]


@pytest.mark.parametrize("rows,D,dtype", CASES)
def test_masked_mse_accumulator_is_bit_reproducible_and_close_to_float64(rows, D, dtype):
    g = torch.Generator().manual_seed(rows + D)
    pred = torch.randn(rows, D, generator=g).to(dtype).cuda()
    tgt = torch.randn(rows, D, generator=g).cuda()
    mask = (torch.rand(rows, generator=g) < 0.6).float().cuda()
    outs = []
    for _ in range(12):
        acc = torch.zeros(2, device="cuda")
        K.mse_masked_fwd(pred, tgt, mask, acc, rows, D)
        outs.append(acc)
    got = torch.stack(outs).cpu()
    assert (got == got[0]).all(), got[:, 0].tolist()          # every launch: the same bits
    d = pred.double().cpu() - tgt.double().cpu()
    m = mask.double().cpu()
    num, den = float((m * (d * d).mean(1)).sum()), float(m.sum())
    assert float(got[0, 1]) == den                            # a count: exact
    tol = max(rows / 256, 8) * 2.0 ** -24
    print(f"rows {rows} D {D} {dtype}: num {float(got[0, 0])!r} vs {num!r}, rel {abs(float(got[0, 0]) - num) / num:.2e}, bound {tol:.2e}")
    assert abs(float(got[0, 0]) - num) <= tol * num
    acc = torch.full((2,), 3.0, device="cuda")                # += onto what acc holds
    K.mse_masked_fwd(pred, tgt, mask, acc, rows, D)
    assert float(acc[1]) == den + 3.0 and abs(float(acc[0]) - 3.0 - num) <= tol * (num + 3.0)
