"""GPU: the fused RNA Block (mh_rna_block_fwd / mh_rna_block_bwd, csrc/rna_block.hip) through functional.rna_block against the
emulating f64 reference of tests/rna_block_ref.py — the same operation with the kernels' rounding points and the host Philox
masks — at the geometry edges of the file, in eval and in train mode.

Shapes (B, D, H, Hh), each the smallest that reaches its path:
  (1, 32, 8, 32)                       one k-step (three of the four split-K waves idle), a single row
  (15 / 16 / 17 / 31 / 32, 96, 12, 192) the MT = 1 / 2 boundary; the second row tile with one live row and min(m, B - 1) clamped loads
  (5, 64, 8, 128) without a qkv bias   b_qkv = NULL
  (4, 1024, 8, 1024)                   the QPL = 4 instances; the qkv data gradient at M = 3072: two chunks, the second clamped
  (16, 256, 8, 4096)                   K = 4096: two non-LayerNorm chunks, four trips of the s += 32 loop; fc1 data gradient at M = 4096
  (2, 1632, 17, 64), (17, 768, 12, 1536) the largest D the admission rule takes per row tile (H = 17 and 12: mh_headattn takes any
                                       H <= 64 that divides D, and 1632 = 2^5 3 17 offers an odd head count, hd = 96)
  (16, 512, 8, 2048)                   the workload's own Block

Bound.  Per case, dropout mode and tensor: 4 x floor in both measures (relative Frobenius error; max-abs error over max |ref|).  The
floor is the distance between the reference in f64 and the same emulation in f32 arithmetic with another summation order, i.e. what
another draw of the bf16 rounding-boundary flips costs, measured on the CPU over many redraws of the inputs (rna_block_ref.floor_draws)
and recorded in tests/golden/rna_block_floors.json; never under 2^-20 (device rsqrt / exp / erf are not correctly rounded).  The margin
of 4 is the issue's: the kernels' 4-wave split-K and MFMA order are one more draw of the same flips.  test_rna_block_ref_cpu.py measures
the floors again and shows that eight mutations of the reference (a bias gradient short of a row, mask2 missing from GELU', a dW strip
left at zero, ...) all land outside these bounds.  Recorded floors, Frobenius / max-abs, the smallest .. the largest over the eleven
cases above one row (eval mode and p = 0.1; the bound is four times these):

    y          2.3e-4 .. 1.0e-3 / 7.0e-4 .. 1.9e-3        stats         4.4e-6 .. 7.0e-5 / 1.8e-5 .. 3.2e-4
    u, f       3.8e-4 .. 1.7e-3 / 1.4e-3 .. 7.1e-3        dx            4.4e-4 .. 1.9e-3 / 1.6e-3 .. 3.3e-3
    dw_*       2.9e-4 .. 3.2e-3 / 1.3e-3 .. 8.3e-3        db_qkv, db_proj, db_fc1  3.2e-4 .. 3.2e-3 / 7.7e-4 .. 4.9e-3
    dg*, dbe*  3.1e-4 .. 3.2e-3 / 3.1e-4 .. 3.4e-3        db_fc2        2^-20 (a column sum of bf16 values: exact in f32 here)

At (1, 32, 8, 32) no bf16 rounding flipped in 128 draws of the eval mode (raw distances around 1e-7) and a few did at p = 0.1 (up to
6e-5): that case is held to 4 x 2^-20 = 3.8e-6 almost throughout.  The largest Frobenius floor is 3.2e-3 (db_qkv at B = 2, D = 1632: a
column sum of two bf16 values), so the widest bound is 1.3e-2; from 15 rows on it is 8.0e-3.  The band of test_rna_block_gpu.py
(cosine > 0.995, norm within 3 %) lets a relative error of about 0.1 through.  Measured on an MI355X when this file was written, the
kernels' distances were at most 0.54 of their bound (f at (2, 1632, 17, 64), p = 0.1) and 0.008 of it in the median.
"""
import functools
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

from mirror_amd import MirrorHipError, functional as Fn, kernels as K  # noqa: E402
from tests import rna_block_ref as R  # noqa: E402

mm = importlib.import_module("mirror_amd.models.mirror")
PREC = Fn.POLICIES["bf16"]
SEED = 0x51C0FFEE


@pytest.fixture(autouse=True)
def _dropout_state_restored():
    yield
    Fn.set_grad_sink(None)
    Fn.dropout_device_base_off()
    Fn.manual_seed(0x5EED)


def _block(case, p, P):
    B, D, H, Hh, qkv_bias = case
    blk = mm.Block(D, H, (Hh + 0.5) / D, qkv_bias, p, 1e-6)
    assert blk.mlp.fc1.weight.shape[0] == Hh
    with torch.no_grad():
        for name, prm in blk.named_parameters():
            prm.copy_(P[R.MODULE_NAMES[name]])
    return blk.to(DEV)


@functools.lru_cache(maxsize=None)
def _case(case, seed=0):
    return R.make_case(*case, seed=seed)


@functools.lru_cache(maxsize=None)
def _ref(case, p, offset, base=None, seed=0):
    x, dy, P = _case(case, seed)
    return R.block(x, dy, P, case[2], p=p, seed=SEED, offset=offset, base=base)


def _arm(offset, base=None, dev=None):
    Fn.manual_seed(SEED)
    if base is None:
        Fn.dropout_device_base_off()
    else:                                   # the engine's protocol: a per-step base on the device, host offsets on top of it
        Fn.dropout_step_begin(dev)
        Fn._dropout_state["base"].fill_(base)
    Fn._dropout_state["offset"] = offset


def _fused(blk, x, training):
    blk.train(training)
    xg = x.to(DEV).requires_grad_(True)
    y = Fn.rna_block(xg, blk, PREC, training)
    assert y is not None, "the fused path did not take this geometry"
    return xg, y, dict(y.grad_fn.saved)


def _compare(got, ref, bd, names, tag):
    bad = []
    for k in names:
        a, b = R.dist(got[k], ref[k])
        print("%s %-8s fro %.2e (bound %.2e)  max %.2e (bound %.2e)" % (tag, k, a, bd[k][0], b, bd[k][1]))
        if not (a <= bd[k][0] and b <= bd[k][1]):
            bad.append((k, a, b, bd[k]))
    assert not bad, (tag, bad)


def _grads(blk, xg):
    got = {"dx": xg.grad}
    for name, prm in blk.named_parameters():
        got[R.GRAD_OF[R.MODULE_NAMES[name]]] = prm.grad
    return got


def _one(case, p, offset, base=None):
    B, D, H, Hh, qkv_bias = case
    x, dy, P = _case(case)
    blk = _block(case, max(p, 0.1), P)          # eval mode runs a Block that has dropout configured, as the model's does
    _arm(offset, base, torch.device("cuda", torch.cuda.current_device()))
    xg, y, saved = _fused(blk, x, p > 0.0)
    if p > 0.0:
        assert Fn._dropout_state["offset"] == offset + 2 * B * D + B * Hh
    y.backward(dy.to(DEV))
    ref, bd = _ref(case, p, offset, base), R.bound(*case, p=p)
    got = _grads(blk, xg)
    got.update(y=y, stats=saved["stats"], u=saved["u"], f=saved["f"])
    assert ("db_qkv" in got) == qkv_bias
    _compare(got, ref, bd, [k for k in R.CHECKED if k in ref], "%s p=%g" % (R.case_key(*case), p))


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: R.case_key(*c))
def test_eval_mode_matches_the_emulating_reference(case):
    _one(case, 0.0, 0)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: R.case_key(*c))
def test_train_mode_matches_the_reference_under_the_host_philox_masks(case):
    _one(case, 0.1, 40)                      # not at the start of the stream


@pytest.mark.parametrize("case", R.P50_CASES, ids=lambda c: R.case_key(*c))
def test_train_mode_at_p_one_half(case):
    _one(case, 0.5, 12)


def test_train_mode_under_a_device_side_base():
    """The base lives on the device (dropout_step_begin) and the kernels add it themselves, in both directions."""
    _one((31, 96, 12, 192, True), 0.1, 16, base=80)


class _Sink:
    """A gradient sink as TrainEngine installs one: the kernels accumulate straight into these buffers."""

    def __init__(self, blk):
        self.buf = {p.data_ptr(): torch.zeros_like(p, dtype=torch.float32) for p in blk.parameters()}

    def slot(self, t):
        return self.buf.get(t.data_ptr())

    def done(self, t):
        pass


@pytest.mark.parametrize("case", [(16, 96, 12, 192, True), (17, 96, 12, 192, True)], ids=lambda c: R.case_key(*c))
def test_gradients_accumulate_into_buffers_that_are_not_zero(case):
    """Two forward + backward passes into the same gradient buffers (dw_*, db_*, dg*, dbe* are `+=` in the kernels), with different
    dy and dropout offsets: every parameter gradient is the sum of the two references.  The two passes' errors are independent
    draws, so the sum is held to the bound of one pass."""
    x, _, P = _case(case)
    blk = _block(case, 0.1, P)
    sink = _Sink(blk)
    Fn.set_grad_sink(sink)
    total, bd = {}, R.bound(*case, p=0.1)
    for i, offset in enumerate((40, 4000)):
        dy = _case(case, seed=1 + i)[1]
        _arm(offset)
        xg, y, _ = _fused(blk, x, True)
        y.backward(dy.to(DEV))
        ref = R.block(x, dy, P, case[2], p=0.1, seed=SEED, offset=offset)
        _compare({"dx": xg.grad}, ref, bd, ["dx"], "pass %d" % i)
        for k in R.GRAD_OF.values():
            total[k] = total.get(k, 0) + ref[k]
    assert all(p.grad is None for p in blk.parameters())          # everything went through the sink
    got = {R.GRAD_OF[R.MODULE_NAMES[n]]: sink.buf[p.data_ptr()] for n, p in blk.named_parameters()}
    _compare(got, total, bd, sorted(got), "sum of two passes")


@pytest.mark.parametrize("case", [(32, 1024, 8, 2048, True), (2, 2048, 8, 64, True)], ids=lambda c: R.case_key(*c))
def test_geometries_whose_qkv_data_gradient_does_not_fit_fall_back_and_still_train(case):
    """Both passed the old admission rule, ran their forward and failed in the fourth backward launch after the first three had
    accumulated.  Now functional.rna_block declines them and Block.forward trains through the composed ops: checked against the
    exact f64 Block (same host masks: the composed dropouts draw the same stream at the same offsets) within the band the
    composed path is held to in test_rna_block_gpu.py."""
    B, D, H, Hh, _ = case
    x, dy, P = _case(case)
    blk = _block(case, 0.1, P).train()
    _arm(40)
    assert Fn.rna_block(x.to(DEV), blk, PREC, True) is None
    assert Fn._dropout_state["offset"] == 40
    params = {k: v if v is None else (v.to(DEV).bfloat16() if k.startswith("w_") else v.to(DEV)) for k, v in P.items()}
    with pytest.raises(MirrorHipError, match="LDS budget"):          # the entry point itself refuses before it launches anything
        K.rna_block_fwd(x.to(DEV), params, H, 1e-6, 0.0, 0, 0, None)
    xg = x.to(DEV).requires_grad_(True)
    y = blk(xg, PREC)
    y.backward(dy.to(DEV))
    assert Fn._dropout_state["offset"] == 40 + 2 * B * D + B * Hh
    ref = R.block(x, dy, P, H, p=0.1, seed=SEED, offset=40, emulate=False)
    assert R.dist(y, ref["y"])[1] < 2e-2
    for k, g in _grads(blk, xg).items():
        a, b = g.detach().double().cpu().reshape(-1), ref[k].reshape(-1)
        cos, ratio = float(torch.dot(a, b) / (a.norm() * b.norm())), float(a.norm() / b.norm())
        print("%s %-8s cos %.5f ratio %.4f" % (R.case_key(*case), k, cos, ratio))
        assert cos > 0.995 and 0.97 < ratio < 1.03, (k, cos, ratio)
