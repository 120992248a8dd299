"""InfoNCE with explicit negative keys on the GPU (mirror_amd/csrc/infonce.hip) against the f64 fixture and the f64 restatement
of tests/test_infonce_neg_cpu.py (`nce_ref`).

Bounds: loss rtol 1e-4 / atol 1e-6, gradients rtol 2e-3 / atol 2e-6 — this class's own bounds (tests/test_model_gpu.py:266-269).
At the generated sizes a gradient entry is a mean over N rows of a softmax weight over up to 65537 columns, far below 2e-6 in
absolute terms, so there the absolute part is scaled by max|reference gradient| as tests/test_model_gpu.py:251-252 does.
"""

import numpy as np
import pytest
import torch

from mirror_amd import functional as Fn
from mirror_amd.losses import InfoNCE
from tests.test_infonce_neg_cpu import GOLDEN, MODES, REDUCTIONS, TEMPERATURES, nce_ref_grads

pytestmark = pytest.mark.gpu

LOSS_TOL = dict(rtol=1e-4, atol=1e-6)
GRAD_RTOL, GRAD_ATOL = 2e-3, 2e-6
NAMES = ("loss", "dquery", "dpositive_key", "dnegative_keys")


def run(q, k, n, temperature, reduction, mode, w=None, symmetric=False, grads=(True, True, True)):
    """(loss, dq, dk, dn) of the build; a gradient is None where it was not asked for."""
    q, k, n = (x.detach().clone().requires_grad_(r) for x, r in zip((q, k, n), grads))
    loss = InfoNCE(temperature=temperature, reduction=reduction, negative_mode=mode, symmetric=symmetric)(q, k, n)
    ((loss * w).sum() if reduction == "none" else loss).backward()
    return loss.detach(), q.grad, k.grad, n.grad


def check(got, want, scaled_atol=None, what=""):
    """scaled_atol: None = the plain bounds; "tensor" = atol times max|reference| of the tensor; "row" = times max|reference| of
    each last-dim row (used where single rows are O(1 / eps) and must not loosen the others)."""
    for g, r, nm in zip(got, want, NAMES):
        g, r = g.detach().double().cpu().numpy(), r.detach().double().cpu().numpy()
        assert g.shape == r.shape and np.isfinite(g).all(), (what, nm)
        if nm == "loss":
            rtol, atol = LOSS_TOL["rtol"], LOSS_TOL["atol"]
        else:
            rtol, atol = GRAD_RTOL, GRAD_ATOL
            if scaled_atol == "tensor":
                atol = atol * float(np.abs(r).max())
            elif scaled_atol == "row":
                atol = atol * np.abs(r).max(axis=-1, keepdims=True)
        over = np.abs(g - r) - rtol * np.abs(r) - atol
        print(f"{what} {nm}: max|ref| {np.abs(r).max():.3e} max abs err {np.abs(g - r).max():.3e} worst (err - rtol|ref| - atol) {over.max():.3e}")
        assert (over <= 0).all(), f"{what} {nm}: {int((over > 0).sum())} of {over.size} entries out of bounds, worst by {over.max():.3e}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("reduction", REDUCTIONS)
def test_matches_f64_fixture(mode, reduction):
    z = np.load(GOLDEN)
    q, k, n, w = (torch.from_numpy(z[f"{mode}/{nm}"]).float().cuda() for nm in ("query", "positive_key", "negative_keys", "w"))
    for t in TEMPERATURES:
        got = run(q, k, n, t, reduction, mode, w)
        assert got[0].dtype == torch.float32 and got[0].shape == (() if reduction != "none" else (q.shape[0],))
        want = [torch.from_numpy(z[f"{mode}/t{t}/{reduction}/{nm}"]) for nm in NAMES]
        check(got, want, what=f"fixture {mode} t{t} {reduction}")


def _case(mode, N, M, D, seed, dtype=torch.float32):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn(N, D, device="cuda", generator=g)
    k = 0.8 * q + 0.6 * torch.randn(N, D, device="cuda", generator=g)
    shape = (M, D) if mode == "unpaired" else (N, M, D)
    n = torch.randn(*shape, device="cuda", generator=g) * (0.1 + 4.0 * torch.rand(*shape[:-1], 1, device="cuda", generator=g))
    w = torch.rand(N, device="cuda", generator=g) * 2 - 0.5
    return q, k, n.to(dtype), w


@pytest.mark.parametrize("mode, N, M, D", [
    ("paired", 16, 4096, 768), ("paired", 256, 1024, 512), ("paired", 5, 37, 100),
    ("unpaired", 256, 65536, 512), ("unpaired", 7, 1000, 96)])
@pytest.mark.parametrize("reduction", ["mean", "none"])
def test_generated_sizes_match_f64_restatement(mode, N, M, D, reduction):
    q, k, n, w = _case(mode, N, M, D, seed=N + M + D)
    got = run(q, k, n, 0.07, reduction, mode, w)
    want = nce_ref_grads(q.double(), k.double(), n.double(), 0.07, reduction, mode, w.double())
    check(got, want, scaled_atol="tensor", what=f"{mode} {N}x{M}x{D} {reduction}")


@pytest.mark.parametrize("mode, N, M, D", [("paired", 16, 512, 768), ("paired", 5, 37, 100), ("unpaired", 64, 4096, 512),
                                           ("unpaired", 7, 1000, 96)])
def test_bf16_negatives_read_in_place(mode, N, M, D):
    """The restatement is evaluated on the bf16-rounded negatives (upcast exactly).  Loss and the f32 gradients keep the f32
    bounds; d negative_keys comes back in bf16, i.e. the f32 result rounded once: half a bf16 ulp (2^-9 relative) on top of them."""
    q, k, n, w = _case(mode, N, M, D, seed=3 * N + M, dtype=torch.bfloat16)
    got = run(q, k, n, 0.1, "mean", mode)
    assert got[3].dtype == torch.bfloat16
    want = nce_ref_grads(q.double(), k.double(), n.double(), 0.1, "mean", mode)
    check(got[:3], want[:3], scaled_atol="tensor", what=f"bf16 {mode} {N}x{M}x{D}")
    g, r = got[3].double().cpu().numpy(), want[3].cpu().numpy()
    err = np.abs(g - r)
    print(f"bf16 {mode} dnegative_keys: max|ref| {np.abs(r).max():.3e} max rel err {np.max(err / np.maximum(np.abs(r), 1e-300)):.3e}")
    np.testing.assert_allclose(g, r, rtol=GRAD_RTOL + 2.0 ** -9, atol=GRAD_ATOL * float(np.abs(r).max()))
    # and the f32 path on the same (upcast) values gives the gradient this one rounds
    got32 = run(q, k, n.float(), 0.1, "mean", mode)
    assert torch.equal(got32[0], got[0])
    np.testing.assert_allclose(got[3].float().cpu().numpy(), got32[3].cpu().numpy(), rtol=2.0 ** -8, atol=GRAD_ATOL * float(np.abs(r).max()))


@pytest.mark.parametrize("mode", MODES)
def test_zero_rows_follow_the_eps_rule(mode):
    """A zero negative row normalises to zero (x / max(|x|, 1e-12)): cosine 0, finite gradient q^ dl / 1e-12; a zero query gives
    all-zero logits, loss log(1 + M)."""
    q, k, n, w = _case(mode, 6, 20, 64, seed=11)
    if mode == "unpaired":
        n[3] = 0
    else:
        n[2, 5] = 0
    q[4] = 0
    for reduction in ("mean", "none"):
        got = run(q, k, n, 0.2, reduction, mode, w)
        want = nce_ref_grads(q.double(), k.double(), n.double(), 0.2, reduction, mode, w.double())
        assert all(torch.isfinite(x).all() for x in got)
        # gradients of the zero rows are O(1 / eps): the absolute part scales with each row's own largest reference entry
        check(got, want, scaled_atol="row", what=f"zero rows {mode} {reduction}")
    rows = run(q, k, n, 0.2, "none", mode, w)[0]
    np.testing.assert_allclose(float(rows[4]), np.log(21.0), rtol=1e-6)


@pytest.mark.parametrize("mode", MODES)
def test_negatives_without_grad_cost_no_pass_over_them(mode):
    q, k, n, w = _case(mode, 8, 300, 128, seed=5)
    full = run(q, k, n, 0.1, "mean", mode)
    Fn.infonce_launches = tap = []
    try:
        got = run(q, k, n, 0.1, "mean", mode, grads=(True, True, False))
    finally:
        Fn.infonce_launches = None
    assert got[3] is None
    for a, b in zip(got[:3], full[:3]):
        assert torch.equal(a, b)
    wrote = ",".join(w_ for _, w_ in tap)
    assert tap and "dneg" not in wrote and "dbank" not in wrote and "dn^" not in wrote, tap
    if mode == "paired":
        assert ("mh_infonce_paired_bwd", "dq_part[N,chunks,D]") in tap          # one read of the negatives, no [N, M, D] write
    # nothing needs a gradient but the positive key: no launch touches the negatives in the backward at all
    Fn.infonce_launches = tap = []
    try:
        only_k = run(q, k, n, 0.1, "mean", mode, grads=(False, True, False))
    finally:
        Fn.infonce_launches = None
    assert only_k[1] is None and only_k[2] is not None and only_k[3] is None
    assert torch.equal(only_k[2], full[2])
    assert not [t for t in tap if t[0] in ("mh_infonce_paired_bwd", "mh_l2norm_bwd") or t[1] in ("dq_part[N,S,D]", "dn^[M,D]")], tap
    # and with the tap on a full backward, the [N, M, D] write is there (the tap sees what it claims to see)
    Fn.infonce_launches = tap = []
    try:
        run(q, k, n, 0.1, "mean", mode)
    finally:
        Fn.infonce_launches = None
    assert any("dneg[N,M,D]" in t[1] or "dbank[M,D]" in t[1] for t in tap), tap


@pytest.mark.parametrize("mode", MODES)
def test_symmetric_is_ignored_with_negatives(mode):
    q, k, n, w = _case(mode, 9, 50, 72, seed=21)
    a = run(q, k, n, 0.1, "sum", mode, symmetric=False)
    b = run(q, k, n, 0.1, "sum", mode, symmetric=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("mode, N, M, D", [("paired", 16, 700, 256), ("unpaired", 32, 3000, 256)])
def test_deterministic_and_graph_capturable(mode, N, M, D):
    q, k, n, w = _case(mode, N, M, D, seed=31)

    def step(q_, k_, n_):
        return run(q_, k_, n_, 0.1, "mean", mode)

    r1, r2 = step(q, k, n), step(q, k, n)
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)
    sq, sk, sn = q.clone(), k.clone(), n.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(sq, sk, sn)                                 # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = step(sq, sk, sn)
    sq.copy_(q * 0.5 + 0.1)
    sn.copy_(n * 0.7 - 0.05)
    g.replay()
    torch.cuda.synchronize()
    eager = step(q * 0.5 + 0.1, k, n * 0.7 - 0.05)
    for x, y in zip(captured, eager):
        assert torch.equal(x, y)
    sq.copy_(q)
    sn.copy_(n)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(captured, r1):
        assert torch.equal(x, y)


@pytest.mark.parametrize("symmetric", [False, True])
def test_implicit_negatives_path_repeats_bit_for_bit(symmetric):
    q, k, _, _ = _case("unpaired", 16, 4, 128, seed=41)

    def step():
        qq, kk = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
        loss = InfoNCE(temperature=0.1, symmetric=symmetric)(qq, kk)
        loss.backward()
        return loss.detach(), qq.grad, kk.grad

    for x, y in zip(step(), step()):
        assert torch.equal(x, y)
