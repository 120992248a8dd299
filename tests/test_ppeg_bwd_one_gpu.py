"""GPU: PPEG's backward in one pass (mh_ppeg_bwd) — data, filter and bias gradients from one read of dy and x, and layer 1's to_out
Dropout backward (masked bf16 gradient + its column sums) in the same launch.

Reference: torch on the CPU as in test_kernels_gpu.py::test_ppeg (three depthwise conv2d + identity, gradients from autograd), with
test_ppeg's tolerances.  The Dropout site is pinned bit for bit to K.dropout_lite of the kernel's own dx (models/mirror.py:312,
:324-331).  Shapes: (5, 64, 2) a grid smaller than the filter, every tap clipped; (9, 256, 3) ragged 4-pixel x-tiles, an odd batch;
(33, 64, 4) several strips with a short last one; (16, 512, 2) the workload's D, 8 channel blocks; (70, 64, 2) more than 64 rows;
(24, 2048, 6) enough workgroups that the host keeps ONE 24-row strip: 30 row steps, so the 14-step unrolled walk wraps twice (the small
grids above are cut into strips of 5-8 rows, 11-14 steps), and the largest D the Dropout site takes."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

bf16, f32 = torch.bfloat16, torch.float32
SHAPES = [(5, 64, 2), (9, 256, 3), (33, 64, 4), (16, 512, 2), (70, 64, 2), (24, 2048, 6)]
_cache = {}


def _case(S, D, B):
    """Inputs, the CPU reference gradients and one run of the kernel with a Dropout site — computed once per shape and left unchanged."""
    key = (S, D, B)
    if key in _cache:
        return _cache[key]
    from mirror_amd import kernels as K
    gen = torch.Generator().manual_seed(1000 + S)
    x = torch.randn(B, 1 + S * S, D, generator=gen)
    ws = [torch.randn(D, 1, k, k, generator=gen) * 0.2 for k in (7, 5, 3)]
    bs = [torch.randn(D, generator=gen) * 0.1 for _ in range(3)]
    dy = torch.randn(B, 1 + S * S, D, generator=gen)
    xr = x.clone().requires_grad_(True)
    wr = [w.clone().requires_grad_(True) for w in ws]
    br = [b.clone().requires_grad_(True) for b in bs]
    grid = xr[:, 1:].transpose(1, 2).reshape(B, D, S, S)
    y = sum(F.conv2d(grid, wr[i], br[i], padding=(7 - 2 * i) // 2, groups=D) for i in range(3)) + grid
    torch.cat([xr[:, :1], y.flatten(2).transpose(1, 2)], dim=1).backward(dy)
    merged, bsum = K.ppeg_merge(*[w.cuda() for w in ws], *[b.cuda() for b in bs])
    xd, dyd = x.cuda(), dy.cuda()
    # plain form
    dm0, dbs0 = torch.zeros_like(merged), torch.zeros_like(bsum)
    dx0 = K.ppeg_bwd(xd, dyd, merged, dm0, dbs0, S)
    # with a Dropout site: p = 0.1, a call offset that is a non-zero multiple of 8, and a device-side base
    p, seed, offset = 0.1, 0x1234567, 4096 + 8 * S
    base = torch.tensor([80], dtype=torch.int64, device="cuda")
    dm1, dbs1 = torch.zeros_like(merged), torch.zeros_like(bsum)
    out = torch.full(xd.shape, float("nan"), device="cuda", dtype=bf16)
    db = torch.zeros(D, device="cuda")
    dx1 = K.ppeg_bwd(xd, dyd, merged, dm1, dbs1, S, drop=(out, p, seed, offset, base, db))
    want = K.dropout_lite(dx1, p, seed, offset, base, out=torch.empty_like(out))
    torch.cuda.synchronize()
    _cache[key] = dict(xg=xr.grad, wg=[w.grad[:, 0] for w in wr], bg=br[0].grad, plain=(dx0, dm0, dbs0), drop=(dx1, dm1, dbs1, out, db, want))
    return _cache[key]


def _close(got, ref, rtol, atol, what):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    print(f"{what}: max abs err {float(err.max()):.3e} (atol {atol:.3e}, rtol {rtol:.0e})")
    assert not bool(bad.any()), f"{what}: max abs err {float(err.max()):.3e} at tolerance {atol:.3e} + {rtol:.0e} |ref|"


def _wtol(terms):
    return 1e-3 * max(1.0, terms ** 0.5 / 100)      # f32 sums of `terms` unit-variance terms (test_ppeg)


@pytest.mark.parametrize("S,D,B", SHAPES)
@pytest.mark.parametrize("form", ["plain", "drop"])
def test_gradients_match_cpu_autograd(S, D, B, form):
    c = _case(S, D, B)
    dx, dm, dbs = c[form][:3]
    _close(dx, c["xg"], 1e-5, 1e-5, "dx")
    dm = dm.cpu().t().reshape(D, 7, 7)
    atol = _wtol(B * S * S)
    _close(dm, c["wg"][0], 1e-4, atol, "dw7")
    _close(dm[:, 1:6, 1:6], c["wg"][1], 1e-4, atol, "dw5")
    _close(dm[:, 2:5, 2:5], c["wg"][2], 1e-4, atol, "dw3")
    _close(dbs, c["bg"], 1e-4, atol, "dbsum")


@pytest.mark.parametrize("S,D,B", SHAPES)
def test_dropout_site_is_dropout_lite_of_the_kernels_own_dx(S, D, B):
    c = _case(S, D, B)
    dx1, _, _, out, db, want = c["drop"]
    assert torch.equal(dx1, c["plain"][0]), "the site does not change dx"
    assert torch.equal(out.view(torch.int16), want.view(torch.int16)), int((out.view(torch.int16) != want.view(torch.int16)).sum())
    zeros = float((want == 0).float().mean())
    assert 0.05 < zeros < 0.2, zeros
    _close(db, want.double().sum((0, 1)), 1e-4, _wtol(B * (1 + S * S)), "drop_db")


def _chain(fused, clone_between=False):
    """to_out + Dropout + residual add of a layer (ToOutDropAddFn) feeding PPEGFn at the smallest size the fused projection takes:
    S = 16 (257 rows per slide), 2 slides, D = 256."""
    from mirror_amd import functional as Fn
    S, Bn, D, Kd, r0 = 16, 2, 256, 64, 7
    R = 1 + S * S
    prec = Fn.POLICIES["bf16"]
    g = torch.Generator().manual_seed(5)
    core = torch.randn(Bn, r0 + R, Kd, generator=g).cuda().to(bf16).requires_grad_(True)
    resid = torch.randn(Bn, R, D, generator=g).cuda().requires_grad_(True)
    w = (torch.randn(D, Kd, generator=g) / Kd ** 0.5).cuda().requires_grad_(True)
    b = (torch.randn(D, generator=g) * 0.1).cuda().requires_grad_(True)
    cw = [(torch.randn(D, 1, k, k, generator=g) * 0.2).cuda().requires_grad_(True) for k in (7, 5, 3)]
    cb = [(torch.randn(D, generator=g) * 0.1).cuda().requires_grad_(True) for _ in range(3)]
    up = torch.randn(Bn, R, D, generator=g).cuda()
    Fn.manual_seed(77)
    Fn._dropout_state["offset"] = 4096
    seen = {}
    orig = Fn._linear_rows_bwd

    def spy(needs, x, wa, w_, b_, r0_, R_, prec_, dy, **kw):
        seen["gb"] = dy.detach().clone()
        return orig(needs, x, wa, w_, b_, r0_, R_, prec_, dy, **kw)

    tap = []
    Fn._handover_tap, Fn._linear_rows_bwd = tap, spy
    try:
        h = Fn.to_out_dropout_add(resid, core, w, b, r0, R, 0.1, True, prec)
        assert h.grad_fn.__class__.__name__.startswith("ToOutDropAddFn") and hasattr(h, "_drop_site")
        if not fused:
            del h._drop_site
        hin = h
        if clone_between:
            site = h._drop_site
            hin = h * 1.0              # PPEG's dx reaches the projection as ANOTHER tensor: the hand-over must be refused
            hin._drop_site = site
        y = Fn.PPEGFn.apply(hin, cw[0], cb[0], cw[1], cb[1], cw[2], cb[2], S)
        y.backward(up)
        torch.cuda.synchronize()
    finally:
        Fn._handover_tap, Fn._linear_rows_bwd = None, orig
    return dict(tap=tap, gb=seen["gb"], db=b.grad.clone(), dw=w.grad.clone(), dcore=core.grad.clone(), dresid=resid.grad.clone())


def test_site_through_ppegfn_and_to_out():
    a, c = _chain(True), _chain(False)
    assert a["tap"] == [("drop", "offered"), ("drop", "accepted")], a["tap"]
    assert c["tap"] == [], c["tap"]
    assert torch.equal(a["gb"].view(torch.int16), c["gb"].view(torch.int16)), "the bf16 gradient handed to to_out's products"
    assert torch.equal(a["dcore"], c["dcore"]) and torch.equal(a["dresid"], c["dresid"])
    rows = a["gb"].shape[0] * a["gb"].shape[1]
    _close(a["db"], c["db"], 1e-4, _wtol(rows), "to_out bias gradient")
    _close(a["dw"], c["dw"], 1e-4, _wtol(rows), "to_out weight gradient")
    r = _chain(True, clone_between=True)
    assert r["tap"] == [("drop", "offered"), ("drop", "rejected")], r["tap"]
    assert torch.equal(r["gb"].view(torch.int16), c["gb"].view(torch.int16))
    _close(r["db"], c["db"], 1e-4, _wtol(rows), "to_out bias gradient after a rejected hand-over (counted once)")
