"""Every launch form of PPEG, res_conv and the landmark kernels against f64: every case of tests/seq_form_cases.py is placed, run through
its kernels.py wrapper, must have reached the form it names (kernels.last_form()), is compared with the f64 reference (integer cases:
equality; random cases: the case's own bound, nothing of it measured here) and must have left the 7.0-filled buffer around every output
as it was.  tests/test_seq_forms_cpu.py pins what those comparisons rest on."""
import pytest
import torch

from mirror_amd import _lib
from mirror_amd import kernels as K
from tests import seq_form_cases as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32, bf16 = torch.float32, torch.bfloat16


def _within(tag, got, want, tol):
    err = (got.detach().cpu().double() - want).abs()
    bad = ~(err <= tol)                         # (a nan is bad)
    ratio = float((err / tol.clamp_min(1e-300))[err > 0].max()) if bool((err > 0).any()) else 0.0
    print(f"{tag}: max |err| {float(err.max()):.3e}, max err / tol {ratio:.3f}")
    assert not bool(bad.any()), f"{tag}: {int(bad.sum())} of {bad.numel()} off, max |err| {float(err.max()):.3e}, max err / tol {ratio:.2f}"


@pytest.mark.parametrize("c", Q.CASES, ids=str)
def test_seq_form(c):
    b = Q.build(c)
    if c.form:
        assert _lib.load().mh_cast(None, None, 0, 0, 0, None) == 0 and K.last_form() == "cast:none"      # the note below is this call's
    outs = Q.run(c, K, DEV)
    if c.form:
        assert K.last_form() == c.form
    torch.cuda.synchronize()
    assert set(outs) == set(b.want)
    for name, o in outs.items():
        got, want = o.win.detach().cpu().double(), b.want[name]
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert o.guards_ok(), f"{c}: {name} wrote outside its window"
        if c.kind == "integer":
            err = (got - want).abs()
            assert bool((got == want).all()), f"{c}: {name} differs in {int((got != want).sum())} of {got.numel()} places, first at {int((got != want).reshape(-1).nonzero()[0])}, max |err| {float(err.max()):.3e}"
        else:
            _within(f"{c} {name}", got, want, b.tol[name])


def test_resconv_refuses_more_heads_than_its_weight_table_holds():
    """heads = 16 of dh = 16: a 256-column block would meet 17 heads and the kernels keep 8 in LDS.  The call raises and touches nothing."""
    B, n_p, heads, dh, taps = 2, 17, 16, 16, 3
    v = torch.randn(B, n_p, heads * dh, device=DEV)
    w = torch.randn(heads * taps, device=DEV)
    o = Q.window((B, n_p, heads * dh), f32, "a", DEV)
    with pytest.raises(K.MirrorHipError, match="more than 8 heads"):
        K.resconv(v, w, o.win, heads, False, False)
    assert K.last_form() == "resconv_fwd:none"
    dv, dw = Q.window((B, n_p, heads * dh), f32, "a", DEV), Q.window((heads * taps,), f32, "a", DEV)
    with pytest.raises(K.MirrorHipError, match="more than 8 heads"):        # the two-pass backward: before its first pass has added to dw
        K.resconv_bwd(v, v, w, dv.win, dw.win, heads)
    assert K.last_form() == "resconv_bwd:none"
    torch.cuda.synchronize()
    assert o.untouched() and dv.untouched() and dw.untouched()


def test_an_unknown_dtype_code_is_refused_before_any_launch():
    """The four dtype dispatches end in an `else`: a code that is neither f32 nor bf16 used to run as some (bf16, f32) pair."""
    B, S, D, bad = 2, 4, 8, 7
    n = 1 + S * S
    x = torch.randn(B, n, D, device=DEV)
    merged, bsum = torch.randn(49, D, device=DEV), torch.randn(D, device=DEV)
    y, dm, dbs = Q.window((B, n, D), f32, "a", DEV), Q.window((49, D), f32, "a", DEV), Q.window((D,), f32, "a", DEV)
    w = torch.randn(3, device=DEV)
    dw = Q.window((3,), f32, "a", DEV)
    st = K._stream()
    calls = (
        ("ppeg_fwd", ("mh_ppeg_fwd", x.data_ptr(), y.win.data_ptr(), merged.data_ptr(), bsum.data_ptr(), B, S, D, 0, bad, _lib.MH_F32)),
        ("ppeg_fwd", ("mh_ppeg_fwd", x.data_ptr(), y.win.data_ptr(), merged.data_ptr(), bsum.data_ptr(), B, S, D, 0, _lib.MH_F32, -1)),
        ("ppeg_wgrad", ("mh_ppeg_wgrad", x.data_ptr(), x.data_ptr(), dm.win.data_ptr(), dbs.win.data_ptr(), B, S, D, _lib.MH_BF16, bad)),
        ("resconv_fwd", ("mh_resconv_fwd", x.data_ptr(), D, n * D, w.data_ptr(), y.win.data_ptr(), D, n * D, B, n, 1, D, 3, 0, 0, bad, _lib.MH_F32)),
        ("resconv_wgrad", ("mh_resconv_wgrad", x.data_ptr(), D, n * D, x.data_ptr(), D, n * D, dw.win.data_ptr(), B, n, 1, D, 3, _lib.MH_F32, bad)),
    )
    for entry, args in calls:
        with pytest.raises(K.MirrorHipError, match="unknown dtype code"):
            _lib.call(*args, stream=st)
        assert K.last_form() == f"{entry}:none"
    torch.cuda.synchronize()
    assert y.untouched() and dm.untouched() and dbs.untouched() and dw.untouched()


def _ppeg_params(gen, D):
    """Filters and biases in multiples of 1 / 64: the merged 7 x 7 (w7 + w5 + w3 + the identity) and the summed bias are f32 numbers, so
    the merge adds no rounding of its own to the bounds below."""
    ws = [torch.randint(-24, 25, (D, 1, k, k), generator=gen).float() / 64 for k in (7, 5, 3)]
    bs = [torch.randint(-64, 65, (D,), generator=gen).float() / 64 for _ in range(3)]
    merged = ws[0].double().reshape(D, 7, 7).clone()
    merged[:, 1:6, 1:6] += ws[1].double().reshape(D, 5, 5)
    merged[:, 2:5, 2:5] += ws[2].double().reshape(D, 3, 3)
    merged[:, 3, 3] += 1.0
    return ws, bs, merged.reshape(D, 49).t().contiguous(), sum(b.double() for b in bs)


def _ppeg_bounds(x, dy, merged, bsum, S, dt_y, dt_dx):
    """f64 references and derived bounds of PPEG's forward and backward (x, dy: the stored values)."""
    B = x.shape[0]
    y, dx = Q.ppeg64(x, merged, bsum, S, 0), Q.ppeg64(dy, merged, bsum, S, 1)
    my, mdx = Q.ppeg64(x.abs(), merged.abs(), bsum.abs(), S, 0), Q.ppeg64(dy.abs(), merged.abs(), bsum, S, 1)
    my[:, 0], mdx[:, 0] = 0.0, 0.0
    dm, dbs = Q.ppeg_wgrad64(x, dy, S)
    am, ab = Q.ppeg_wgrad64(x.abs(), dy.abs(), S)
    T = B * S * S
    return {"y": (y, 52 * Q.EPS * my + Q._bf16_term(dt_y, y)), "dx": (dx, 52 * Q.EPS * mdx + Q._bf16_term(dt_dx, dx)),
            "dmerged": (dm, (T + 2) * Q.EPS * am), "dbsum": (dbs, (T + 2) * Q.EPS * ab)}


def _check_param_grads(tag, grads, dm, tol_m, dbs, tol_b, D):
    """The six parameter gradients are windows of the merged filter's gradient [49, D] and copies of the summed bias' gradient."""
    dm3, tol3 = dm.t().reshape(D, 7, 7), tol_m.t().reshape(D, 7, 7)
    for (name, g), lo in zip(grads[:3], (0, 1, 2)):
        k = 7 - 2 * lo
        _within(f"{tag} {name}", g.reshape(D, k, k), dm3[:, lo:7 - lo, lo:7 - lo], tol3[:, lo:7 - lo, lo:7 - lo])
    for name, g in grads[3:]:
        _within(f"{tag} {name}", g, dbs, tol_b)


def test_ppegfn_with_bf16_x_takes_the_fallback_backward(monkeypatch):
    """PPEGFn on a bf16 sequence: ppeg_bwd_ok says no, so the backward is the strip kernel's adjoint form and ppeg_wgrad_strip_kernel,
    both bf16 x bf16.  dx and all six parameter gradients against f64, at S = 9 (two x-tiles, one strip), D = 40."""
    from mirror_amd import functional as Fn
    B, S, D = 2, 9, 40
    gen = torch.Generator().manual_seed(3)
    ws, bs, merged, bsum = _ppeg_params(gen, D)
    x = Q.stored(torch.randn(B, 1 + S * S, D, generator=gen), bf16)
    dy = Q.stored(torch.randn(B, 1 + S * S, D, generator=gen), bf16)
    want = _ppeg_bounds(x, dy, merged, bsum, S, bf16, bf16)

    def no_one_pass(*a, **k):
        raise AssertionError("the one-pass backward was taken")
    monkeypatch.setattr(K, "ppeg_bwd", no_one_pass)
    xd = x.to(DEV, bf16).requires_grad_(True)
    p = [t.to(DEV).requires_grad_(True) for t in (ws[0], bs[0], ws[1], bs[1], ws[2], bs[2])]
    y = Fn.PPEGFn.apply(xd, *p, S)
    assert y.dtype == bf16 and K.last_form() == "ppeg_fwd:strip"
    y.backward(dy.to(DEV, bf16))
    torch.cuda.synchronize()
    _within("PPEGFn bf16 y", y.float(), *want["y"])
    assert xd.grad.dtype == bf16
    _within("PPEGFn bf16 dx", xd.grad.float(), *want["dx"])
    grads = [("dw7", p[0].grad), ("dw5", p[2].grad), ("dw3", p[4].grad), ("db7", p[1].grad), ("db5", p[3].grad), ("db3", p[5].grad)]
    _check_param_grads("PPEGFn bf16", grads, *want["dmerged"], *want["dbsum"], D)


def test_ppeg_bwd_notes_its_form():
    """The one-pass backward (f32, aligned) notes "ppeg_bwd:one"; its results within the same derived bounds as the two kernels it replaces."""
    B, S, D = 2, 9, 40
    gen = torch.Generator().manual_seed(4)
    _, _, merged, bsum = _ppeg_params(gen, D)
    x, dy = torch.randn(B, 1 + S * S, D, generator=gen), torch.randn(B, 1 + S * S, D, generator=gen)
    want = _ppeg_bounds(x, dy, merged, bsum, S, f32, f32)
    dm, dbs = Q.window((49, D), f32, "a", DEV, torch.zeros(49, D)), Q.window((D,), f32, "a", DEV, torch.zeros(D))
    dx = K.ppeg_bwd(x.to(DEV), dy.to(DEV), merged.float().to(DEV), dm.win, dbs.win, S)
    assert K.last_form() == "ppeg_bwd:one"
    torch.cuda.synchronize()
    assert dm.guards_ok() and dbs.guards_ok()
    _within("ppeg_bwd dx", dx, *want["dx"])
    _within("ppeg_bwd dmerged", dm.win, *want["dmerged"])
    _within("ppeg_bwd dbsum", dbs.win, *want["dbsum"])
