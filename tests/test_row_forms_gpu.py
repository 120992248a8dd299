"""The scalar, tail and mixed-dtype forms of the elementwise and row kernels against f64: every case of tests/row_form_cases.py is
placed, run through its kernels.py wrapper, must have reached the form it names (kernels.last_form()), is compared with the f64
reference (integer cases: equality; random cases: the case's own bound, nothing of it measured here) and must have left the 7.0-filled
buffer around every output as it was.  tests/test_row_forms_cpu.py pins what those comparisons rest on."""
import pytest
import torch

from mirror_amd import kernels as K
from tests import row_form_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", R.CASES, ids=str)
def test_row_form(c):
    b = R.build(c)
    outs = R.run(c, K, DEV)
    assert K.last_form() == c.form
    torch.cuda.synchronize()
    assert set(outs) == set(b.want)
    for name, o in outs.items():
        got, want = o.win.detach().cpu().double(), b.want[name]
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert o.guards_ok(), f"{c}: {name} wrote outside its window"
        if o.zero_rows is not None:
            assert float(o.zero_rows.float().abs().max()) == 0.0, f"{c}: {name} touched its pad rows"
        err = (got - want).abs()
        if c.kind == "integer":
            assert bool((got == want).all()), f"{c}: {name} differs in {int((got != want).sum())} of {got.numel()} places, first at {int((got != want).reshape(-1).nonzero()[0])}, max |err| {float(err.max()):.3e}"
        else:
            tol = b.tol[name]
            bad = ~(err <= tol)                     # (a nan is bad)
            ratio = float((err / tol.clamp_min(1e-300))[err > 0].max()) if bool((err > 0).any()) else 0.0
            print(f"{c} {name}: max |err| {float(err.max()):.3e}, max err / tol {ratio:.3f}")
            assert not bool(bad.any()), f"{c}: {name} {int(bad.sum())} of {bad.numel()} off, max |err| {float(err.max()):.3e}, max err / tol {ratio:.2f}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_layernorm_refuses_a_row_it_cannot_hold(dtype):
    """D = 2049 is one past what a lane's registers hold (64 x 32): both directions raise, and no output buffer is touched."""
    B, rpb, D = 1, 5, R.LN_MAX_D + 1
    x = torch.randn(B, rpb, D, device=DEV).to(dtype)
    gam, bet = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    y, mean, rstd = (R.window(s, t, "a", DEV) for s, t in (((B, rpb, D), dtype), ((rpb,), torch.float32), ((rpb,), torch.float32)))
    with pytest.raises(K.MirrorHipError, match="D=2049"):
        K.layernorm_fwd(x, gam, bet, y.win, mean.win, rstd.win, B, rpb, D, rpb * D, rpb * D, R.LN_EPS)
    assert K.last_form() == "layernorm_fwd:none"
    dx, dg, db = (R.window(s, t, "a", DEV) for s, t in (((B, rpb, D), dtype), ((D,), torch.float32), ((D,), torch.float32)))
    with pytest.raises(K.MirrorHipError, match="D=2049"):
        K.layernorm_bwd(x, x, gam, mean.win, rstd.win, dx.win, dg.win, db.win, B, rpb, D, rpb * D, rpb * D)
    assert K.last_form() == "layernorm_bwd:none"
    torch.cuda.synchronize()
    for o in (y, mean, rstd, dx, dg, db):
        assert bool((o.full == R.FILL).all())
