"""Without a device: the preconditions of tests/test_row_forms_gpu.py.  The table of tests/row_form_cases.py only tests the scalar, tail
and mixed-dtype forms of the row kernels while it holds a case for every form and dtype instance the host can select, and its exact /
toleranced comparisons only mean something while the data has the properties they rest on — both are pinned here."""
import collections
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from mirror_amd import _lib
from mirror_amd import kernels as K
from tests import row_form_cases as R

f64 = torch.float64
CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")

# Every form an entry point of the table can note beside a launch (":none" = it returned before any), written out: a form added to
# the library later without a case fails test_the_table_has_a_case_for_every_form.
FORMS = {
    "add": ["none", "quad", "scalar"],
    "cast": ["none", "quad", "scalar"],
    "relu_bwd": ["none", "quad", "scalar"],
    "gelu_fwd": ["none", "scalar"],
    "gelu_bwd": ["none", "scalar"],
    "row_scale": ["none", "quad", "scalar"],
    "colsum": ["none", "f32quad", "bf16oct", "scalar"],
    "softmax_fwd": ["none", "wave,quad", "wave,scalar", "block,quad", "block,scalar"],
    "softmax_bwd": ["none", "wave,quad", "wave,scalar", "block,quad", "block,scalar"],
    "layernorm_fwd": ["none", "quad", "scalar"],
    "layernorm_bwd": ["none", "ws", "quad", "scalar"],
    "fanout_bwd": ["none", "quad", "scalar"],
    "mask_apply_fwd": ["none", "quad", "scalar"],
    "mask_apply_bwd": ["none", "d1", "quad", "scalar"],
    "mse_masked_fwd": ["none", "flat", "quad", "scalar"],
    "mse_masked_bwd": ["none", "colsum", "quad", "scalar"],
}
# ":none" is reached without a device (test_early_returns_note_none) where the issue's sizes hold no empty call
NONE_IN_TABLE = {"add", "cast", "relu_bwd"}
# The dtype instances each dispatch macro names (f = f32, b = bf16, operands in the entry point's order)
PAIRS = ["ff", "fb", "bf", "bb"]
TRIPLES = ["fff", "ffb", "fbf", "fbb", "bff", "bfb", "bbf", "bbb"]
INSTANCES = {
    "add": TRIPLES, "cast": PAIRS, "relu_bwd": TRIPLES, "gelu_fwd": PAIRS, "gelu_bwd": PAIRS, "row_scale": ["f", "b"], "colsum": ["f", "b"],
    "softmax_fwd": PAIRS, "softmax_bwd": PAIRS, "layernorm_fwd": PAIRS, "layernorm_bwd": PAIRS,
    "fanout_bwd": ["f", "b"], "mask_apply_fwd": PAIRS, "mask_apply_bwd": PAIRS, "mse_masked_fwd": PAIRS, "mse_masked_bwd": TRIPLES,
}
RANDOM = [c for c in R.CASES if c.kind == "random"]
INTEGER = [c for c in R.CASES if c.kind == "integer"]


def _noted_in_the_sources():
    """entry -> forms, from the mh_note_form("...") literals of the three sources (a `cond ? "a" : "b"` argument holds two)."""
    noted = collections.defaultdict(set)
    for name in ("elementwise.hip", "norm_softmax.hip", "loss.hip"):
        with open(os.path.join(CSRC, name)) as fh:
            for call in re.findall(r"mh_note_form\(([^;]*)\);", fh.read()):
                for entry, form in re.findall(r'"(\w+):([\w,]+)"', call):
                    noted[entry].add(form)
    return noted


def test_the_written_out_forms_are_the_ones_the_library_notes():
    noted = _noted_in_the_sources()
    assert set(noted) == set(FORMS)
    for entry, forms in FORMS.items():
        assert noted[entry] == set(forms), entry


def test_the_table_has_a_case_for_every_form_and_dtype_instance():
    assert {c.entry for c in R.CASES} == set(FORMS) == set(INSTANCES)
    for entry, forms in FORMS.items():
        have = {c.form for c in R.CASES if c.entry == entry}
        need = {f"{entry}:{f}" for f in forms if f != "none" or entry in NONE_IN_TABLE}
        assert have == need, (entry, have ^ need)
        insts = {R._dn(c.dtypes) for c in R.CASES if c.entry == entry}
        assert insts == set(INSTANCES[entry]), (entry, insts)
    # every dtype instance in BOTH forms of the flat kernels, and of the forms the softmax and LayerNorm hosts select
    for entry in ("add", "cast", "relu_bwd", "row_scale"):
        for form in ("quad", "scalar"):
            assert {R._dn(c.dtypes) for c in R.CASES if c.form == f"{entry}:{form}"} == set(INSTANCES[entry]), (entry, form)
    for entry in ("softmax_fwd", "softmax_bwd"):
        for form in ("wave,quad", "wave,scalar", "block,scalar", "block,quad"):
            assert {R._dn(c.dtypes) for c in R.CASES if c.form == f"{entry}:{form}"} == set(PAIRS), (entry, form)
    for entry in ("fanout_bwd", "mask_apply_bwd", "mse_masked_fwd", "mse_masked_bwd"):
        assert {R._dn(c.dtypes) for c in R.CASES if c.form == f"{entry}:scalar"} == set(INSTANCES[entry]), entry
    assert {R._dn(c.dtypes) for c in R.CASES if c.form == "mse_masked_bwd:quad"} == set(TRIPLES)
    for form in ("layernorm_fwd:scalar", "layernorm_fwd:quad", "layernorm_bwd:scalar", "layernorm_bwd:quad", "layernorm_bwd:ws"):
        assert {R._dn(c.dtypes) for c in R.CASES if c.form == form} == set(PAIRS), form


def test_the_boundaries_the_table_claims():
    n = R.by_id("add-wrap-scalar").sizes[0]
    assert -(-n // 256) > R.EW_CAP and R.by_id("add-wrap-quad").sizes[0] == 4 * n and R.by_id("cast-wrap-scalar").sizes[0] == n
    assert -(-R.by_id("relu_bwd-wrap-scalar").sizes[0] // 256) > R.RELU_CAP
    assert -(-65541 // 4) > 16384                                            # row_scale: rows past the 16384-block cap
    assert -(-2053 // 4) > 512                                               # layernorm_bwd: ln_bwd_blocks() = 512 blocks of 4 rows
    assert (9 * 8) % 4 == 0 and (9 * 7) % 4 != 0                             # relu_bwd's batch strides
    sizes = {c.sizes for c in R.CASES if c.entry == "colsum"}
    assert {(31, 8, 8), (32, 8, 8), (1023, 16, 16), (1024, 16, 16), (513, 5, 5)} <= sizes      # both row thresholds, CS_BAND + 1
    cols = {c.sizes[1] for c in R.CASES if c.entry == "softmax_fwd"}
    assert cols == set(R.SOFTMAX_COLS) and {1024, 1025, 12288, 12292} <= cols
    assert {c.sizes[2] for c in R.CASES if c.entry == "layernorm_fwd"} == set(R.LN_D) | {512} and max(R.LN_D) == R.LN_MAX_D
    for c in R.CASES:                                                        # every size of the flat kernels, in every instance
        if c.entry in ("add", "cast", "relu_bwd") and not c.place and c.opt == "" and "wrap" not in c.id:
            assert c.sizes[0] in R.FLAT_SIZES
    for entry in ("add", "cast", "relu_bwd"):
        for inst in INSTANCES[entry]:
            assert {c.sizes[0] for c in R.CASES if c.entry == entry and R._dn(c.dtypes) == inst and not c.place and c.opt == ""} >= set(R.FLAT_SIZES)


@pytest.mark.parametrize("c", INTEGER, ids=str)
def test_integer_cases_are_exact_by_construction(c):
    b = R.build(c)
    assert not b.tol and b.f32_sum_bound < 2 ** 24
    for name, dtype in R.out_dtypes(c).items():
        want = b.want[name]
        assert want.dtype == f64 and bool(torch.isfinite(want).all())
        assert bool((want.to(dtype).double() == want).all()), f"{c}: {name} holds a value that is no {dtype} number"
    for name, t in b.inputs.items():
        if (c.entry, name) not in (("row_scale", "scale"), ("fanout_bwd", "alpha")):
            assert bool((t == t.round()).all()), (str(c), name)
    if c.entry == "cast" and c.dtypes == (torch.float32, torch.bfloat16) and c.sizes[0] >= 255:
        assert bool((b.want["y"] != b.inputs["x"].double()).any())          # the cast has something to round
    if c.entry == "relu_bwd" and c.sizes[0] >= 255:
        assert bool((b.inputs["y"] == 0).any()) and bool((b.inputs["y"] < 0).any())
    if c.opt == "const":
        assert bool((b.want["mean"] == 3.0).all()) and bool((b.want["rstd"] == 256.0).all())
        assert bool((b.want["y"] == b.inputs["beta"].double().expand_as(b.want["y"])).all())


# outputs that are zero by the mathematics: one column has no deviation from its mean
ZERO_BY_MATH = {("layernorm_bwd", 1): {"dx", "dgamma"}}


@pytest.mark.parametrize("c", RANDOM, ids=str)
def test_random_cases_would_notice_a_lost_tail(c):
    """No output is all zero, every bound is finite and positive where the reference is not zero, and leaving the tail out of the
    reference moves some output by more than 10 tolerances."""
    b = R.build(c)
    assert set(b.tol) == set(b.want) == set(b.dropped) == set(R.out_dtypes(c))
    moved = 0.0
    for name, want in b.want.items():
        tol, drop = b.tol[name], b.dropped[name]
        assert want.shape == drop.shape and bool(torch.isfinite(want).all()) and bool(torch.isfinite(tol).all()) and bool((tol >= 0).all())
        if name not in ZERO_BY_MATH.get((c.entry, c.sizes[-1]), ()):
            assert float(want.abs().max()) > 0.0, (str(c), name)
        diff = (want - drop).abs()
        far = diff > 10 * tol
        moved = max(moved, float((diff / tol.clamp_min(1e-300))[far].max()) if bool(far.any()) else 0.0)
    assert moved > 10.0, f"{c}: dropping the tail moves no output by more than 10 tolerances"


def test_the_tolerances_are_the_stated_ones():
    b = R.build(R.by_id("softmax_fwd-ff-6x257"))
    x, want, tol = b.inputs["x"].double(), b.want["y"], b.tol["y"]
    assert float((x[3].max() - x[3].min())) == 60.0 and bool((x[1] == x[1, 0]).all()) and bool(torch.isinf(x[2]).any())
    rel = (tol / want)[3]
    assert abs(float(rel.max()) - 2.0 ** -22 * 64.0) < 1e-12 and float((tol / want)[0].max()) < 6e-6       # 1.5e-5 at a spread of 60
    assert bool((tol[2][torch.isinf(x[2])] == 0).all()) and bool((want[2][torch.isinf(x[2])] == 0).all())
    big = R.build(R.by_id("layernorm_bwd-ff-2053x30"))
    small = R.build(R.by_id("layernorm_bwd-ff-69x30"))
    scale = (2053 / 69) ** 0.5
    assert abs(float((big.tol["dbeta"] - 1e-4 * big.want["dbeta"].abs()).max()) - 2e-4 * scale) < 1e-12
    assert abs(float((small.tol["dbeta"] - 1e-4 * small.want["dbeta"].abs()).max()) - 2e-4) < 1e-12


def test_the_references_agree_with_f64_autograd():
    gen = torch.Generator().manual_seed(5)
    x = (torch.randn(6, 37, generator=gen, dtype=f64) * 3).requires_grad_(True)
    dy = torch.randn(6, 37, generator=gen, dtype=f64)
    y = x.softmax(-1)
    assert float((R.softmax64(x.detach()) - y.detach()).abs().max()) < 1e-12
    y.backward(dy)
    assert float((R.softmax_bwd64(y.detach(), dy) - x.grad).abs().max()) < 1e-12
    xg = (torch.randn(500, generator=gen, dtype=f64) * 2).requires_grad_(True)
    g = F.gelu(xg)
    assert float((R.gelu64(xg.detach()) - g.detach()).abs().max()) < 1e-12
    g.backward(torch.ones_like(g))
    assert float((R.gelu_grad64(xg.detach()) - xg.grad).abs().max()) < 1e-12
    for D in (1, 3, 30):
        xl = (torch.randn(3, 5, D, generator=gen, dtype=f64) * 2 + 0.5).requires_grad_(True)
        gam = torch.randn(D, generator=gen, dtype=f64).requires_grad_(True)
        bet = torch.randn(D, generator=gen, dtype=f64).requires_grad_(True)
        ref = F.layer_norm(xl, (D,), gam, bet, R.LN_EPS)
        yl, mean, rstd = R.layernorm64(xl.detach(), gam.detach(), bet.detach(), R.LN_EPS)
        assert float((yl - ref.detach()).abs().max()) < 1e-12
        dl = torch.randn(3, 5, D, generator=gen, dtype=f64)
        ref.backward(dl)
        dx, dg, db = R.layernorm_bwd64(dl, xl.detach(), gam.detach(), mean, rstd)
        # at D = 1 the variance is 0 and rstd = eps^-1/2 = 316: autograd's dx carries rounding noise of that size times 1e-16
        assert float((dx - xl.grad).abs().max()) < 1e-12 and float((dg - gam.grad).abs().max()) < 1e-12 and float((db - bet.grad).abs().max()) < 1e-12
    # masked MSE, the target a row window of a larger buffer (rows 1.. of [B, N + 1, D]) as the model hands it over
    for D in (1, 23, 24):
        B, N = 3, 6
        pr = torch.randn(B, N, D, generator=gen, dtype=f64).requires_grad_(True)
        buf = torch.randn(B, N + 1, D, generator=gen, dtype=f64).requires_grad_(True)
        tg = buf[:, 1:]
        assert not tg.is_contiguous()
        mask = (torch.rand(B, N, generator=gen) > 0.4).double()
        mask[0, 0], mask[-1, -1] = 0.0, 1.0
        loss = (((pr - tg) ** 2).mean(-1) * mask).sum() / mask.sum()
        num, den = R.mse_masked64(pr.detach(), tg.detach(), mask)
        assert abs(float(num / den - loss.detach())) < 1e-12 and float(den) == float(mask.sum())
        (0.7 * loss).backward()
        dp, dt = R.mse_masked_bwd64(pr.detach(), tg.detach(), mask, 0.7)
        assert float((dp - pr.grad).abs().max()) < 1e-12 and float((dt - buf.grad[:, 1:]).abs().max()) < 1e-12
        assert float(buf.grad[:, 0].abs().max()) == 0.0 and float(dp[0, 0].abs().max()) == 0.0


def test_early_returns_note_none():
    """Every entry point notes "<entry>:none" when it returns before any launch: reached here with empty calls, which touch no device."""
    lib = _lib.load()
    assert isinstance(K.last_form(), str)
    calls = {
        "add": lambda: lib.mh_add(None, None, None, 0, 0, 0, 0, None),
        "cast": lambda: lib.mh_cast(None, None, 0, 0, 0, None),
        "gelu_fwd": lambda: lib.mh_gelu_fwd(None, None, 0, 0, 0, None),
        "gelu_bwd": lambda: lib.mh_gelu_bwd(None, None, None, 0, 0, 0, 0, None),
        "relu_bwd": lambda: lib.mh_relu_bwd(None, None, None, 0, 1, 0, 0, 0, 0, 0, 0, None),
        "colsum": lambda: lib.mh_colsum(None, None, 0, 8, 8, 0, None),
        "row_scale": lambda: lib.mh_row_scale(None, None, None, 0, 8, 0, None),
        "softmax_fwd": lambda: lib.mh_softmax_fwd(None, None, 0, 8, 8, 8, 0, 0, None),
        "softmax_bwd": lambda: lib.mh_softmax_bwd(None, None, None, 0, 8, 8, 8, 8, 0, 0, 0, None),
        "layernorm_fwd": lambda: lib.mh_layernorm_fwd(None, None, None, None, None, None, 0, 5, 8, 40, 40, 1e-5, 0, 0, None),
        "fanout_bwd": lambda: lib.mh_fanout_bwd(None, None, 1.0, None, None, 0, 3, 8, 0, None),
        "mask_apply_fwd": lambda: lib.mh_mask_apply_fwd(None, None, None, None, None, 0, 3, 8, 1, 0, 0, 0, None),
        "mask_apply_bwd": lambda: lib.mh_mask_apply_bwd(None, None, None, None, None, 0, 3, 8, 1, 0, 0, 0, None, None),
        "mse_masked_fwd": lambda: lib.mh_mse_masked_fwd(None, None, None, None, 0, 8, 1, 8, 0, 0, None),
        "mse_masked_bwd": lambda: lib.mh_mse_masked_bwd(None, None, None, None, None, 1.0, None, None, 0, 8, 1, 8, 0, 0, 0, None, 0, None),
    }
    for entry, call in calls.items():
        assert call() == 0, entry
        assert K.last_form() == f"{entry}:none", entry
    d = _lib.LnBwdDesc()
    d.D, d.rows_per_batch, d.batches = 8, 5, 0
    assert lib.mh_layernorm_bwd(ctypes.byref(d), None) == 0 and K.last_form() == "layernorm_bwd:none"
    # a refused call has launched nothing either
    assert lib.mh_layernorm_fwd(None, None, None, None, None, None, 1, 5, R.LN_MAX_D + 1, 0, 0, 1e-5, 0, 0, None) != 0
    assert K.last_form() == "layernorm_fwd:none" and "D=2049" in lib.mh_last_error().decode()


def test_gelu_bwd_refuses_what_its_launch_cannot_walk(monkeypatch):
    """kernels.gelu_bwd launches x.numel() elements of x, dy and dx: an x of another size or with strides is refused before the launch."""
    monkeypatch.setattr(K, "_chk", lambda *ts: None)
    monkeypatch.setattr(K, "_stream", lambda: 0)

    def no_launch(*a, **k):
        raise AssertionError("gelu_bwd reached the library")
    monkeypatch.setattr(K._lib, "call", no_launch)
    dy = torch.zeros(6, 8)
    with pytest.raises(K.MirrorHipError, match="elements"):
        K.gelu_bwd(torch.zeros(6, 9), dy)
    with pytest.raises(K.MirrorHipError, match="elements"):
        K.gelu_bwd(torch.zeros(5, 8), dy)
    with pytest.raises(K.MirrorHipError, match="contiguous"):
        K.gelu_bwd(torch.zeros(8, 6).t(), dy)
    with pytest.raises(K.MirrorHipError, match="contiguous"):
        K.gelu_bwd(torch.zeros(6, 8), torch.zeros(8, 6).t())
    with pytest.raises(K.MirrorHipError):
        K.gelu_bwd(torch.zeros(6, 8), dy, out=torch.zeros(6, 9))
    with pytest.raises(K.MirrorHipError, match="expected"):                # the same count in another shape is refused too
        K.gelu_bwd(torch.zeros(6, 8), dy, out=torch.zeros(8, 6))
    with pytest.raises(K.MirrorHipError, match="expected"):
        K.relu_bwd(torch.zeros(6, 8), dy, out=torch.zeros(48))
    with pytest.raises(AssertionError, match="reached the library"):       # and what is well-formed goes through
        K.gelu_bwd(torch.zeros(6, 8), dy)
