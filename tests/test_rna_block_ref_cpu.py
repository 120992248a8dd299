"""No GPU: the hand-written reference of the RNA Block (tests/rna_block_ref.py) pinned to the oracle, the floor its bound is built on
measured again, and the bound shown to be sharp: every mutation of the reference that models a subtly wrong kernel lands outside it.

1. `emulate=False` against oracle.mirror_oracle.rna_block in f64 under autograd, masks handed to both: the forward and all thirteen
   gradients agree at f64 accuracy.  This pins the explicit backward formulas to something independent.
2. The floor (rna_block_ref.measure_floor: f64 against f32 arithmetic in another summation order, between the same rounding points) is
   measured again on every case's first draw and stays inside the bound = 4 x the recorded floor (tests/golden/rna_block_floors.json,
   many draws), and every bound is under 1e-2 in the Frobenius measure from 15 rows on (2e-2 below): a tenth of the relative error the
   cosine band of test_rna_block_gpu.py lets through.
3. Eight mutations, each at every case where it applies: mutated against unmutated is outside the bound in every tensor the mutation
   touches directly.
"""
import pytest
import torch

from oracle import mirror_oracle as O
from tests import rna_block_ref as R


def _oracle(x, dy, P, H, drop):
    inv = {v: k for k, v in R.MODULE_NAMES.items()}
    leaf = {"b." + inv[k]: v.double().clone().requires_grad_(True) for k, v in P.items() if v is not None}
    D, Hh = x.shape[1], P["w_fc1"].shape[0]
    cfg = O.Cfg(wsi_embed_dim=8, rna_embed_dim=8, embed_dim=D, rna_num_heads=H, rna_mlp_ratio=Hh / D, rna_norm_eps=1e-6)
    xr = x.double().clone().requires_grad_(True)
    y = O.rna_block(xr, leaf, "b", cfg, None if drop is None else iter([m.double() for m in drop]))
    y.backward(dy.double())
    grads = {R.GRAD_OF[k]: leaf["b." + inv[k]].grad for k in P if P[k] is not None}
    return y.detach(), xr.grad, grads


@pytest.mark.parametrize("B,D,H,Hh,qkv_bias,p", [(1, 32, 8, 32, True, 0.0), (17, 96, 12, 192, True, 0.1), (5, 64, 8, 128, False, 0.0),
                                                 (5, 64, 8, 128, False, 0.5), (3, 160, 5, 96, True, 0.1)])
def test_exact_reference_equals_the_oracle_under_autograd_in_f64(B, D, H, Hh, qkv_bias, p):
    x, dy, P = R.make_case(B, D, H, Hh, qkv_bias, seed=1)
    drop = R.masks(B, D, Hh, p, seed=11, offset=20)
    got = R.block(x, dy, P, H, drop=drop, emulate=False)
    y, dx, grads = _oracle(x, dy, P, H, drop)
    assert ("db_qkv" in got) == qkv_bias and len(grads) == (12 if qkv_bias else 11)
    for name, want in [("y", y), ("dx", dx)] + sorted(grads.items()):
        fro, mx = R.dist(got[name], want)
        assert fro < 1e-12 and mx < 1e-12, (name, fro, mx)
    if p > 0.0:          # the masks are the host stream's, at the documented sites
        again = R.block(x, dy, P, H, p=p, seed=11, offset=20, emulate=False)
        assert torch.equal(again["y"], got["y"]) and torch.equal(again["dw_fc1"], got["dw_fc1"])
        moved = R.block(x, dy, P, H, p=p, seed=11, offset=24, emulate=False)
        assert not torch.equal(moved["y"], got["y"])
        based = R.block(x, dy, P, H, p=p, seed=11, offset=16, base=7, emulate=False)          # a device base is rounded down to 4
        assert torch.equal(based["y"], got["y"])


def test_emulation_stays_close_to_the_exact_block():
    """The rounding points only round: the emulating reference is the exact Block to bf16 accuracy."""
    x, dy, P = R.make_case(16, 96, 12, 192, seed=2)
    a, b = R.block(x, dy, P, 12, p=0.1, seed=3, offset=8), R.block(x, dy, P, 12, p=0.1, seed=3, offset=8, emulate=False)
    for k in R.CHECKED:
        assert R.dist(a[k], b[k])[0] < 2e-2, k
        assert R.dist(a[k], b[k])[0] > 0.0 or k == "stats"


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: R.case_key(*c))
def test_measured_floor_is_under_the_recorded_one_and_the_bound_is_tight(case, capsys):
    """Few rows make a large relative floor (one flipped bf16 of two in a column sum at B = 2): under 1e-2, a tenth of the relative error
    that cosine > 0.995 lets through, from 15 rows on; under 2e-2 below.  The mutation test is what shows each bound sharp."""
    assert R.MARGIN == 4.0
    for p in R.floor_modes(case):
        rec, bd = R.floor(*case, p=p), R.bound(*case, p=p)
        got = R.measure_floor(*case, p=p, draws=1)
        assert set(got) == set(rec)
        for k, (a, b) in got.items():
            # the first of the recorded draws.  Here it is under the recorded floor itself; another BLAS may sum the f32 run in
            # yet another order and draw other flips, and is then held to what the kernels are held to: the bound
            assert a <= bd[k][0] and b <= bd[k][1], (k, p, (a, b), rec[k])
        with capsys.disabled():
            print("\n%s p=%g floor (Frobenius, max-abs): " % (R.case_key(*case), p)
                  + "  ".join("%s %.1e %.1e" % (k, *rec[k]) for k in R.CHECKED if k in rec))
        for k, (a, b) in bd.items():
            assert a < (1e-2 if case[0] >= 15 else 2e-2), (k, p, a)
            assert b < 4e-2, (k, p, b)


# mutation -> (applies(case, p), the tensors it must push outside the bound)
_W = ("dw_qkv", "dw_proj", "dw_fc1", "dw_fc2")
_B = ("db_qkv", "db_proj", "db_fc1", "db_fc2")
MUT = {
    "db_skip_last_row": (lambda c, p: True, _B),
    "db_last_row_twice": (lambda c, p: True, _B),
    "gelu_grad_without_mask2": (lambda c, p: p > 0.0, ("dw_fc1", "db_fc1", "dg2", "dbe2", "dx")),
    "fc1_offset_plus_4": (lambda c, p: p > 0.0, ("f", "y", "dw_fc2", "dw_fc1", "db_fc1")),
    "dx1_without_residual": (lambda c, p: True, ("dx", "dw_proj", "db_proj")),
    "dw_last_strip_zero": (lambda c, p: True, _W),
    "ln2_operand_row16_zero": (lambda c, p: c[0] == 17, ("u", "f", "y")),
    "dgamma_rows_0_15": (lambda c, p: c[0] == 17, ("dg1", "dg2")),
}


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: R.case_key(*c))
def test_every_mutation_lands_outside_the_bound(case):
    """Train mode, p = 0.1 (the mode in which all eight apply).  A mutation that stayed inside the bound would mean the GPU test
    cannot see that defect: the answer would be a tighter emulation, not a wider list of exceptions."""
    B, D, H, Hh, qkv_bias = case
    p = 0.1
    assert set(MUT) == set(R.MUTATIONS)
    x, dy, P = R.make_case(B, D, H, Hh, qkv_bias, seed=5)
    kw = dict(H=H, p=p, seed=0xABCD, offset=40)
    ref, bd = R.block(x, dy, P, **kw), R.bound(*case, p=p)
    inside = []
    for mut in R.MUTATIONS:
        applies, touched = MUT[mut]
        if not applies(case, p):
            continue
        bad = R.block(x, dy, P, mut=mut, **kw)
        for k in touched:
            if k in ref and not R.outside(bad[k], ref[k], bd[k]):
                inside.append((mut, k, R.dist(bad[k], ref[k]), bd[k]))
    assert not inside, inside


def test_mutations_that_need_seventeen_rows_are_exercised():
    assert sum(c[0] == 17 for c in R.CASES) >= 2
