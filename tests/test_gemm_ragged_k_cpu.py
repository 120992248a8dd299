"""Without a device: the preconditions of tests/test_gemm_ragged_k_gpu.py.  The table of tests/gemm_ragged_cases.py only tests the
remainder routes of mh_gemm while the host still sends each case down the route it names, and its exact / toleranced comparisons
only mean something while the data has the properties they rest on — both are pinned here, where every pull request runs them."""
import ctypes

import pytest
import torch

from mirror_amd import _lib
from mirror_amd import functional as Fn
from tests import gemm_ragged_cases as G


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_the_table_has_every_row_of_the_plan():
    ids = [c.id for c in G.CASES]
    assert len(set(ids)) == len(ids)
    heads = {i.split("-")[0] for i in ids}
    assert heads == {"F4", "F1", "FB", "FBL", "FBX", "FW", "RA", "RU", "RF", "T", "NA", "NP"}
    for c in G.CASES:
        assert c.tail == c.K % G.bk(c.mma) and c.K >= 8 * G.bk(c.mma), c.id       # mh_gemm's condition for splitting the product


@pytest.mark.parametrize("c", G.CASES, ids=str)
def test_workspace_bytes_pins_the_fold_route_to_the_table(lib, c):
    """Partial tiles + fold (route 1's precondition) exactly for the fold rows: kernels.gemm allocates what mh_gemm_workspace_bytes
    asks for when it is in (0, 2^29], and launch_big folds when it has that workspace."""
    wsb = G.workspace_bytes(lib, c)
    if c.id.split("-")[0] in G.FOLD_IDS:
        assert c.folds
        assert 0 < wsb <= 2 ** 29, (c.id, wsb)
        parts = c.split_k * c.batch
        assert wsb == parts * c.M * c.N * 2 and wsb <= 34 << 20
        assert parts >= 8 and len(G.k_slices(c.kmain, c.split_k)) == c.split_k
        assert G.big_kernel_workgroups(c.M, c.N, c.kmain, c.split_k, c.batch) >= 128
        blocks1 = -(-(c.M * c.N // 4) // 256)
        tail_fits = c.tail <= 16 and c.batch * c.tail <= 256
        assert c.route == ("fold_notail" if not tail_fits else ("fold4" if blocks1 < 1024 else "fold1")), c.id
    else:
        assert not c.folds
        assert wsb == 0, (c.id, wsb)


def test_the_boundaries_the_table_claims():
    assert -(-(1024 * 1024 // 4) // 256) == 1024                       # F1: blocks1 exactly at launch_fold's threshold
    assert G.by_id("FBL").batch * G.by_id("FBL").tail == 256           # the rank update's limit
    assert G.by_id("FBX").batch * G.by_id("FBX").tail > 256
    totals = {c.batch * c.tail for c in G.CASES if c.id.startswith("FB-")}
    assert totals == {8, 128}                                          # PS = 4: the remainder loop alone, and the 8-in-flight loop


@pytest.mark.parametrize("c", G.CASES, ids=str)
def test_integer_cases_are_exact_by_construction(c):
    """integer_case asserts that every K-slice's partial tile is a bf16 number (fold rows); here also: the values are integers in
    range, every f32 sum of the product is exact (all intermediate magnitudes far below 2^24), the tail moves most elements."""
    d = G.integer_case(c)
    assert float(d.at[:, :c.kmain].abs().max()) <= 1 and float(d.b[:, :c.kmain].abs().max()) <= 1
    assert float(d.at[:, c.kmain:].abs().max()) <= 3 and float(d.b[:, c.kmain:].abs().max()) <= 3
    assert bool((d.at == d.at.round()).all()) and bool((d.b == d.b.round()).all())
    assert c.batch * (c.kmain + 9 * c.tail) + 16 < 2 ** 24
    assert bool((d.want * 2 == (d.want * 2).round()).all())
    tail = torch.matmul(d.at[:, c.kmain:].double().transpose(-1, -2), d.b[:, c.kmain:].double())
    assert float((tail != 0).double().mean()) > 0.5, "a dropped remainder must change most of the result"


@pytest.mark.parametrize("c", G.RANDOM_CASES, ids=str)
def test_random_cases_see_their_tail(c):
    r = G.random_case(c)
    assert r.parts == c.split_k * c.batch
    frac = G.tail_visible_fraction(r)
    print(f"{c.id}: parts {r.parts}, max |partial| {r.partial_max:.2f}, tail above the tolerance in {100 * frac:.1f} % of the elements")
    assert frac >= G.TAIL_VISIBLE_FRACTION, (c.id, frac)


@pytest.mark.parametrize("N,Kd", [(512, 1024), (512, 512)])
def test_production_weight_gradients_are_fold_cases_with_a_tail(lib, N, Kd):
    """The link to the real step: dW of the big projections contracts over 16 slides x 4097 rows; the split functional._split_k_for
    picks must still put that product on partial tiles + fold, with a remainder of K % 64 = 16 rows that the fold can take."""
    rows = 16 * 4097
    split = Fn._split_k_for(rows, N, Kd)
    tail = rows % 64
    assert tail == 16 and rows >= 8 * 64
    d = G.desc_for(N, Kd, rows, split, 1, True, G.bf16, G.bf16, G.MH_BF16, True)
    wsb = int(lib.mh_gemm_workspace_bytes(ctypes.byref(d)))
    assert 0 < wsb <= 2 ** 29, (split, wsb)
    assert split >= 8 and len(G.k_slices(rows - tail, split)) == split
    assert G.big_kernel_workgroups(N, Kd, rows - tail, split, 1) >= 128
    assert tail <= 16 and Kd % 4 == 0                                  # rank_update_ok and launch_fold's alignment of B's rows
