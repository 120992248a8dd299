"""No GPU: the host side of the grouped retrieval metric (several slides per RNA sample).  The float64 restatement of the definition
(tests/retrieval_ref.py) against hand-worked cases, the first-of-group summary, the argument checks that need no device, and the
declaration of the entry point against its ctypes row."""
import os
import re

import numpy as np
import pytest
import torch

from mirror_amd import _lib
from mirror_amd import kernels as K
from mirror_amd._lib import MirrorHipError
from mirror_amd.retrieval import CrossModalRetrieval, first_of_group, retrieval_ranks
from tests import retrieval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement, by hand
def test_restatement_on_a_hand_worked_case():
    # D = 1: s_ij = q_i k_j.  keys 3, 5, 4, 5, 1 in groups a, a, b, c, c (a = 7, b = -2, c = 7 + 2^32)
    a, b, c = 7, -2, 7 + (1 << 32)
    k = np.array([[3.0], [5.0], [4.0], [5.0], [1.0]])
    kg = np.array([a, a, b, c, c])
    q = np.array([[1.0], [1.0], [1.0], [-1.0], [1.0]])
    qg = np.array([a, b, c, a, 99])
    # q0 (a): best positive 5 (key 1); others: 4 < 5, 5 ties and counts, 1 < 5               -> 2
    # q1 (b): best 4; others 3, 5, 5, 1: two are not below                                    -> 3
    # q2 (c): best 5 (key 3); others 3, 5 (ties), 4                                           -> 2
    # q3 (a, negated): s = -3, -5, -4, -5, -1: best positive -3; others -4, -5, -1: one       -> 2
    # q4 (no key of its group): d = NaN, all five count                                       -> 6
    assert R.grouped_ranks_np(q, k, qg, kg).tolist() == [2, 3, 2, 2, 6]
    # kcount takes keys 1 and 3 out of the competitors; key 1 stays q0's best positive
    cnt = np.array([1, 0, 1, 0, 1])
    assert R.grouped_ranks_np(q, k, qg, kg, cnt).tolist() == [1, 1, 1, 2, 4]
    d, pos = R.best_positive(R.similarities(q, k), qg, kg)
    assert d[:4].tolist() == [5.0, 4.0, 5.0, -3.0] and np.isnan(d[4])
    assert pos.sum(1).tolist() == [2, 1, 2, 2, 0]


def test_restatement_nan_rules():
    k = np.array([[1.0], [np.nan], [2.0], [0.5]])
    kg = np.array([0, 0, 0, 1])
    q = np.array([[1.0], [1.0]])
    # q0: a NaN among its positives -> d NaN -> the one key of another group counts
    # q1 (group 1): best 0.5; the others 1, NaN, 2 all count (NaN is not below)
    assert R.grouped_ranks_np(q, k, np.array([0, 1]), kg).tolist() == [2, 4]


def test_restatement_with_distinct_groups_is_the_one_positive_definition():
    rng = np.random.default_rng(0)
    q, k = rng.integers(-3, 4, (9, 2)).astype(np.float64), rng.integers(-3, 4, (9, 2)).astype(np.float64)
    S = q @ k.T
    want = [1 + sum(1 for j in range(9) if j != i and not S[i, j] < S[i, i]) for i in range(9)]
    ids = rng.permutation(9) * 1000 - 4000
    assert R.grouped_ranks_np(q, k, ids, ids).tolist() == want


def test_same_forces_copied_columns_equal():
    q = np.array([[0.1, 0.2, 0.3]])
    k = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]])
    S = R.similarities(q, k, same=[(0, 1)])
    assert S[0, 0] == S[0, 1]
    assert R.grouped_ranks_np(q, k, [0], [0, 1], same=[(0, 1)]).tolist() == [2]      # the copy in another group ties and counts
    assert R.grouped_ranks_np(q, k, [0], [0, 0], same=[(0, 1)]).tolist() == [1]      # in the own group it does not


# ------------------------------------------------------------------ first of group and the summary over it
def test_first_of_group_on_host_arrays_and_tensors():
    g = np.array([5, 3, 5, 5, -1, 3, 1 << 40], dtype=np.int64)
    want = [True, True, False, False, True, False, True]
    assert R.first_of_group_np(g).tolist() == want
    perm = np.argsort(g, kind="stable")
    assert first_of_group(g[perm], perm).tolist() == want
    t = torch.from_numpy(g)
    assert first_of_group(*torch.sort(t, stable=True)).tolist() == want
    assert first_of_group(*torch.sort(torch.tensor([4]), stable=True)).tolist() == [True]


def test_metric_restatement_counts_a_sample_once():
    # three samples; sample 0 has three slides, sample 1 one, sample 2 two.  RNA rows repeat per slide.  D = 2.
    group = np.array([10, 10, 11, 12, 10, 12])
    rna_of = {10: [4.0, 0.0], 11: [0.0, 4.0], 12: [-4.0, 0.0]}
    r = np.array([rna_of[g] for g in group.tolist()])
    w = r + np.array([[0, 1], [1, 0], [0, 0], [0, 1], [0, -1], [-1, 0]], dtype=np.float64)
    got = R.grouped_metric_np(w, r, group, ks=(1, 2))
    assert got["retrieval_n"] == 6 and got["retrieval_groups"] == 3
    assert got["wsi2rna_r@1"] == 1.0 and got["rna2wsi_r@1"] == 1.0 and got["r_mean"] == 1.0
    assert got["wsi2rna_meanr"] == 1.0 and got["rna2wsi_medr"] == 1.0
    assert list(got) == ["wsi2rna_r@1", "wsi2rna_r@2", "wsi2rna_medr", "wsi2rna_meanr", "rna2wsi_r@1", "rna2wsi_r@2", "rna2wsi_medr",
                         "rna2wsi_meanr", "r_mean", "retrieval_n", "retrieval_groups"]
    # one bad sample: its single slide points at sample 10's profile.  wsi2rna: 1 of 6 slides wrong; rna2wsi: 1 of 3 SAMPLES wrong
    w[2] = [4.5, 0.0]
    got = R.grouped_metric_np(w, r, group, ks=(1, 2))
    assert got["wsi2rna_r@1"] == 5 / 6 and got["rna2wsi_r@1"] == 2 / 3
    # the one-to-one definition on the same rows is capped by the duplicated RNA rows: only sample 11's slide could rank first
    S = w @ r.T
    plain = [1 + sum(1 for j in range(6) if j != i and not S[i, j] < S[i, i]) for i in range(6)]
    assert sum(1 for x in plain if x == 1) == 0


# ------------------------------------------------------------------ argument checks that need no device
def test_mixed_group_and_plain_updates_raise_at_the_offending_update():
    x = torch.randn(4, 8)
    m = CrossModalRetrieval(device="cuda:0")
    m.wsi.append(x), m.rna.append(x), m.group.append(torch.arange(4))        # the state after a grouped update (no device touched)
    with pytest.raises(ValueError, match="every update"):
        m.update(x, x)
    m = CrossModalRetrieval(device="cuda:0")
    m.wsi.append(x), m.rna.append(x)                                          # ... and after a plain one
    with pytest.raises(ValueError, match="every update"):
        m.update(x, x, group=torch.arange(4))
    a, b = CrossModalRetrieval(device="cuda:0"), CrossModalRetrieval(device="cuda:0")
    a.wsi.append(x), a.rna.append(x), a.group.append(torch.arange(4))
    b.wsi.append(x), b.rna.append(x)
    with pytest.raises(ValueError, match="merge"):
        a.merge_state([b])
    assert a.reset().group == []


def test_update_checks_the_group_tensor():
    x = torch.randn(4, 8)
    m = CrossModalRetrieval(device="cuda:0")
    for bad in (torch.arange(5), torch.arange(4).float(), torch.zeros(4, 1, dtype=torch.int64), [0, 1, 2, 3]):
        with pytest.raises(ValueError, match="group"):
            m.update(x, x, group=bad)
    assert m.wsi == [] and m.group == []


def test_target_and_groups_together_raise():
    q, k = torch.randn(3, 8), torch.randn(5, 8)
    with pytest.raises(ValueError, match="target"):
        retrieval_ranks(q, k, torch.tensor([0, 1, 2]), query_group=torch.arange(3), key_group=torch.arange(5))
    with pytest.raises(ValueError, match="go together"):
        retrieval_ranks(q, k, query_group=torch.arange(3))
    with pytest.raises(ValueError, match="key_count"):
        retrieval_ranks(q, q, key_count=torch.ones(3, dtype=torch.bool))


def test_wrong_id_length_or_dtype_raises():
    q, k = torch.randn(3, 8), torch.randn(5, 8)
    qg, kg = torch.arange(3), torch.arange(5)
    for fn in (K.retrieval_ranks_grouped, lambda *a: retrieval_ranks(a[0], a[1], query_group=a[2], key_group=a[3],
                                                                      key_count=a[4] if len(a) > 4 else None)):
        with pytest.raises(ValueError, match="qgroup"):
            fn(q, k, torch.arange(4), kg)
        with pytest.raises(ValueError, match="kgroup"):
            fn(q, k, qg, torch.arange(3))
        with pytest.raises(ValueError, match="qgroup"):
            fn(q, k, qg.float(), kg)
        with pytest.raises(ValueError, match="kgroup"):
            fn(q, k, qg, kg.to(torch.int16))
        with pytest.raises(ValueError, match="kcount"):
            fn(q, k, qg, kg, torch.ones(3, dtype=torch.bool))
        with pytest.raises(ValueError, match="kcount"):
            fn(q, k, qg, kg, torch.ones(5))
        with pytest.raises(ValueError, match="share D"):
            fn(q, torch.randn(5, 9), qg, kg)
        with pytest.raises(MirrorHipError):                  # all checks passed: host tensors are refused, not computed on the host
            fn(q, k, qg, kg)
        with pytest.raises(MirrorHipError):
            fn(q, k, qg.to(torch.int32), kg.to(torch.int32), torch.ones(5, dtype=torch.bool))


# ------------------------------------------------------------------ the declaration
def test_header_declares_the_entry_point_and_the_ctypes_row_matches():
    with open(os.path.join(ROOT, "include", "mirror_hip.h")) as f:
        header = f.read()
    m = re.search(r"\bint\s+mh_retrieval_ranks_grouped\s*\(([^)]*)\)\s*;", header)
    assert m, "include/mirror_hip.h does not declare mh_retrieval_ranks_grouped"
    args = [a.strip() for a in m.group(1).split(",")]
    assert args[-1] == "mh_stream s"
    P, L, I = _lib.P, _lib.L, _lib.I
    want = []
    for a in args[:-1]:
        if "*" in a:
            want.append(P)
        elif a.startswith("int64_t"):
            want.append(L)
        else:
            assert a.startswith("int "), a
            want.append(I)
    assert _lib._SIGS["mh_retrieval_ranks_grouped"] == want
    assert [a.split()[-1].lstrip("*") for a in args[:-1]] == ["q", "k", "nq", "nk", "D", "qgroup", "kgroup", "kgroup_sorted", "kperm",
                                                              "kcount", "ranks", "workspace"]
    assert "mh_retrieval_ranks_grouped" in _lib.EXPORTS and "mh_retrieval_workspace_bytes" in _lib.EXPORTS
    assert re.search(r"\bint64_t\s+mh_retrieval_workspace_bytes\s*\(", header)
    assert _lib._SIGS["mh_retrieval_ranks"] == [P, P, L, L, I, P, P, P]      # the ungrouped call is as it was
    assert _lib.ABI_VERSION == 123
