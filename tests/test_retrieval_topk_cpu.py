"""No GPU: the host side of top-k retrieval and the kNN probe.  The float64 restatements (tests/retrieval_topk_ref.py) against hand-worked
cases, the argument checks of the wrappers that raise before any launch, and the declarations against their ctypes rows."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from mirror_amd import _lib
from mirror_amd import kernels as K
from mirror_amd._lib import MirrorHipError
from mirror_amd.knn import KNNProbe
from mirror_amd.retrieval import CrossModalRetrieval, retrieval_topk
from tests import retrieval_topk_ref as R

INF = np.inf


# ------------------------------------------------------------------ the restatements, by hand
def test_topk_ties_are_broken_by_the_smaller_index():
    # D = 1: s_0j = k_j = 2, 5, 5, 1, 5
    k = np.array([[2.0], [5.0], [5.0], [1.0], [5.0]])
    idx, val = R.topk_np(np.array([[1.0]]), k, 4)
    assert idx.tolist() == [[1, 2, 4, 0]] and val.tolist() == [[5.0, 5.0, 5.0, 2.0]]
    idx, val = R.topk_np(np.array([[-1.0]]), k, 2)                     # negated: -1 is the largest, then -2
    assert idx.tolist() == [[3, 0]] and val.tolist() == [[-1.0, -2.0]]


def test_topk_group_exclusion_compares_all_64_bits():
    a, b = 7, 7 + (1 << 32)
    k = np.array([[3.0], [5.0], [4.0], [6.0]])
    kg = np.array([a, a, b, b])
    q = np.array([[1.0], [1.0], [1.0]])
    idx, val = R.topk_np(q, k, 3, qgroup=np.array([a, b, 99]), kgroup=kg)
    # q0 (a): keys 2, 3 remain; q1 (b): keys 0, 1; q2: nothing excluded
    assert idx.tolist() == [[3, 2, -1], [1, 0, -1], [3, 1, 2]]
    assert val.tolist() == [[6.0, 4.0, -INF], [5.0, 3.0, -INF], [6.0, 5.0, 4.0]]


def test_topk_kk_above_nk_leaves_empty_slots():
    idx, val = R.topk_np(np.array([[2.0]]), np.array([[1.0], [3.0]]), 5)
    assert idx.tolist() == [[1, 0, -1, -1, -1]] and val.tolist() == [[6.0, 2.0, -INF, -INF, -INF]]


def test_topk_nan_key_is_never_listed_and_nan_query_lists_nothing():
    k = np.array([[1.0], [np.nan], [3.0]])
    q = np.array([[1.0], [np.nan]])
    idx, val = R.topk_np(q, k, 3)
    assert idx.tolist() == [[2, 0, -1], [-1, -1, -1]]
    assert val.tolist() == [[3.0, 1.0, -INF], [-INF, -INF, -INF]]
    # a key whose similarity is really -inf is eligible and sorts before the empty slots
    idx, val = R.topk_np(None, None, 3, S=np.array([[-INF, np.nan, 0.0]]))
    assert idx.tolist() == [[2, 0, -1]]


def test_knn_vote_with_empty_slots_and_an_out_of_range_label():
    labels = np.array([0, 1, 1, 7, 2])                                  # label 7 is outside [0, 3)
    idx = np.array([[1, 0, 3, 2, -1], [-1, -1, -1, -1, -1], [3, -1, -1, -1, -1]])
    val = np.array([[2.0, 1.0, 1.0, 0.0, -INF], [-INF] * 5, [4.0] + [-INF] * 4])
    s = R.knn_scores_np(idx, val, labels, 3, 1.0)
    e1, e2 = math.exp(-1.0), math.exp(-2.0)
    tot = 1.0 + e1 + e2                                                 # slot 2 (label 7) and slot 4 (empty) contribute nothing
    np.testing.assert_allclose(s[0], [e1 / tot, (1.0 + e2) / tot, 0.0], rtol=1e-15)
    assert s[1].tolist() == [0.0, 0.0, 0.0] and s[2].tolist() == [0.0, 0.0, 0.0]
    u = R.knn_scores_np(idx, val, labels, 3, 0.0)                       # the unweighted vote
    np.testing.assert_allclose(u[0], [1 / 3, 2 / 3, 0.0], rtol=1e-15)
    assert R.knn_scores_np(idx[:1], val[:1], labels, 1, 1.0).tolist() == [[1.0]]      # C = 1: only label 0 votes


# ------------------------------------------------------------------ argument checks that raise before any launch
def _f(*shape):
    return torch.zeros(shape, dtype=torch.float32)


def test_retrieval_topk_argument_checks():
    q, k = _f(4, 8), _f(6, 8)
    with pytest.raises(ValueError, match="share D"):
        K.retrieval_topk(q, _f(6, 7), 2)
    with pytest.raises(ValueError, match="share D"):
        K.retrieval_topk(_f(4), k, 2)
    for bad in (0, 65, -1, 2.0, True):
        with pytest.raises(ValueError, match="kk must be"):
            K.retrieval_topk(q, k, bad)
    with pytest.raises(ValueError, match="parts must be"):
        K.retrieval_topk(q, k, 2, parts=-1)
    ids4, ids6 = torch.arange(4), torch.arange(6)
    with pytest.raises(ValueError, match="go together"):
        K.retrieval_topk(q, k, 2, qgroup=ids4)
    with pytest.raises(ValueError, match="go together"):
        retrieval_topk(q, k, 2, key_group=ids6)
    with pytest.raises(ValueError, match="qgroup must be int32 / int64"):
        K.retrieval_topk(q, k, 2, ids4.float(), ids6)
    with pytest.raises(ValueError, match=r"kgroup must be int32 / int64 \[6\]"):
        K.retrieval_topk(q, k, 2, ids4, ids4)
    with pytest.raises(MirrorHipError, match="HIP device tensors"):    # host tensors: no CPU fallback
        K.retrieval_topk(q, k, 2)
    with pytest.raises(ValueError, match=r"must be \[n, D\]"):
        retrieval_topk(_f(4), k, 2, normalize=True)


def test_knn_scores_argument_checks():
    idx, val, labels = torch.zeros((3, 4), dtype=torch.int32), _f(3, 4), torch.zeros(9, dtype=torch.int64)
    with pytest.raises(ValueError, match="both be"):
        K.knn_scores(idx, _f(3, 5), labels, 2, 1.0)
    with pytest.raises(ValueError, match="int32 and val f32"):
        K.knn_scores(idx.long(), val, labels, 2, 1.0)
    with pytest.raises(ValueError, match="labels must be"):
        K.knn_scores(idx, val, labels.float(), 2, 1.0)
    for bad in (0, 1025, 2.0):
        with pytest.raises(ValueError, match="num_classes must be"):
            K.knn_scores(idx, val, labels, bad, 1.0)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="inv_temperature must be"):
            K.knn_scores(idx, val, labels, 2, bad)
    with pytest.raises(ValueError, match="outside"):
        K.knn_scores(torch.zeros((3, 65), dtype=torch.int32), _f(3, 65), labels, 2, 1.0)
    with pytest.raises(MirrorHipError, match="HIP device tensors"):
        K.knn_scores(idx, val, labels, 2, 1.0)


def test_public_argument_checks():
    with pytest.raises(ValueError, match="direction"):
        CrossModalRetrieval.topk(object.__new__(CrossModalRetrieval), 3, direction="both")
    for kw in (dict(num_classes=1), dict(num_classes=4, k=0), dict(num_classes=4, k=65), dict(num_classes=4, temperature=0.0),
               dict(num_classes=4, average="none")):
        with pytest.raises(ValueError):
            KNNProbe(device="cuda", **kw)
    with pytest.raises(MirrorHipError, match="HIP device"):
        KNNProbe(4, device="cpu")
    p = KNNProbe(4, k=5, temperature=math.inf, device="cuda")
    assert p.inv_temperature == 0.0 and KNNProbe(4, device="cuda").inv_temperature == pytest.approx(1 / 0.07)
    with pytest.raises(ValueError, match="emb must be"):
        p.fit(torch.zeros((3, 2), dtype=torch.int64), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="labels must be"):
        p.fit(_f(3, 2), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="group must be"):
        p.fit(_f(3, 2), torch.zeros(3, dtype=torch.int64), group=torch.zeros(3))
    with pytest.raises(ValueError, match="bank is empty"):
        p.leave_one_out()
    with pytest.raises(ValueError, match="bank is empty"):
        p.scores(_f(3, 2))


# ------------------------------------------------------------------ the declarations
def test_the_three_entry_points_are_bound_within_the_same_abi_generation():
    assert _lib.ABI_VERSION == 123
    assert _lib._SIGS["mh_retrieval_topk"] == [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert _lib._SIGS["mh_knn_scores"] == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_void_p]
    for name in ("mh_retrieval_topk", "mh_knn_scores", "mh_retrieval_topk_workspace_bytes"):
        assert name in _lib.EXPORTS
    assert "mh_retrieval_topk_workspace_bytes" not in _lib._SIGS      # no stream argument: bound by hand, with its int64 result
    lib = _lib.load()
    assert lib.mh_version() == 123
    ws = lib.mh_retrieval_topk_workspace_bytes
    assert ws.restype is C.c_int64
    # 8 bytes per (query, strip, slot); parts above the number of key tiles (ceil(nk / 128)) is cut to it
    assert ws(1000, 1000, 256, 16, 3) == 1000 * 3 * 16 * 8
    assert ws(5, 3, 7, 5, 3) == 5 * 1 * 5 * 8
    assert ws(200, 700, 96, 32, 9) == 200 * 6 * 32 * 8
    chosen = ws(1024, 1 << 17, 512, 20, 0)                              # the library's own choice: whole strips, at least one
    assert chosen % (1024 * 20 * 8) == 0 and 1 <= chosen // (1024 * 20 * 8) <= 1024
    assert ws(1 << 20, 1 << 20, 512, 64, 16) == (1 << 20) * 16 * 64 * 8 > (1 << 32)    # a size that needs the 64-bit result
