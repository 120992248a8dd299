"""Host side of the cross-modal retrieval metrics (mirror_amd/retrieval.py): summarize_ranks against hand-worked vectors, the
key order of the dicts, and the argument checks that need no device."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from mirror_amd import kernels as K
from mirror_amd._lib import MirrorHipError
from mirror_amd.retrieval import CrossModalRetrieval, retrieval_ranks, summarize_ranks


def test_summarize_ranks_hand_worked():
    got = summarize_ranks(np.array([1, 3, 7, 12, 2], dtype=np.int32))
    assert isinstance(got, OrderedDict)
    assert list(got) == ["r@1", "r@5", "r@10", "medr", "meanr"]
    assert got == {"r@1": 1 / 5, "r@5": 3 / 5, "r@10": 4 / 5, "medr": 3.0, "meanr": 5.0}


def test_summarize_ranks_even_length_median_and_k_beyond_the_gallery():
    got = summarize_ranks([4, 1, 2, 3], ks=(2, 50))         # a gallery of 4: every rank is <= 50
    assert list(got) == ["r@2", "r@50", "medr", "meanr"]
    assert got == {"r@2": 0.5, "r@50": 1.0, "medr": 2.5, "meanr": 2.5}
    got = summarize_ranks(np.array([6, 6]), ks=(1, 5, 10))
    assert got == {"r@1": 0.0, "r@5": 0.0, "r@10": 1.0, "medr": 6.0, "meanr": 6.0}


def test_summarize_ranks_takes_a_2d_or_int64_array_and_refuses_an_empty_one():
    assert summarize_ranks(np.array([[1], [2]], dtype=np.int64), ks=(1,)) == {"r@1": 0.5, "medr": 1.5, "meanr": 1.5}
    with pytest.raises(ValueError):
        summarize_ranks(np.zeros((0,), dtype=np.int32))


def test_cpu_tensors_are_refused_not_computed_on_the_host():
    q, k = torch.randn(6, 8), torch.randn(6, 8)
    for fn in (K.retrieval_ranks, retrieval_ranks):
        with pytest.raises(MirrorHipError):
            fn(q, k)
    with pytest.raises(MirrorHipError):
        retrieval_ranks(q, k, normalize=True)
    with pytest.raises(MirrorHipError):
        retrieval_ranks(q, k, torch.arange(6))


def test_missing_target_needs_a_square_problem():
    q, k = torch.randn(6, 8), torch.randn(7, 8)
    for fn in (K.retrieval_ranks, retrieval_ranks):
        with pytest.raises(ValueError, match="nq == nk"):
            fn(q, k)


def test_host_target_is_range_and_shape_checked():
    q, k = torch.randn(3, 8), torch.randn(7, 8)
    with pytest.raises(ValueError, match="outside"):
        K.retrieval_ranks(q, k, torch.tensor([0, 7, 1]))
    with pytest.raises(ValueError, match="outside"):
        K.retrieval_ranks(q, k, torch.tensor([0, -1, 1]))
    with pytest.raises(ValueError):
        K.retrieval_ranks(q, k, torch.tensor([0, 1]))                 # one target per query
    with pytest.raises(ValueError):
        K.retrieval_ranks(q, k, torch.tensor([0.0, 1.0, 2.0]))        # integer targets
    with pytest.raises(ValueError):
        K.retrieval_ranks(q, torch.randn(7, 9))                       # one D


def test_metric_object_checks_without_a_device():
    with pytest.raises(MirrorHipError):
        CrossModalRetrieval(device="cpu")
    with pytest.raises(ValueError):
        CrossModalRetrieval(ks=(0, 5), device="cuda:0")
    m = CrossModalRetrieval(device="cuda:0")                           # constructing touches no device
    assert m.ks == (1, 5, 10) and m.normalize is False
    with pytest.raises(ValueError, match="no samples"):
        m.compute()
    with pytest.raises(ValueError):
        m.update(torch.randn(4, 8), torch.randn(5, 8))
    assert m.reset() is m and m.merge_state([]) is m
    with pytest.raises(ValueError, match="no samples"):
        m.compute()
