"""InfoNCE with explicit negative keys: what can be checked without a GPU — the ABI, the input checks of losses/info_nce.py:85-120
with `negative_keys` present, and the self-consistency of tests/golden/golden_infonce_neg.npz (tools/make_golden_infonce_neg.py).

`nce_ref` below is the definition the feature implements, restated in torch (any dtype; the tests use f64): the reference's
logits (losses/info_nce.py:126-143) followed by the `F.cross_entropy(logits / temperature, labels)` its branch forgets.
"""
import os
import re

import numpy as np
import pytest
import torch

from mirror_amd import _lib
from mirror_amd.losses import InfoNCE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_infonce_neg.npz")
ENTRY_POINTS = ("mh_infonce_paired_fwd", "mh_infonce_paired_bwd", "mh_infonce_rows_fwd", "mh_infonce_rows_bwd", "mh_infonce_fold")
MODES = ("paired", "unpaired")
TEMPERATURES = (0.07, 0.5)
REDUCTIONS = ("mean", "sum", "none")


def nce_ref(query, positive_key, negative_keys, temperature, reduction, mode):
    """F.normalize(dim=-1) on all three, pos = q^.k^, neg = q^ n^T (unpaired) or q^[i].n^[i, j] (paired),
    CE(cat([pos, neg], 1) / temperature, label 0) with the given reduction."""
    def normalize(x):
        return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    q, k, n = normalize(query), normalize(positive_key), normalize(negative_keys)
    pos = (q * k).sum(-1, keepdim=True)
    neg = q @ n.t() if mode == "unpaired" else torch.einsum("id,ijd->ij", q, n)
    logits = torch.cat([pos, neg], 1) / temperature
    rows = torch.logsumexp(logits, 1) - logits[:, 0]
    return rows.mean() if reduction == "mean" else rows.sum() if reduction == "sum" else rows


def nce_ref_grads(query, positive_key, negative_keys, temperature, reduction, mode, w=None):
    """(loss, dquery, dpositive_key, dnegative_keys) of nce_ref in the inputs' dtype; "none" differentiates sum(w * loss)."""
    q, k, n = (x.detach().clone().requires_grad_(True) for x in (query, positive_key, negative_keys))
    loss = nce_ref(q, k, n, temperature, reduction, mode)
    ((loss * w).sum() if reduction == "none" else loss).backward()
    return loss.detach(), q.grad, k.grad, n.grad


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mirror_hip.h")).read()
    declared = set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert name in _lib.EXPORTS and name in _lib._SIGS, name
        assert hasattr(lib, name), name
    assert lib.mh_version() == 123 and _lib.ABI_VERSION == 123
    assert "losses/info_nce.py:126-143" in header


def _t(*shape):
    return torch.randn(*shape)


@pytest.mark.parametrize("args, kw, msg", [
    ((_t(4), _t(4, 8), _t(5, 8)), {}, "<query> must have 2 dimensions."),
    ((_t(4, 8), _t(4), _t(5, 8)), {}, "<positive_key> must have 2 dimensions."),
    ((_t(4, 8), _t(4, 8), _t(4, 5, 8)), {"negative_mode": "unpaired"}, "<negative_keys> must have 2 dimensions if <negative_mode> == 'unpaired'."),
    ((_t(4, 8), _t(4, 8), _t(5, 8)), {"negative_mode": "paired"}, "<negative_keys> must have 3 dimensions if <negative_mode> == 'paired'."),
    ((_t(4, 8), _t(3, 8), _t(5, 8)), {}, "<query> and <positive_key> must must have the same number of samples."),
    ((_t(4, 8), _t(4, 8), _t(3, 5, 8)), {"negative_mode": "paired"},
     "If negative_mode == 'paired', then <negative_keys> must have the same number of samples as <query>."),
    ((_t(4, 8), _t(4, 7), _t(5, 8)), {}, "Vectors of <query> and <positive_key> should have the same number of components."),
    ((_t(4, 8), _t(4, 8), _t(5, 7)), {}, "Vectors of <query> and <negative_keys> should have the same number of components."),
    ((_t(4, 8), _t(4, 8), _t(4, 5, 7)), {"negative_mode": "paired"},
     "Vectors of <query> and <negative_keys> should have the same number of components."),
])
def test_input_checks_keep_the_reference_messages(args, kw, msg):
    with pytest.raises(ValueError, match=re.escape(msg)):
        InfoNCE(**kw)(*args)


def test_checks_keep_the_reference_order():
    # two violations at once: the earlier check of losses/info_nce.py:85-120 speaks
    with pytest.raises(ValueError, match="<query> must have 2 dimensions."):
        InfoNCE()(_t(4), _t(3), _t(5, 7))
    with pytest.raises(ValueError, match="same number of samples"):
        InfoNCE()(_t(4, 8), _t(3, 7), _t(5, 6))
    with pytest.raises(ValueError, match="<query> and <negative_keys> should have"):
        InfoNCE(reduction="bogus")(_t(4, 8), _t(4, 8), _t(5, 7))


@pytest.mark.parametrize("mode, neg", [("unpaired", (5, 8)), ("paired", (4, 5, 8))])
def test_bad_reduction_mode_and_empty_negatives_are_value_errors(mode, neg):
    q, k, n = _t(4, 8), _t(4, 8), _t(*neg)
    with pytest.raises(ValueError, match="bogus is not a valid value for reduction"):
        InfoNCE(reduction="bogus", negative_mode=mode)(q, k, n)
    with pytest.raises(ValueError, match="bogus is not a valid value for reduction"):
        InfoNCE(reduction="bogus")(q, k)                               # the implicit branch's message is the same one
    with pytest.raises(ValueError, match="negative_mode"):
        InfoNCE(negative_mode="both")(q, k, n)
    with pytest.raises(ValueError, match="negative_mode"):
        InfoNCE(negative_mode=None)(q, k, n)
    empty = n[:0] if mode == "unpaired" else n[:, :0]
    with pytest.raises(ValueError, match="at least one negative key"):
        InfoNCE(negative_mode=mode)(q, k, empty)


@pytest.mark.parametrize("mode, neg", [("unpaired", (5, 8)), ("paired", (4, 5, 8))])
@pytest.mark.parametrize("symmetric", [False, True])
def test_cpu_tensors_are_refused_not_unimplemented(mode, neg, symmetric):
    """Valid shapes on the CPU: there is no CPU fallback, and the branch is no longer `NotImplementedError`."""
    with pytest.raises(_lib.MirrorHipError):
        InfoNCE(negative_mode=mode, symmetric=symmetric)(_t(4, 8), _t(4, 8), _t(*neg))


@pytest.mark.parametrize("mode", MODES)
def test_fixture_is_self_consistent(mode):
    z = np.load(GOLDEN)
    q, k, n, w = (torch.from_numpy(z[f"{mode}/{nm}"]) for nm in ("query", "positive_key", "negative_keys", "w"))
    assert q.dtype == torch.float64 and n.shape[-1] == q.shape[1]
    for x in (q, k, n):
        assert torch.equal(x.float().double(), x)                      # the inputs are exact in f32
    for t in TEMPERATURES:
        for red in REDUCTIONS:
            got = nce_ref_grads(q, k, n, t, red, mode, w)
            for g, nm in zip(got, ("loss", "dquery", "dpositive_key", "dnegative_keys")):
                want = z[f"{mode}/t{t}/{red}/{nm}"]
                assert g.shape == want.shape
                np.testing.assert_allclose(g.numpy(), want, rtol=1e-12, atol=1e-12, err_msg=f"{mode} t{t} {red} {nm}")
