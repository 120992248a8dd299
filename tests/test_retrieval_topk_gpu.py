"""MI355X: mh_retrieval_topk (csrc/retrieval_topk.hip) and its public face (mirror_amd/retrieval.py), against the float64 restatement of
tests/retrieval_topk_ref.py: a stable descending sort of the eligible similarities.  Integer-valued inputs make every f32 dot product
exact, so indices and values must be EQUAL, ties (broken by the smaller index) included; Gaussian inputs are compared on queries that
float64 decides with the project's margin 1e-5 |q_i| |k_j|; the ranks kernel decides by the bit-identical chain, so against it there is
no tolerance at all."""
import numpy as np
import pytest
import torch

from mirror_amd.retrieval import CrossModalRetrieval, retrieval_ranks, retrieval_topk
from tests import retrieval_topk_ref as R

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()       # a copy: the shared inputs are read-only


def int_data(n, D, seed):
    return np.random.default_rng(seed).integers(-3, 4, size=(n, D)).astype(np.float32)


def got(q, k, kk, qgroup=None, kgroup=None, **kw):
    val, idx = retrieval_topk(dev(q), dev(k), kk, None if qgroup is None else dev(np.asarray(qgroup)),
                              None if kgroup is None else dev(np.asarray(kgroup)), **kw)
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and tuple(idx.shape) == tuple(val.shape) == (q.shape[0], kk)
    return idx.cpu().numpy().astype(np.int64), val.cpu().numpy().astype(np.float64)


def assert_equal(res, want, what=""):
    (idx, val), (widx, wval) = res, want
    bad = int((idx != widx).any(1).sum())
    print(f"{what}: {bad} rows differ, {int((widx < 0).sum())} empty slots")
    assert np.array_equal(idx, widx)
    assert np.array_equal(val, wval)                       # -inf == -inf; exact products


# ------------------------------------------------------------------ 1. exact, integer-valued inputs
INT_SHAPES = [(1, 1, 1, 1), (5, 3, 7, 5), (67, 67, 40, 1), (130, 257, 100, 10), (257, 130, 513, 64), (200, 700, 96, 32)]
_INT = {}


def int_case(nq, nk, D, kk):
    """Inputs and the restatement, computed once per shape and left unchanged."""
    key = (nq, nk, D, kk)
    if key not in _INT:
        q, k = int_data(nq, D, 1), int_data(nk, D, 2)
        q[-1] = -k[nk // 2]                                # every similarity of this row tends negative: a zero-filled column past nk would outrank real keys
        for a in (q, k):
            a.setflags(write=False)
        _INT[key] = (q, k, R.topk_np(q, k, kk))
    return _INT[key]


@pytest.mark.parametrize("parts", [0, 1, 2, 3])
@pytest.mark.parametrize("nq,nk,D,kk", INT_SHAPES)
def test_integer_inputs_give_exactly_the_restated_neighbours(nq, nk, D, kk, parts):
    q, k, want = int_case(nq, nk, D, kk)
    res = got(q, k, kk, parts=parts)
    assert_equal(res, want, f"shape {(nq, nk, D, kk)} parts {parts}")
    idx, val = res
    assert (idx[:, :min(kk, nk)] >= 0).all() and (idx[:, nk:] == -1).all() and idx.max() < nk
    assert (val[:, 1:] <= val[:, :-1]).all()


def test_integer_inputs_tie_often_at_the_last_place():
    """The integer cases only test the tie rule if ties occur where the cut falls: at D = 1 at least half of the lists have a key equal to
    their kk-th just outside."""
    nq = nk = 300
    q, k = int_data(nq, 1, 4), int_data(nk, 1, 5)
    widx, wval = R.topk_np(q, k, 11)
    tied = int((wval[:, 9] == wval[:, 10]).sum())
    print(f"{tied} of {nq} lists tie at the 10th place")
    assert tied >= nq // 2
    for parts in (0, 3):
        assert_equal(got(q, k, 10, parts=parts), (widx[:, :10], wval[:, :10]), f"D = 1, parts {parts}")


# ------------------------------------------------------------------ 2. groups
def test_groups_exclude_by_all_64_bits_of_the_id():
    nq, nk, D, kk = 200, 700, 96, 32
    q, k, _ = int_case(nq, nk, D, kk)
    rng = np.random.default_rng(12)
    sizes = []
    while sum(sizes) < nk:
        sizes.append(int(rng.integers(1, 5)))
    kg = np.repeat(np.arange(len(sizes)) * 3 - 50, sizes)[:nk]         # groups of 1-4 keys, negative ids among them
    kg = kg[rng.permutation(nk)].astype(np.int64)
    low, high = int(kg[0]), int(kg[0]) + (1 << 32)                      # one id differs from another in its high word only
    kg[kg == kg[kg != low][0]] = high
    assert (kg == low).any() and (kg == high).any()
    qg = kg[rng.integers(0, nk, nq)].copy()
    qg[3], qg[4], qg[5] = low, high, 10 ** 15                           # and a query whose group has no key
    want = R.topk_np(q, k, kk, qg, kg)
    assert (want[0][[3, 4]] >= 0).all() and not np.array_equal(want[0][3], want[0][4])
    for parts in (0, 3):
        assert_equal(got(q, k, kk, qg, kg, parts=parts), want, f"int64 ids, parts {parts}")
    # int32 ids (widened by the wrapper): the same problem with the high id folded to a small fresh one
    kg32, qg32 = kg.copy(), qg.copy()
    kg32[kg == high], qg32[qg == high], qg32[5] = 10 ** 6, 10 ** 6, 10 ** 6 + 1
    assert_equal(got(q, k, kk, qg32.astype(np.int32), kg32.astype(np.int32)), R.topk_np(q, k, kk, qg32, kg32), "int32 ids")
    assert_equal(got(q, k, kk, qg32, kg32), R.topk_np(q, k, kk, qg32, kg32), "the same as int64")
    # one query's group covers all but 3 keys: 29 empty slots
    kg2, qg2 = kg.copy(), qg.copy()
    keep = np.array([1, 350, 699])
    big = -(1 << 40)
    kg2[np.setdiff1d(np.arange(nk), keep)] = big
    qg2[7] = big
    want2 = R.topk_np(q, k, kk, qg2, kg2)
    assert sorted(want2[0][7, :3].tolist()) == keep.tolist() and (want2[0][7, 3:] == -1).all()
    assert_equal(got(q, k, kk, qg2, kg2, parts=2), want2, "a group of 697 keys")


# ------------------------------------------------------------------ 3. Gaussian against float64
GAUSS = [(300, 512, 10, False, 17), (300, 512, 10, True, 11), (150, 768, 20, False, 0), (150, 768, 20, True, 0)]


@pytest.mark.parametrize("n,D,kk,normalize,seed", GAUSS)
def test_gaussian_neighbours_equal_float64_on_decided_queries(n, D, kk, normalize, seed):
    q, k = R.gauss_pairs(n, D, seed)
    q64, k64 = (R.unit(q), R.unit(k)) if normalize else (q.astype(np.float64), k.astype(np.float64))
    und = R.undecided_rows(q64, k64, kk)
    widx, wval = R.topk_np(q64, k64, kk)
    idx, val = got(q, k, kk, normalize=normalize)
    margin = R.MARGIN * np.linalg.norm(q64, axis=1)[:, None] * np.linalg.norm(k64, axis=1)[widx]
    print(f"n {n} D {D} kk {kk} normalize {normalize}: undecided {int(und.sum())} of {n}, decided rows that differ "
          f"{int((idx != widx).any(1)[~und].sum())}, max |val - f64| / margin {float((np.abs(val - wval) / margin).max()):.4f}")
    assert und.sum() <= 0.15 * n
    assert np.array_equal(idx[~und], widx[~und])
    assert (np.abs(val - wval) <= margin).all()            # on ALL queries: no row escapes


# ------------------------------------------------------------------ 4. agreement with the ranks, oracle-free
@pytest.mark.parametrize("parts", [0, 3])
def test_topk_and_ranks_decide_by_the_same_numbers(parts):
    n, D, kk = 1000, 256, 16
    q0, k0 = R.gauss_pairs(n, D, 40)
    q, k = dev(q0), dev(k0)
    ranks = retrieval_ranks(q, k).cpu().numpy().astype(np.int64)
    val, idx = retrieval_topk(q, k, kk, parts=parts)
    idx, val = idx.cpu().numpy().astype(np.int64), val.cpu().numpy()
    own = idx == np.arange(n)[:, None]
    listed = own.any(1)
    slot = own.argmax(1)
    print(f"parts {parts}: {int(listed.sum())} positives listed, {int((ranks <= kk).sum())} ranked <= {kk}")
    assert listed[ranks <= kk].all()                       # rank <= kk: the positive is among the kk best
    assert (ranks[listed] >= slot[listed] + 1).all()       # at slot s at least s keys are not below it (ties count against the rank)
    assert (ranks[listed] == slot[listed] + 1).sum() > n // 4
    assert (val[:, 1:] <= val[:, :-1]).all() and (idx >= 0).all()


# ------------------------------------------------------------------ 5. NaN
def test_a_nan_key_is_never_listed_and_a_nan_query_lists_nothing():
    nq, nk, D, kk = 150, 150, 24, 12
    q, k = int_data(nq, D, 7), int_data(nk, D, 8)
    base = got(q, k, kk)
    assert_equal(base, R.topk_np(q, k, kk), "no NaN")
    kn = k.copy()
    kn[140, 3] = np.nan
    idx, val = got(q, kn, kk, parts=2)
    assert not (idx == 140).any()
    widx, wval = R.topk_np(q, np.delete(k, 140, axis=0), kk)          # the problem with that key deleted, indices shifted
    assert_equal((idx, val), (widx + (widx >= 140), wval), "a NaN key")
    qn = q.copy()
    qn[41, 5] = np.nan
    idx, val = got(qn, k, kk)
    assert (idx[41] == -1).all() and np.isneginf(val[41]).all()
    rows = np.arange(nq) != 41
    assert np.array_equal(idx[rows], base[0][rows]) and np.array_equal(val[rows], base[1][rows])
    idx, val = got(q, np.full_like(k, np.nan), kk)                     # no eligible key at all
    assert (idx == -1).all() and np.isneginf(val).all()


# ------------------------------------------------------------------ 6. determinism and capture
def test_two_launches_are_bit_equal_and_a_graph_replay_follows_its_inputs():
    n, D, kk = 257, 96, 10
    q0, k0 = R.gauss_pairs(n, D, 30)
    q, k = dev(q0), dev(k0)
    a, b = retrieval_topk(q, k, kk, parts=2), retrieval_topk(q, k, kk, parts=2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    one = retrieval_topk(q, k, kk, parts=1)                # and the split of the keys does not show
    assert torch.equal(a[0], one[0]) and torch.equal(a[1], one[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        retrieval_topk(q, k, kk, parts=2)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = retrieval_topk(q, k, kk, parts=2)
    g.replay()
    assert torch.equal(out[0], a[0]) and torch.equal(out[1], a[1])
    q1, k1 = R.gauss_pairs(n, D, 31)
    q.copy_(dev(q1))
    k.copy_(dev(k1))
    g.replay()
    eager = retrieval_topk(q, k, kk, parts=2)
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    assert not torch.equal(eager[1], a[1])


# ------------------------------------------------------------------ 9. the metric object
@pytest.mark.parametrize("grouped", [False, True])
def test_metric_topk_in_chunks_both_directions(grouped):
    n, D, kk = 150, 64, 8
    w = int_data(n, D, 9) * 0.25
    r = (w + int_data(n, D, 10) * 0.5).astype(np.float32)             # multiples of 1/4: exact dot products, partly aligned pairs
    group = np.repeat(np.arange(60) * 5 + (1 << 33), 3)[:n] if grouped else None      # 50 samples of 3 slides
    m = CrossModalRetrieval()
    for sl in (slice(0, 50), slice(50, 51), slice(51, n)):
        m.update(dev(w[sl]), dev(r[sl]), None if group is None else dev(group[sl]))
    before = m.compute()
    own = group if grouped else np.arange(n)
    for direction, (a, b) in (("wsi2rna", (w, r)), ("rna2wsi", (r, w))):
        val, idx = m.topk(kk, direction)
        assert_equal((idx.cpu().numpy().astype(np.int64), val.cpu().numpy().astype(np.float64)), R.topk_np(a, b, kk), f"{direction}")
        val, idx = m.topk(kk, direction, exclude_own_group=True)
        idx = idx.cpu().numpy().astype(np.int64)
        assert_equal((idx, val.cpu().numpy().astype(np.float64)), R.topk_np(a, b, kk, own, own), f"{direction}, own group excluded")
        assert (own[idx] != own[:, None]).all()
    listed = (m.topk(kk)[1].cpu().numpy() == np.arange(n)[:, None]).any(1)
    assert 0 < listed.sum()                                # without the flag the positive appears where it ranks
    assert m.compute() == before and list(m.compute()) == list(before)
    with pytest.raises(ValueError, match="direction"):
        m.topk(kk, "both")
    with pytest.raises(ValueError, match="no samples"):
        CrossModalRetrieval().topk(kk)
