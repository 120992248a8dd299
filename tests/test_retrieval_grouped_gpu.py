"""MI355X: mh_retrieval_ranks_grouped (csrc/retrieval.hip), the ranks with several positives per query, and what is built on it:
retrieval.retrieval_ranks(query_group=, key_group=, key_count=), CrossModalRetrieval.update(group=), TrainEngine.validate with
three-item batches and metrics.sync_and_compute.  The yardstick is tests/retrieval_ref.py, the definition of include/mirror_hip.h in
float64 numpy.  Integer-valued inputs in [-8, 8] make every f32 dot product exact, so those ranks must be EQUAL, ties included;
Gaussian inputs are compared on queries that float64 decides with a margin of 1e-5 |q_i| |k_j| around the best positive (about 30x
the f32 fmaf-chain error at D <= 1024), at seeds where float64 decides every query (chosen on the host; asserted here)."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from mirror_amd.metrics import sync_and_compute
from mirror_amd.retrieval import CrossModalRetrieval, retrieval_ranks
from tests import retrieval_ref as R

pytestmark = pytest.mark.gpu

T = 128          # the kernel's tile edge (RT_TILE of csrc/retrieval.hip)


def int_data(n, D, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=(n, D)).astype(np.float32)


def random_groups(n, rng, lo=1, hi=7, ids=None):
    """n rows dealt to groups of random sizes lo..hi, rows shuffled; ids: the id of group g (default: scattered 64-bit values)."""
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(rng.integers(lo, hi + 1)))
    g = np.repeat(np.arange(len(sizes)), sizes)[:n]
    if ids is None:
        ids = rng.permutation(len(sizes)).astype(np.int64) * 7919 - 1000
    return np.asarray(ids, dtype=np.int64)[g][rng.permutation(n)]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def got(q, k, qg, kg, kc=None, **kw):
    r = retrieval_ranks(dev(q), dev(k), query_group=dev(np.asarray(qg, dtype=np.int64)), key_group=dev(np.asarray(kg, dtype=np.int64)),
                        key_count=None if kc is None else dev(np.asarray(kc)), **kw)
    assert r.dtype == torch.int32 and tuple(r.shape) == (q.shape[0],)
    return r.cpu().numpy().astype(np.int64)


def _unit(x):
    x = x.astype(np.float64)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)


# ------------------------------------------------------------------ 1. exact ranks on random groups
INT_SHAPES = [(1, 1, 1), (67, 67, 40), (130, 257, 96), (257, 130, 513), (2 * T + 1, 2 * T + 1, 33)]


@pytest.mark.parametrize("nq,nk,D", INT_SHAPES)
def test_integer_inputs_give_exactly_the_restated_ranks(nq, nk, D):
    q, k = int_data(nq, D, 1), int_data(nk, D, 2)
    rng = np.random.default_rng(3)
    kg = random_groups(nk, rng)
    qg = kg[rng.integers(0, nk, size=nq)]                  # every query's group has keys ...
    if nq > 4:
        qg[nq // 2] = 123456789012                         # ... but one
    if D > 1:
        # the last query (an edge tile in every shape) gets a negative best positive: a zero-filled column past nk would beat it
        kg[0] = qg[-1] = 555555                            # a group of one key
        q[-1] = -k[0]
        q[-1, 0] -= 1.0
        assert float(q[-1].astype(np.float64) @ k[0].astype(np.float64)) < 0
    kc = rng.integers(0, 2, size=nk)
    for cnt in (None, kc, kc.astype(bool)):
        want = R.grouped_ranks_np(q, k, qg, kg, cnt)
        r = got(q, k, qg, kg, cnt)
        print(f"shape {(nq, nk, D)} kcount {'no' if cnt is None else cnt.dtype}: {int((r != want).sum())} ranks differ; "
              f"{int((want > 1).sum())} rows ranked > 1, max {int(want.max())}")
        assert np.array_equal(r, want)
        assert r.min() >= 1 and r.max() <= nk + 1
    # int32 ids and host ids go through the same launch
    r32 = retrieval_ranks(dev(q), dev(k), query_group=dev((qg % 1000).astype(np.int32)), key_group=dev((kg % 1000).astype(np.int32)))
    assert np.array_equal(r32.cpu().numpy(), R.grouped_ranks_np(q, k, qg % 1000, kg % 1000))
    rh = retrieval_ranks(dev(q), dev(k), query_group=torch.from_numpy(qg), key_group=torch.from_numpy(kg), key_count=torch.from_numpy(kc))
    assert np.array_equal(rh.cpu().numpy(), R.grouped_ranks_np(q, k, qg, kg, kc))


# ------------------------------------------------------------------ 2. positives across tile borders
def test_positives_in_several_column_tiles_and_uncounted_border_columns():
    nq, nk, D = 70, 2 * T + 5, 24
    q, k = int_data(nq, D, 11), int_data(nk, D, 12)
    kg = np.arange(nk, dtype=np.int64) + 1000
    cols = [5, T - 1, T, 2 * T]
    kg[cols] = 77
    qg = kg[np.random.default_rng(13).integers(0, nk, size=nq)]
    qg[9] = 77
    kc = np.ones(nk, dtype=np.int64)
    kc[[T - 1, T, 2 * T - 1]] = 0
    for best in cols:                                       # the best positive sits in each of the three column tiles in turn
        kk = k.copy()
        kk[best] = q[9]                                     # q9 . q9 = |q9|^2 beats the other three positives
        S9 = q[9].astype(np.float64) @ kk.astype(np.float64).T
        assert int(np.argmax(S9[cols])) == cols.index(best)
        for cnt in (None, kc):
            want = R.grouped_ranks_np(q, kk, qg, kg, cnt)
            assert np.array_equal(got(q, kk, qg, kg, cnt), want)
    # kcount == 0 on a positive does not remove it from P_i: with only column T as the group, the rank uses its similarity
    kg2 = np.arange(nk, dtype=np.int64) + 1000
    kg2[T] = 77
    want = R.grouped_ranks_np(q, k, qg, kg2, kc)
    d, _ = R.best_positive(R.similarities(q, k), qg, kg2)
    assert not np.isnan(d[9])
    assert np.array_equal(got(q, k, qg, kg2, kc), want)


# ------------------------------------------------------------------ 3. extreme group shapes
def test_one_group_holding_every_key_ranks_everything_first():
    nq, nk, D = 131, 300, 17
    q, k = int_data(nq, D, 14), int_data(nk, D, 15)
    r = got(q, k, np.full(nq, -5), np.full(nk, -5))
    assert np.array_equal(r, np.ones(nq, dtype=np.int64))


def test_a_group_of_200_keys_and_a_query_without_any():
    nq, nk, D = 140, 330, 40
    q, k = int_data(nq, D, 16), int_data(nk, D, 17)
    rng = np.random.default_rng(18)
    kg = np.arange(nk, dtype=np.int64)
    big = rng.permutation(nk)[:200]                         # 200 keys of one group, scattered over the three column tiles
    kg[big] = 9999
    qg = kg[rng.integers(0, nk, size=nq)]
    qg[:20] = 9999
    qg[77] = -1                                             # no key has this id
    kc = rng.integers(0, 2, size=nk)
    for cnt in (None, kc):
        want = R.grouped_ranks_np(q, k, qg, kg, cnt)
        r = got(q, k, qg, kg, cnt)
        assert np.array_equal(r, want)
        assert r[77] == 1 + (nk if cnt is None else int(kc.sum()))
        assert (want[:20] <= nk - 200 + 1).all()


# ------------------------------------------------------------------ 4. 64-bit ids
def test_ids_that_differ_only_above_bit_31_are_different_groups_and_negative_ids_work():
    nq, nk, D = 133, 133, 20
    q, k = int_data(nq, D, 19), int_data(nk, D, 20)
    g0 = 123457
    ids = np.array([g0, g0 + (1 << 32), -g0, -g0 - (1 << 32), -(1 << 62), (1 << 62), 0, 1 << 32], dtype=np.int64)
    rng = np.random.default_rng(21)
    kg = ids[rng.integers(0, len(ids), size=nk)]
    qg = ids[rng.integers(0, len(ids), size=nq)]
    want = R.grouped_ranks_np(q, k, qg, kg)
    folded = R.grouped_ranks_np(q, k, qg.astype(np.int32), kg.astype(np.int32))
    assert not np.array_equal(want, folded)                 # a truncation to 32 bits would be seen
    assert np.array_equal(got(q, k, qg, kg), want)


# ------------------------------------------------------------------ 5. bit-exact ties
def gauss_pairs(n, D, seed):
    """Gaussian q; k_i = a_i q_i + sqrt(1 - a_i^2) noise with a_i spread over [0, 0.5]: some positives are weak enough to be
    outranked, the rest win, as in a half-trained alignment."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n, D)).astype(np.float32)
    a = rng.permutation(np.linspace(0.0, 0.5, n)).astype(np.float32)[:, None]
    k = (a * q + np.sqrt(1 - a * a) * rng.standard_normal((n, D)).astype(np.float32)).astype(np.float32)
    return q, k


@pytest.mark.parametrize("D,seed", [(40, 3), (513, 0)])
def test_a_copy_of_the_best_positive_counts_in_another_group_and_not_in_its_own(D, seed):
    n = 200
    q, k = gauss_pairs(n, D, seed)
    g = np.repeat(np.arange(n // 2, dtype=np.int64), 2)     # pairs (2m, 2m + 1) are one group
    same = []
    for i, own, other in ((4, 5, (60, 131, 197)), (150, 151, (0, 129)), (198, 199, (33,))):
        k[i] = 2.0 * q[i]                                   # key i is query i's best positive by a wide margin ...
        k[own] = k[i]                                       # ... its copy inside the group must not count
        same.append((i, own))
        for j in other:                                     # ... and its copies in other groups must
            k[j] = k[i]
            same.append((i, j))
    # the overwritten rows 60, 131, ... stay members of their own groups: only rows are copied, never ids
    assert R.grouped_undecided_np(q, k, g, g) == 0          # apart from the copies, float64 decides every query
    want = R.grouped_ranks_np(q, k, g, g, same=same)
    r = got(q, k, g, g)
    for i, copies in ((4, 3), (150, 2), (198, 1)):
        print(f"D {D} query {i}: rank {r[i]}, want {want[i]}, {copies} copies in other groups")
        assert r[i] == want[i] == 1 + copies                # the copies in other groups count, the one in the own group does not
    assert np.array_equal(r, want)                          # queries 5, 151, 199 included: both their positives are copies


# ------------------------------------------------------------------ 6. NaN
def test_nan_in_a_positive_and_in_a_competitor():
    nq = nk = 150
    q, k = int_data(nq, 24, 22), int_data(nk, 24, 23)
    g = np.arange(nk, dtype=np.int64) * 3
    g[[10, 70, 140]] = 5000                                 # a three-positive group, one positive per column tile
    kc = np.ones(nk, dtype=np.int64)
    kc[[3, 70, 99]] = 0
    base = got(q, k, g, g)
    assert np.array_equal(base, R.grouped_ranks_np(q, k, g, g))
    kn = k.copy()
    kn[70, 5] = np.nan                                      # a NaN in ONE of the three positives: d is NaN for queries 10, 70, 140
    for cnt in (None, kc):
        r = got(q, kn, g, g, cnt)
        counted = nk if cnt is None else int(kc.sum())
        want = R.grouped_ranks_np(q, kn, g, g, cnt)
        assert np.array_equal(r, want)
        for i in (10, 70, 140):                             # all counted non-positives: key 70 is uncounted AND a positive
            assert r[i] == 1 + counted - (3 if cnt is None else 2)
    others = np.setdiff1d(np.arange(nq), [10, 70, 140])
    without = R.grouped_ranks_np(q, np.delete(k, 70, axis=0), g, np.delete(g, 70))          # the same problem with key 70 taken out
    assert np.array_equal(got(q, kn, g, g)[others], without[others] + 1)  # the NaN key counts against every query of another group
    assert np.array_equal(got(q, kn, g, g, kc)[others], got(q, k, g, g, kc)[others])      # ... unless it is not counted
    kn = k.copy()
    kn[33, 0] = np.nan                                      # a NaN in a single-key group
    r = got(q, kn, g, g)
    rows = np.arange(nq) != 33
    without = R.grouped_ranks_np(q, np.delete(k, 33, axis=0), g, np.delete(g, 33))
    assert np.array_equal(r[rows], without[rows] + 1) and r[33] == nk
    qn = q.copy()
    qn[41, 2] = np.nan                                      # a NaN query: every key of another group counts
    r = got(qn, k, g, g)
    want = base.copy()
    want[41] = nk
    assert np.array_equal(r, want)


# ------------------------------------------------------------------ 7. Gaussian against float64
def gauss_groups(n, D, seed):
    """gauss_pairs with rows dealt to groups of 1..3: a query's positives are its own aligned key and its siblings' keys."""
    q, k = gauss_pairs(n, D, seed)
    g = random_groups(n, np.random.default_rng(seed + 1000), 1, 3)
    return q, k, g


# seeds at which float64 decides every query (searched on the host with retrieval_ref.grouped_undecided_np; asserted below)
GAUSS = [(130, 96, False, 0), (130, 96, True, 0), (130, 512, False, 2), (130, 512, True, 0),
         (257, 96, False, 3), (257, 96, True, 0), (257, 512, False, 2), (257, 512, True, 5)]


@pytest.mark.parametrize("n,D,normalize,seed", GAUSS)
def test_gaussian_ranks_equal_float64_on_decided_queries(n, D, normalize, seed):
    q, k, g = gauss_groups(n, D, seed)
    first = R.first_of_group_np(g)
    q64, k64 = (_unit(q), _unit(k)) if normalize else (q, k)
    for cnt in (None, first):
        und = R.grouped_undecided_np(q64, k64, g, g, cnt)
        want = R.grouped_ranks_np(q64, k64, g, g, cnt)
        r = got(q, k, g, g, cnt, normalize=normalize)
        print(f"n {n} D {D} normalize {normalize} kcount {cnt is not None}: undecided {und}, differing ranks {int((r != want).sum())}, "
              f"ranks > 1: {int((want > 1).sum())}, max {int(want.max())}")
        assert und == 0                                     # every query is decided, so every rank is compared
        assert int((want > 1).sum()) >= n // 8              # and the case is not the trivial all-ones one
        assert np.array_equal(r, want)


# ------------------------------------------------------------------ 8. reduction to the ungrouped path
@pytest.mark.parametrize("n,D", [(2 * T + 1, 96), (130, 513)])
def test_all_distinct_groups_equal_the_ungrouped_ranks(n, D):
    q, k = gauss_pairs(n, D, 40)
    k[7] = k[100]                                           # a bitwise tie, counted the same way by both
    ids = np.random.default_rng(41).permutation(n).astype(np.int64) * ((1 << 33) + 1) - (1 << 40)
    plain = retrieval_ranks(dev(q), dev(k))
    grouped = retrieval_ranks(dev(q), dev(k), query_group=dev(ids), key_group=dev(ids))
    assert torch.equal(plain, grouped)
    assert int(plain[100]) >= 2 and int(plain.max()) > 2
    qi, ki = int_data(n, D, 42), int_data(n, D, 43)
    assert torch.equal(retrieval_ranks(dev(qi), dev(ki)), retrieval_ranks(dev(qi), dev(ki), query_group=dev(ids), key_group=dev(ids)))


# ------------------------------------------------------------------ 9. determinism and capture
def test_two_launches_are_bit_equal_and_a_graph_replay_follows_inputs_and_ids():
    n, D = 2 * T + 1, 96
    q0, k0, g0 = gauss_groups(n, D, 30)
    c0 = R.first_of_group_np(g0)
    q, k, g, c = dev(q0), dev(k0), dev(g0), dev(c0)

    def run():
        return retrieval_ranks(q, k, query_group=g, key_group=g, key_count=c)

    a, b = run(), run()
    assert torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    assert torch.equal(out, a)
    g1 = random_groups(n, np.random.default_rng(32), 1, 5)
    g.copy_(dev(g1))                                        # the ids alone
    c.copy_(dev(R.first_of_group_np(g1)))
    graph.replay()
    ids_only = run()
    assert torch.equal(out, ids_only) and not torch.equal(ids_only, a)
    q1, k1 = gauss_pairs(n, D, 31)
    q.copy_(dev(q1))
    k.copy_(dev(k1))
    graph.replay()
    eager = run()
    assert torch.equal(out, eager) and not torch.equal(eager, ids_only)
    assert np.array_equal(eager.cpu().numpy(), got(q1, k1, g1, g1, R.first_of_group_np(g1)))


# ------------------------------------------------------------------ 10. the metric on a duplicated-RNA set
def duplicated_rna_set(seed=50, samples=40, D=64):
    """40 samples with 1..3 slides each, slides shuffled; the RNA row of a sample repeated for each of its slides; a slide embedding =
    its RNA embedding + integer noise in [-1, 1] (all values integers: exact dot products), so every sample wins."""
    rng = np.random.default_rng(seed)
    per = rng.integers(1, 4, size=samples)
    group = np.repeat(np.arange(samples, dtype=np.int64) * 1001 + 17, per)[rng.permutation(int(per.sum()))]
    table = rng.integers(-8, 9, size=(samples, D)).astype(np.float32)
    r = table[(group - 17) // 1001]
    w = (r + rng.integers(-1, 2, size=r.shape)).astype(np.float32)
    return w, r, group


def test_metric_on_a_set_with_duplicated_rna_rows():
    w, r, group = duplicated_rna_set()
    n = len(group)
    assert 40 < n <= 120 and len(np.unique(group)) == 40
    W, Rr, G = dev(w), dev(r), dev(group)
    plain = CrossModalRetrieval().update(W, Rr).compute()
    assert plain["wsi2rna_r@1"] < 1.0 and "retrieval_groups" not in plain        # capped by the data: the duplicated RNA rows tie
    whole = CrossModalRetrieval().update(W, Rr, G).compute()
    assert whole["wsi2rna_r@1"] == 1.0 and whole["rna2wsi_r@1"] == 1.0 and whole["r_mean"] == 1.0
    assert whole["retrieval_groups"] == 40 and whole["retrieval_n"] == n
    assert list(whole) == list(plain) + ["retrieval_groups"]
    want = R.grouped_metric_np(w, r, group)
    assert whole == want and list(whole) == list(want)
    chunked = CrossModalRetrieval()
    for sl in (slice(0, 30), slice(30, 31), slice(31, n)):
        assert chunked.update(W[sl], Rr[sl], G[sl].cpu() if sl.start == 30 else G[sl]) is chunked      # a host id tensor too
    a, b = CrossModalRetrieval().update(W[:45], Rr[:45], G[:45]), CrossModalRetrieval().update(W[45:], Rr[45:], G[45:].int())
    merged = CrossModalRetrieval().merge_state([a, b])
    assert chunked.compute() == merged.compute() == want
    assert a.compute()["retrieval_n"] == 45                 # merge_state left its sources alone
    G.zero_()                                               # update() kept copies of the ids
    assert chunked.compute() == want
    with pytest.raises(ValueError, match="every update"):
        chunked.update(W[:3], Rr[:3])
    assert chunked.reset().group == []
    # a harder set (noise as large as the signal): values below 1, still equal to the restatement, in both summaries
    w2 = (r + np.random.default_rng(51).integers(-48, 49, size=r.shape)).astype(np.float32)
    hard = CrossModalRetrieval(ks=(1, 3)).update(dev(w2), Rr, dev(group)).compute()
    assert hard == R.grouped_metric_np(w2, r, group, ks=(1, 3)) and hard["r_mean"] < 1.0
    # all-distinct ids: every value equals the ungrouped one
    distinct = CrossModalRetrieval().update(dev(w2), Rr, torch.arange(n)).compute()
    assert distinct.pop("retrieval_groups") == n
    assert distinct == CrossModalRetrieval().update(dev(w2), Rr).compute()


# ------------------------------------------------------------------ 11. TrainEngine.validate
CFG = dict(wsi_embed_dim=64, rna_embed_dim=48, embed_dim=64, wsi_num_tokens=60, rna_encoder_depth=1, rna_num_heads=8,
           style_mlp_hidden_dim=64, style_mlp_out_dim=32, style_latent_dim=16, num_prototypes=50)


def _batch(b, seed, cfg=CFG):
    gen = torch.Generator().manual_seed(seed)
    n, f, gd, d, lat = cfg["wsi_num_tokens"], cfg["wsi_embed_dim"], cfg["rna_embed_dim"], cfg["embed_dim"], cfg["style_latent_dim"]
    wsi, rna = torch.randn(b, n, f, generator=gen), torch.randn(b, gd, generator=gen)
    noise = {"wsi_mask": torch.rand(b, n, generator=gen), "rna_mask": torch.rand(b, d, generator=gen),
             "wsi_eps": torch.randn(b, lat, generator=gen), "rna_eps": torch.randn(b, lat, generator=gen)}
    return wsi, rna, {k: v.cuda() for k, v in noise.items()}


def _validate_setup():
    import mirror_amd.models as M
    from mirror_amd.engine import TrainEngine
    from mirror_amd.losses import MIRRORLoss
    torch.manual_seed(0)
    model = M.mirror(**CFG).cuda().train()
    eng = TrainEngine(model, MIRRORLoss(), lr=1e-3, precision="fp32", graph=False)
    groups = [torch.tensor([3, 3, 8, 1]), torch.tensor([8, 2, 2, 2]), torch.tensor([5, 1, 9, 9])]       # samples that span batches
    two, noises = [], []
    for i in range(3):
        wsi, rna, noise = _batch(4, 90 + i)
        two.append((wsi, rna))
        noises.append(noise)
    as_tensor = [(w, r, g) for (w, r), g in zip(two, groups)]
    as_dict = [(w, r, {"group": g.cuda(), "label": torch.zeros(4)}) for (w, r), g in zip(two, groups)]
    return model, eng, groups, two, as_tensor, as_dict, noises


def test_validate_takes_three_item_batches_as_a_tensor_and_as_a_dict():
    from mirror_amd.engine import TrainEngine
    model, eng, groups, two, as_tensor, as_dict, noises = _validate_setup()
    m = CrossModalRetrieval()
    res_t = eng.validate(as_tensor, noise=noises, retrieval=m)
    res_d = eng.validate(as_dict, noise=noises, retrieval=CrossModalRetrieval())
    assert model.training
    model.eval()
    hand = CrossModalRetrieval()
    with torch.no_grad():
        for (wsi, rna), noise, g in zip(two, noises, groups):
            outs = model(wsi.cuda(), rna.cuda(), noise=noise)
            hand.update(outs[0], outs[7], g)
    model.train()
    want = hand.compute()
    names = list(TrainEngine.LOSS_NAMES)
    assert list(res_t) == list(res_d) == names + list(want) and list(want)[-2:] == ["retrieval_n", "retrieval_groups"]
    assert {k: res_t[k] for k in want} == {k: res_d[k] for k in want} == want
    assert want["retrieval_n"] == 12 and want["retrieval_groups"] == 6 and m.compute() == want
    assert list(eng.validate(as_tensor, noise=noises)) == names        # without a metric the third item is ignored
    assert list(eng.validate(two, noise=noises, retrieval=m)) == names + list(want)[:-1]      # two items: the ungrouped entries, as before


def test_validate_losses_of_three_item_batches_are_bit_identical_to_the_two_item_loader():
    """validate() forms the losses of a batch before it looks at the batch's third item, and the masked-MSE accumulator of the
    retention loss adds its blocks' partial sums in block order (mh_mse_masked_fwd_ordered), so the same loader gives the same bits
    on every call.  With the float atomics of mh_mse_masked_fwd this test failed in two runs of three: wsi_retention_loss
    2.106048822402954 against 2.106048901875814, one f32 ulp of one batch's term."""
    from mirror_amd.engine import TrainEngine
    model, eng, groups, two, as_tensor, as_dict, noises = _validate_setup()
    names = list(TrainEngine.LOSS_NAMES)
    plain = eng.validate(two, noise=noises)
    res_t = eng.validate(as_tensor, noise=noises, retrieval=CrossModalRetrieval())
    res_d = eng.validate(as_dict, noise=noises, retrieval=CrossModalRetrieval())
    print({k: (plain[k].hex(), res_t[k].hex(), res_d[k].hex()) for k in names})
    for res in (res_t, res_d):
        assert [res[k] for k in names] == [plain[k] for k in names]


# ------------------------------------------------------------------ 12. two gloo ranks on the one GPU
def _shards():
    w, r, group = duplicated_rna_set(seed=60)
    order = np.argsort(group, kind="stable")                # slides of one sample next to each other ...
    gs = group[order]
    cut = next(c for c in range(40, len(gs)) if gs[c - 1] == gs[c])      # ... and the cut goes through a sample: its slides sit on both ranks
    return [(w[order[:cut]], r[order[:cut]], group[order[:cut]]), (w[order[cut:]], r[order[cut:]], group[order[cut:]])]


def _worker_sync(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        w, r, group = _shards()[rank]
        m = CrossModalRetrieval().update(dev(w), dev(r), dev(group))
        res = sync_and_compute(m)
        q.put((rank, dict(res), list(res), m.compute()["retrieval_n"]))
    finally:
        dist.destroy_process_group()


def test_sync_and_compute_over_two_gloo_ranks_merges_a_split_sample_by_id():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + (os.getpid() % 90)
    procs = [ctx.Process(target=_worker_sync, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(2)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (w0, r0, g0), (w1, r1, g1) = _shards()
    w, r, group = np.concatenate([w0, w1]), np.concatenate([r0, r1]), np.concatenate([g0, g1])
    single = CrossModalRetrieval().update(dev(w), dev(r), dev(group)).compute()
    want = R.grouped_metric_np(w, r, group)
    assert res[0][1] == res[1][1] == dict(single) == dict(want)
    assert res[0][2] == res[1][2] == list(single) == list(want)
    assert single["retrieval_groups"] == 40 and single["retrieval_n"] == len(group)
    assert (res[0][3], res[1][3]) == (len(g0), len(g1)) and g0[-1] == g1[0]      # each rank's own metric kept its state
