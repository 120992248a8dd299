"""MI355X: mh_retrieval_ranks (csrc/retrieval.hip) and the metric built on it (mirror_amd/retrieval.py).  The yardstick is `ranks_np`
below: the one-line definition of include/mirror_hip.h restated in float64 numpy,
    ranks[i] = 1 + #{ j != target[i] : not (q_i . k_j < q_i . k_target[i]) }.
Integer-valued inputs make every f32 dot product exact, so the ranks must be EQUAL, ties included; Gaussian inputs are compared
on queries that float64 decides with a margin of 1e-5 |q_i| |k_j| (about 30x the f32 fmaf-chain error at D <= 1024), with seeds
at which float64 decides every query."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from mirror_amd.metrics import sync_and_compute
from mirror_amd.retrieval import CrossModalRetrieval, retrieval_ranks, summarize_ranks

pytestmark = pytest.mark.gpu

T = 128          # the kernel's tile edge (RT_TILE of csrc/retrieval.hip)


def ranks_np(q, k, target=None, same=()):
    """The definition in float64.  same: (src, dst) key-row pairs that are copies of each other, whose similarities are forced to be
    the same number (a float64 BLAS may sum two equal columns in different orders)."""
    S = q.astype(np.float64) @ k.astype(np.float64).T
    for src, dst in same:
        S[:, dst] = S[:, src]
    rows = np.arange(q.shape[0])
    t = rows if target is None else np.asarray(target)
    d = S[rows, t]
    beats = ~(S < d[:, None])
    beats[rows, t] = False
    return (1 + beats.sum(1)).astype(np.int64)


def undecided_np(q, k, normalize=False):
    """Queries with a competitor inside the float64 margin 1e-5 |q_i| |k_j| of the positive (identity target)."""
    q, k = q.astype(np.float64), k.astype(np.float64)
    if normalize:
        q, k = _unit(q), _unit(k)
    S = q @ k.T
    rows = np.arange(q.shape[0])
    close = np.abs(S - S[rows, rows][:, None]) <= 1e-5 * np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(k, axis=1)[None, :]
    close[(k[:, None, :] == k[None, :, :]).all(-1)] = False      # an exact copy of the positive is a tie by construction, not a near miss
    return int(close.any(1).sum())


def _unit(x):
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)


def int_data(n, D, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=(n, D)).astype(np.float32)


def gauss_pairs(n, D, seed):
    """Gaussian q; k_i = a_i q_i + sqrt(1 - a_i^2) noise with a_i spread over [0, 0.5]: about a quarter of the positives are weak
    enough to be outranked, the rest win, as in a half-trained alignment."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n, D)).astype(np.float32)
    a = rng.permutation(np.linspace(0.0, 0.5, n)).astype(np.float32)[:, None]
    k = (a * q + np.sqrt(1 - a * a) * rng.standard_normal((n, D)).astype(np.float32)).astype(np.float32)
    return q, k


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def got(q, k, target=None, **kw):
    r = retrieval_ranks(dev(q), dev(k), None if target is None else dev(np.asarray(target, dtype=np.int64)), **kw)
    assert r.dtype == torch.int32 and tuple(r.shape) == (q.shape[0],)
    return r.cpu().numpy().astype(np.int64)


# ------------------------------------------------------------------ 1. exact, integer-valued inputs
INT_SHAPES = [(1, 1, 1), (67, 67, 40), (130, 257, 96), (257, 130, 513), (2 * T + 1, 2 * T + 1, 33)]


@pytest.mark.parametrize("nq,nk,D", INT_SHAPES)
def test_integer_inputs_give_exactly_the_restated_ranks(nq, nk, D):
    q, k = int_data(nq, D, 1), int_data(nk, D, 2)
    rng = np.random.default_rng(3)
    if nq == nk:
        target = None
    elif nk > nq:
        target = rng.integers(0, nk // 3, size=nq)         # repeats keys, and leaves the upper two thirds unused
    else:
        target = rng.integers(0, nk, size=nq)
    t = np.arange(nq) if target is None else target
    if D > 1:
        # the last query (an edge tile in every shape) gets a negative positive: a zero-filled column past nk would beat it
        q[-1] = -k[t[-1]]
        q[-1, 0] -= 1.0
        assert float(q[-1].astype(np.float64) @ k[t[-1]].astype(np.float64)) < 0
    want = ranks_np(q, k, target)
    r = got(q, k, target)
    print(f"shape {(nq, nk, D)}: {int((r != want).sum())} ranks differ; ties with the positive: {int((want > 1).sum())} rows ranked > 1")
    assert np.array_equal(r, want)
    assert r.min() >= 1 and r.max() <= nk
    if target is not None:      # a host target goes through the same launch
        r2 = retrieval_ranks(dev(q), dev(k), torch.from_numpy(np.asarray(target, dtype=np.int64))).cpu().numpy()
        assert np.array_equal(r2, want)
        r3 = retrieval_ranks(dev(q), dev(k), dev(np.asarray(target, dtype=np.int32))).cpu().numpy()
        assert np.array_equal(r3, want)


def test_integer_inputs_tie_often():
    """The integer cases are only a test of the tie rule if ties occur: at D = 1 nearly every competitor ties or beats."""
    q, k = int_data(300, 1, 4), int_data(300, 1, 5)
    S = q.astype(np.float64) @ k.astype(np.float64).T
    assert int((S == np.diag(S)[:, None]).sum()) > 3000
    assert np.array_equal(got(q, k), ranks_np(q, k))


# ------------------------------------------------------------------ 2. bitwise ties
@pytest.mark.parametrize("D,seed", [(96, 0), (512, 7)])
def test_copies_of_the_positive_tie_with_it_bit_for_bit(D, seed):
    n = 200
    q, k = gauss_pairs(n, D, seed)
    same = []
    for i, dsts in ((3, (10, 77, 199)), (150, (0, 64, 131)), (198, (32, 33, 129))):
        for j in dsts:
            k[j] = k[i]
            same.append((i, j))
    assert undecided_np(q, k) == 0
    want = ranks_np(q, k, same=same)
    r = got(q, k)
    for i in (3, 150, 198):
        S = q[i].astype(np.float64) @ k.astype(np.float64).T
        others = int((np.delete(S, [i] + [j for s, j in same if s == i]) >= S[i]).sum())
        print(f"D {D} query {i}: rank {r[i]}, {others} other keys beat it, 3 copies")
        assert r[i] == want[i] == 1 + others + 3          # all three copies count, none of them is excluded
    assert np.array_equal(r, want)


# ------------------------------------------------------------------ 3. Gaussian against float64
GAUSS = [(300, 512, False, 17), (300, 512, True, 11), (150, 768, False, 0), (150, 768, True, 0)]


@pytest.mark.parametrize("n,D,normalize,seed", GAUSS)
def test_gaussian_ranks_equal_float64_on_decided_queries(n, D, normalize, seed):
    q, k = gauss_pairs(n, D, seed)
    und = undecided_np(q, k, normalize)
    want = ranks_np(_unit(q.astype(np.float64)), _unit(k.astype(np.float64))) if normalize else ranks_np(q, k)
    r = got(q, k, normalize=normalize)
    print(f"n {n} D {D} normalize {normalize}: undecided {und}, differing ranks {int((r != want).sum())}, "
          f"ranks > 1: {int((want > 1).sum())}, max {int(want.max())}")
    assert und == 0                                       # every query is decided, so every rank is compared
    assert int((want > 1).sum()) >= n // 6                # and the case is not the trivial all-ones one
    assert np.array_equal(r, want)


# ------------------------------------------------------------------ 4. the pessimistic rule
def test_collapsed_embeddings_rank_last_everywhere():
    nk = 131
    row = np.random.default_rng(6).standard_normal((1, 40)).astype(np.float32)
    x = np.repeat(row, nk, axis=0)
    r = got(x, x)
    assert np.array_equal(r, np.full(nk, nk))
    s = summarize_ranks(r, ks=(1, 5, 10, nk - 1, nk))
    assert [s[f"r@{k}"] for k in (1, 5, 10, nk - 1, nk)] == [0.0, 0.0, 0.0, 0.0, 1.0]
    assert s["medr"] == nk and s["meanr"] == nk


def test_nan_counts_against_the_query():
    nq = nk = 150
    q, k = int_data(nq, 24, 7), int_data(nk, 24, 8)
    base = got(q, k)
    assert np.array_equal(base, ranks_np(q, k))
    qn = q.copy()
    qn[41, 5] = np.nan                                    # a NaN query: its rank is nk, every other row is untouched
    r = got(qn, k)
    want = base.copy()
    want[41] = nk
    assert np.array_equal(r, want)
    kn = k.copy()
    kn[140, 0] = np.nan                                   # a NaN key: one more key that every query fails to beat
    r = got(q, kn)
    rows = np.arange(nq) != 140
    t = np.arange(nq)[rows]
    without = ranks_np(q[rows], np.delete(k, 140, axis=0), target=t - (t > 140))       # the same problem with key 140 taken out
    assert np.array_equal(r[rows], without + 1)
    assert r[140] == nk                                   # and the query whose positive it is ranks last


# ------------------------------------------------------------------ 5. determinism and capture
def test_two_launches_are_bit_equal_and_a_graph_replay_follows_its_inputs():
    n, D = 2 * T + 1, 96
    q0, k0 = gauss_pairs(n, D, 30)
    q, k = dev(q0), dev(k0)
    a, b = retrieval_ranks(q, k), retrieval_ranks(q, k)
    assert torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        retrieval_ranks(q, k)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = retrieval_ranks(q, k)
    g.replay()
    assert torch.equal(out, a)
    q1, k1 = gauss_pairs(n, D, 31)
    q.copy_(dev(q1))
    k.copy_(dev(k1))
    g.replay()
    eager = retrieval_ranks(q, k)
    assert torch.equal(out, eager)
    assert not torch.equal(eager, a)


# ------------------------------------------------------------------ 6. the metric object
def _want_dict(w, r, ks=(1, 5, 10), normalize=False):
    if normalize:
        w, r = _unit(w.astype(np.float64)), _unit(r.astype(np.float64))
    out, rec = OrderedDict(), []
    for name, ranks in (("wsi2rna", ranks_np(w, r)), ("rna2wsi", ranks_np(r, w))):
        for key, v in summarize_ranks(ranks, ks).items():
            out[f"{name}_{key}"] = v
            if key.startswith("r@"):
                rec.append(v)
    out["r_mean"] = float(np.mean(rec))
    out["retrieval_n"] = w.shape[0]
    return out


def test_metric_chunked_merged_and_whole_agree_with_the_restatement():
    w = int_data(150, 64, 9) * 0.25
    r = (w + int_data(150, 64, 10) * 0.5).astype(np.float32)          # multiples of 1/4: exact dot products, partly aligned pairs
    W, R = dev(w), dev(r)
    whole = CrossModalRetrieval().update(W, R).compute()
    chunked = CrossModalRetrieval()
    for sl in (slice(0, 50), slice(50, 51), slice(51, 150)):
        assert chunked.update(W[sl], R[sl]) is chunked
    a, b = CrossModalRetrieval().update(W[:70], R[:70]), CrossModalRetrieval().update(W[70:], R[70:])
    merged = CrossModalRetrieval().merge_state([a, b])
    want = _want_dict(w, r)
    assert list(whole) == ["wsi2rna_r@1", "wsi2rna_r@5", "wsi2rna_r@10", "wsi2rna_medr", "wsi2rna_meanr", "rna2wsi_r@1", "rna2wsi_r@5",
                           "rna2wsi_r@10", "rna2wsi_medr", "rna2wsi_meanr", "r_mean", "retrieval_n"]
    assert whole == chunked.compute() == merged.compute() == want
    assert list(chunked.compute()) == list(want) and whole["retrieval_n"] == 150
    assert 0.0 < whole["r_mean"] < 1.0 and all(0.0 <= v <= 1.0 for k_, v in whole.items() if "r@" in k_)
    assert a.compute()["retrieval_n"] == 70                          # merge_state left its sources alone
    W.zero_()                                                        # update() kept copies, not views
    assert chunked.compute() == want
    assert chunked.reset().wsi == [] and CrossModalRetrieval(ks=(1, 3)).update(dev(w), dev(r)).compute() == _want_dict(w, r, ks=(1, 3))
    cos = CrossModalRetrieval(normalize=True).update(dev(w), dev(r).to(torch.bfloat16).float()).compute()
    assert list(cos) == list(want)


# ------------------------------------------------------------------ 7. TrainEngine.validate
CFG = dict(wsi_embed_dim=64, rna_embed_dim=48, embed_dim=64, wsi_num_tokens=60, rna_encoder_depth=1, rna_num_heads=8,
           style_mlp_hidden_dim=64, style_mlp_out_dim=32, style_latent_dim=16, num_prototypes=50)


def _batch(b, seed, cfg=CFG):
    g = torch.Generator().manual_seed(seed)
    n, f, gd, d, lat = cfg["wsi_num_tokens"], cfg["wsi_embed_dim"], cfg["rna_embed_dim"], cfg["embed_dim"], cfg["style_latent_dim"]
    wsi, rna = torch.randn(b, n, f, generator=g), torch.randn(b, gd, generator=g)
    noise = {"wsi_mask": torch.rand(b, n, generator=g), "rna_mask": torch.rand(b, d, generator=g),
             "wsi_eps": torch.randn(b, lat, generator=g), "rna_eps": torch.randn(b, lat, generator=g)}
    return wsi, rna, {k: v.cuda() for k, v in noise.items()}


def _validate_setup():
    import mirror_amd.models as M
    from mirror_amd.engine import TrainEngine
    from mirror_amd.losses import MIRRORLoss
    torch.manual_seed(0)
    model = M.mirror(**CFG).cuda().train()
    eng = TrainEngine(model, MIRRORLoss(), lr=1e-3, precision="fp32", graph=False)
    batches, noises = [], []
    for i in range(3):
        wsi, rna, noise = _batch(4, 90 + i)
        batches.append((wsi, rna))
        noises.append(noise)
    return model, eng, batches, noises


def test_validate_appends_the_retrieval_entries_behind_the_six_losses():
    from mirror_amd.engine import TrainEngine
    model, eng, batches, noises = _validate_setup()
    m = CrossModalRetrieval()
    m.update(torch.randn(5, 64).cuda(), torch.randn(5, 64).cuda())       # stale state: validate() resets it
    both = eng.validate(batches, noise=noises, retrieval=m)
    assert model.training                                                 # mode restored
    model.eval()
    hand = CrossModalRetrieval()
    with torch.no_grad():
        for (wsi, rna), noise in zip(batches, noises):
            outs = model(wsi.cuda(), rna.cuda(), noise=noise)
            hand.update(outs[0], outs[7])
    want = hand.compute()
    assert list(both) == list(TrainEngine.LOSS_NAMES) + list(want)        # the six losses, then the metric's entries
    assert {k: both[k] for k in want} == want and both["retrieval_n"] == 12
    assert m.compute() == want                                            # the caller's metric holds the validation set
    model.train()
    assert list(eng.validate(batches, noise=noises)) == list(TrainEngine.LOSS_NAMES)     # without it: the six losses, as before
    assert model.training


def test_validate_losses_are_bit_identical_with_and_without_retrieval():
    """validate() forms a batch's losses before it touches the metric, and every loss kernel on that path adds its blocks' partial
    sums in a fixed order: the WSI retention MSE through mh_mse_masked_fwd_ordered, the cluster rows and the RNA MSE of
    mh_loss_terms_fwd through per-block slots that its last block folds (csrc/loss_fused.hip).  With float atomics in their place
    this test failed intermittently, by one f32 ulp of one batch's term: wsi_retention_loss first (2.1060487429300943 against
    2.106048901875814), cluster_loss after that one was fixed (0x1.8070f6aaaaaabp-2 against 0x1.8070f60000000p-2)."""
    from mirror_amd.engine import TrainEngine
    model, eng, batches, noises = _validate_setup()
    plain = eng.validate(batches, noise=noises)
    both = eng.validate(batches, noise=noises, retrieval=CrossModalRetrieval())
    print({k: (plain[k].hex(), both[k].hex()) for k in plain})
    assert list(plain) == list(TrainEngine.LOSS_NAMES) == list(both)[:6]
    assert [both[k] for k in plain] == list(plain.values())


# ------------------------------------------------------------------ 8. two gloo ranks on the one GPU
def _worker_sync(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        n = 90 + 47 * rank                                # unequal shards: the padded gather
        w = int_data(n, 40, 50 + rank) * 0.25
        r = (w + int_data(n, 40, 60 + rank) * 0.5).astype(np.float32)
        m = CrossModalRetrieval().update(dev(w), dev(r))
        res = sync_and_compute(m)
        q.put((rank, dict(res), list(res), m.compute()["retrieval_n"], w, r))
    finally:
        dist.destroy_process_group()


def test_sync_and_compute_over_two_gloo_ranks_equals_the_union():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29800 + (os.getpid() % 90)
    procs = [ctx.Process(target=_worker_sync, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(2)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    w, r = np.concatenate([res[0][4], res[1][4]]), np.concatenate([res[0][5], res[1][5]])
    single = CrossModalRetrieval().update(dev(w), dev(r)).compute()
    assert res[0][1] == res[1][1] == dict(single) == dict(_want_dict(w, r))
    assert res[0][2] == res[1][2] == list(single) and single["retrieval_n"] == 90 + 137
    assert (res[0][3], res[1][3]) == (90, 137)            # each rank's own metric kept its state
