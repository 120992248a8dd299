"""MI355X: the few-shot prototype probe (csrc/fewshot.hip, mirror_amd/fewshot.py) against the float64 restatement of tests/fewshot_ref.py.

Every stage is compared on what the device itself handed to it (prepared features -> prototypes -> scores), so a stage's tolerance is
that stage's f32 rounding; the end-to-end test compares with float64 from the raw embeddings and leaves out the pairs float64 itself
decides by less than MARGIN_E2E.  The tally is integer arithmetic: no tolerance."""
import numpy as np
import pytest
import torch

from mirror_amd import FewShotProbe, kernels as K
from tests import fewshot_ref as R
from tests.retrieval_topk_ref import MARGIN

pytestmark = pytest.mark.gpu

# f32 rounding of unit-norm rows at D <= 512 (the issue's figures): a prepared row to 2e-6 absolute, mu to 1e-6 of its own size (the
# kernel sums in f64 and rounds once: half an f32 ulp, 6e-8), a prototype to 1e-6 of its norm; -|p|^2 / 2 inherits twice the last one
TOL_Y, TOL_MU, TOL_P = 2e-6, 1e-6, 1e-6


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()       # a copy: the shared inputs are read-only


def host(t):
    return t.detach().cpu().numpy()


def gauss_pool(n, D, C, seed):
    """Gaussian rows around a common offset, labels cycling through the classes (every class has a row once n >= C)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, D)) + 3.0 * rng.standard_normal(D)).astype(np.float32)
    return x, (np.arange(n) % C).astype(np.int64)


# ------------------------------------------------------------------ 1. preparation
@pytest.mark.parametrize("D", [70, 512])
def test_preparation_against_float64_and_bit_equal_twice(D):
    x, _ = gauss_pool(130 + 37, D, 3, seed=D)
    x, q = x[:130], x[130:]
    xd, qd = dev(x), dev(q)
    mu = K.colmean(xd)
    y, yq = K.center_l2norm(xd, mu), K.center_l2norm(qd, mu)
    want_y, want_mu = R.prepare(x, x)
    want_q, _ = R.prepare(x, q)
    e_mu = np.abs(host(mu) - want_mu) / np.abs(want_mu)
    e_y, e_q = np.abs(host(y) - want_y).max(), np.abs(host(yq) - want_q).max()
    print(f"D = {D}: mu {e_mu.max():.2e} relative, pool rows {e_y:.2e}, query rows {e_q:.2e} absolute")
    assert e_mu.max() <= TOL_MU and e_y <= TOL_Y and e_q <= TOL_Y
    assert np.abs(np.linalg.norm(host(y).astype(np.float64), axis=1) - 1).max() <= 1e-6
    assert torch.equal(K.colmean(xd), mu) and torch.equal(K.center_l2norm(xd, mu), y)
    # the device rows given the device's own mu: the subtraction and the scaling alone
    own = (x.astype(np.float64) - host(mu)) / np.linalg.norm(x.astype(np.float64) - host(mu), axis=1, keepdims=True)
    assert np.abs(host(y) - own).max() <= TOL_Y
    zero = K.center_l2norm(mu[None, :].contiguous(), mu)                 # a row equal to the mean: 0 / eps, not NaN
    assert torch.equal(zero, torch.zeros_like(zero))


def test_center_false_is_the_plain_normalisation():
    x, yl = gauss_pool(50, 70, 2, seed=2)
    p = FewShotProbe(2, shots=3, episodes=2, center=False, device="cuda").fit(dev(x), dev(yl))
    P = p._pool()
    assert P["mu"] is None
    assert np.abs(host(P["y"]) - R.prepare(x, x, center=False)[0]).max() <= TOL_Y


# ------------------------------------------------------------------ 2. the draw
def test_draw_is_the_data_feed_draw_through_the_class_permutation():
    C, Kk, E, seed, offset = 3, 10, 6, 77, (3 << 32) + 5
    labels = np.random.default_rng(1).permutation(np.repeat(np.arange(C), [40, 7, 12])).astype(np.int64)
    x = np.random.default_rng(2).standard_normal((len(labels), 8)).astype(np.float32)
    mk = lambda off: FewShotProbe(C, shots=Kk, episodes=E, seed=seed, offset=off, device="cuda").fit(dev(x), dev(labels))  # noqa: E731
    p = mk(offset)
    sup = p.draw()
    assert sup.dtype == torch.int64 and tuple(sup.shape) == (E, C, Kk) and sup.is_cuda
    got = host(sup)
    assert np.array_equal(got, R.draw(labels, C, Kk, E, seed, offset))            # bit for bit
    for c in range(C):
        assert (labels[got[:, c]] == c).all()                                     # rows of class c only
    for e in range(E):
        assert len(set(got[e, 0])) == Kk and len(set(got[e, 2])) == Kk            # 40 and 12 >= 10 rows: no repeats
    assert any(len(set(got[e, 1])) < Kk for e in range(E))                        # 7 < 10 rows: with replacement
    assert torch.equal(p.draw(), sup) and torch.equal(mk(offset).draw(), sup)
    other = host(mk(offset + 1).draw())
    assert not np.array_equal(other, got) and np.array_equal(other, R.draw(labels, C, Kk, E, seed, offset + 1))
    with pytest.raises(ValueError, match=r"no row of class\(es\) \[3\]"):
        FewShotProbe(4, shots=2, episodes=2, device="cuda").fit(dev(x), dev(labels)).draw()


# ------------------------------------------------------------------ 3. prototypes
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("C,Kk,D", [(3, 5, 70), (33, 3, 96), (2, 10, 512)])
def test_prototypes_against_float64_from_the_device_features(metric, C, Kk, D):
    E, Cp = 5, R.cp_of(C)
    x, yl = gauss_pool(4 * C + 9, D, C, seed=C + D)
    p = FewShotProbe(C, shots=Kk, episodes=E, metric=metric, seed=4, device="cuda").fit(dev(x), dev(yl))
    y = host(p._pool()["y"]).astype(np.float64)
    sup = p.draw()
    protos, bias = p.prototypes()
    assert tuple(protos.shape) == (E, Cp, D) and protos.dtype == torch.float32
    direct = p.prototypes(sup)                                                    # the same rows without the permutation: the same bits
    assert torch.equal(direct[0], protos) and (bias is None) == (metric == "cosine") and (bias is None or torch.equal(direct[1], bias))
    want_p, want_b = R.prototypes(y, host(sup), metric)
    norm = np.linalg.norm(want_p[:, :C], axis=2)
    e_p = (np.abs(host(protos)[:, :C] - want_p[:, :C]).max(2) / norm).max()
    print(f"{metric} C = {C} K = {Kk} D = {D}: prototypes {e_p:.2e} of their norm")
    assert e_p <= TOL_P
    assert (host(protos)[:, C:] == 0).all()                                       # the pads
    if metric == "euclidean":
        b = host(bias)
        e_b = (np.abs(b[:, :C] - want_b[:, :C]) / np.abs(want_b[:, :C])).max()
        print(f"    bias {e_b:.2e} relative")
        assert e_b <= 2 * TOL_P and np.isneginf(b[:, C:]).all() and tuple(b.shape) == (E, Cp)
    else:
        assert np.abs(np.linalg.norm(host(protos)[:, :C].astype(np.float64), axis=2) - 1).max() <= 1e-6
    # an index outside the pool: NaN in that prototype (and its bias) only
    broken = sup.clone()
    broken[1, 0, Kk - 1] = x.shape[0]
    broken[3, C - 1, 0] = -1
    bp, bb = p.prototypes(broken)
    nan = torch.isnan(bp).all(2)
    want_nan = torch.zeros_like(nan)
    want_nan[1, 0] = want_nan[3, C - 1] = True
    assert torch.equal(nan, want_nan) and torch.equal(torch.isnan(bp).any(2), want_nan)
    assert torch.equal(bp[~want_nan], protos[~want_nan])
    if bb is not None:
        assert torch.equal(torch.isnan(bb), want_nan) and torch.equal(bb[~want_nan], bias[~want_nan])


# ------------------------------------------------------------------ 4. prediction from the device's own prototypes
#          (nq,  E,  C,  K, D)     Cp, keys
SHAPES = [(130, 40, 3, 5, 70),     # 4, 160: two key tiles, two row tiles, D with a scalar tail
          (64, 3, 64, 2, 128),     # 64, 192: a run spans both wn waves
          (257, 5, 33, 3, 96),     # 64, 320: 31 pad classes
          (128, 64, 2, 1, 512),    # 2, 128: the smallest Cp
          (1, 1, 2, 1, 1)]         # the smallest everything


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("nq,E,C,Kk,D", SHAPES)
def test_prediction_against_float64_scores_of_the_device_prototypes(metric, nq, E, C, Kk, D):
    n = 3 * C + 5
    x, yl = gauss_pool(n + nq, D, C, seed=nq + C)                                  # pool and queries around the same offset
    x, yl, q = x[:n], yl[:n], x[n:]
    p = FewShotProbe(C, shots=Kk, episodes=E, metric=metric, seed=9, offset=17, device="cuda").fit(dev(x), dev(yl))
    pred = p.predict(dev(q))
    assert pred.dtype == torch.int32 and tuple(pred.shape) == (E, nq)
    qd = K.center_l2norm(dev(q), p._pool()["mu"])
    protos, bias = p.prototypes()
    assert torch.equal(K.fewshot_predict(qd, protos, bias, C), pred) and torch.equal(p.predict(dev(q)), pred)
    q64, p64 = host(qd).astype(np.float64), host(protos).astype(np.float64)
    b64 = host(bias).astype(np.float64) if bias is not None else np.where(np.arange(R.cp_of(C)) < C, 0.0, -np.inf)[None, :].repeat(E, 0)
    S = R.scores(q64, p64, b64)
    want = R.predict(S, C)
    # the project's margin on the products: 1e-5 |q| |p| with the largest |p| of the episode (the one f32 add of the bias rounds by
    # 6e-8 of a score of size <= 1.5, far inside it)
    margin = MARGIN * np.linalg.norm(q64, axis=1)[None, :] * np.linalg.norm(p64, axis=2).max(1)[:, None]
    decided = R.top_two_gap(S, C) > margin
    got = host(pred).astype(np.int64)
    print(f"{metric} {(nq, E, C, Kk, D)}: {decided.mean():.4f} decided, {(got != want)[decided].sum()} of them differ, "
          f"{(got != want).sum()} differ at all")
    assert (got >= 0).all() and (got < C).all()
    if D == 1:
        assert np.array_equal(got, want)                                          # rows are +-1 exactly: exact scores, an exact tie included
    else:
        assert decided.mean() >= 0.9                                              # the comparison is not empty
    assert np.array_equal(got[decided], want[decided])


# ------------------------------------------------------------------ 5. ties and NaN through an explicit support
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_ties_go_to_the_smaller_class_and_nan_is_never_predicted(metric):
    C, D, nq = 4, 70, 130
    x, yl = gauss_pool(40 + nq, D, C, seed=5)
    x, yl, q = x[:40], yl[:40], x[40:].copy()
    q[7] = np.nan                                                                 # a query without any eligible class
    ql = (np.arange(nq) % C).astype(np.int64)
    rng = np.random.default_rng(7)
    sup = rng.integers(0, 40, size=(3, C, 5)).astype(np.int64)
    sup[:, 2] = sup[:, 1]                                                         # classes 1 and 2: identical supports, identical scores
    sup[1, 3, 2] = 40                                                             # episode 1: class 3 is a NaN prototype
    sup[2, 0, 0] = -1                                                             # episode 2: class 0 is
    p = FewShotProbe(C, shots=5, episodes=9, metric=metric, device="cuda").fit(dev(x), dev(yl))
    p.run(dev(q), dev(ql), support=dev(sup))
    pred = host(p.pred)
    assert pred.shape == (3, nq)
    rows = np.arange(nq) != 7
    assert (pred[:, 7] == -1).all() and (pred[:, rows] >= 0).all()
    assert (pred != 2).all() and (pred[:, rows] == 1).sum() > 20                  # the tie is met, and always goes to class 1
    assert (pred[1] != 3).all() and (pred[2] != 0).all() and (pred[0] == 3).any() and (pred[0] == 0).any()
    assert np.array_equal(host(p.bad), [1, 1, 1])                                 # the NaN row, and nothing else
    conf, bad, summary = R.tally(pred, ql, C)
    assert np.array_equal(host(p.confusion), conf) and conf.sum() == 3 * (nq - 1)
    assert np.allclose(host(p.per_episode), summary, rtol=1e-12, atol=0)
    # labels outside the classes are left out as well
    ql2 = ql.copy()
    ql2[[0, 1, 2]] = [-1, C, 1 << 40]
    p.run(dev(q), dev(ql2), support=dev(sup))
    conf2, bad2, summary2 = R.tally(pred, ql2, C)
    assert np.array_equal(host(p.bad), bad2) and (bad2 == 4).all() and np.array_equal(host(p.confusion), conf2)
    assert np.allclose(host(p.per_episode), summary2, rtol=1e-12, atol=0)


# ------------------------------------------------------------------ 6. end to end
# the noise of the clusters is chosen from float64 alone (tests/fewshot_ref.py on the CPU: about 78 % accuracy at these values)
E2E = [(4, 64, 5, 2.5), (5, 512, 10, 5.5), (2, 64, 10, 4.5)]
E2E_E, E2E_NQ = 64, 130


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("C,D,Kk,noise", E2E)
def test_evaluate_end_to_end_against_float64(metric, C, D, Kk, noise):
    pool, yl, q, ql = R.clusters(C, D, 40, E2E_NQ, noise, seed=C * 1000 + D)
    p = FewShotProbe(C, shots=Kk, episodes=E2E_E, metric=metric, seed=5, device="cuda").fit(dev(pool), dev(yl))
    sup = host(p.draw())
    out = p.evaluate(dev(q), dev(ql))
    got = host(p.pred).astype(np.int64)
    # float64 from the raw embeddings, with the support ids the device drew
    assert np.array_equal(sup, R.draw(yl, C, Kk, E2E_E, 5, 0))
    y64, _ = R.prepare(pool, pool)
    q64, _ = R.prepare(pool, q)
    S = R.scores(q64, *R.prototypes(y64, sup, metric))
    want = R.predict(S, C)
    acc64 = (want == ql[None, :]).mean()
    undecided = R.top_two_gap(S, C) <= R.MARGIN_E2E
    print(f"{metric} {(C, D, Kk)}: float64 accuracy {acc64:.4f}, {100 * undecided.mean():.4f} % undecided, "
          f"{(got != want).sum()} predictions differ, {(got != want)[~undecided].sum()} of them decided")
    assert 0.6 <= acc64 <= 0.95                                                   # input conditions, from float64 alone
    assert undecided.mean() <= 0.01
    assert np.array_equal(got[~undecided], want[~undecided])
    # the tally is integer arithmetic on the device's predictions: exact counts, f64 summaries
    conf, bad, summary = R.tally(got, ql, C)
    assert np.array_equal(host(p.confusion), conf) and not host(p.bad).any() and p.confusion.dtype == torch.int32
    assert p.per_episode.dtype == torch.float64 and np.allclose(host(p.per_episode), summary, rtol=1e-12, atol=0)
    clean = ~undecided.any(1)                                                     # episodes float64 decides everywhere: its own counts
    conf64, _, summary64 = R.tally(want, ql, C)
    assert clean.sum() >= E2E_E // 8
    assert np.array_equal(host(p.confusion)[clean], conf64[clean])
    assert np.allclose(host(p.per_episode)[clean], summary64[clean], rtol=1e-12, atol=0)
    rep = R.report(summary, Kk, len(yl))
    assert list(out) == ["fewshot_acc", "fewshot_acc_std", "fewshot_acc_ci95", "fewshot_bacc", "fewshot_bacc_std", "fewshot_bacc_ci95",
                         "fewshot_f1", "fewshot_f1_std", "fewshot_f1_ci95", "fewshot_shots", "fewshot_episodes", "fewshot_n"]
    for k, v in rep.items():
        assert out[k] == pytest.approx(v, rel=1e-9, abs=0), k
    assert out["fewshot_acc_std"] > 0 and out["fewshot_episodes"] == E2E_E and out["fewshot_n"] == 40 * C


def test_explicit_support_chunked_fit_and_graph_replay():
    C, D, Kk, noise = E2E[0]
    pool, yl, q, ql = R.clusters(C, D, 40, E2E_NQ, noise, seed=1)
    mk = lambda: FewShotProbe(C, shots=Kk, episodes=E2E_E, seed=5, offset=3, device="cuda")  # noqa: E731
    p = mk().fit(dev(pool), dev(yl))
    qd, qld = dev(q), dev(ql)
    table = p.run(qd, qld).clone()
    pred, conf, sup = p.pred.clone(), p.confusion.clone(), p.draw()
    # one explicit episode (the rows of a split file) reproduces episode 0
    one = p.evaluate(qd, qld, support=sup[:1])
    assert torch.equal(p.pred, pred[:1]) and torch.equal(p.confusion, conf[:1]) and torch.equal(p.per_episode, table[:1])
    assert one["fewshot_episodes"] == 1 and one["fewshot_acc_std"] == 0.0 and one["fewshot_acc_ci95"] == 0.0
    assert one["fewshot_acc"] == float(table[0, 0]) and one["fewshot_shots"] == Kk
    for bad in (sup[:, :3], sup.int(), sup[0]):
        with pytest.raises(ValueError, match="support must be"):
            p.predict(qd, support=bad)
    # three fits concatenate to the same pool; merge_state does the same
    a, b = 37, 101
    p3 = mk().fit(dev(pool[:a]), dev(yl[:a])).fit(dev(pool[a:b]), dev(yl[a:b])).fit(dev(pool[b:]), dev(yl[b:]))
    assert torch.equal(p3.draw(), sup) and torch.equal(p3.predict(qd), pred)
    pm = mk().fit(dev(pool[:a]), dev(yl[:a])).merge_state([mk().fit(dev(pool[a:]), dev(yl[a:]))])
    assert torch.equal(pm.predict(qd), pred)
    assert pm.reset().emb == [] and pm.pred is None
    # the device part of evaluate in a graph: one eager call has built the pool's tables, the replay waits for nothing
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = p.run(qd, qld)
        gpred = p.pred
    g.replay()
    assert torch.equal(gpred, pred) and torch.equal(out, table)
    q2 = R.clusters(C, D, 40, E2E_NQ, noise, seed=2)[2]
    qd.copy_(dev(q2))                                                             # the replay follows its inputs
    g.replay()
    eager = mk().fit(dev(pool), dev(yl)).predict(dev(q2))
    assert torch.equal(gpred, eager) and not torch.equal(eager, pred)
