"""MI355X: the scores of the linear probe (mh_linprobe_proba, mh_auroc_counts_many, LinearProbe.evaluate(auroc=True) / oof_proba /
predict_proba) against the float64 restatement of tests/linprobe_scores_ref.py.  Shapes, inputs and tolerances of the kernel tests are
those of tests/test_linprobe_gpu.py (make_case, delta, TOL_P, TOL_CE: its docstring derives them).

  probabilities  mh_linprobe_proba shares the device functions of mh_linprobe_grad, so with rscale = 1 its P is G bit for bit off the
                 label's column, and its error against float64 is delta[i, j] + TOL_P.  The expf / logf part is MEASURED again here on
                 the dyadic inputs (exact logits): observed figures below.
  pair counts    integers: equal to the restatement, and to mh_auroc_counts table by table.
  end to end     on the overlapping case of linprobe_scores_ref.E2E the device's AUROC must lie in the interval that float64 leaves
                 when every (positive, negative) pair closer than linprobe_ref.MARGIN is counted both ways.  That gap assumes the
                 device's probabilities stay within MARGIN / 2 of float64's after 300 steps; the largest difference is printed.

Observed (MI355X, 2026-10-21): on the dyadic inputs over the five shapes the largest |P - P_ref| was 4.47e-07 (TOL_P = 1.93e-06) and
the largest mean |nll - nll_ref| per counted row 1.03e-07 (TOL_CE = 3.7e-07); end to end the largest |P_device - P_f64| over the
held-out rows was 2.80e-06, against MARGIN / 2 = 5e-04, with at most 1.86 % of a (fold, strength, class)'s pairs undecided.
"""
import numpy as np
import pytest
import torch

from mirror_amd import LinearProbe, kernels as K
from tests import linprobe_ref as R
from tests import linprobe_scores_ref as SR
from tests.test_linprobe_gpu import CASES, TOL_CE, TOL_P, U, dev, host, make_case

pytestmark = pytest.mark.gpu

IDS = lambda s: "n%d-D%d-C%d-E%d" % s  # noqa: E731


def run_proba(c, y=None, labels=True):
    return K.linprobe_proba(dev(c["y"] if y is None else y), dev(c["W"]), dev(c["b"]), c["C"],
                            labels=dev(c["labels"]) if labels else None, want_nll=labels)


def proba_reference(c):
    """(P_ref [E, n, C], nll_ref [n, E] (0 for rows without a valid label), counted [n], delta [n, E]) in float64 from the f32 inputs."""
    y = c["y"].astype(np.float64)
    n, E, C = c["n"], c["J"], c["C"]
    P, nll, delta = np.zeros((E, n, C)), np.zeros((n, E)), np.zeros((n, E))
    for e in range(E):
        W, b = c["W"][e, :C].astype(np.float64), c["b"][e, :C].astype(np.float64)
        P[e] = SR.proba(W, b, y)
        nll[:, e], ok = SR.row_nll(W, b, y, c["labels"])
        delta[:, e] = 2 * c["D"] * U * np.linalg.norm(y, axis=1) * np.linalg.norm(W, axis=1).max()
    return P, nll, ok, delta


# ------------------------------------------------------------------ 1. the link to mh_linprobe_grad
@pytest.mark.parametrize("shape", CASES, ids=IDS)
def test_proba_is_the_gradient_kernels_softmax_bit_for_bit(shape):
    c = make_case(*shape)
    n, E, C, Cp = c["n"], c["J"], c["C"], c["Cp"]
    fold, held, one = torch.zeros(n, dtype=torch.int32).cuda(), torch.full((E,), -1, dtype=torch.int32).cuda(), torch.ones(E).cuda()
    G, loss_part = K.linprobe_grad(dev(c["y"]), dev(c["W"]), dev(c["b"]), dev(c["labels"]), fold, held, one, C, want_loss=True)
    P, nll_part = run_proba(c)
    assert P.dtype == torch.float32 and tuple(P.shape) == (E, n, C)
    assert nll_part.dtype == torch.float64 and tuple(nll_part.shape) == ((n + 127) // 128, E)
    lab = c["labels"]
    trains = (lab >= 0) & (lab < C)
    off_label = trains[:, None] & (np.arange(C)[None, :] != lab[:, None])     # [n, C]
    assert trains[0] and off_label.any()
    Gp = host(G).reshape(n, E, Cp)[:, :, :C].transpose(1, 0, 2)               # [E, n, C]
    Ph = host(P)
    sel = np.broadcast_to(off_label[None], Ph.shape)
    assert np.array_equal(Ph[sel].view(np.uint32), Gp[sel].view(np.uint32))
    assert torch.equal(nll_part, loss_part)
    P2, nll2 = run_proba(c)
    assert torch.equal(P, P2) and torch.equal(nll_part, nll2)
    P3, none = run_proba(c, labels=False)                                     # without labels: the same probabilities, no log-loss
    assert none is None and torch.equal(P, P3)


# ------------------------------------------------------------------ 2. mh_linprobe_proba against float64
def test_transcendental_error_of_proba_is_what_the_constants_say():
    """test_linprobe_gpu.py's measurement, repeated for this kernel: with exact logits the whole error of P and of the log-loss is
    expf / logf's and the final roundings'.  Printed on every run; asserted against the constants (4x the figures measured there)."""
    worst_p = worst_ce = 0.0
    for shape in CASES:
        c = make_case(*shape, dyadic=True)
        P, part = run_proba(c)
        Pr, nll, ok, _ = proba_reference(c)
        e_p = np.abs(host(P).astype(np.float64) - Pr).max()
        e_ce = (np.abs(host(part).sum(0) - nll.sum(0)) / max(int(ok.sum()), 1)).max()
        print(f"{shape}: |P - P_ref| <= {e_p:.3e}, mean |nll - nll_ref| per counted row <= {e_ce:.3e}")
        worst_p, worst_ce = max(worst_p, e_p), max(worst_ce, e_ce)
    print(f"measured: probabilities {worst_p:.3e} (TOL_P {TOL_P:.1e}), log-loss {worst_ce:.3e} (TOL_CE {TOL_CE:.1e})")
    assert worst_p <= TOL_P and worst_ce <= TOL_CE


@pytest.mark.parametrize("shape", CASES, ids=IDS)
def test_proba_against_float64(shape):
    c = make_case(*shape)
    n, E, C = c["n"], c["J"], c["C"]
    P, part = run_proba(c)
    got = host(P).astype(np.float64)
    Pr, nll, ok, delta = proba_reference(c)
    assert not np.isnan(got).any() and ok[0] and (n == 1 or not ok.all())
    err = np.abs(got - Pr)
    tol = delta.T[:, :, None] + TOL_P
    print(f"{shape}: max |P - P_ref| = {err.max():.3e}, max delta = {delta.max():.3e}, worst err / tol = {(err / tol).max():.3f}")
    assert (err <= tol).all()
    rowsum = np.abs(got.sum(2) - 1.0)
    assert (rowsum <= TOL_P + 2 * C * U).all(), rowsum.max()
    loss = host(part).sum(0)
    ltol = ((2 * delta + TOL_CE) * ok[:, None]).sum(0)
    print(f"{shape}: max |nll - nll_ref| = {np.abs(loss - nll.sum(0)).max():.3e}, worst err / tol = "
          f"{(np.abs(loss - nll.sum(0)) / np.maximum(ltol, 1e-300)).max():.3f}")
    assert (np.abs(loss - nll.sum(0)) <= ltol).all()
    # a NaN query row: NaN under every job, every other row as before
    bad = n // 2
    y = c["y"].copy()
    y[bad, c["D"] // 2] = np.nan
    Pn, _ = run_proba(c, y=y)
    Pn, keep = host(Pn), np.arange(n) != bad
    assert np.isnan(Pn[:, bad]).all() and np.array_equal(Pn[:, keep], host(P)[:, keep])


def test_proba_wrapper_checks_its_later_arguments():
    c = make_case(6, 8, 3, 2)
    y, W, b, lab = dev(c["y"]), dev(c["W"]), dev(c["b"]), dev(c["labels"])
    with pytest.raises(ValueError, match=r"labels must be int64 \[6\]"):
        K.linprobe_proba(y, W, b, 3, labels=lab[:5])
    with pytest.raises(ValueError, match=r"labels must be int64 \[6\]"):
        K.linprobe_proba(y, W, b, 3, labels=lab.int())
    with pytest.raises(ValueError, match="the log-loss needs labels"):
        K.linprobe_proba(y, W, b, 3, want_nll=True)
    with pytest.raises(ValueError, match=r"P must be a contiguous f32 \[2, 6, 3\]"):
        K.linprobe_proba(y, W, b, 3, P=torch.zeros((2, 6, 4), device="cuda"))
    with pytest.raises(ValueError, match=r"nll_part must be a contiguous f64 \[1, 2\]"):
        K.linprobe_proba(y, W, b, 3, labels=lab, nll_part=torch.zeros((1, 2), device="cuda"))


# ------------------------------------------------------------------ 3. mh_auroc_counts_many
def auroc_case(N, C, E):
    """Scores in eighths (ties everywhere), class C - 1 without a positive, labels -1 and C among the rows, column 0 of the last table
    all NaN and one more NaN in table 0."""
    rng = np.random.default_rng(100 * N + C + E)
    s = (rng.integers(-16, 17, (E, N, C)) / 8.0).astype(np.float32)
    labels = rng.integers(-1, C + 1, N).astype(np.int64)
    labels[labels == C - 1] = 0
    s[E - 1, :, 0] = np.nan
    s[0, N // 2, 1] = np.nan
    return s, labels


@pytest.mark.parametrize("CE", [(2, 1), (3, 5), (64, 3)], ids=lambda v: "C%d-E%d" % v)
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1025, 2049])
def test_auroc_counts_many_are_the_exact_pair_counts(N, CE):
    C, E = CE
    s, labels = auroc_case(N, C, E)
    sd, ld = dev(s), dev(labels)
    got = K.auroc_counts_many(sd, ld)
    assert got.dtype == torch.int64 and tuple(got.shape) == (E, C, 4)
    want = np.stack([SR.pair_counts(s[e], labels) for e in range(E)])
    assert (want[:, C - 1, 1] == 0).all() and (want[E - 1, 0, 3] == N) and want[0, 1, 3] >= 1
    assert np.array_equal(host(got), want)
    for e in range(E):
        assert torch.equal(got[e], K.auroc_counts(sd[e], ld)), e
    assert torch.equal(got, K.auroc_counts_many(sd, ld, counts=torch.full((E, C, 4), -7, device="cuda")))   # zeroed by the call


def test_auroc_counts_many_take_padded_rows_and_tables():
    N, C, E = 257, 3, 5
    s, labels = auroc_case(N, C, E)
    buf = torch.full((E, N + 3, C + 5), 99.0, device="cuda")                  # ld_row = C + 5 > C, ld_table = (N + 3) ld_row > N ld_row
    view = buf[:, :N, :C]
    view.copy_(dev(s))
    assert view.stride() == ((N + 3) * (C + 5), C + 5, 1)
    got = K.auroc_counts_many(view, dev(labels))
    assert np.array_equal(host(got), np.stack([SR.pair_counts(s[e], labels) for e in range(E)]))


# ------------------------------------------------------------------ 4. - 6. the probe
@pytest.fixture(scope="module")
def e2e():
    """The overlapping case, fitted once; out0 / out1: evaluate() with the defaults before and after evaluate(auroc=True)."""
    x, labels, fold = SR.e2e_case()
    c = SR.E2E
    p = LinearProbe(c["C"], strengths=c["strengths"], max_iter=c["steps"], tol=0.0, device="cuda")
    p.fit(dev(x), dev(labels), dev(fold))
    out0 = p.evaluate()
    assert p.per_job_auc is None and p.per_job_nll is None
    out = p.evaluate(auroc=True)
    oof = [host(p.oof_proba(strength=s)) for s in c["strengths"]]
    out1 = p.evaluate()
    return dict(x=x, labels=labels, fold=fold, p=p, out0=out0, out=out, out1=out1, oof=oof)


DEFAULT_KEYS = ["linprobe_acc", "linprobe_acc_mean", "linprobe_acc_std", "linprobe_bacc", "linprobe_bacc_mean", "linprobe_bacc_std",
                "linprobe_f1", "linprobe_f1_mean", "linprobe_f1_std", "linprobe_best_strength", "linprobe_strengths", "linprobe_folds",
                "linprobe_n", "per_job"]
ADDED_KEYS = ["linprobe_auc", "linprobe_auc_mean", "linprobe_auc_std", "linprobe_nll", "linprobe_nll_mean", "linprobe_nll_std",
              "per_job_auc", "per_job_nll"]


def test_evaluate_with_the_defaults_is_unchanged(e2e):
    c, p, labels, fold = SR.E2E, e2e["p"], e2e["labels"], e2e["fold"]
    S = len(c["strengths"])
    for out in (e2e["out0"], e2e["out1"]):
        assert list(out) == DEFAULT_KEYS
    assert list(e2e["out"]) == DEFAULT_KEYS + ADDED_KEYS
    per_job = host(e2e["out0"]["per_job"])
    for f in range(c["F"]):                                                   # the figures of the device's own predictions: integer counts
        rows = np.flatnonzero(fold == f)
        got = host(K.fewshot_predict(p._y.index_select(0, dev(rows)), p._Wx[f * S:(f + 1) * S], p._bx[f * S:(f + 1) * S], c["C"]))
        assert np.array_equal(per_job[f], R.tally(got, labels[rows], c["C"])[2])
    mean = per_job.mean(0)
    best = max(range(S), key=lambda s: (mean[s, 0], c["strengths"][s]))
    for out in (e2e["out0"], e2e["out"], e2e["out1"]):
        assert out["linprobe_best_strength"] == c["strengths"][best] and out["linprobe_acc"] == mean[best, 0]
        assert out["linprobe_acc_mean"] == tuple(mean[:, 0]) and out["linprobe_f1_mean"] == tuple(mean[:, 2])
        assert np.allclose(out["linprobe_bacc_std"], per_job[:, :, 1].std(0, ddof=1), rtol=1e-12, atol=0)
        assert out["linprobe_folds"] == c["F"] and out["linprobe_n"] == c["n"] and out["linprobe_strengths"] == c["strengths"]
        for k in DEFAULT_KEYS[:-1]:
            assert out[k] == e2e["out0"][k], k
        assert torch.equal(out["per_job"], e2e["out0"]["per_job"])


def test_evaluate_auroc_is_the_exact_figure_of_its_own_probabilities(e2e):
    c, p, labels, fold, out = SR.E2E, e2e["p"], e2e["labels"], e2e["fold"], e2e["out"]
    F, S, C = c["F"], len(c["strengths"]), c["C"]
    auc, nll = host(out["per_job_auc"]), host(out["per_job_nll"])
    assert auc.shape == (F, S, C) and auc.dtype == np.float64 and nll.shape == (F, S) and nll.dtype == np.float64
    counts = np.zeros((F, S, C, 4), dtype=np.int64)
    for f in range(F):
        rows = np.flatnonzero(fold == f)
        for s in range(S):
            P = e2e["oof"][s][rows]
            counts[f, s] = SR.pair_counts(P, labels[rows])
            want_nll = -np.log(P.astype(np.float64)[np.arange(len(rows)), labels[rows]]).mean()
            assert abs(nll[f, s] - want_nll) <= TOL_CE, (f, s, nll[f, s], want_nll)
    assert np.allclose(auc, SR.auroc(counts), rtol=1e-12, atol=0) and not np.isnan(auc).any()
    assert 0.6 < auc.min() and auc.max() < 0.95                               # the case overlaps: nothing here is decided by a 1.0

    def check(o, job_auc):
        m, sd = job_auc.mean(0), job_auc.std(0, ddof=1)
        assert np.allclose(o["linprobe_auc_mean"], m, rtol=1e-12, atol=0) and np.allclose(o["linprobe_auc_std"], sd, rtol=1e-12, atol=0)
        assert np.allclose(o["linprobe_nll_mean"], nll.mean(0), rtol=1e-12, atol=0)
        assert np.allclose(o["linprobe_nll_std"], nll.std(0, ddof=1), rtol=1e-12, atol=0)
        return m

    m = check(out, SR.averaged(auc, counts, "macro"))
    assert np.allclose(SR.averaged(auc, counts, "macro"), auc.mean(2), rtol=1e-12, atol=0)      # every class counts in every fold here
    by_auc = max(range(S), key=lambda s: (m[s], c["strengths"][s]))
    by_nll = max(range(S), key=lambda s: (-nll.mean(0)[s], c["strengths"][s]))
    o = p.evaluate(auroc=True, select="auc")
    assert o["linprobe_best_strength"] == c["strengths"][by_auc] == p.best_strength_ and o["linprobe_auc"] == o["linprobe_auc_mean"][by_auc]
    o = p.evaluate(auroc=True, select="nll")
    assert o["linprobe_best_strength"] == c["strengths"][by_nll] and o["linprobe_nll"] == o["linprobe_nll_mean"][by_nll]
    assert o["linprobe_acc"] == o["linprobe_acc_mean"][by_nll]                # every figure is reported at the chosen strength
    o = p.evaluate(auroc=True, average="weighted", select="auc")
    mw = check(o, SR.averaged(auc, counts, "weighted"))
    assert o["linprobe_best_strength"] == c["strengths"][max(range(S), key=lambda s: (mw[s], c["strengths"][s]))]
    o = p.evaluate(auroc=True, average=None)
    assert np.allclose(np.array(o["linprobe_auc_mean"]), auc.mean(0), rtol=1e-12, atol=0) and len(o["linprobe_auc"]) == C
    assert np.allclose(np.array(o["linprobe_auc_std"]), auc.std(0, ddof=1), rtol=1e-12, atol=0)
    assert torch.equal(o["per_job_auc"], out["per_job_auc"]) and torch.equal(o["per_job_nll"], out["per_job_nll"])
    p.evaluate()                                                              # leave the shared probe as the fixture left it


def test_end_to_end_auroc_lies_in_the_interval_float64_leaves(e2e):
    c, labels, fold = SR.E2E, e2e["labels"], e2e["fold"]
    _, Pref = SR.e2e_reference()
    auc = host(e2e["out"]["per_job_auc"])
    worst_p = worst_share = 0.0
    for f in range(c["F"]):
        rows = np.flatnonzero(fold == f)
        for s in range(len(c["strengths"])):
            worst_p = max(worst_p, np.abs(e2e["oof"][s][rows].astype(np.float64) - Pref[f, s, rows]).max())
            for k in range(c["C"]):
                lo, hi, share = SR.auc_interval(Pref[f, s, rows, k], labels[rows], k, R.MARGIN)
                worst_share = max(worst_share, share)
                assert lo <= auc[f, s, k] <= hi, (f, s, k, lo, auc[f, s, k], hi)
    print(f"largest |P_device - P_f64| over the held-out rows {worst_p:.3e} (MARGIN / 2 = {R.MARGIN / 2:.1e}); "
          f"undecided pairs at most {100 * worst_share:.2f} %")
    assert worst_share <= R.MAX_UNDECIDED


# ------------------------------------------------------------------ 5. oof_proba and predict_proba
def test_oof_proba_and_predict_proba():
    x, labels, fold = R.e2e_case()                                            # 6 rows in no fold, 2 labels outside the classes
    C, strengths = R.E2E["C"], (1e-2, 1e-1)
    p = LinearProbe(C, strengths=strengths, max_iter=40, tol=0.0, device="cuda").fit(dev(x), dev(labels), dev(fold))
    S = len(strengths)
    for s, lam in enumerate(strengths):
        oof = p.oof_proba(strength=lam)
        assert oof.dtype == torch.float32 and tuple(oof.shape) == (len(x), C)
        assert torch.isnan(oof[dev(np.flatnonzero(fold < 0))]).all() and not torch.isnan(oof[dev(np.flatnonzero(fold >= 0))]).any()
        for f in range(R.E2E["F"]):
            rows = dev(np.flatnonzero(fold == f))
            j = f * S + s
            want, _ = K.linprobe_proba(p._y.index_select(0, rows), p._Wx[j:j + 1], p._bx[j:j + 1], C)
            assert torch.equal(oof.index_select(0, rows), want[0]), (s, f)
    best = p.evaluate()["linprobe_best_strength"]
    assert torch.equal(p.oof_proba().nan_to_num(nan=-1.0), p.oof_proba(strength=best).nan_to_num(nan=-1.0))
    rng = np.random.default_rng(3)
    fresh = dev((x[rng.choice(len(x), 50, replace=False)] + rng.standard_normal((50, x.shape[1]))).astype(np.float32))
    for lam in (None,) + strengths:
        P = p.predict_proba(fresh, strength=lam)
        assert P.dtype == torch.float32 and tuple(P.shape) == (50, C)
        top = torch.sort(P, dim=1, descending=True).values
        clear = top[:, 0] != top[:, 1]                                        # where they tie exactly, predict answers the smaller class
        assert int(clear.sum()) >= 45
        assert torch.equal(P.argmax(1)[clear].int(), p.predict(fresh, strength=lam)[clear])
        assert float((P.double().sum(1) - 1).abs().max()) <= TOL_P + 2 * C * U
    with pytest.raises(ValueError, match="strength must be one of"):
        p.predict_proba(fresh, strength=0.5)
    q = LinearProbe(C, strengths=strengths, max_iter=8, tol=0.0, device="cuda").fit(dev(x), dev(labels))
    with pytest.raises(ValueError, match="needs folds"):
        q.oof_proba()
    with pytest.raises(ValueError, match="no best strength"):
        q.predict_proba(fresh)


# ------------------------------------------------------------------ 7. graph replay
def test_a_folds_scores_replay_bit_for_bit_from_a_graph():
    c = make_case(300, 40, 3, 33)
    n, E, C = c["n"], c["J"], c["C"]
    y, W, b, lab = dev(c["y"]), dev(c["W"]), dev(c["b"]), dev(c["labels"])
    P, part = K.linprobe_proba(y, W, b, C, labels=lab, want_nll=True)
    counts = K.auroc_counts_many(P, lab)
    torch.cuda.synchronize()
    gP, gpart, gcounts = torch.empty_like(P), torch.empty_like(part), torch.empty_like(counts)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.linprobe_proba(y, W, b, C, labels=lab, P=gP, nll_part=gpart)
        K.auroc_counts_many(gP, lab, counts=gcounts)
    for _ in range(2):
        gP.fill_(-1.0)
        gpart.fill_(-1.0)
        gcounts.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gP, P) and torch.equal(gpart, part) and torch.equal(gcounts, counts)
    assert int(counts[:, :, 0].min()) > 0 and (n, E) == (300, 33)
