"""MI355X: mh_knn_scores (csrc/retrieval_topk.hip) and the kNN probe built on it and on mh_retrieval_topk (mirror_amd/knn.py), against the
float64 restatements of tests/retrieval_topk_ref.py.

The vote is compared on the neighbours the device selected (so its tolerance is the vote's own: one f32 exp and kk f32 adds of terms
<= 1, 1e-5 absolute).  The probe is compared end to end: its data are four Gaussian class clusters whose noise puts the restated
accuracy inside [0.6, 0.95], at seeds where float64 DECIDES what the metrics depend on (asserted below from float64 alone): every
row's top two scores, and every pair of scores of one class that the AUROC orders, differ by more than 1e-4 or are exactly equal
(rows voted for by one class only score exactly 1 and 0 in f32 as in f64)."""
import math

import numpy as np
import pytest
import torch
from sklearn.metrics import f1_score, roc_auc_score

from mirror_amd import kernels as K
from mirror_amd.knn import KNNProbe
from mirror_amd.retrieval import retrieval_topk
from tests import retrieval_topk_ref as R

pytestmark = pytest.mark.gpu

DECIDED = 1e-4
C4 = 4


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ------------------------------------------------------------------ 7. the vote
@pytest.fixture(scope="module")
def neighbours():
    """n = 400 unit rows in 64 dimensions, leave-one-out top-20 from the device, and labels with two entries outside [0, 4)."""
    n, D, kk = 400, 64, 20
    rng = np.random.default_rng(21)
    x = rng.standard_normal((n, D)).astype(np.float32)
    labels = rng.integers(0, C4, n)
    labels[5], labels[17] = 9, -1
    ids = torch.arange(n)
    val, idx = retrieval_topk(dev(x), dev(x), kk, ids, ids, normalize=True)
    return idx, val, labels


@pytest.mark.parametrize("inv_t", [1.0 / 0.07, 0.0])
def test_scores_equal_the_restated_vote_on_the_device_neighbours(neighbours, inv_t):
    idx, val, labels = neighbours
    idx = idx.clone()
    val = val.clone()
    idx[3] = -1                                            # an all-empty row
    val[3] = -math.inf
    idx[8, 10:] = -1                                       # and a half-empty one
    val[8, 10:] = -math.inf
    got = K.knn_scores(idx, val, dev(labels), C4, inv_t).cpu().numpy()
    want = R.knn_scores_np(idx.cpu().numpy(), val.cpu().numpy(), labels, C4, inv_t)
    assert got.dtype == np.float32 and got.shape == (400, C4)
    sums = got.astype(np.float64).sum(1)
    votes = (want.sum(1) > 0)
    print(f"inv_t {inv_t:.4f}: max |score - f64| {np.abs(got - want).max():.3e}, max |row sum - 1| {np.abs(sums[votes] - 1).max():.3e}, "
          f"rows without a vote {int((~votes).sum())}")
    assert not votes[3] and votes.sum() >= 398
    assert np.all(got[~votes] == 0.0)
    assert np.abs(sums[votes] - 1.0).max() <= 1e-6
    assert np.abs(got - want).max() <= 1e-5
    if inv_t == 0.0:                                       # the unweighted vote: multiples of 1 / (contributing slots)
        assert np.allclose(got[0] * 20, np.round(got[0] * 20), atol=1e-5)
    # labels from the host and as int32 go through the same launch
    again = K.knn_scores(idx, val, torch.from_numpy(labels.astype(np.int32)), C4, inv_t).cpu().numpy()
    assert np.array_equal(again, got)


def test_one_class_and_labels_outside_it(neighbours):
    idx, val, labels = neighbours
    got = K.knn_scores(idx, val, dev(labels), 1, 1.0 / 0.07).cpu().numpy()
    want = R.knn_scores_np(idx.cpu().numpy(), val.cpu().numpy(), labels, 1, 1.0 / 0.07)
    assert got.shape == (400, 1)
    assert np.array_equal(got[:, 0] > 0, want[:, 0] > 0)               # a row whose 20 neighbours all have other labels is all zero
    assert np.abs(got - want).max() <= 1e-5 and set(np.unique(got.round(5))) <= {0.0, 1.0}
    wide = K.knn_scores(idx, val, dev(labels), 1024, 0.0).cpu().numpy()  # the widest class row: label 9 now counts
    assert np.abs(wide - R.knn_scores_np(idx.cpu().numpy(), val.cpu().numpy(), labels, 1024, 0.0)).max() <= 1e-5
    assert wide[:, C4:9].sum() == 0 and wide[:, 9].sum() > 0


# ------------------------------------------------------------------ 8. the probe
def clusters(n, seed, sigma, D=64):
    """Four Gaussian class clusters: unit-variance noise of size sigma around four Gaussian centres."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((C4, D))
    y = rng.integers(0, C4, n)
    x = (centres[y] + sigma * rng.standard_normal((n, D))).astype(np.float32)
    return x, y


def patients(n_pat, seed, sigma, D=64):
    """2-3 slides per patient, near-copies of the patient's embedding (noise 0.05 of its own)."""
    px, py = clusters(n_pat, seed, sigma, D)
    rng = np.random.default_rng(seed + 1000)
    reps = rng.integers(2, 4, n_pat)
    group = np.repeat(np.arange(n_pat) * 7 + 3, reps)
    x = (np.repeat(px, reps, axis=0) + 0.05 * rng.standard_normal((group.size, D))).astype(np.float32)
    return x, np.repeat(py, reps), group


def probe_np(q, bank, labels, k, T, qgroup=None, kgroup=None):
    """float64 scores [nq, 4] of the probe with normalize=True."""
    idx, val = R.topk_np(R.unit(q), R.unit(bank), k, qgroup, kgroup)
    return R.knn_scores_np(idx, val, labels, C4, 0.0 if math.isinf(T) else 1.0 / T)


def decided(scores, y):
    """(rows whose top two scores differ by more than 1e-4, does float64 decide every pair the one-vs-rest AUROC orders)."""
    top = np.sort(scores, axis=1)
    rows = top[:, -1] - top[:, -2] > DECIDED
    pairs = True
    for c in range(scores.shape[1]):
        d = np.abs(scores[y == c, c][:, None] - scores[y != c, c][None, :])
        pairs = pairs and not ((d > 0) & (d <= DECIDED)).any()
    return rows, pairs


def want_dict(scores, y, k, n_bank, rows):
    pred = scores.argmax(1)
    return {"correct": int((pred == y).sum()), "undecided": int((~rows).sum()),
            "knn_auroc": float(roc_auc_score(y, scores, multi_class="ovr", average="macro")),
            "knn_f1": float(f1_score(y, pred, average="weighted")), "knn_k": k, "knn_n": n_bank}


def check(got, want, n):
    print(f"acc {got['knn_acc']:.3f} (f64: {100.0 * want['correct'] / n:.3f}, undecided rows {want['undecided']}), auroc {got['knn_auroc']:.6f} "
          f"(sklearn {want['knn_auroc']:.6f}), f1 {got['knn_f1']:.6f} (sklearn {want['knn_f1']:.6f})")
    assert list(got) == ["knn_acc", "knn_auroc", "knn_f1", "knn_k", "knn_n"]
    assert want["undecided"] == 0                          # every row is decided, so the accuracy is compared as it stands
    assert got["knn_acc"] == np.float32(want["correct"]) * np.float32(100.0) / n       # metrics.accuracy's f32 expression
    assert abs(got["knn_auroc"] - want["knn_auroc"]) <= 1e-12
    assert abs(got["knn_f1"] - want["knn_f1"]) <= 1e-12
    assert got["knn_k"] == want["knn_k"] and got["knn_n"] == want["knn_n"]


SIGMA, K20, T07 = 2.75, 20, 0.07


@pytest.fixture(scope="module")
def cohort():
    """240 rows of the four clusters: a bank of 160 and 80 queries.  Restated accuracies 0.831 (leave-one-out) and 0.825."""
    x, y = clusters(240, 47, SIGMA)
    return x[:160], y[:160], x[160:], y[160:]


def _neighbours_decided(q, bank, k, qgroup=None, kgroup=None, normalize=True):
    """No query has its k-th and (k + 1)-th float64 neighbour within the project's margin 1e-5 |q_i| |k_j|: f32 selects the same SET of
    neighbours (two close ones inside the set may swap slots, which moves no score by more than the order of a sum)."""
    q, bank = (R.unit(q), R.unit(bank)) if normalize else (np.asarray(q, dtype=np.float64), np.asarray(bank, dtype=np.float64))
    idx, val = R.topk_np(q, bank, k + 1, qgroup, kgroup)
    m = R.MARGIN * np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(bank, axis=1)[np.maximum(idx[:, -2:], 0)]
    return not ((idx[:, -1] >= 0) & (val[:, -2] - val[:, -1] <= m.max(1))).any()


def test_leave_one_out_and_evaluate_equal_the_restatement(cohort):
    bx, by, qx, qy = cohort
    ids = np.arange(160)
    probe = KNNProbe(C4, k=K20, temperature=T07).fit(dev(bx), dev(by))
    # leave-one-out
    s = probe_np(bx, bx, by, K20, T07, ids, ids)
    rows, pairs = decided(s, by)
    assert pairs and _neighbours_decided(bx, bx, K20, ids, ids)
    want = want_dict(s, by, K20, 160, rows)
    assert 0.6 <= want["correct"] / 160 <= 0.95
    check(probe.leave_one_out(), want, 160)
    # a validation split against the bank
    s = probe_np(qx, bx, by, K20, T07)
    rows, pairs = decided(s, qy)
    assert pairs and _neighbours_decided(qx, bx, K20)
    want = want_dict(s, qy, K20, 160, rows)
    assert 0.6 <= want["correct"] / 80 <= 0.95
    check(probe.evaluate(dev(qx), dev(qy)), want, 80)
    # the scores themselves, and their argmax row by row
    got = probe.scores(dev(qx)).cpu().numpy()
    assert np.abs(got - s).max() <= 1e-5 and np.array_equal(got.argmax(1)[rows], s.argmax(1)[rows])
    # fit in three chunks equals fit at once; labels from the host
    chunked = KNNProbe(C4, k=K20, temperature=T07)
    for sl in (slice(0, 50), slice(50, 51), slice(51, 160)):
        assert chunked.fit(dev(bx[sl]), torch.from_numpy(by[sl])) is chunked
    assert chunked.leave_one_out() == probe.leave_one_out()
    assert chunked.evaluate(dev(qx), dev(qy)) == probe.evaluate(dev(qx), dev(qy))
    merged = KNNProbe(C4, k=K20, temperature=T07).merge_state([KNNProbe(C4).fit(dev(bx[:70]), dev(by[:70])),
                                                               KNNProbe(C4).fit(dev(bx[70:]), dev(by[70:]))])
    assert merged.leave_one_out() == probe.leave_one_out()
    assert probe.reset().emb == [] and probe.labels == [] and probe.group == []
    with pytest.raises(ValueError, match="bank is empty"):
        probe.leave_one_out()


def test_patient_groups_stop_the_leakage_between_slides_of_one_patient():
    x, y, g = patients(70, 10, SIGMA)
    n = y.size
    assert n == 172 and np.unique(g).size == 70
    s_grouped = probe_np(x, x, y, K20, T07, g, g)
    s_rows = probe_np(x, x, y, K20, T07, np.arange(n), np.arange(n))
    rows, pairs = decided(s_grouped, y)
    assert pairs and _neighbours_decided(x, x, K20, g, g)
    want = want_dict(s_grouped, y, K20, n, rows)
    leaky = 100.0 * float((s_rows.argmax(1) == y).mean())
    assert 0.6 <= want["correct"] / n <= 0.95 and leaky >= 100.0 * want["correct"] / n + 10.0      # the restatement: 76.7 % against 100 %
    with_groups = KNNProbe(C4, k=K20, temperature=T07).fit(dev(x), dev(y), group=dev(g)).leave_one_out()
    without = KNNProbe(C4, k=K20, temperature=T07).fit(dev(x), dev(y)).leave_one_out()
    check(with_groups, want, n)
    print(f"leave-one-slide-out {without['knn_acc']:.2f} % (f64 {leaky:.2f}), leave-one-patient-out {with_groups['knn_acc']:.2f} %")
    assert without["knn_acc"] >= with_groups["knn_acc"] + 10.0
    # a query set with its patients: evaluate(query_group=) leaves the patient's bank rows out, here the same as leave-one-out
    same = KNNProbe(C4, k=K20, temperature=T07).fit(dev(x), dev(y), group=dev(g.astype(np.int32)))
    assert same.evaluate(dev(x), dev(y), query_group=dev(g)) == with_groups
    with pytest.raises(ValueError, match="needs a bank fitted with"):
        KNNProbe(C4).fit(dev(x), dev(y)).scores(dev(x), query_group=dev(g))
    with pytest.raises(ValueError, match="every fit"):
        same.fit(dev(x), dev(y))


def test_the_unweighted_vote_on_raw_dot_products():
    """temperature = inf (inv_temperature 0) and normalize=False go through the same two kernels."""
    x, y = clusters(150, 5, SIGMA)
    ids = np.arange(150)
    assert _neighbours_decided(x, x, 7, ids, ids, normalize=False)
    idx, val = R.topk_np(x, x, 7, ids, ids)
    want = R.knn_scores_np(idx, val, y, C4, 0.0)
    probe = KNNProbe(C4, k=7, temperature=math.inf, normalize=False).fit(dev(x), dev(y), group=dev(ids))
    got = probe.scores(dev(x), query_group=dev(ids)).cpu().numpy()
    assert np.abs(got - want).max() <= 1e-5
    assert np.allclose(got * 7, np.round(got * 7), atol=1e-5) and np.abs(got.sum(1) - 1).max() <= 1e-6
