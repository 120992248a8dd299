"""CPU (no GPU): the host reference of the data feed draws (tests/datafeed_ref.py, written from include/mirror_hip.h) has the
properties and the distribution of `np.random.choice(n, N, replace=n < N)` and of WeightedRandomSampler over class-balanced weights;
the host side of the new surface (weights against the reference's own, refusals, the epoch plan).

Every statistical bound is 5 sigma of the binomial: a count X ~ Bin(D, p) must satisfy |X - D p| <= 5 sqrt(D p (1 - p)).  The worst |z|
of the definition as it stands is recorded beside each check (a condition, not a measurement: the draws are fixed by their seeds)."""
import os

import numpy as np
import pytest
import torch

import mirror_amd
from mirror_amd import data as D, kernels as K
from tests import datafeed_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_sampler.npz")


def _z(counts, draws, p):
    p = np.broadcast_to(np.asarray(p, dtype=np.float64), np.shape(counts))
    return np.abs(np.asarray(counts, dtype=np.float64) - draws * p) / np.sqrt(draws * p * (1.0 - p))


@pytest.fixture(scope="module")
def subset_draws():
    """int64 [4000, 64]: n = 200, N = 64, seed 1234, draws 0 .. 3999."""
    return np.stack([R.sample_local(200, 64, 1234, d) for d in range(4000)])


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def id_draws(golden):
    """(labels, ids [8000]): the 80-slide class-balanced cdf (classes 50 / 7 / 20 / 3), seed 99, draw 0."""
    return golden["labels"], R.sample_weighted(R.cdf_of(golden["weights"]), 8000, 99, 0)


# ----------------------------------------------------------------------------- properties of the reference itself
def test_rows_without_replacement_are_distinct_and_in_range(subset_draws):
    assert subset_draws.min() >= 0 and subset_draws.max() < 200
    assert all(len(set(r.tolist())) == 64 for r in subset_draws[:200])
    big = R.sample_local(20000, 2048, 7, 3)
    assert len(set(big.tolist())) == 2048 and big.min() >= 0 and big.max() < 20000


def test_a_shorter_draw_is_a_prefix_of_a_longer_one():
    full = R.sample_local(300, 300, 5, 11)
    for N in (1, 17, 64, 299):
        assert np.array_equal(R.sample_local(300, N, 5, 11), full[:N])


def test_n_equal_N_is_a_permutation():
    for n in (1, 2, 63, 64, 257):
        assert sorted(R.sample_local(n, n, 3, n).tolist()) == list(range(n))


def test_short_slides_follow_the_multiply_shift_rule():
    n, N = 37, 64
    w = R.draw_words(N, R.KIND_ROWS, 9, 21)
    got = R.sample_local(n, N, 21, 9)
    assert got.tolist() == [(int(x) * n) >> 32 for x in w]
    assert got.min() >= 0 and got.max() < n and len(set(got.tolist())) < N
    assert R.sample_local(1, 8, 21, 9).tolist() == [0] * 8


def test_different_draws_and_kinds_give_different_values():
    a, b = R.sample_local(200, 64, 1234, 0), R.sample_local(200, 64, 1234, 1)
    assert not np.array_equal(a, b)
    assert not np.array_equal(a, R.sample_local(200, 64, 1235, 0))
    assert not np.array_equal(R.sample_local(200, 64, 1234, 1 << 32), a)          # the high half of the draw id counts
    assert not np.array_equal(R.draw_words(64, R.KIND_ROWS, 0, 1), R.draw_words(64, R.KIND_IDS, 0, 1))
    # two slots that hold the same slide get different rows; offset and base add up
    rows = R.sample_rows([2, 2], [5, 6, 200], [0, 5, 11], 64, 1234, 10)
    assert not np.array_equal(rows[0], rows[1]) and rows.min() >= 11 and rows.max() < 211
    assert np.array_equal(rows, R.sample_rows([2, 2], [5, 6, 200], [0, 5, 11], 64, 1234, 4, base=6))
    assert np.array_equal(rows[1] - 11, R.sample_local(200, 64, 1234, 11))


def test_slots_without_a_slide_have_the_documented_rows():
    rows = R.sample_rows([-1, 3, 1, 0], [4, 0, 9], [0, 4, 4], 5, 1, 0)
    assert rows[0].tolist() == [-1] * 5 and rows[1].tolist() == [-1] * 5 and rows[2].tolist() == [4] * 5
    assert rows[3].min() >= 0 and rows[3].max() < 4


# ----------------------------------------------------------------------------- distribution
def test_every_row_is_included_equally_often(subset_draws):
    """Inclusion count of each of the 200 rows over 4000 draws ~ Bin(4000, 64 / 200).  Worst |z| of the definition: 2.95."""
    counts = np.bincount(subset_draws.reshape(-1), minlength=200)
    z = _z(counts, 4000, 64 / 200)
    print("inclusion worst |z|", z.max())
    assert z.max() <= 5.0


def test_the_first_position_is_uniform(subset_draws):
    """Row at position 0 over 4000 draws ~ Bin(4000, 1 / 200) per row (an ORDERED subset).  Worst |z| of the definition: 2.47."""
    counts = np.bincount(subset_draws[:, 0], minlength=200)
    z = _z(counts, 4000, 1 / 200)
    print("position-0 worst |z|", z.max())
    assert z.max() <= 5.0


def test_slide_ids_are_class_balanced(id_draws):
    """8000 ids: each of the 4 classes ~ Bin(8000, 1 / 4) (worst |z| 0.85), each slide ~ Bin(8000, 1 / (4 count[label])) (3.12)."""
    labels, ids = id_draws
    assert ids.min() >= 0 and ids.max() < 80
    zc = _z(np.bincount(labels[ids], minlength=4), 8000, 0.25)
    zs = _z(np.bincount(ids, minlength=80), 8000, 1.0 / (4.0 * np.bincount(labels)[labels]))
    print("class worst |z|", zc.max(), "slide worst |z|", zs.max())
    assert zc.max() <= 5.0 and zs.max() <= 5.0


def test_a_zero_weight_slide_is_never_drawn():
    w = np.array([0.0, 1.0, 0.0, 0.0, 2.0, 1.0, 0.0])
    ids = R.sample_weighted(R.cdf_of(w), 4000, 5, 2)
    assert set(ids.tolist()) == {1, 4, 5}
    z = _z(np.bincount(ids, minlength=7)[[1, 4, 5]], 4000, [0.25, 0.5, 0.25])
    assert z.max() <= 5.0
    u = R.uniforms53(4000, 5, 2)
    assert u.min() >= 0.0 and u.max() < 1.0 and len(set(u.tolist())) == 4000


# ----------------------------------------------------------------------------- surface
def test_balanced_weights_equal_the_reference_samplers(golden):
    """tools/make_golden_sampler.py recorded the weights utils/loader.py:15-26 handed to WeightedRandomSampler for these labels."""
    assert np.bincount(golden["labels"]).tolist() == [50, 7, 20, 3] and int(golden["num_samples"]) == 80
    assert np.array_equal(D.balanced_weights(golden["labels"]), golden["weights"])
    assert np.array_equal(D.balanced_weights(torch.from_numpy(golden["labels"])), golden["weights"])
    assert np.array_equal(R.balanced_weights(golden["labels"]), golden["weights"])


def test_the_new_surface_refuses_cpu_tensors():
    i64 = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(mirror_amd.MirrorHipError):
        K.sample_rows(i64, i64, i64, 8, 1, 0)
    with pytest.raises(mirror_amd.MirrorHipError):
        K.sample_weighted(torch.linspace(0.1, 1.0, 10, dtype=torch.float64), 8, 1, 0)
    with pytest.raises(mirror_amd.MirrorHipError):
        D.ClassBalancedSampler([0, 1, 1], device="cpu", seed=1)
    with pytest.raises(mirror_amd.MirrorHipError):
        D.DeviceSlideBank([torch.zeros(3, 4)], torch.zeros(1, 2), 2, device="cpu", targets={"label": torch.zeros(1)})
    with pytest.raises(ValueError):
        D.DeviceSlideBank([torch.zeros(3, 4)], torch.zeros(1, 2), 2, device="cpu", targets={"label": torch.zeros(2)})


def test_the_binding_declares_the_new_entry_points():
    from mirror_amd import _lib
    lib = _lib.load()
    assert {"mh_sample_rows", "mh_sample_weighted"} <= set(_lib._SIGS) and _lib.ABI_VERSION == 123
    assert hasattr(lib, "mh_sample_rows") and hasattr(lib, "mh_sample_weighted")


def test_an_epoch_is_reproducible_from_seed_and_epoch():
    """The id order is torch.randperm under seed + epoch, the token draw ids are (epoch << 32) + first slot of the batch: any batch of
    any epoch can be restated (and an epoch resumed) from (seed, epoch, batch index) alone."""
    n, bs = 23, 4
    ids = D.epoch_ids(n, epoch=3, seed=40)
    assert ids == torch.randperm(n, generator=torch.Generator().manual_seed(43)).tolist() and sorted(ids) == list(range(n))
    assert ids == D.epoch_ids(n, epoch=3, seed=40) and ids != D.epoch_ids(n, epoch=4, seed=40)
    assert D.epoch_ids(n, epoch=3, seed=40, shuffle=False) == list(range(n))
    for drop_last in (False, True):
        plan = D.epoch_plan(n, bs, epoch=3, drop_last=drop_last)
        assert plan == R.epoch_offsets(n, bs, 3, drop_last) and len(plan) == (5 if drop_last else 6)
        assert plan[2] == (8, 4, (3 << 32) + 8)
    # the rows of batch 2, restated from (seed, epoch, batch index) through the reference: slot b of the batch uses draw id offset + b
    lengths, first, count, offset = [5 + 7 * i for i in range(n)], *D.epoch_plan(n, bs, epoch=3)[2]
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    rows = R.sample_rows(ids[first:first + count], lengths, starts, 16, 40, offset)
    for b in range(count):
        sl = ids[first + b]
        assert np.array_equal(rows[b] - starts[sl], R.sample_local(lengths[sl], 16, 40, (3 << 32) + 8 + b))
    assert not np.array_equal(rows, R.sample_rows(ids[first:first + count], lengths, starts, 16, 40, (4 << 32) + 8))
    with pytest.raises(ValueError):
        D.epoch_plan(n, 0, epoch=0)
