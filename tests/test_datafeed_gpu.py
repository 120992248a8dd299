"""GPU: mh_sample_rows / mh_sample_weighted are bit-equal to the host reference (tests/datafeed_ref.py) on every path of the kernel —
short slides (with replacement), slides sorted whole in LDS, the threshold path with and without its retries — and
DeviceSlideBank.batch_sampled / epoch / ClassBalancedSampler deliver those rows, eagerly and from a captured graph."""
import os

import numpy as np
import pytest
import torch

import mirror_amd
from mirror_amd import _lib, data as D, kernels as K
from tests import datafeed_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(x, dtype=torch.int64):
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(DEV)


def _tables(lengths):
    lengths = np.asarray(lengths, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    return lengths, starts


def _rows(slots, lengths, starts, N, seed, offset, **kw):
    return K.sample_rows(_dev(slots), _dev(lengths), _dev(starts), N, seed, offset, **kw).cpu().numpy()


# ----------------------------------------------------------------------------- K.sample_rows
def test_every_length_class_in_one_batch():
    """N = 64: below N (with replacement); N and N + 1 (sorted whole: they fit the 128-key sort that N + 8 sqrt(N) candidates need);
    200 and up on the threshold path, on both sides of the 16384 keys that LDS holds; slide 200 in two slots."""
    lengths, starts = _tables([1, 37, 63, 64, 65, 200, 16384, 16385, 20000])
    slots = [0, 1, 2, 3, 4, 5, 6, 7, 8, 5]
    got = _rows(slots, lengths, starts, 64, 1234, 5)
    assert np.array_equal(got, R.sample_rows(slots, lengths, starts, 64, 1234, 5))
    assert not np.array_equal(got[5], got[9])
    for b, sl in enumerate(slots):
        assert got[b].min() >= starts[sl] and got[b].max() < starts[sl] + lengths[sl]


# (300, 256), (8192, 8192), (16384, 8192): sorted whole at 512, 8192 and 16384 keys; the others take the threshold pass
@pytest.mark.parametrize("n,N", [(20000, 2048), (100000, 4096), (16385, 8192), (8192, 8192), (16384, 8192), (300, 256)])
def test_large_draws_match_the_reference(n, N):
    lengths, starts = _tables([3, n])
    got = _rows([1, 1], lengths, starts, N, 7, 1 << 40)
    assert np.array_equal(got, R.sample_rows([1, 1], lengths, starts, N, 7, 1 << 40))
    assert len(set(got[0].tolist())) == N


def test_offset_and_dev_base_add_up():
    lengths, starts = _tables([50, 300, 17000])
    slots = [2, 1, 0, 2]
    want = R.sample_rows(slots, lengths, starts, 128, 3, 10)
    assert np.array_equal(_rows(slots, lengths, starts, 128, 3, 10), want)
    assert np.array_equal(_rows(slots, lengths, starts, 128, 3, 4, dev_base=_dev([6])), want)
    assert np.array_equal(_rows(slots, lengths, starts, 128, 3, 0, dev_base=_dev([10])), want)
    assert not np.array_equal(_rows(slots, lengths, starts, 128, 3, 11), want)
    out = torch.empty((4, 128), dtype=torch.int64, device=DEV)
    assert K.sample_rows(_dev(slots), _dev(lengths), _dev(starts), 128, 3, 10, out=out) is out and np.array_equal(out.cpu().numpy(), want)


def test_the_threshold_retries_do_not_change_the_rows():
    """(n, N) = (20000, 2048), seed 7, draws 0 .. 15: with slack = 0 the first threshold lets fewer than N keys through in 12 of the 16
    slots (the threshold grows), with slack = 1000 it lets all 20000 through in every slot (the threshold is halved); slack = 8 needs
    neither.  The rows are the definition's in all three."""
    lengths, starts = _tables([20000])
    want = R.sample_rows([0] * 16, lengths, starts, 2048, 7, 0)
    for slack in (8.0, 0.0, 1000.0):
        assert np.array_equal(_rows([0] * 16, lengths, starts, 2048, 7, 0, slack=slack), want), slack


def test_slots_without_a_slide_and_refused_shapes():
    lengths, starts = _tables([4, 0, 9])
    slots = [-1, 3, 1, 0, 2]
    got = _rows(slots, lengths, starts, 5, 1, 0)
    assert np.array_equal(got, R.sample_rows(slots, lengths, starts, 5, 1, 0))
    assert got[0].tolist() == [-1] * 5 and got[1].tolist() == [-1] * 5 and got[2].tolist() == [4] * 5
    t = _dev([0])
    with pytest.raises(mirror_amd.MirrorHipError, match="N=8193"):
        K.sample_rows(t, _dev([9000]), t, 8193, 1, 0)
    with pytest.raises(mirror_amd.MirrorHipError, match="B=-1"):
        _lib.call("mh_sample_rows", t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), -1, 4, 1, 1, 0, None, 8.0, stream=K._stream())
    with pytest.raises(mirror_amd.MirrorHipError):
        K.sample_rows(t, _dev([9000]), t, 8, 1, 1 << 63)
    with pytest.raises(mirror_amd.MirrorHipError):
        K.sample_rows(t.int(), _dev([9000]), t, 8, 1, 0)
    assert K.sample_rows(t[:0], _dev([9000]), t, 8, 1, 0).shape == (0, 8)


# ----------------------------------------------------------------------------- K.sample_weighted
def test_weighted_ids_match_the_reference():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_sampler.npz"))
    cdf = R.cdf_of(g["weights"])
    want = R.sample_weighted(cdf, 8000, 99, 0)
    dcdf = _dev(cdf, torch.float64)
    assert np.array_equal(K.sample_weighted(dcdf, 8000, 99, 0).cpu().numpy(), want)
    assert np.array_equal(K.sample_weighted(dcdf, 7, 99, 0).cpu().numpy(), want[:7])                 # a ragged last block
    want3 = R.sample_weighted(cdf, 333, 99, 3)
    assert np.array_equal(K.sample_weighted(dcdf, 333, 99, 1, dev_base=_dev([2])).cpu().numpy(), want3)
    assert not np.array_equal(want3, want[:333])
    zero = R.cdf_of([0.0, 1.0, 0.0, 0.0, 2.0, 1.0, 0.0])
    got = K.sample_weighted(_dev(zero, torch.float64), 4000, 5, 2).cpu().numpy()
    assert np.array_equal(got, R.sample_weighted(zero, 4000, 5, 2)) and set(got.tolist()) == {1, 4, 5}
    with pytest.raises(mirror_amd.MirrorHipError):
        K.sample_weighted(dcdf.float(), 8, 1, 0)


# ----------------------------------------------------------------------------- DeviceSlideBank
LENGTHS = [1, 37, 64, 200, 16385, 20000, 90, 64]
NTOK, FEAT = 64, 8


@pytest.fixture(scope="module")
def slides():
    g = torch.Generator().manual_seed(11)
    sl = [torch.randn(n, FEAT, generator=g) for n in LENGTHS]
    rna = torch.randn(len(LENGTHS), 6, generator=g)
    targets = {"label": torch.tensor([0, 1, 1, 2, 0, 1, 1, 1]), "event_time": torch.rand(len(LENGTHS), generator=g) * 100,
               "censorship": torch.tensor([[0.0], [1.0], [0.0], [0.0], [1.0], [1.0], [0.0], [1.0]])}
    return sl, rna, targets


def _check_batch(bank, slides_cast, rna, targets, ids, seed, offset, wsi, rna_out, tg):
    starts = bank.offsets.numpy()
    rows = R.sample_rows(ids, LENGTHS, starts, NTOK, seed, offset)
    for b, sl in enumerate(ids):
        assert torch.equal(wsi[b].cpu(), slides_cast[sl][torch.from_numpy(rows[b] - starts[sl])]), (b, sl)
    assert torch.equal(rna_out.cpu(), rna[list(ids)])
    assert set(tg) == set(targets)
    for k, v in targets.items():
        assert torch.equal(tg[k].cpu(), v[list(ids)]) and tg[k].dtype == v.dtype
    return rows


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batch_sampled_gathers_the_reference_rows(slides, dtype, monkeypatch):
    sl, rna, targets = slides
    bank = D.DeviceSlideBank(sl, rna, NTOK, device=DEV, dtype=dtype, targets=targets)
    cast = [s.to(dtype) for s in sl]
    ids = [5, 0, 3, 3, 4, 1, 7]
    real, names = _lib.call, []

    def counting(name, *a, **kw):
        names.append(name)
        return real(name, *a, **kw)

    monkeypatch.setattr(_lib, "call", counting)
    wsi, rna_out, tg = bank.batch_sampled(ids, seed=21, offset=100)
    assert names.count("mh_sample_rows") == 1 and sorted(names) == ["mh_gather_rows", "mh_gather_rows", "mh_sample_rows"]
    monkeypatch.setattr(_lib, "call", real)
    assert wsi.dtype == dtype and tuple(wsi.shape) == (len(ids), NTOK, FEAT)
    rows = _check_batch(bank, cast, rna, targets, ids, 21, 100, wsi, rna_out, tg)
    assert np.array_equal(bank.sample(_dev(ids), seed=21, offset=100).cpu().numpy(), rows)           # device ids: the same draw
    plain = D.DeviceSlideBank(sl, rna, NTOK, device=DEV, dtype=dtype)
    out = plain.batch_sampled(_dev(ids), seed=21, offset=100)
    assert len(out) == 2 and torch.equal(out[0], wsi) and torch.equal(out[1], rna_out)
    with pytest.raises(mirror_amd.MirrorHipError):
        bank.sample(torch.tensor(ids), seed=21)


def test_batch_sampled_in_a_captured_graph_draws_fresh_rows_per_replay(slides):
    sl, rna, targets = slides
    bank = D.DeviceSlideBank(sl, rna, NTOK, device=DEV, targets=targets)
    ids = [4, 3, 5, 3]
    dids, base = _dev(ids), _dev([0])
    bank.batch_sampled(dids, seed=5, offset=1000, dev_base=base)            # the kernels' one-time set-up happens outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rows = bank.sample(dids, seed=5, offset=1000, dev_base=base)
        wsi, rna_out, tg = bank.batch_sampled(dids, seed=5, offset=1000, dev_base=base)
    seen = []
    for step in (3, 4):
        base.fill_(step * len(ids))
        graph.replay()
        torch.cuda.synchronize()
        want = _check_batch(bank, sl, rna, targets, ids, 5, 1000 + step * len(ids), wsi, rna_out, tg)
        assert np.array_equal(rows.cpu().numpy(), want)
        seen.append(want)
    assert not np.array_equal(seen[0], seen[1])


def test_an_epoch_under_the_balanced_sampler(slides):
    sl, rna, targets = slides
    bank = D.DeviceSlideBank(sl, rna, NTOK, device=DEV, targets=targets)
    labels = targets["label"]
    sampler = D.ClassBalancedSampler(labels, device=DEV, seed=77)
    assert np.array_equal(sampler.weights, R.balanced_weights(labels.numpy())) and len(sampler) == len(bank)
    cdf = sampler.cdf.cpu().numpy()
    assert np.array_equal(cdf, R.cdf_of(sampler.weights))
    ids = R.sample_weighted(cdf, len(bank), 77, 2).tolist()
    batches = list(bank.epoch(3, epoch=2, seed=9, sampler=sampler))
    plan = R.epoch_offsets(len(bank), 3, 2)
    assert len(batches) == len(plan) == 3 and sum(b[0].shape[0] for b in batches) == len(bank)
    for (first, count, offset), (wsi, rna_out, tg) in zip(plan, batches):
        _check_batch(bank, sl, rna, targets, ids[first:first + count], 9, offset, wsi, rna_out, tg)
    # resumed at batch 1, and without a sampler: the host permutation under seed + epoch
    resumed = list(bank.epoch(3, epoch=2, seed=9, sampler=sampler, start_batch=1))
    assert len(resumed) == 2 and all(torch.equal(a[0], b[0]) for a, b in zip(resumed, batches[1:]))
    perm = D.epoch_ids(len(bank), epoch=2, seed=9)
    got = list(bank.epoch(3, epoch=2, seed=9, drop_last=True))
    assert len(got) == 2
    for (first, count, offset), (wsi, rna_out, tg) in zip(R.epoch_offsets(len(bank), 3, 2, True), got):
        _check_batch(bank, sl, rna, targets, perm[first:first + count], 9, offset, wsi, rna_out, tg)
