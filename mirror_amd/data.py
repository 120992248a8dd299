"""On-device data feed for the pre-training step: the work of `TCGAWSIRNAPretrainDataset.__getitem__`
(datasets/dataset_pretrain.py:150-167) for a whole batch, without a host round trip.

The reference loads one slide's patch features [n_i, F] per item, draws `num_wsi_feature_tokens` row indices with
`np.random.choice(n_i, N, replace=n_i < N)` (:157-161), gathers them (:162) and looks the RNA vector up by slide id
(:164-166).  Here every slide of the split sits in ONE HBM bank ([sum n_i, F], 288 GB is room for thousands of slides in
bf16), the index draw runs on the device (a random permutation prefix when the slide is long enough, i.i.d. uniform
draws — i.e. sampling WITH replacement — when it is short: the two branches of :157) and the gather is one HIP kernel
launch per batch (mh_gather_rows, HBM bound: N * F * 2 bytes per sample).

`DeviceSlideBank.sample` / `batch_sampled` / `epoch` are the same feed on the library's own Philox stream: the index draw of a whole batch
is ONE launch (mh_sample_rows) that reads the slide ids and lengths on the device, so it can be captured in a graph and restated from
(seed, draw id) on the host.  With a `targets` table the bank also serves the downstream datasets (dataset_subtyping.py:187-200: label;
dataset_survival.py:293-314: disc_label, event_time, censorship), and `ClassBalancedSampler` is `utils/loader.py:15-26`
(train_survival.py:948-949 --weighted-sampler) on the same stream.
"""
from __future__ import annotations

from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import kernels as K
from .kernels import MirrorHipError


def sample_indices(n: int, num_tokens: int, generator: Optional[torch.Generator] = None, device="cpu") -> torch.Tensor:
    """The index draw of dataset_pretrain.py:157-161 for one slide: without replacement when n >= num_tokens (a uniformly
    random ordered subset), with replacement otherwise."""
    if n <= 0:
        raise ValueError("a slide needs at least one patch")
    if n >= num_tokens:
        return torch.randperm(n, generator=generator, device=device)[:num_tokens]
    return torch.randint(0, n, (num_tokens,), generator=generator, device=device)


class DeviceSlideBank:
    """All slides of a split resident in HBM + the RNA table; `batch(ids)` returns what a DataLoader over the reference
    dataset would collate: (wsi [B, N, F], rna [B, G] float32)."""

    def __init__(self, slides: Sequence[torch.Tensor], rna: torch.Tensor, num_wsi_feature_tokens: int, device="cuda",
                 dtype: Optional[torch.dtype] = None, targets: Optional[Dict[str, torch.Tensor]] = None):
        if len(slides) == 0 or len(slides) != rna.shape[0]:
            raise ValueError("need one RNA row per slide")
        for name, t in (targets or {}).items():
            if t.dim() < 1 or t.shape[0] != len(slides):
                raise ValueError(f"target table {name!r} needs one row per slide")
        Fd = slides[0].shape[1]
        for sl in slides:
            if sl.dim() != 2 or sl.shape[1] != Fd or sl.shape[0] == 0:
                raise ValueError("every slide must be a non-empty [n_i, F] tensor with the same F")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise MirrorHipError("DeviceSlideBank lives in MI355X HBM (no CPU path); use the reference dataset on the host")
        dtype = dtype or slides[0].dtype
        self.num_tokens = int(num_wsi_feature_tokens)
        self.lengths = torch.tensor([int(sl.shape[0]) for sl in slides], dtype=torch.int64)
        self.offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(self.lengths, 0)[:-1]])
        self.bank = torch.cat([sl.to(dtype) for sl in slides], dim=0).to(dev).contiguous()
        self.rna = rna.to(dev, torch.float32).contiguous()
        self.device = dev
        if int(self.lengths.max()) >= 1 << 31:
            raise MirrorHipError("DeviceSlideBank: a slide of 2^31 rows or more is beyond the device draw's 31-bit row index")
        # the tables mh_sample_rows reads, and the per-slide targets of the downstream datasets (label / disc_label, event_time, censorship)
        self.lengths_dev = self.lengths.to(dev)
        self.offsets_dev = self.offsets.to(dev)
        self.targets = {name: t.to(dev).contiguous() for name, t in (targets or {}).items()}

    def __len__(self) -> int:
        return int(self.lengths.numel())

    def draw(self, ids: Sequence[int], generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """[B, N] global row indices into the bank for the slides `ids` (device tensor)."""
        rows = [sample_indices(int(self.lengths[i]), self.num_tokens, generator, self.device) + int(self.offsets[i]) for i in ids]
        return torch.stack(rows).contiguous()

    def batch(self, ids: Sequence[int], generator: Optional[torch.Generator] = None, rows: Optional[torch.Tensor] = None):
        """`rows` ([B, N] global indices, e.g. from the oracle's draw) overrides the device draw — parity tests."""
        if rows is None:
            rows = self.draw(ids, generator)
        rows = rows.to(self.device, torch.int64).contiguous()
        wsi = K.gather_rows(self.bank, rows)
        idx = torch.as_tensor(list(ids), device=self.device, dtype=torch.int64)
        return wsi, K.gather_rows(self.rna, idx)

    def _ids(self, ids) -> torch.Tensor:
        if isinstance(ids, torch.Tensor):
            if not ids.is_cuda:
                raise MirrorHipError("DeviceSlideBank: slide ids are a sequence of ints or a device int64 tensor (no CPU path)")
            if ids.dtype != torch.int64 or ids.dim() != 1:
                raise MirrorHipError(f"DeviceSlideBank: device slide ids must be 1-d int64, got {tuple(ids.shape)} {ids.dtype}")
            return ids.contiguous()
        return torch.as_tensor([int(i) for i in ids], device=self.device, dtype=torch.int64)

    def sample(self, ids, *, seed: int, offset: int = 0, dev_base: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[B, N] global row indices for the slides `ids` in ONE launch (mh_sample_rows): slot b uses draw id offset + *dev_base + b
        under `seed`.  With a device tensor for `ids` nothing touches the host, and the call can be captured in a graph (after one call
        outside a capture: the first launch of a process opts the kernel in to its 128 KiB of LDS)."""
        return K.sample_rows(self._ids(ids), self.lengths_dev, self.offsets_dev, self.num_tokens, seed, offset, dev_base)

    def batch_sampled(self, ids, *, seed: int, offset: int = 0, dev_base: Optional[torch.Tensor] = None):
        """(wsi [B, N, F], rna [B, G]) — and, for a bank with targets, a dict of the target rows of `ids` — on the device draw."""
        idx = self._ids(ids)
        rows = K.sample_rows(idx, self.lengths_dev, self.offsets_dev, self.num_tokens, seed, offset, dev_base)
        wsi, rna = K.gather_rows(self.bank, rows), K.gather_rows(self.rna, idx)
        if not self.targets:
            return wsi, rna
        return wsi, rna, {name: t.index_select(0, idx) for name, t in self.targets.items()}

    def epoch(self, batch_size: int, *, epoch: int, seed: int, sampler: Optional["ClassBalancedSampler"] = None, shuffle: bool = True,
              drop_last: bool = False, start_batch: int = 0) -> Iterator:
        """`batch_sampled` results over one epoch of slide ids.  The ids are the sampler's single draw of len(bank) ids (draw id `epoch`
        under the sampler's seed), or a host permutation seeded by seed + epoch (`shuffle`), or range(len(bank)); the batch whose first
        slot is k draws its tokens with draw ids (epoch << 32) + k + b under `seed`.  Everything follows from (seed, epoch, batch
        index): `start_batch` resumes an interrupted epoch with the batches it would have seen."""
        if sampler is not None:
            ids = sampler.draw(len(self), offset=int(epoch))
        else:
            ids = torch.as_tensor(epoch_ids(len(self), epoch=epoch, seed=seed, shuffle=shuffle), device=self.device, dtype=torch.int64)
        for first, count, offset in epoch_plan(len(self), batch_size, epoch=epoch, drop_last=drop_last)[int(start_batch):]:
            yield self.batch_sampled(ids[first:first + count], seed=seed, offset=offset)


def epoch_ids(n: int, *, epoch: int, seed: int, shuffle: bool = True) -> List[int]:
    """The slide ids of one epoch without a sampler: torch.randperm(n) under seed + epoch, or 0 .. n - 1."""
    if not shuffle:
        return list(range(n))
    return torch.randperm(n, generator=torch.Generator().manual_seed(int(seed) + int(epoch))).tolist()


def epoch_plan(n: int, batch_size: int, *, epoch: int, drop_last: bool = False) -> List[Tuple[int, int, int]]:
    """(first slot, slots, token draw offset) of every batch of an epoch of n ids: offset = (epoch << 32) + first slot."""
    if batch_size <= 0 or not 0 <= int(epoch) < 1 << 30 or n >= 1 << 32:
        raise ValueError("epoch_plan: batch_size >= 1, 0 <= epoch < 2^30, fewer than 2^32 ids")
    plan = []
    for first in range(0, n, batch_size):
        count = min(batch_size, n - first)
        if count == batch_size or not drop_last:
            plan.append((first, count, (int(epoch) << 32) + first))
    return plan


def balanced_weights(labels) -> np.ndarray:
    """`make_weights_for_balanced_classes` of utils/loader.py:16-23: len / count[label] per sample, f64."""
    labels = np.asarray(torch.as_tensor(labels).cpu().numpy(), dtype=np.int64).reshape(-1)
    if labels.size == 0 or labels.min() < 0:
        raise ValueError("balanced_weights: need at least one label, none negative")
    counts = np.bincount(labels)
    return float(labels.size) / counts[labels].astype(np.float64)


class ClassBalancedSampler:
    """`class_balanced_sampler(dataset)` of utils/loader.py:15-26 — WeightedRandomSampler(len / count[label], len(dataset)), with
    replacement — as one launch on the library's stream (mh_sample_weighted).  The cdf (cumsum / sum, f64) is built once on the host;
    `draw(count, offset)` returns `count` device ids for draw id offset + *dev_base under `seed`.  torch's sampler draws other values
    from the same distribution."""

    def __init__(self, labels, *, device, seed: int):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise MirrorHipError("ClassBalancedSampler draws on an MI355X device (no CPU path); use utils/loader.py on the host")
        self.weights = balanced_weights(labels)
        csum = np.cumsum(self.weights)
        self.cdf = torch.from_numpy(csum / csum[-1]).to(dev)
        self.device, self.seed = dev, int(seed)

    def __len__(self) -> int:
        return int(self.weights.size)

    def draw(self, count: int, offset: int = 0, dev_base: Optional[torch.Tensor] = None) -> torch.Tensor:
        return K.sample_weighted(self.cdf, count, self.seed, offset, dev_base)


class HostFeeder:
    """Pipelined host -> HBM hand-off of DataLoader batches: what `train_mirror.py:1138-1139` does synchronously
    (`wsi_features.to(device)`, `rna_features.to(device)` at the top of every step) moved onto a copy stream, double
    buffered, so that batch k + 1 crosses PCIe (B * N * F * 4 bytes as f32: 268 MB at c2, ~5 ms at PCIe Gen5 rates; half that
    when the loader already holds bf16) while the GPU runs step k.

        feeder = HostFeeder(loader, device, wsi_dtype=torch.bfloat16)
        for wsi, rna in feeder:          # device tensors; valid until the NEXT iteration step
            engine.step(wsi, rna)

    Three slots by default (a slot is reused when the step that read it lies two steps back: the host-side wait for it never blocks).
    Host batches are staged in pinned buffers (allocated once, sized by the first batch); the f32 -> bf16 cast, when asked for,
    happens on the device on the copy stream (a host-side cast would cost more CPU time than the copy saves).  The consumer
    stream waits on an event, never on the host."""

    def __init__(self, loader, device, wsi_dtype: Optional[torch.dtype] = None, depth: int = 3):
        self.loader, self.device, self.wsi_dtype = loader, torch.device(device), wsi_dtype
        if self.device.type != "cuda":
            raise MirrorHipError("HostFeeder feeds an MI355X device")
        self.depth = max(3, int(depth))       # slots; batches in flight ahead of the consumer = depth - 2 (see _issue: the slot that is
                                              # refilled was last read TWO steps back, so the host-side wait for it does not block)
        self.stream = torch.cuda.Stream(device=self.device)
        self._slots = []          # per slot: (pinned wsi, pinned rna, device wsi raw, device wsi, device rna, ready event, free event)
        self._k = 0               # running slot counter: NOT reset per epoch, so two consecutive batches never share a slot

    def _slot(self, k: int, wsi: torch.Tensor, rna: torch.Tensor):
        while len(self._slots) <= k:
            self._slots.append(None)
        sl = self._slots[k]
        if sl is None or sl[0].shape != wsi.shape or sl[0].dtype != wsi.dtype or sl[1].shape != rna.shape:
            pw = torch.empty(wsi.shape, dtype=wsi.dtype, pin_memory=True)
            pr = torch.empty(rna.shape, dtype=torch.float32, pin_memory=True)
            # the slot's device buffers are first written on the copy stream: allocate them there (after the copy stream has
            # caught up with the consumer's stream), so that a block the caching allocator just took back from the consumer's
            # stream with kernels still pending cannot be handed out and overwritten
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(self.stream):
                dw_raw = torch.empty(wsi.shape, dtype=wsi.dtype, device=self.device)
                dw = dw_raw if self.wsi_dtype in (None, wsi.dtype) else torch.empty(wsi.shape, dtype=self.wsi_dtype, device=self.device)
                dr = torch.empty(rna.shape, dtype=torch.float32, device=self.device)
            sl = self._slots[k] = [pw, pr, dw_raw, dw, dr, torch.cuda.Event(), None, False]
        return sl

    def _issue(self, k: int, batch):
        wsi, rna = batch[0], batch[1]
        sl = self._slot(k, wsi, rna)
        pw, pr, dw_raw, dw, dr, ready, free, used = sl
        if used:
            ready.synchronize()                   # the slot's previous host -> device copy has left the pinned buffer (depth steps ago)
        if free is not None:
            # the step that consumed this slot's device tensors has finished: waited for on the HOST.  With three slots that step lies two
            # steps back and the wait never blocks — and the copy stream must not carry a device-side wait: on this platform ANY
            # hipStreamWaitEvent on the stream that issues the pinned -> device copy (even on an event that completed long ago) takes the
            # copy out from under the replayed step, which then runs one whole PCIe transfer late (measured, tools/exp/h2d_overlap3.py:
            # replay 7.81 ms; + copy behind a host wait 8.12; + copy behind a stream wait on the same, complete, event 9.52; behind the
            # previous replay's event 10.24 — rounds 2-4 reported 22-37 % for --feed host-bf16 / host without finding this)
            free.synchronize()
        sl[7] = True
        # a pinned batch (DataLoader(pin_memory=True), what train_mirror.py builds with --pin-mem) goes to the device as it is;
        # a pageable one is staged through the slot's pinned buffer first (one host memcpy: ~10 GB/s on one core, i.e. the
        # bottleneck for 268 MB batches — pin in the loader's workers)
        src_w = wsi if wsi.is_pinned() else pw.copy_(wsi)
        src_r = rna if (rna.is_pinned() and rna.dtype == torch.float32) else pr.copy_(rna)
        with torch.cuda.stream(self.stream):
            dw_raw.copy_(src_w, non_blocking=True)
            dr.copy_(src_r, non_blocking=True)
            if dw is not dw_raw:
                K.cast(dw_raw, self.wsi_dtype, out=dw)
                # the raw kernel wrote through a pointer: tell torch the tensor changed (TrainEngine.step's graph replay skips the
                # copy into its static input when it sees the same tensor object at the same version)
                torch.autograd.graph.increment_version(dw)
            ready.record(self.stream)
        return sl

    def __iter__(self):
        it = iter(self.loader)
        pending = []
        k = self._k
        for _ in range(self.depth - 2):
            try:
                pending.append(self._issue(k % self.depth, next(it)))
                k += 1
            except StopIteration:
                break
        while pending:
            sl = pending.pop(0)
            try:                                   # request batch k + 1 before handing batch k to the consumer
                pending.append(self._issue(k % self.depth, next(it)))
                k += 1
            except StopIteration:
                pass
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(sl[5])
            try:
                yield sl[3], sl[4]
            finally:
                # also when the consumer breaks out of its loop (the generator is closed at the yield): the slot's next
                # user must wait for everything queued on this batch, and the slot counter must keep running
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))
                sl[6] = ev
                self._k = k
