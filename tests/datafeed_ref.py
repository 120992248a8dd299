"""Host reference of the data feed draws (mh_sample_rows, mh_sample_weighted), for the bit-exact tests (test_datafeed_cpu.py / _gpu.py).

Written from the text of include/mirror_hip.h ("Data feed draws"); numpy integers only, Philox from tests/philox_ref.py; shares no code
with mirror_amd.

    counter = (lo32(blk), kind, lo32(draw), 0x80000000 | hi32(draw))     key = (lo32(seed), hi32(seed)), 10 rounds
    kind = 0 token draws, 1 slide-id draws; element e of a draw = word e & 3 of block e >> 2
"""
import numpy as np

from tests.philox_ref import philox4x32

KIND_ROWS, KIND_IDS = 0, 1


def draw_words(n, kind, draw, seed):
    """uint64 [n] (32-bit values): elements 0 .. n - 1 of draw `draw`."""
    draw, seed = int(draw), int(seed)
    assert 0 <= draw < 1 << 63 and n >= 0
    blks = np.arange((n + 3) // 4, dtype=np.uint64)
    w = philox4x32((blks, kind, draw & 0xFFFFFFFF, 0x80000000 | (draw >> 32)), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), 10)
    return w.T.reshape(-1)[:n]                  # [blocks, 4] flattened: element e = word e & 3 of block e >> 2


def sample_local(n, N, seed, draw):
    """int64 [N]: the slide-local row indices of one slot (a slide of n >= 1 rows), as the header defines them."""
    n, N = int(n), int(N)
    assert 1 <= n < 1 << 31
    if n < N:                                   # with replacement: multiply-shift of one word per row
        return ((draw_words(N, KIND_ROWS, draw, seed) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    keys = (draw_words(n, KIND_ROWS, draw, seed) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    keys.sort()                                 # distinct: the index is part of the key
    return (keys[:N] & np.uint64(0xFFFFFFFF)).astype(np.int64)


def sample_rows(slot_slide, lengths, starts, N, seed, offset, base=None):
    """int64 [B, N]: mh_sample_rows.  Slot b uses draw = offset + base + b; a slide id outside [0, S) gives -1 in every row, a length
    <= 0 or >= 2^31 gives starts[sl] in every row."""
    first = int(offset) + (int(base) if base is not None else 0)
    out = np.empty((len(slot_slide), N), dtype=np.int64)
    for b, sl in enumerate(int(x) for x in slot_slide):
        if not 0 <= sl < len(lengths):
            out[b] = -1
        elif not 0 < int(lengths[sl]) < 1 << 31:
            out[b] = int(starts[sl])
        else:
            out[b] = int(starts[sl]) + sample_local(lengths[sl], N, seed, first + b)
    return out


def uniforms53(count, seed, draw):
    """float64 [count]: u_i = (((w_{2i} >> 5) << 26) | (w_{2i+1} >> 6)) * 2^-53 of the slide-id draw `draw`."""
    w = draw_words(2 * count, KIND_IDS, draw, seed)
    bits = ((w[0::2] >> np.uint64(5)) << np.uint64(26)) | (w[1::2] >> np.uint64(6))
    return bits.astype(np.float64) * 2.0 ** -53               # bits < 2^53: the conversion and the product are exact


def sample_weighted(cdf, count, seed, offset, base=None):
    """int64 [count]: mh_sample_weighted — the number of cdf entries <= u_i, clamped to S - 1."""
    cdf = np.asarray(cdf, dtype=np.float64)
    u = uniforms53(count, seed, int(offset) + (int(base) if base is not None else 0))
    return np.minimum(np.searchsorted(cdf, u, side="right"), len(cdf) - 1).astype(np.int64)


def balanced_weights(labels):
    """utils/loader.py:17-22: len / count[label] per sample, f64."""
    labels = np.asarray(labels, dtype=np.int64)
    counts = np.bincount(labels)
    return len(labels) / counts[labels].astype(np.float64)


def cdf_of(weights):
    w = np.asarray(weights, dtype=np.float64)
    c = np.cumsum(w)
    return c / c[-1]


def epoch_offsets(n_ids, batch_size, epoch, drop_last=False):
    """[(first slot, slots, token draw offset)] of the batches of one epoch: draw ids are (epoch << 32) + first slot of the batch."""
    out = []
    for first in range(0, n_ids, batch_size):
        k = min(batch_size, n_ids - first)
        if k < batch_size and drop_last:
            break
        out.append((first, k, (int(epoch) << 32) + first))
    return out
