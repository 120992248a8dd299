"""Host reference of the library's two random streams, for the bit-exact tests (test_random_streams_cpu.py / _gpu.py).

Written from the published definition of Philox4x32 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
SC'11, and the Random123 known-answer vectors) and from the addressing rules that include/mirror_hip.h states for mh_dropout,
mh_dropout_lite and mh_noise_draws.  numpy integers only; shares no code with mirror_amd.

One round of Philox4x32 on the counter (c0, c1, c2, c3) under the key (k0, k1):

    hi0:lo0 = M0 * c0        hi1:lo1 = M1 * c2        (32 x 32 -> 64 bit products, M0 = 0xD2511F53, M1 = 0xCD9E8D57)
    (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)

and the key is bumped by the Weyl constants (W0, W1) = (0x9E3779B9, 0xBB67AE85) between rounds (not after the last).
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(ctr4, key2, rounds):
    """ctr4: four integers or integer arrays (32 bit each, broadcast against each other), key2: two integers.  Returns the four
    output words as a uint64 array [4, ...] holding 32-bit values."""
    c = [np.asarray(x, dtype=np.uint64) & _LO for x in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in ctr4])]
    k0, k1 = int(key2[0]) & 0xFFFFFFFF, int(key2[1]) & 0xFFFFFFFF
    for _ in range(rounds):
        p0 = np.uint64(M0) * c[0]              # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c)


def _blocks(first_elem, n, per_block, seed, rounds):
    """Words [4, n_blocks] of the blocks that elements first_elem .. first_elem + n - 1 address, and each element's (block index
    into that array, position inside its block).  Counter = (lo32(blk), hi32(blk), 0, 0), key = (lo32(seed), hi32(seed))."""
    sh = per_block.bit_length() - 1
    blk0, blk1 = first_elem >> sh, (first_elem + n - 1) >> sh
    blks = [blk0 + j for j in range(blk1 - blk0 + 1)]         # Python integers: no 64-bit wrap-around on the way
    lo = np.array([b & 0xFFFFFFFF for b in blks], dtype=np.uint64)
    hi = np.array([(b >> 32) & 0xFFFFFFFF for b in blks], dtype=np.uint64)
    w = philox4x32((lo, hi, 0, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), rounds)
    e = np.array([first_elem + i - (blk0 << sh) for i in range(n)], dtype=np.int64)
    return w, e >> sh, e & (per_block - 1)


def stream_words(n, seed, offset, base=None):
    """The 32-bit word of each of n elements of the 10-round stream: element i = word (i & 3) of block (offset + (base & ~3) + i) >> 2."""
    first = int(offset) + ((int(base) & ~3) if base is not None else 0)
    w, b, pos = _blocks(first, n, 4, int(seed), 10)
    return w[pos, b]


def dropout_mult(n, p, seed, offset, base=None):
    """f32 [n]: the multiplier mh_dropout applies to element i — 0, or float32(1) / (float32(1) - float32(p)) where the element's
    word >= floor(float32(p) * 2^32)."""
    p32 = np.float32(p)
    thr = int(float(p32) * 4294967296.0)                      # exact: a float32 times a power of two, in double
    scale = np.float32(1.0) / (np.float32(1.0) - p32)
    return np.where(stream_words(n, seed, offset, base) >= np.uint64(thr), scale, np.float32(0.0)).astype(np.float32)


def lite_thr16(p):
    """min(floor(float32(p) * 65536 + 0.5), 65535): the 16-bit threshold of the lite stream."""
    return min(int(float(np.float32(p)) * 65536.0 + 0.5), 65535)


def lite_fields(n, seed, offset, base=None):
    """The 16-bit field of each of n elements of the lite stream: 7 rounds, element i = field (i & 7) of block
    (offset + (base & ~7) + i) >> 3; field f = the low half of word f >> 1 for even f, the high half for odd f."""
    first = int(offset) + ((int(base) & ~7) if base is not None else 0)
    w, b, f = _blocks(first, n, 8, int(seed), 7)
    word = w[f >> 1, b]
    return np.where(f & 1, word >> np.uint64(16), word & np.uint64(0xFFFF))


def lite_mult(n, p, seed, offset, base=None):
    """f32 [n]: the multiplier of mh_dropout_lite — 0, or float32(65536) / float32(65536 - thr16) where field >= thr16."""
    thr = lite_thr16(p)
    scale = np.float32(65536.0) / np.float32(65536 - thr)
    return np.where(lite_fields(n, seed, offset, base) >= np.uint64(thr), scale, np.float32(0.0)).astype(np.float32)


def box_muller(w0, w1, dtype=np.float64):
    """The normal pair of the word pair (w0, w1) as noise_draws_kernel documents it: u1 = ((w0 >> 8) + 1) * 2^-24 in (0, 1],
    u2 = (w1 >> 8) * 2^-24, r = sqrt(-2 ln u1), pair = (r cos(2 pi u2), r sin(2 pi u2)); evaluated in `dtype`."""
    t = dtype
    u1 = ((np.asarray(w0, dtype=np.uint64) >> np.uint64(8)).astype(t) + t(1.0)) * t(2.0 ** -24)
    u2 = (np.asarray(w1, dtype=np.uint64) >> np.uint64(8)).astype(t) * t(2.0 ** -24)
    r = np.sqrt(t(-2.0) * np.log(u1))
    a = t(6.283185307179586) * u2
    return r * np.cos(a), r * np.sin(a)


def noise(n_uniform, n_normal, seed, offset, base=None, dtype=np.float64):
    """float64 [n_uniform + n_normal]: the buffer of mh_noise_draws.  Elements below n_uniform (a multiple of 4) are (word >> 8) * 2^-24;
    behind them every block yields two Box-Muller pairs, from the words (0, 1) and (2, 3): elements 4 q + 2 h, 4 q + 2 h + 1 =
    r cos, r sin.  A ragged tail keeps the leading elements of its block."""
    assert n_uniform % 4 == 0
    n = n_uniform + n_normal
    w = stream_words((n + 3) // 4 * 4, seed, offset, base)
    out = np.empty(w.shape[0], dtype=dtype)
    out[:n_uniform] = (w[:n_uniform] >> np.uint64(8)).astype(dtype) * dtype(2.0 ** -24)
    z0, z1 = box_muller(w[n_uniform::2], w[n_uniform + 1::2], dtype)
    out[n_uniform::2], out[n_uniform + 1::2] = z0, z1
    return out[:n]
