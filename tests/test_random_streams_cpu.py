"""No GPU: the host reference of the Philox streams (tests/philox_ref.py) against the Random123 known-answer vectors and the
project's block addressing, and the host bookkeeping that places the noise draws of consecutive forwards (functional.noise_draws /
noise_draws_advance / manual_seed)."""
import numpy as np
import pytest
import torch

from tests import philox_ref as R


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


# counter, key, 10 rounds, 7 rounds: the Random123 known-answer vectors (kat_vectors: philox4x32), recomputed independently
KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8", "5f6fb709 0d893f64 4f121f81 4f730a48"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd", "5207ddc2 45165e59 4d8ee751 8c52f662"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1", "4dfccaba 190a87f0 c47362ba b6b5242a"),
]


@pytest.mark.parametrize("ctr,key,want10,want7", KAT)
def test_reference_reproduces_the_random123_known_answers(ctr, key, want10, want7):
    assert _hex(R.philox4x32(ctr, key, 10)) == want10
    assert _hex(R.philox4x32(ctr, key, 7)) == want7


# block, 10 rounds, 7 rounds under seed 123: counter = (lo32(blk), hi32(blk), 0, 0), key = (lo32(seed), hi32(seed))
ADDR = [
    (0, "11237cdc 66ff3dd8 bfb09d90 30db7e52", "08548447 64b4c7b7 3dab4ced ae350c71"),
    (1 << 42, "d009ccde e9e73ceb 53df3eb7 b7335ea8", "d74ed6e8 acf9369d 3cf14971 add4393c"),
]


@pytest.mark.parametrize("blk,want10,want7", ADDR)
def test_project_addressing_of_a_block(blk, want10, want7):
    """Element 4 blk + e of the 10-round stream is word e of block blk; element 8 blk + f of the lite stream is the low / high half
    of word f >> 1.  Block 2^42 is where the noise range starts (offset 2^44): its high counter word is 2^10."""
    assert _hex(R.stream_words(4, 123, 4 * blk)) == want10
    assert _hex(R.philox4x32((blk & 0xFFFFFFFF, blk >> 32, 0, 0), (123, 0), 10)) == want10
    w7 = [int(x, 16) for x in want7.split()]
    fields = [(w7[f >> 1] >> 16) if f & 1 else (w7[f >> 1] & 0xFFFF) for f in range(8)]
    assert [int(v) for v in R.lite_fields(8, 123, 8 * blk)] == fields
    # an unaligned start and a base whose low bits the kernels mask away address the same blocks
    assert _hex(R.stream_words(3, 123, 4 * blk, base=3)) == " ".join(want10.split()[:3])
    assert _hex(R.stream_words(2, 123, 4 * blk - 4, base=6)[:2]) == " ".join(want10.split()[:2])
    assert [int(v) for v in R.lite_fields(8, 123, 8 * blk - 8, base=13)] == fields


def test_high_key_word_and_thresholds():
    a, b = R.stream_words(8, 5, 0), R.stream_words(8, (1 << 32) + 5, 0)
    assert not np.array_equal(a, b)
    assert _hex(b[:4]) == _hex(R.philox4x32((0, 0, 0, 0), (5, 1), 10))
    assert [R.lite_thr16(p) for p in (0.0, 0.1, 0.5 / 65536, 1.5 / 65536, 0.999995)] == [0, 6554, 1, 2, 65535]
    m = R.lite_mult(4096, 0.999995, 123, 0)
    assert set(np.unique(m)) <= {np.float32(0.0), np.float32(65536.0)}
    assert (R.lite_mult(64, 0.0, 123, 0) == np.float32(1.0)).all()
    d = R.dropout_mult(4096, 0.5, 123, 0)
    assert set(np.unique(d)) == {np.float32(0.0), np.float32(2.0)} and abs(float((d > 0).mean()) - 0.5) < 0.05


def test_noise_reference_layout():
    """Uniforms are k / 2^24; the normals of a block are (r0 cos, r0 sin, r1 cos, r1 sin) of its word pairs; a ragged tail is a prefix."""
    w = R.stream_words(16, 9, 1 << 44)
    z = R.noise(8, 8, 9, 1 << 44)
    assert np.array_equal(z[:8], (w[:8] >> np.uint64(8)).astype(np.float64) / 2.0 ** 24)
    u1 = (float(int(w[10]) >> 8) + 1.0) / 2.0 ** 24
    u2 = float(int(w[11]) >> 8) / 2.0 ** 24
    r = (-2.0 * np.log(u1)) ** 0.5
    assert abs(z[10] - r * np.cos(2 * np.pi * u2)) < 1e-12 and abs(z[11] - r * np.sin(2 * np.pi * u2)) < 1e-12
    assert np.array_equal(R.noise(8, 6, 9, 1 << 44), z[:14]) and np.array_equal(R.noise(8, 1, 9, 1 << 44), z[:9])
    # u1 = (k + 1) * 2^-24: the all-zero word is finite, the all-one word gives r = 0
    z0, z1 = R.box_muller(np.array([0, 0xFFFFFFFF]), np.array([0, 0]))
    assert np.isfinite(z0).all() and abs(z0[0] - (2 * 24 * np.log(2.0)) ** 0.5) < 1e-12 and z0[1] == 0.0 and (z1 == 0.0).all()


# ------------------------------------------------------------------------------------------ host bookkeeping of the noise range
@pytest.fixture
def noise_log(monkeypatch):
    """functional's stream state saved and restored; K.noise_draws replaced by a recorder of (n_uniform, n_normal, seed, offset, base)."""
    from mirror_amd import functional as Fn
    saved = dict(Fn._dropout_state)
    calls = []

    def fake(n_uniform, n_normal, seed, offset, dev_base, device):
        calls.append((n_uniform, n_normal, seed, offset, dev_base))
        return torch.zeros(n_uniform + n_normal)
    monkeypatch.setattr(Fn.K, "noise_draws", fake)
    Fn._dropout_state["base"] = None
    yield Fn, calls
    Fn._dropout_state.clear()
    Fn._dropout_state.update(saved)


def _bare_forward(Fn, dropout_elems, B=3, N=10, D=7, L=5):
    """What MIRROR.forward does to the stream state outside an engine: the draws, its dropout sites, the advance."""
    Fn.noise_draws(B, N, D, L, "cpu")
    Fn._dropout_state["offset"] += dropout_elems
    Fn.noise_draws_advance()


def _blocks4(call):
    nu, nn, _, off, _ = call
    return set(range(off >> 2, (off + nu + nn + 3) >> 2))


@pytest.mark.parametrize("dropout_elems", [0, 4, 1001])
def test_successive_bare_forwards_draw_at_disjoint_offsets(noise_log, dropout_elems):
    Fn, calls = noise_log
    Fn.manual_seed(11)
    for _ in range(4):
        _bare_forward(Fn, dropout_elems)
    assert len(calls) == 4 and all(c[2] == 11 and c[3] % 4 == 0 and c[3] >= Fn._NOISE_OFFSET for c in calls)
    seen = set()
    for c in calls:
        assert c[0] + c[1] == 32 + 24 + 30
        assert not (seen & _blocks4(c)), [x[3] - Fn._NOISE_OFFSET for x in calls]
        seen |= _blocks4(c)
    # the dropout range of a forward never reaches the noise range, and the noise offsets grow
    assert [c[3] for c in calls] == sorted(c[3] for c in calls)


def test_noise_draws_advance_moves_past_the_draws(noise_log):
    Fn, calls = noise_log
    Fn.manual_seed(3)
    Fn._dropout_state["offset"] = 6
    Fn.noise_draws(3, 10, 7, 5, "cpu")
    assert Fn._dropout_state["offset"] == 6 and calls[0][3] == Fn._NOISE_OFFSET + 8
    Fn.noise_draws_advance()
    assert Fn._dropout_state["offset"] == 96                # the draws start at 8 and are 32 + 24 + 30 = 86 elements: their end, 94, rounded up to 8 (one block past 6 is only 16)
    # inside an engine step the host offset is 0 when the draws are issued: the launch's offset is the constant a captured step bakes in
    Fn.dropout_step_begin("cpu")
    Fn.noise_draws(3, 10, 7, 5, "cpu")
    assert calls[1][3] == Fn._NOISE_OFFSET and calls[1][4] is Fn._dropout_state["base"]
    Fn.noise_draws_advance()
    base, used = Fn.dropout_step_take()
    assert used == 88 and used >= calls[1][0] + calls[1][1]


def test_a_forward_that_consumed_more_dropout_than_noise_ends_one_block_behind_its_sites(noise_log):
    """86 noise elements from offset 0 end at 88; dropout sites that ran to 1001 put the end of the forward at the next lite block
    (1008) plus one, dropout sites that ran to 40 leave it at 88: the larger of the two, never a flat 8 past a short forward."""
    Fn, _ = noise_log
    for sites, want in ((1001, 1016), (40, 88), (88, 96), (0, 88)):
        Fn.manual_seed(3)
        _bare_forward(Fn, sites)
        assert Fn._dropout_state["offset"] == want and Fn._dropout_state["noise"] == 0, sites
    Fn.noise_draws_advance()                 # without draws in front of it: one block on, as before
    assert Fn._dropout_state["offset"] == 96


def test_step_consumption_is_handed_over_in_whole_lite_blocks(noise_log):
    """The kernels mask the device base with ~7 on the lite stream: a step that consumed 12 elements hands over 16, or the next step's
    first lite block would be this step's last."""
    Fn, _ = noise_log
    Fn.dropout_step_begin("cpu")
    Fn._dropout_state["offset"] = 12
    assert Fn.dropout_step_take()[1] == 16
    Fn._dropout_state["offset"] = 12
    Fn.dropout_step_end()
    assert int(Fn._dropout_state["base"]) == 16 and Fn._dropout_state["offset"] == 0


def test_manual_seed_makes_the_sequence_reproducible(noise_log):
    Fn, calls = noise_log
    runs = []
    for _ in range(2):
        Fn.manual_seed(7)
        del calls[:]
        for k in range(3):
            _bare_forward(Fn, 100 * k)
        runs.append([(c[2], c[3]) for c in calls])
    assert runs[0] == runs[1] and runs[0][0] == (7, Fn._NOISE_OFFSET)
    Fn.manual_seed(8)
    del calls[:]
    _bare_forward(Fn, 0)
    assert calls[0][2:4] == (8, Fn._NOISE_OFFSET)
