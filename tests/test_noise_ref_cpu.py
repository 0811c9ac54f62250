"""tests/fp64_noise_ref.py against the published algorithm, and the numpy emulation of the stream against fp64_noise_ref (no GPU).

The known-answer vectors guard the reference; tests/test_gpu_noise_stream.py guards the kernel against the reference."""
import numpy as np
import pytest

import emu_eval_ops
import fp64_noise_ref as N

# Random123's kat_vectors for philox4x32 with 10 rounds: counter, key -> output
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
N_EMU = 1_000_003
EMU_SEEDS = [0, 1234567890123, 2 ** 64 - 1, 0x0123456789ABCDEF]
# Measured: max |_philox_normal_np - normal_stream| over N_EMU elements is 1.621e-06, 1.559e-06, 1.633e-06, 1.525e-06 for the four seeds
# (float32 log / sqrt / cos / sin and the float32 angle against float64 ones on the same float32 u).  Asserted: twice the worst.
EMU_ERR = 1.633e-06


@pytest.mark.parametrize("counter,key,out", KAT)
def test_philox4x32_10_known_answers(counter, key, out):
    got = N.philox4x32_10(counter, key)
    assert tuple(int(w) for w in got) == out
    # the same through arrays (the form normal_stream uses), with the vector in the middle of other counters
    ctr = [np.array([c ^ 1, c, (c + 1) & 0xFFFFFFFF], dtype=np.uint64) for c in counter]
    got = N.philox4x32_10(ctr, key)
    assert tuple(int(w[1]) for w in got) == out and all(w.dtype == np.uint64 and int(w.max()) <= 0xFFFFFFFF for w in got)


def test_stream_addressing_of_the_reference():
    """element e = lane e & 3 of block e >> 2; counter = (blk low, blk high, 0, 0); key = (seed low, seed high)"""
    seed = 0x0123456789ABCDEF
    z = N.normal_stream(23, seed)
    for blk in (0, 3, 5):
        words = N.philox4x32_10((blk, 0, 0, 0), (0x89ABCDEF, 0x01234567))
        assert np.array_equal(z[4 * blk: 4 * blk + 4], N.box_muller([np.asarray(w).reshape(1) for w in words])[0][: 23 - 4 * blk])
    assert np.array_equal(N.normal_stream(10, seed, first=7), z[7:17])  # a window of the stream that starts inside a block
    big = (1 << 34) + 5  # block index 2^32 + 1: the high counter word
    words = N.philox4x32_10((1, 1, 0, 0), (0x89ABCDEF, 0x01234567))
    assert np.array_equal(N.normal_stream(3, seed, first=big), N.box_muller([np.asarray(w).reshape(1) for w in words])[0][1:4])
    u = N.uniform_f32(np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000], dtype=np.uint64))
    assert u.dtype == np.float32 and list(u) == [2.0 ** -25, 2.0 ** -25, 1.5 * 2.0 ** -24, (2.0 ** 23 - 0.5) * 2.0 ** -24, 0.5]


@pytest.mark.parametrize("seed", EMU_SEEDS)
def test_numpy_emulation_of_the_stream_against_the_reference(seed):
    got = emu_eval_ops._philox_normal_np(N_EMU, seed)
    assert got.dtype == np.float32 and got.shape == (N_EMU,) and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - N.normal_stream(N_EMU, seed)).max()
    print(f"emulation vs float64 stream, seed {seed:#x}: max err {err:.3e}")
    assert err <= 2 * EMU_ERR


def test_planted_defects_move_the_reference():
    """every defect normal_stream can plant changes (nearly) every element it is meant to change, by O(1)"""
    n, seed = 4099, 0x0123456789ABCDEF
    z = N.normal_stream(n, seed)
    moved = lambda w: (np.abs(w - z) > 1e-3).mean()
    assert moved(N.normal_stream(n, seed + 1)) > 0.99 and moved(N.normal_stream(n, seed ^ (1 << 32))) > 0.99
    assert moved(N.normal_stream(n, seed, swap_key=True)) > 0.99 and moved(N.normal_stream(n, seed, block_shift=1)) > 0.99
    assert moved(N.normal_stream(n, seed, swap_trig=True)) > 0.98
    sw = N.normal_stream(n, seed, lanes=(0, 2, 1, 3))
    lane = np.arange(n) & 3
    assert np.array_equal(sw[(lane == 0) | (lane == 3)], z[(lane == 0) | (lane == 3)]) and moved(sw) > 0.49
    assert np.array_equal(N.normal_stream(n - 4, seed, block_shift=1), z[4:])


def test_u_that_rounds_to_one_gives_zero_not_nan():
    """c >> 8 == 2^24 - 1: (float)(2^24 - 1) + 0.5f is a tie and rounds to 2^24, u == 1.0, ln u == 0: both lanes of that radius are 0"""
    top = np.array([0xFFFFFF00, 0xFFFFFFFF, 0xFFFFFE00, 0xFFFFFEFF], dtype=np.uint64)  # the last two: the largest u below 1
    assert list(N.uniform_f32(top)) == [1.0, 1.0, 1.0 - 2.0 ** -23, 1.0 - 2.0 ** -23]
    other = np.array([0x12345678, 0x9ABCDEF0, 0x0, 0xFFFFFFFF], dtype=np.uint64)
    z = N.box_muller((top, other, other, top))
    assert np.isfinite(z).all()
    assert (z[:2, :2] == 0).all() and (z[2:, :2] != 0).all()  # u0 == 1 in blocks 0 and 1
    assert (z[3, 2:] == 0).all() and (z[:3, 2:] != 0).all()   # u2 == 1 in block 3


def test_a_seed_whose_stream_holds_such_a_u():
    """seed 5947, block 41 (found by a search over small seeds): the GPU test reads these elements from the kernel"""
    m = N.unit_u0_mask(256, 5947)
    assert m.sum() == 2 and set(np.flatnonzero(m) >> 2) == {41}
    z = N.normal_stream(256, 5947)
    assert (z[m] == 0).all() and np.isfinite(z).all() and (z[~m] != 0).all()
