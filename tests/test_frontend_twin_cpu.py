"""CPU: the references of tests/frontend_twin.py pinned without the device, so that a GPU comparison against them means something.

  * chain_twin at the (2048, 1024) shape equals values frozen from the arithmetic tests/test_gpu_chain.py used before the twin moved
    here (tests/golden/frontend/chain_twin_pin.npz: 26 LLRs of two frames for each of that test's eight cells, sent words and all-zero);
  * upstream's recorded interleaver maps, passed as arguments, are the ones the library builds for the same config;
  * count_twin on hand-written frames: single flips at R - 1, R and N - 1, a negative iteration count;
  * random_info_twin: shape, group boundaries, independence of the window;
  * the saturating-demapper cases really saturate: 0.2 .. 0.8 of the reference LLRs equal +-T, none is NaN.
"""
import os

import numpy as np
import pytest

from frontend_twin import (SATURATION_CASES, T_CUT, chain_twin, chain_twin_of_mode, code_a, code_b, code_c, code_d, count_twin,
                           random_info_twin, recorded_interleavers, saturation_reference)
from ldpc_testlib import GOLDEN_DIR, load_base_matrix, philox4x32_10, relift

CHAIN_CELLS = [(0, 1.5, 0, None), (0, 1.5, 2, (1, 128, 1)), (1, 2.0, 0, (3, 64, 1)), (2, 6.0, 0, (3, 64, 1)), (2, 6.0, 3, None),
               (3, 10.0, 1, (2, 128, 1)), (4, 14.0, 0, (4, 128, 8)), (4, 14.0, 2, (1, 128, 1))]


def test_chain_twin_at_the_old_shape_equals_the_frozen_values():
    import ldpc_lib_amd  # noqa: F401
    from ldpc_lib_amd.binding import encode
    g = np.load(os.path.join(GOLDEN_DIR, "frontend", "chain_twin_pin.npz"))
    idx, want = g["index"], g["values"]
    H = relift(load_base_matrix(), 64)
    first, seed = 4_000_000_123, (3 << 32) | 19
    for c, (mod, snr, punct, perm) in enumerate(CHAIN_CELLS):
        rng = np.random.RandomState(11 + mod)
        cws = np.stack([encode(H, 64, rng.randint(0, 2, size=1024).astype(np.uint8)) for _ in range(3)])
        got = chain_twin_of_mode(H, 64, cws, first, 2, seed, snr, mod, punct, perm, 0.5)
        assert np.array_equal(got[:, idx], want[2 * c]), (mod, perm)
        zero = chain_twin(H, 64, None, first, 1, seed, snr, mod, punct, None, None, 0.5)
        assert np.array_equal(zero[0, idx], want[2 * c + 1][0]), (mod, perm)
        if punct:
            assert (got[:, 2048 - 64 * punct:] == 0.5).all() and not (got[:, :2048 - 64 * punct] == 0.5).any()


def test_the_shapes_are_the_ones_the_gpu_tests_are_written_for():
    for (H, M), shape, N, R in ((code_a(), (16, 33), 297, 144), (code_b(), (16, 30), 210, 112), (code_c(), (16, 33), 2211, 1072),
                                (code_d(), (3, 7), 35, 15)):
        assert H.shape == shape and H.shape[1] * M == N and H.shape[0] * M == R and H.max() < M
    assert 297 % 2 == 1 and 210 % 2 == 0 and 210 % 4 and 144 % 32 == 16 and 112 % 32 == 16 and 1072 % 32 == 16
    assert (2211 + 31) // 32 == 70 and (35 + 31) // 32 == 2


@pytest.mark.parametrize("shape,M", [((16, 33), 9), ((16, 30), 7)])
def test_recorded_maps_are_what_the_library_builds(shape, M):
    """the twin gets the recorded maps, the device gets set_interleaver(mode, block, step): the same interleaver"""
    import ldpc_lib_amd  # noqa: F401
    from ldpc_lib_amd.binding import build_interleaver
    maps, H = recorded_interleavers(shape, M)
    assert set(maps) == {(h, mode) for h in (1, 2, 3, 4) for mode in (1, 2, 3, 4)}
    N = shape[1] * M
    for (h, mode), (bs, st, direct, inverse) in maps.items():
        d, i = build_interleaver(H, M, mode, h, bs, st)
        assert np.array_equal(d, direct) and np.array_equal(i, inverse)
        assert np.array_equal(np.sort(direct), np.arange(N)) and np.array_equal(direct[inverse], np.arange(N))
    assert any(not np.array_equal(d, np.arange(N)) for _, _, d, _ in maps.values())


def test_count_twin_on_hand_written_frames():
    N, R = 35, 15
    sent = np.zeros((6, N), dtype=np.uint8)
    sent[:, ::3] = 1
    bits = sent.copy()
    bits[1, R - 1] ^= 1                      # last parity bit: an errored frame with no information bit wrong
    bits[2, R] ^= 1                          # first information bit
    bits[3, N - 1] ^= 1                      # last bit
    bits[4, R] ^= 1
    bits[4, 0] ^= 1
    bits[5, [R - 1, R, R + 1, N - 1]] ^= 1
    iters = np.array([7, 3, -50, 0, -4, 50])
    cnt, info = count_twin(bits, iters, R, sent)
    # nse = 0 + 1 + 1 + 1 + 3, five errored frames, of which iters >= 0: frames 1, 3, 5
    assert cnt == [6, 5, 3, 6, 7 + 3 + 50 + 0 + 4 + 50]
    assert info.tolist() == [0, 1 << 30, (1 << 30) | 1, (1 << 30) | 1, (1 << 30) | 1, (1 << 30) | 3] and info.dtype == np.int32
    # against the all-zero word the sent ones themselves are errors
    cnt0, info0 = count_twin(sent, np.zeros(6, dtype=np.int32), R)
    assert cnt0 == [6 * int(sent[0, R:].sum()), 6, 6, 6, 0] and (info0 == ((1 << 30) | int(sent[0, R:].sum()))).all()
    c, i = count_twin(np.zeros((2, N), dtype=np.uint8), [-3, 3], R)
    assert c == [0, 0, 0, 2, 6] and i.tolist() == [0, 0]


def test_random_info_twin_restates_the_kernels_bit_order():
    seed, K = (0xABCDEF << 32) | 12345, 153          # two groups, the second of 25 bits
    a = random_info_twin(seed, 0, 7, K)
    assert a.shape == (7, K) and a.dtype == np.uint8 and set(np.unique(a)) == {0, 1}
    # one word by hand: idx 4, group 1, bit 20 is bit 20 of x[0]; group 0 bit 97 is bit 1 of x[3]
    x1 = philox4x32_10(np.uint64(4), np.uint64(0), np.uint64(1), np.uint64(2), seed & 0xFFFFFFFF, seed >> 32)
    x0 = philox4x32_10(np.uint64(4), np.uint64(0), np.uint64(0), np.uint64(2), seed & 0xFFFFFFFF, seed >> 32)
    assert a[4, 128 + 20] == (int(x1[0]) >> 20) & 1 and a[4, 97] == (int(x0[3]) >> 1) & 1 and a[4, 0] == int(x0[0]) & 1
    # keyed by the word's global index, beyond 2^32 too
    assert np.array_equal(random_info_twin(seed, 3, 4, K), a[3:7])
    big = random_info_twin(seed, (1 << 32) + 1, 1, K)
    xb = philox4x32_10(np.uint64(1), np.uint64(1), np.uint64(0), np.uint64(2), seed & 0xFFFFFFFF, seed >> 32)
    assert big[0, 33] == (int(xb[1]) >> 1) & 1
    assert 0.4 < random_info_twin(seed, 0, 64, 1024).mean() < 0.6


@pytest.mark.parametrize("mod,snr", SATURATION_CASES)
def test_the_saturation_cases_saturate(mod, snr):
    """Measured on this reference at N = 297: 0.42, 0.50 and 0.56 of the LLRs equal +-T at 14, 18 and 22 dB, none is NaN."""
    _, _, _, _, ref = saturation_reference(mod, snr)
    assert ref.shape == (5, 297) and not np.isnan(ref).any()
    share = (np.abs(ref) == T_CUT).mean()
    assert 0.2 <= share <= 0.8, share
