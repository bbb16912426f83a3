"""GPU: the carried block rows of ms_m64_body form their check-to-variable magnitudes from prefix and suffix minima.

A carried row (block rows [0, KR), see test_gpu_ms_m64_eqslot.py) no longer computes min1 and min2: ascending through its slots it
keeps the prefix minima pf[s] = min(K, v_0 .. v_s) of its |v2c| values, descending it meets them with the suffix minima, and slot s
takes min(pf[s - 1], suf) -- the smallest of K and the other slots' values, which is what (s == min1 slot ? min2 : min1) is.  Its
sign is the v2c's own sign xor the row parity, now taken from an xor chain on bit 31 instead of a word with one bit per slot.  The
argument is next to `keep` in ms_m64_body and runs as text in test_ms_m64_prefix_cpu.py.  What can go wrong, and what this file
aims at:

  - the three forms of the suffix pass: mag[RW - 1] = pf[RW - 2], mag[0] = suf, and min(pf[s - 1], suf) in between first appear at
    row weights 1 (the clamp alone), 2 and 3: a 4 x 5 code with rows of weight 2, 3, 2, 3 (one local block column among them), and a
    3 x 16 with rows of weight 16, 8 and 1;
  - the minimum on every slot of every row width, two-, three- and all-way ties, every |y| exactly at the clamp 32767.0, just below
    and just above it, |y| = 1e300 (every magnitude is the clamp), +-0.0, the adversarial LLRs of ldpc_testlib;
  - both tiers and their seam: a 4 x 8 with every row carried, a 14 x 28 whose last rows keep their record (a column of the dual
    diagonal has one edge on each side), the shipped code (rows 0-12 of 16 carried, ahead-of-time instance);
  - maxiter 1, 2, 3 and 50, frames that stop at once and frames that never do;
  - several frames per wave of the persistent launch.

Every carried row takes the new form (KP == KR: no instance of the body spills with it, profiles/r23_flagship_isa_histogram.txt);
prefix_rows restates that.  Everything is compared with the CPU oracle bit for bit: hard decisions, signed iteration counts, soft
values."""
import itertools

import numpy as np
import pytest

from ldpc_testlib import MS_DEC, Oracle, adversarial_llr, assert_bits_equal, awgn_llr, pack_bits
from test_gpu_ms_m64_carry import _all_rows_kept, _expect_equal, _signs, _slot_matrix
from test_gpu_ms_m64_eqslot import AOT_NAME, KMAX, _record_rows_last, _shipped, _small_on, carried_rows
from test_gpu_ms_m64_local import _matrix, local_columns

gpu = pytest.mark.gpu   # the tests that decode; those that only look at the matrices and the inputs run anywhere

M = 64
FRAMES = 16


def _weights_two_and_three():
    """4 x 5, rows of weight 2, 3, 2, 3.  Block column 1 has shifts 0 and 63, block column 3 is local (shift 0 in rows 1 and 3: the
    last slot of row 1, the middle slot of row 3), the others are rotated."""
    return _matrix(4, 5, [(0, 0, 5), (0, 1, 0),
                          (1, 1, 63), (1, 2, 17), (1, 3, 0),
                          (2, 0, 32), (2, 4, 9),
                          (3, 2, 1), (3, 3, 0), (3, 4, 40)])


CODES = {"weights_16_8_1_3x16": _slot_matrix, "weights_2_and_3_4x5": _weights_two_and_three, "every_row_carried_4x8": _all_rows_kept,
         "record_rows_last_14x28": _record_rows_last, "shipped_16x32": _shipped}


def prefix_rows(H):
    """ms_m64_prefix_rows of ldpc_spec.hpp, restated: every carried row forms its magnitudes from prefix and suffix minima"""
    return carried_rows(H)


def test_the_matrices_hold_what_they_are_meant_to_exercise():
    w = lambda H: [int(x) for x in (H >= 0).sum(axis=1)]
    H = _slot_matrix()
    assert w(H) == [16, 8, 1] and prefix_rows(H) == 3
    H = _weights_two_and_three()
    assert w(H) == [2, 3, 2, 3] and prefix_rows(H) == 4 and list(local_columns(H)) == [3]
    assert prefix_rows(_all_rows_kept()) == 4
    H = _record_rows_last()
    kp = prefix_rows(H)
    assert kp == 9 and kp < H.shape[0]          # block rows 0-8 by prefix / suffix minima, rows 9-13 keep their record
    assert kp - 1 in local_columns(H) and H[kp - 1, kp - 1] == 0 and H[kp, kp - 1] == 0   # a local column with an edge on each side
    assert min(w(H)[:kp]) >= 3                  # first, middle and last slots in every carried row
    assert prefix_rows(_shipped()) == 13        # block rows 0-12 of 16


def _inputs(H, no):
    """name -> LLRs [FRAMES, N] (the adversarial set has its own number of frames)"""
    Hi = np.asarray(H, dtype=np.int32)
    nh = H.shape[1]
    N = nh * M
    rng = np.random.RandomState(2310 + no)
    # a frame per block column: every slot of every carried row holds the row's minimum in some frame (for codes with more than
    # FRAMES block columns: the columns of the widest carried row first)
    kp = prefix_rows(H)
    wide = max(range(kp), key=lambda j: int((H[j] >= 0).sum()))
    cols = [int(k) for k in np.flatnonzero(H[wide] >= 0)]
    cols = (cols + [k for k in range(nh) if k not in cols])[:FRAMES]
    cols = (cols * FRAMES)[:FRAMES]
    pairs = list(itertools.combinations(cols[:5], 2))[:7]
    triples = list(itertools.combinations(cols[:5], 3))[:7]
    ties = np.concatenate([_small_on(H, pairs, 2320 + no), _small_on(H, triples, 2330 + no),
                           2.0 * _signs(2340 + no, (1, N)), _small_on(H, [cols[:8]], 2350 + no, small=5e-324, big=1.0)])
    below, above = np.nextafter(KMAX, 0.0), np.nextafter(KMAX, np.inf)
    clamp = np.empty((FRAMES, N))
    for f, mags in enumerate([[KMAX], [KMAX], [below], [below], [above], [above], [1e300], [1e300], [below, KMAX, above],
                              [below, KMAX, above], [KMAX, 1e300], [1.0, below, KMAX, above, 1e300], [0.0, 5e-324, KMAX, 1e300],
                              [0.0], [0.0], [0.0]]):
        clamp[f] = rng.choice(np.asarray(mags), size=N) * _signs(2360 + 16 * no + f, (N,))
    clamp[13] = 0.0                                   # +0.0 everywhere
    clamp[14] = -0.0                                  # -0.0 everywhere; frame 15: random signs on 0.0
    return {"minimum on every slot": _small_on(H, [(k,) for k in cols], 2300 + no),
            "ties of two, three and all": ties,
            "at the clamp, 1e300 and +-0.0": np.ascontiguousarray(clamp),
            "adversarial": adversarial_llr(H, M, 60 + no)[0],
            # the Es/N0 of a rate-1/2 code at Eb/N0 = 12 dB (a code of lower rate gets the difference on top): the first iteration's
            # hard decisions are a codeword; random signs on one magnitude: no iteration's are
            "both exits": np.concatenate([awgn_llr(Hi, M, 12.0 + max(0.0, 10.0 * np.log10(0.5 * nh / (nh - H.shape[0]))), 2380 + no,
                                                   FRAMES // 2, burn_codeword=False),
                                          3.0 * _signs(2390 + no, (FRAMES // 2, N))])}


def test_the_inputs_hold_what_they_are_meant_to_exercise():
    for no, (case, make) in enumerate(CODES.items()):
        H = make()
        nh = H.shape[1]
        inp = _inputs(H, no)
        a = np.abs(inp["minimum on every slot"]).reshape(FRAMES, nh, M)
        small = {int(np.flatnonzero((a[f] == 1.0).all(axis=1))[0]) for f in range(FRAMES)}
        for j in range(prefix_rows(H)):
            if nh <= FRAMES or j == max(range(prefix_rows(H)), key=lambda jj: int((H[jj] >= 0).sum())):
                assert set(int(k) for k in np.flatnonzero(H[j] >= 0)) <= small, (case, j)   # the minimum visits every slot of the row
        t = np.abs(inp["ties of two, three and all"]).reshape(FRAMES, nh, M)
        assert [int((t[f] == t[f].min()).all(axis=1).sum()) for f in range(14)] == [2] * 7 + [3] * 7, case
        assert (t[14] == 2.0).all(), case
        c = inp["at the clamp, 1e300 and +-0.0"]
        assert (np.abs(c[0]) == KMAX).all() and (np.abs(c[2]) < KMAX).all() and (np.abs(c[2]) > 32766.9).all(), case
        assert (np.abs(c[4]) > KMAX).all() and (np.abs(c[4]) < 32767.1).all() and (np.abs(c[6]) == 1e300).all(), case
        assert np.signbit(c[14]).all() and not np.signbit(c[13]).any() and np.signbit(c[15]).any() and (c[13:] == 0.0).all(), case
        for name, llr in inp.items():
            assert llr.shape[1] == nh * M and np.isfinite(llr).all(), (case, name)
            assert llr.shape[0] == FRAMES or name == "adversarial", (case, name)


@gpu
@pytest.mark.parametrize("case", list(CODES))
def test_ms_m64_with_prefix_and_suffix_minima_equals_the_oracle(case):
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H = CODES[case]()
    oracle = Oracle(H, M)
    with ldpc_lib_amd.LdpcHip(MS_DEC, H, M) as dec:
        if case == "shipped_16x32":
            assert dec.kernel_name == AOT_NAME, dec.kernel_name
        else:
            assert "ms_m64_body" in dec.kernel_name and "hiprtc" in dec.kernel_name, dec.kernel_name
        for name, llr in _inputs(H, list(CODES).index(case)).items():
            for maxiter in (1, 2, 3, 50):
                it = _expect_equal(dec, oracle, llr, maxiter, f"{case}, {name}, maxiter {maxiter}", torch)
                if name == "both exits" and maxiter == 50:
                    assert (it[:FRAMES // 2] == 1).sum() >= 6 and (it[FRAMES // 2:] == -50).all(), it


@gpu
def test_a_persistent_wave_alternates_frames_that_stop_at_once_and_frames_that_never_do():
    """4096 frames of the 14 x 28 code (both tiers), twice the 2048 resident waves of an MI355X: frames that converge at once
    alternate with frames that never do, so a wave starts a frame with the prefix minima, the parity word and the carried values
    of a frame that stopped at another iteration."""
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H = _record_rows_last()
    both = _inputs(H, list(CODES).index("record_rows_last_14x28"))["both exits"]
    oracle = Oracle(H, M)
    d_ref, it_ref, _ = oracle.decode(MS_DEC, both, 50, 0)
    s_ref, _, _ = oracle.decode(MS_DEC, both, 50, 1)
    assert ((it_ref[:FRAMES // 2] >= 1) & (it_ref[:FRAMES // 2] <= 2)).all() and (it_ref[FRAMES // 2:] == -50).all(), it_ref
    idx = np.random.RandomState(2399).randint(0, FRAMES // 2, size=4096)
    idx[1::2] += FRAMES // 2   # even places: a frame that converges at once, odd places: one that never does
    with ldpc_lib_amd.LdpcHip(MS_DEC, H, M) as dec:
        assert "ms_m64_body" in dec.kernel_name and "hiprtc" in dec.kernel_name, dec.kernel_name
        hard, iters, soft = dec.decode(torch.from_numpy(both[idx]).cuda(), 50, want_soft=True)
        torch.cuda.synchronize()
    bad = np.flatnonzero(iters.cpu().numpy() != it_ref[idx])
    assert not bad.size, [(int(f), int(idx[f])) for f in bad[:8]]
    assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref)[idx])
    assert_bits_equal(soft.cpu().numpy(), s_ref[idx], "soft values")
