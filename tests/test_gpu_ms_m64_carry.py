"""GPU: ms_m64_body, the slot of the smallest magnitude of a check and what the next iteration makes of it.

STATE3 of an iteration leaves, per check, min1, min2, the signs and the slot of min1; the next iteration sends min2 to that slot and
min1 to every other one.  A wrong slot -- wherever it is taken from: a stored position today, lane masks of the compares in the
variants of tools/ab_flagship.hip that carry the decoded values instead -- shows only in the soft values of the NEXT iteration, and
with random channel values only in some lanes.  This file puts the minimum where it wants it (budgets, shifts and +-0.0 are covered
by test_gpu_ms_m64_retain.py, test_gpu_ms_m64_rotation.py and the adversarial tests):

  - the minimum on every slot of a row of weight 16, of weight 8 and of weight 1 (the smallest the body accepts), in every lane;
  - ties between two slots (the earlier slot is the min1 slot) for every pair of slots of the weight-8 row, and all magnitudes equal;
  - a code whose rows all keep their decoded values in registers (4 x 8), one where the last row alone does not (14 x 28), a code
    of 20 block rows, where a few kept rows are followed by many that are not, and a code of 30 block rows whose budget is cut to
    zero, so that no row is kept at all;
  - several frames per wave of the persistent launch, where frames that converge at once alternate with frames that never do:
    nothing a frame left in registers may survive into the wave's next frame.

The slot tests run maxiter 2 and 3.  Everything is compared with the CPU oracle bit for bit: hard decisions, signed iteration
counts (the syndrome word that ends a frame), soft values."""
import itertools

import numpy as np
import pytest

from ldpc_testlib import (MS_DEC, Oracle, adversarial_llr, assert_bits_equal, awgn_llr, load_base_matrix, pack_bits, random_qc_code,
                          relift)

gpu = pytest.mark.gpu   # the tests that decode; the two that only look at the matrices run anywhere

M = 64
FRAMES = 16
AOT_NAME = "ms_spec_appendix_c_m64_kernel (ahead of time)"
WIDE, EIGHT, ONE = 0, 1, 2   # block rows of _slot_matrix()


def _slot_matrix():
    """3 x 16: row 0 has all 16 block columns, row 1 the 8 odd ones, row 2 block column 4 alone.  Shifts mix 0, 63 and others."""
    H = -np.ones((3, 16), dtype=np.int16)
    for k in range(16):
        H[WIDE, k] = (23 * k + 7) % M if k % 5 else (0 if k % 2 else 63)
    for k in range(1, 16, 2):
        H[EIGHT, k] = (13 * k + 2) % M
    H[ONE, 4] = 31
    return H


def _signs(seed, shape):
    return np.where(np.random.RandomState(seed).randint(0, 2, size=shape) == 1, -1.0, 1.0)


def _frames_with_small_columns(H, column_sets, seed):
    """One frame per entry of column_sets: |y| = 2.0 everywhere, 1.0 on every variable of the named block columns, random signs."""
    N = H.shape[1] * M
    y = 2.0 * _signs(seed, (len(column_sets), N))
    for f, cols in enumerate(column_sets):
        for k in cols:
            y[f, k * M:(k + 1) * M] *= 0.5
    return np.ascontiguousarray(y)


def _expect_equal(dec, oracle, llr, maxiter, what, torch):
    d_ref, it_ref, _ = oracle.decode(MS_DEC, llr, maxiter, 0)
    s_ref, _, _ = oracle.decode(MS_DEC, llr, maxiter, 1)
    hard, iters, soft = dec.decode(torch.from_numpy(llr).cuda(), maxiter, want_soft=True)
    torch.cuda.synchronize()
    assert np.array_equal(iters.cpu().numpy(), it_ref), (what, iters.cpu().numpy(), it_ref)
    assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref)), what
    assert_bits_equal(soft.cpu().numpy(), s_ref, "soft values, " + what)
    return it_ref


def test_the_slot_matrix_holds_what_it_is_meant_to_exercise():
    H = _slot_matrix()
    w = [int(x) for x in (H >= 0).sum(axis=1)]
    assert w == [16, 8, 1] and ((H >= 0).sum(axis=0) >= 1).all()
    y = _frames_with_small_columns(H, [(3,), (1, 5)], 7)
    a = np.abs(y).reshape(2, 16, M)
    assert (a[0, 3] == 1.0).all() and (np.delete(a[0], 3, axis=0) == 2.0).all()
    assert (a[1, [1, 5]] == 1.0).all() and (np.delete(a[1], [1, 5], axis=0) == 2.0).all()
    assert (y < 0).any() and (y > 0).any()


@gpu
def test_the_minimum_on_every_slot_and_every_tie_of_two_slots():
    """Frame s of the first batch has its smallest magnitudes on block column s: in iteration 0 every c2v value is +0.0, so the v2c
    values are the channel values and slot s is the min1 slot of the weight-16 row in every lane (and, for odd s, slot (s - 1) / 2 of
    the weight-8 row; s = 4 reaches the row of weight 1).  The second batch puts the same small magnitude on two block columns for
    every pair of slots of the weight-8 row -- both are slots of the weight-16 row too -- and ends with a frame of equal magnitudes."""
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H = _slot_matrix()
    eight = [int(k) for k in np.flatnonzero(H[EIGHT] >= 0)]
    every_slot = _frames_with_small_columns(H, [(k,) for k in range(16)], 1801)
    pairs = list(itertools.combinations(eight, 2))
    assert len(pairs) == 28
    ties = np.concatenate([_frames_with_small_columns(H, pairs, 1802), 2.0 * _signs(1803, (1, 16 * M))])
    oracle = Oracle(H, M)
    with ldpc_lib_amd.LdpcHip(MS_DEC, H, M) as dec:
        assert "ms_m64_body" in dec.kernel_name and "hiprtc" in dec.kernel_name, dec.kernel_name
        for name, llr in (("minimum on slot = frame", every_slot), ("ties", ties)):
            for maxiter in (2, 3):
                it = _expect_equal(dec, oracle, llr, maxiter, f"{name}, maxiter {maxiter}", torch)
                assert (np.abs(it) >= 2).all(), (name, it)   # the iteration that uses the min1 slot of iteration 1 really runs


def _all_rows_kept():
    """4 x 8, 20 edges"""
    return random_qc_code(np.random.RandomState(1811), 4, 8, M, [2, 3])


def _fourteen_rows():
    """14 x 28 of the usual protograph shape, 75 edges in rows of weight 4-8 (the matrix of test_gpu_ms_m64_retain.py)"""
    return random_qc_code(np.random.RandomState(1364), 14, 28, M, [3, 4, 2])


def _twenty_rows():
    """20 x 40, 148 edges in rows of weight 5-12: a few kept rows, followed by many rows that are not kept"""
    return random_qc_code(np.random.RandomState(1812), 20, 40, M, [5, 6, 5])


def _thirty_rows():
    """30 x 60, rows at most 8 wide: thirty records alone ask for more registers than the budget has to give, no row is kept"""
    return random_qc_code(np.random.RandomState(1813), 30, 60, M, [3, 3, 2])


ROW_SETS = {"all_rows_kept_4x8": _all_rows_kept, "fourteen_rows_14x28": _fourteen_rows, "twenty_rows_20x40": _twenty_rows,
            "no_row_kept_30x60": _thirty_rows}


def _kept_rows(H):
    """ms_m64_keep_budget and ms_m64_keep_rows of ldpc_spec.hpp, restated: 70 edges, less one per register that the records (5 per
    block row), the block columns in flight (2 each, at most 24) and the widest row (2 per slot) need beyond the example code's
    5 * 16 + 2 * 24 + 2 * 8; whole rows in ascending order while their edges fit.  Returns (budget, kept rows)."""
    w = [int(x) for x in (H >= 0).sum(axis=1)]
    rh, nh = H.shape
    others = 5 * rh + 2 * min(nh, 24) + 2 * max(w)
    budget = max(70 - max(others - (5 * 16 + 2 * 24 + 2 * 8), 0), 0)
    edges = rows = 0
    while rows < rh and edges + w[rows] <= budget:
        edges += w[rows]
        rows += 1
    return budget, rows


def test_the_row_set_matrices_hold_what_they_are_meant_to_exercise():
    for name, make in ROW_SETS.items():
        H = make()
        w = (H >= 0).sum(axis=1)
        assert H.shape == tuple(int(x) for x in name.split("_")[-1].split("x")) and 1 <= w.min() and w.max() <= 16, (name, w)
        assert ((H >= 0).sum(axis=0) >= 1).all()
    assert _kept_rows(relift(load_base_matrix(), M)) == (70, 10)   # the restated rule on the shipped shape: block rows 0-9
    assert _kept_rows(_all_rows_kept())[1] == 4                    # every row kept
    assert _kept_rows(_fourteen_rows())[1] == 13                   # a kept row directly followed by the one that is not
    budget, rows = _kept_rows(_twenty_rows())
    assert 0 < rows <= 6 and budget < 70, (budget, rows)           # a few kept rows, many that are not
    assert (_thirty_rows() >= 0).sum(axis=1).max() <= 8 and _kept_rows(_thirty_rows()) == (0, 0)   # budget cut to zero


@gpu
@pytest.mark.parametrize("case", list(ROW_SETS))
def test_ms_m64_row_sets_equal_the_oracle(case):
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H = ROW_SETS[case]()
    Hi = np.asarray(H, dtype=np.int32)
    no = list(ROW_SETS).index(case)
    inputs = {"awgn 0 dB": awgn_llr(Hi, M, 0.0, 1820 + no, FRAMES, burn_codeword=False),
              "awgn 2 dB": awgn_llr(Hi, M, 2.0, 1830 + no, FRAMES, burn_codeword=False),
              "adversarial": adversarial_llr(H, M, 18 + no)[0]}
    oracle = Oracle(H, M)
    with ldpc_lib_amd.LdpcHip(MS_DEC, H, M) as dec:
        assert "ms_m64_body" in dec.kernel_name and "hiprtc" in dec.kernel_name, dec.kernel_name
        for name, llr in inputs.items():
            for maxiter in (1, 2, 50):
                _expect_equal(dec, oracle, llr, maxiter, f"{case}, {name}, maxiter {maxiter}", torch)


@gpu
def test_nothing_survives_into_the_next_frame_of_a_persistent_wave():
    """The shipped shape, 6144 frames = three times the 2048 resident waves of an MI355X: every wave pulls further frames from the
    queue.  Even frames converge in one or two iterations, odd frames never, so a wave starts a frame with the registers of a
    frame that stopped at another iteration.  A new frame must start from +0.0 on every edge and a cleared syndrome word."""
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H = relift(load_base_matrix(), M)
    Hi = np.asarray(H, dtype=np.int32)
    fast = awgn_llr(Hi, M, 12.0, 1841, FRAMES, burn_codeword=False)
    slow = awgn_llr(Hi, M, 0.0, 1842, FRAMES, burn_codeword=False)
    distinct = np.concatenate([fast, slow])
    oracle = Oracle(H, M)
    d_ref, it_ref, _ = oracle.decode(MS_DEC, distinct, 50, 0)
    s_ref, _, _ = oracle.decode(MS_DEC, distinct, 50, 1)
    assert ((it_ref[:FRAMES] >= 1) & (it_ref[:FRAMES] <= 2)).all() and (it_ref[FRAMES:] == -50).all(), it_ref
    rng = np.random.RandomState(1843)
    idx = rng.randint(0, FRAMES, size=6144)
    idx[1::2] += FRAMES   # even places: a frame that converges at once, odd places: one that never does
    with ldpc_lib_amd.LdpcHip(MS_DEC, H, M) as dec:
        assert dec.kernel_name == AOT_NAME, dec.kernel_name
        hard, iters, soft = dec.decode(torch.from_numpy(distinct[idx]).cuda(), 50, want_soft=True)
        torch.cuda.synchronize()
        assert dec.last_launch() == AOT_NAME, dec.last_launch()
    bad = np.flatnonzero(iters.cpu().numpy() != it_ref[idx])
    assert not bad.size, [(int(f), int(idx[f])) for f in bad[:8]]
    assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref)[idx])
    assert_bits_equal(soft.cpu().numpy(), s_ref[idx], "soft values")
