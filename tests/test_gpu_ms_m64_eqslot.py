"""GPU: ms_m64_body carries the decoded check-to-variable values of its first block rows from STATE3 of one iteration to STATE3 of
the next, and such a row finds its min1 slot by value equality.

A carried row has no record (m1, m2, sign word + slot).  After its min loop slot s takes nm2 where |tt[s]| == nm1 and nm1 elsewhere
(the argument is next to `keep` in ms_m64_body and runs as text in test_ms_m64_eqslot_cpu.py); STATE1 of the next iteration
scatters those values as they are, STATE3 takes them out again as keep * |alpha|.  What can go wrong, and what this file aims at:

  - the equality select where it could differ from the stored slot: the minimum on every slot of a row, two-, three- and all-way
    ties, every |y| exactly at the clamp 32767.0, just below and just above it, |y| = 1e300 (min1 == min2 == the clamp), +-0.0;
  - both tiers and their seam: a 3 x 16 code with rows of weight 16, 8 and 1 (all carried), a 4 x 8 with every row carried, a
    14 x 28 whose last rows keep their record (a column of the dual diagonal has one edge on each side), a 30 x 60 whose budget is
    cut to zero (no row carried: the body as it was), and the shipped code (rows 0-12 of 16 carried, ahead-of-time instance);
  - the first iteration of a frame (every carried value +0.0), maxiter 1, 2, 3 and 50, frames that stop at once and frames that
    never do;
  - several frames per wave of the persistent launch: no carried value may survive into the wave's next frame.

Everything is compared with the CPU oracle bit for bit: hard decisions, signed iteration counts, soft values."""
import itertools

import numpy as np
import pytest

from ldpc_testlib import (MS_DEC, Oracle, adversarial_llr, assert_bits_equal, awgn_llr, load_base_matrix, pack_bits, random_qc_code,
                          relift)
from test_gpu_ms_m64_carry import _all_rows_kept, _expect_equal, _signs, _slot_matrix, _thirty_rows
from test_gpu_ms_m64_local import local_columns

gpu = pytest.mark.gpu   # the tests that decode; the one that only looks at the matrices runs anywhere

M = 64
FRAMES = 16
KMAX = 32767.0               # kMaxVal
KEEP_EDGES, KEEP_ROWS = 68, 13   # kMsM64KeepEdges, kMsM64KeepRowsOfExample
AOT_NAME = "ms_spec_appendix_c_m64_kernel (ahead of time)"


def _shipped():
    return relift(load_base_matrix(), M)


def _record_rows_last():
    """14 x 28 of the usual protograph shape, 114 edges in rows of weight 5-13: block rows 0-8 are carried, rows 9-13 keep their
    record, and block column 8 of the dual diagonal has one edge on each side."""
    return random_qc_code(np.random.RandomState(2002), 14, 28, M, [6, 7, 5])


CODES = {"slot_matrix_3x16": _slot_matrix, "every_row_carried_4x8": _all_rows_kept, "record_rows_last_14x28": _record_rows_last,
         "no_row_carried_30x60": _thirty_rows, "shipped_16x32": _shipped}


def carried_rows(H):
    """ms_m64_keep_budget and ms_m64_keep_rows of ldpc_spec.hpp, restated.  A carried row costs 2 registers per edge that goes
    through LDS (edges of local columns are not counted) and gives back the 5 of its record.  The example code leaves
    2 * 68 - 5 * 13 = 71 registers to that, a code that needs more for its records (5 per block row), its channel values in flight
    (2 per block column, at most 24) and its widest row (2 per slot) than the example's 5 * 16 + 2 * 24 + 2 * 8 gives the difference
    back.  Whole rows in ascending order while they fit."""
    rh, nh = H.shape
    loc = local_columns(H)
    w = [int((H[j] >= 0).sum()) for j in range(rh)]
    nl = [w[j] - sum(1 for k in loc if H[j, k] >= 0) for j in range(rh)]
    others = 5 * rh + 2 * min(nh, 24) + 2 * max(w)
    budget = max(2 * KEEP_EDGES - 5 * KEEP_ROWS - max(others - (5 * 16 + 2 * 24 + 2 * 8), 0), 0)
    edges = rows = 0
    while rows < rh and 2 * (edges + nl[rows]) - 5 * (rows + 1) <= budget:
        edges += nl[rows]
        rows += 1
    return rows


def test_the_matrices_hold_what_they_are_meant_to_exercise():
    H = _slot_matrix()
    assert [int(x) for x in (H >= 0).sum(axis=1)] == [16, 8, 1] and carried_rows(H) == 3
    assert carried_rows(_all_rows_kept()) == 4
    H = _record_rows_last()
    kr = carried_rows(H)
    assert kr == 9, kr                          # block rows 0-8 carried, rows 9-13 keep their record
    assert kr - 1 in local_columns(H) and H[kr - 1, kr - 1] == 0 and H[kr, kr - 1] == 0   # a local column with an edge on each side
    assert carried_rows(_thirty_rows()) == 0    # budget cut to zero
    assert carried_rows(_shipped()) == 13       # block rows 0-12, 68 edges through LDS


def _small_on(H, column_sets, seed, small=1.0, big=2.0):
    """One frame per entry of column_sets: |y| = big everywhere, small on every variable of the named block columns, random signs."""
    N = H.shape[1] * M
    y = big * _signs(seed, (len(column_sets), N))
    for f, cols in enumerate(column_sets):
        for k in cols:
            y[f, k * M:(k + 1) * M] *= small / big
    return np.ascontiguousarray(y)


def _inputs(H, no):
    """name -> LLRs [FRAMES, N]"""
    Hi = np.asarray(H, dtype=np.int32)
    nh = H.shape[1]
    N = nh * M
    rng = np.random.RandomState(2010 + no)
    # the block columns of the widest carried row first (every slot of it), then the others
    kr = carried_rows(H)
    wide = max(range(max(kr, 1)), key=lambda j: int((H[j] >= 0).sum()))
    cols = [int(k) for k in np.flatnonzero(H[wide] >= 0)]
    cols = (cols + [k for k in range(nh) if k not in cols])[:FRAMES]
    cols = (cols * FRAMES)[:FRAMES]
    pairs = list(itertools.combinations(cols[:5], 2))[:7]
    triples = list(itertools.combinations(cols[:5], 3))[:7]
    ties = np.concatenate([_small_on(H, pairs, 2020 + no), _small_on(H, triples, 2030 + no),
                           2.0 * _signs(2040 + no, (1, N)), _small_on(H, [cols[:8]], 2050 + no, small=5e-324, big=1.0)])
    below, above = np.nextafter(KMAX, 0.0), np.nextafter(KMAX, np.inf)
    clamp = np.empty((FRAMES, N))
    for f, mags in enumerate([[KMAX], [KMAX], [below], [below], [above], [above], [1e300], [1e300], [below, KMAX, above],
                              [below, KMAX, above], [KMAX, 1e300], [1.0, below, KMAX, above, 1e300], [0.0, 5e-324, KMAX, 1e300],
                              [0.0], [0.0], [0.0]]):
        clamp[f] = rng.choice(np.asarray(mags), size=N) * _signs(2060 + 16 * no + f, (N,))
    clamp[13] = 0.0                                   # +0.0 everywhere
    clamp[14] = -0.0                                  # -0.0 everywhere; frame 15: random signs on 0.0
    assert np.signbit(clamp[14]).all() and not np.signbit(clamp[13]).any() and np.signbit(clamp[15]).any()
    adv = adversarial_llr(H, M, 40 + no)[0]
    return {"minimum on every slot": _small_on(H, [(k,) for k in cols], 2000 + no),
            "ties of two, three and all": ties,
            "at the clamp, 1e300 and +-0.0": np.ascontiguousarray(clamp),
            "adversarial": adv,
            "awgn 0 dB": awgn_llr(Hi, M, 0.0, 2070 + no, FRAMES, burn_codeword=False),
            # 12 dB: the first iteration's hard decisions are a codeword; random signs on one magnitude: no iteration's are
            "both exits": np.concatenate([awgn_llr(Hi, M, 12.0, 2080 + no, FRAMES // 2, burn_codeword=False),
                                          3.0 * _signs(2090 + no, (FRAMES // 2, N))])}


def test_the_inputs_hold_what_they_are_meant_to_exercise():
    H = _slot_matrix()
    inp = _inputs(H, 0)
    a = np.abs(inp["minimum on every slot"]).reshape(FRAMES, 16, M)
    assert sorted(int(np.flatnonzero((a[f] == 1.0).all(axis=1))[0]) for f in range(FRAMES)) == list(range(16))
    t = np.abs(inp["ties of two, three and all"]).reshape(FRAMES, 16, M)
    assert [int((t[f] == t[f].min()).all(axis=1).sum()) for f in range(FRAMES)] == [2] * 7 + [3] * 7 + [16, 8]
    c = np.abs(inp["at the clamp, 1e300 and +-0.0"])
    assert (c[0] == KMAX).all() and (c[2] < KMAX).all() and (c[2] > 32766.9).all() and (c[4] > KMAX).all() and (c[6] == 1e300).all()
    for name, llr in inp.items():
        assert llr.shape[1] == 16 * M and np.isfinite(llr).all(), name
        assert llr.shape[0] == FRAMES or name == "adversarial", name


@gpu
@pytest.mark.parametrize("case", list(CODES))
def test_ms_m64_with_carried_rows_equals_the_oracle(case):
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
def test_carried_values_do_not_survive_into_the_next_frame_of_a_persistent_wave():
    """6144 frames of the 14 x 28 code (both tiers), three times the 2048 resident waves of an MI355X: frames that converge at once
    alternate with frames that never do, so a wave starts a frame with the carried values of a frame that stopped at another
    iteration.  A new frame must start from +0.0 on every carried edge."""
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H = _record_rows_last()
    both = _inputs(H, list(CODES).index("record_rows_last_14x28"))["both exits"]
    oracle = Oracle(H, M)
    d_ref, it_ref, _ = oracle.decode(MS_DEC, both, 50, 0)
    s_ref, _, _ = oracle.decode(MS_DEC, both, 50, 1)
    assert ((it_ref[:FRAMES // 2] >= 1) & (it_ref[:FRAMES // 2] <= 2)).all() and (it_ref[FRAMES // 2:] == -50).all(), it_ref
    idx = np.random.RandomState(2099).randint(0, FRAMES // 2, size=6144)
    idx[1::2] += FRAMES // 2   # even places: a frame that converges at once, odd places: one that never does
    with ldpc_lib_amd.LdpcHip(MS_DEC, H, M) as dec:
        assert "ms_m64_body" in dec.kernel_name and "hiprtc" in dec.kernel_name, dec.kernel_name
        hard, iters, soft = dec.decode(torch.from_numpy(both[idx]).cuda(), 50, want_soft=True)
        torch.cuda.synchronize()
    bad = np.flatnonzero(iters.cpu().numpy() != it_ref[idx])
    assert not bad.size, [(int(f), int(idx[f])) for f in bad[:8]]
    assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref)[idx])
    assert_bits_equal(soft.cpu().numpy(), s_ref[idx], "soft values")
