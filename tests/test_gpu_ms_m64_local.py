"""GPU: ms_m64_body keeps local block columns out of LDS.

A block column is local when it has an edge, every one of its edges has shift 0 and its first and last block row are at most three
apart (ms_m64_local_col of ldpc_spec.hpp): variable `lane` of the column then talks to check `lane` of its rows only.  The body
skips such a column in STATE1 and STATE2 and forms its soft value in STATE3, at the column's first block row, from the records of
its rows; the value reaches the image once per iteration, for the outputs.  What can go wrong, and what this file aims at:

  - which columns are local: degree 1, degree 3 over three rows, a column whose edges share one NON-zero shift (not local), a
    column that mixes shift 0 and 63 (not local), a span over the cap (not local);
  - the sign word of a row around skipped slots: the local edge as the last slot of a row, in the middle of a row, as the first;
  - a code where every column is local (no rotated access, no atomic at all) and one where none is (the body as before);
  - a local column with one edge in a kept row and one in a row that is not kept;
  - +-0.0 and huge magnitudes on a local column (the `+ 0.0` on the channel value, the clamp at 32 767), and equal magnitudes on
    the edges of a local column (min1 == min2);
  - both exits: frames that converge after iteration 1 and frames that never do, at maxiter 1, 2, 3 and 50;
  - several frames per wave of the persistent launch: nothing of a frame's local columns may survive into the next frame.

Everything is compared with the CPU oracle bit for bit: hard decisions, signed iteration counts, soft values."""
import numpy as np
import pytest

from ldpc_testlib import (MS_DEC, Oracle, adversarial_llr, assert_bits_equal, awgn_llr, load_base_matrix, pack_bits, random_qc_code,
                          relift)

gpu = pytest.mark.gpu   # the tests that decode; the one that only looks at the matrices runs anywhere

M = 64
FRAMES = 16
SPAN = 3          # kMsM64LocalSpan
KEEP_EDGES = 57   # kMsM64KeepEdges
AOT_NAME = "ms_spec_appendix_c_m64_kernel (ahead of time)"


def _matrix(rh, nh, entries):
    H = -np.ones((rh, nh), dtype=np.int16)
    for j, k, c in entries:
        assert H[j, k] < 0 and 0 <= c < M
        H[j, k] = c
    assert ((H >= 0).sum(axis=0) >= 1).all() and ((H >= 0).sum(axis=1) >= 1).all()
    return H


def _hand_written():
    """3 x 6.  Block column 0: one common non-zero shift; 1: shifts 0 and 63; 2 and 4: rotated; 3: local, degree 3, rows 0-2;
    5: local, degree 1.  Row 0 ends in its local edge, rows 1 and 2 have one in the middle, row 1 ends in a second one."""
    return _matrix(3, 6, [(0, 0, 5), (0, 1, 0), (0, 2, 17), (0, 3, 0),
                          (1, 0, 5), (1, 1, 63), (1, 3, 0), (1, 4, 9), (1, 5, 0),
                          (2, 0, 5), (2, 2, 40), (2, 3, 0), (2, 4, 33)])


def _every_shift_zero():
    """2 x 4, all eight shifts 0: every column is local, the iteration has no rotated access and no atomic."""
    return _matrix(2, 4, [(j, k, 0) for j in range(2) for k in range(4)])


def _no_shift_zero():
    """3 x 6 without a shift 0: no local column."""
    return _matrix(3, 6, [(j, k, (7 * j + 11 * k + 1) % M) for j in range(3) for k in range(6) if (j + k) % 3 != 2])


def _dual_diagonal_4x8():
    """4 x 8 of the usual protograph shape, every row kept (the matrix of test_gpu_ms_m64_carry.py)"""
    return random_qc_code(np.random.RandomState(1811), 4, 8, M, [2, 3])


def _straddling_14x28():
    """14 x 28 of the usual protograph shape, heavy enough that the last block rows are not kept: a column of the dual diagonal has
    one edge in the last kept row and one in the first row that is not."""
    return random_qc_code(np.random.RandomState(1901), 14, 28, M, [5, 6, 4])


def _shipped():
    return relift(load_base_matrix(), M)


CODES = {"hand_written_3x6": _hand_written, "every_shift_zero_2x4": _every_shift_zero, "no_shift_zero_3x6": _no_shift_zero,
         "dual_diagonal_4x8": _dual_diagonal_4x8, "straddling_14x28": _straddling_14x28, "shipped_16x32": _shipped}


def local_columns(H):
    """ms_m64_local_col of ldpc_spec.hpp, restated"""
    out = []
    for k in range(H.shape[1]):
        rows = np.flatnonzero(H[:, k] >= 0)
        if rows.size and (H[rows, k] == 0).all() and rows[-1] - rows[0] <= SPAN:
            out.append(k)
    return out


def kept_rows(H):
    """ms_m64_keep_budget and ms_m64_keep_rows of ldpc_spec.hpp, restated: the edges of local columns are not counted"""
    rh, nh = H.shape
    loc = local_columns(H)
    w = [int((H[j] >= 0).sum()) for j in range(rh)]
    nl = [w[j] - sum(1 for k in loc if H[j, k] >= 0) for j in range(rh)]
    others = 5 * rh + 2 * min(nh, 24) + 2 * max(w)
    budget = max(KEEP_EDGES - max(others - (5 * 16 + 2 * 24 + 2 * 8), 0), 0)
    edges = rows = 0
    while rows < rh and edges + nl[rows] <= budget:
        edges += nl[rows]
        rows += 1
    return rows


def test_the_matrices_hold_what_they_are_meant_to_exercise():
    assert local_columns(_hand_written()) == [3, 5]
    assert local_columns(_every_shift_zero()) == [0, 1, 2, 3]
    assert local_columns(_no_shift_zero()) == [] and (_no_shift_zero() != 0).all()
    H = _dual_diagonal_4x8()
    assert local_columns(H)[:3] == [0, 1, 2] and 3 not in local_columns(H) and kept_rows(H) == 4
    H = _shipped()
    assert local_columns(H) == list(range(15)) and kept_rows(H) == 11
    H = _straddling_14x28()
    kr = kept_rows(H)
    assert 0 < kr < 14 and kr - 1 in local_columns(H) and H[kr - 1, kr - 1] == 0 and H[kr, kr - 1] == 0, kr
    # over the cap: a column of shifts 0 in block rows 0 and 4 is not local
    assert local_columns(_matrix(5, 2, [(0, 0, 0), (4, 0, 0), (1, 1, 3), (2, 1, 3), (3, 1, 0)])) == []
    # slots: the local edge last, in the middle and first
    H = _hand_written()
    slot = {j: [int(k) for k in np.flatnonzero(H[j] >= 0)] for j in range(3)}
    assert slot[0][-1] == 3 and 0 < slot[1].index(3) < len(slot[1]) - 1 and slot[1][-1] == 5 and 0 < slot[2].index(3) < len(slot[2]) - 1
    assert np.flatnonzero(_every_shift_zero()[0] >= 0)[0] in local_columns(_every_shift_zero())


def _signs(seed, shape):
    return np.where(np.random.RandomState(seed).randint(0, 2, size=shape) == 1, -1.0, 1.0)


def _inputs(H, no):
    """name -> LLRs [FRAMES, N]"""
    Hi = np.asarray(H, dtype=np.int32)
    N = H.shape[1] * M
    loc = local_columns(H)
    edge = 2.0 * _signs(1940 + no, (FRAMES, N))      # equal magnitudes everywhere: min1 == min2 in every check
    edge[1::2] *= np.where(np.arange(N) % 3 == 0, 0.5, 1.0)   # ... and on the edges of a local column, beside smaller ones elsewhere
    extreme = awgn_llr(Hi, M, 2.0, 1950 + no, FRAMES, burn_codeword=False)
    for f, val in enumerate([0.0, -0.0, 1e300, -1e300, 32767.0, -32768.5, 5e-324, -5e-324]):
        for k in loc:
            extreme[f, k * M:(k + 1) * M] = val                       # the whole local column
            extreme[f + 8, k * M:(k + 1) * M:2] = val                 # every other lane of it
    return {"awgn 0 dB": awgn_llr(Hi, M, 0.0, 1910 + no, FRAMES, burn_codeword=False),
            "awgn 2 dB": awgn_llr(Hi, M, 2.0, 1920 + no, FRAMES, burn_codeword=False),
            "adversarial": adversarial_llr(H, M, 30 + no)[0],
            "equal magnitudes": np.ascontiguousarray(edge),
            "+-0.0 and huge on local columns": np.ascontiguousarray(extreme),
            # 12 dB: the first iteration's hard decisions are a codeword; random signs on one magnitude: no iteration's are
            "both exits": np.concatenate([awgn_llr(Hi, M, 12.0, 1930 + no, FRAMES // 2, burn_codeword=False),
                                          3.0 * _signs(1936 + no, (FRAMES // 2, N))])}


def _expect_equal(dec, oracle, llr, maxiter, what, torch):
    d_ref, it_ref, _ = oracle.decode(MS_DEC, llr, maxiter, 0)
    s_ref, _, _ = oracle.decode(MS_DEC, llr, maxiter, 1)
    hard, iters, soft = dec.decode(torch.from_numpy(llr).cuda(), maxiter, want_soft=True)
    torch.cuda.synchronize()
    assert np.array_equal(iters.cpu().numpy(), it_ref), (what, iters.cpu().numpy(), it_ref)
    assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref)), what
    assert_bits_equal(soft.cpu().numpy(), s_ref, "soft values, " + what)
    return it_ref


@gpu
@pytest.mark.parametrize("case", list(CODES))
def test_ms_m64_with_local_columns_equals_the_oracle(case):
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
def test_local_columns_do_not_survive_into_the_next_frame_of_a_persistent_wave():
    """6144 frames of the 4 x 8 code, three times the 2048 resident waves of an MI355X: frames that converge at once alternate with
    frames that never do, so a wave starts a frame with the registers of a frame that stopped at another iteration."""
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H = _dual_diagonal_4x8()
    both = _inputs(H, list(CODES).index("dual_diagonal_4x8"))["both exits"]
    oracle = Oracle(H, M)
    d_ref, it_ref, _ = oracle.decode(MS_DEC, both, 50, 0)
    s_ref, _, _ = oracle.decode(MS_DEC, both, 50, 1)
    assert ((it_ref[:FRAMES // 2] >= 1) & (it_ref[:FRAMES // 2] <= 2)).all() and (it_ref[FRAMES // 2:] == -50).all(), it_ref
    idx = np.random.RandomState(1960).randint(0, FRAMES // 2, size=6144)
    idx[1::2] += FRAMES // 2   # even places: a frame that converges at once, odd places: one that never does
    with ldpc_lib_amd.LdpcHip(MS_DEC, H, M) as dec:
        assert "ms_m64_body" in dec.kernel_name and "hiprtc" in dec.kernel_name, dec.kernel_name
        hard, iters, soft = dec.decode(torch.from_numpy(both[idx]).cuda(), 50, want_soft=True)
        torch.cuda.synchronize()
    bad = np.flatnonzero(iters.cpu().numpy() != it_ref[idx])
    assert not bad.size, [(int(f), int(idx[f])) for f in bad[:8]]
    assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref)[idx])
    assert_bits_equal(soft.cpu().numpy(), s_ref[idx], "soft values")
