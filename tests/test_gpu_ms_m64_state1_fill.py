"""GPU: ms_m64_body with part of STATE3's arithmetic among STATE1's LDS operations (kMsM64State1Fill of ldpc_spec.hpp).

A carried edge that goes through LDS holds x = keep * |alpha| from the moment it was scattered; a local column whose rows are all
carried and none of them a filter row (ms_m64_fill_col, restated below as fill_columns) has its sum, its soft value, its hard bit
and the v2c values of its edges formed in STATE1, and STATE3 takes them from `keep`.  Nothing may change: every result is compared
with the CPU oracle bit for bit -- hard words, signed iteration counts, soft values -- through both instances of one context, with
and without soft_out in turn.  What can go wrong, and what this file aims at:

  - which columns move: every column local with RH <= FR (2 x 4: none moves), local columns of degree 1 and 3 that touch a filter
    row (3 x 6: they stay), every row carried (4 x 8), 33 local columns whose bits fill two bit words in a new order (9 x 36),
    a dual-diagonal column that straddles the carried rows and stays in STATE3 between neighbours that move (14 x 28), a code that
    carries nothing (30 x 60: the body it had), a local column of span 3 behind the filter rows next to a column whose only edge
    is a FIRST store (6 x 8), and the shipped 16 x 32;
  - what a moved product sees: +-0.0, 1e300 and |y| at, just below and just above 32 767 on the local columns and on the columns
    of first-row edges -- the `+ 0.0` of the channel value and the sign of keep * |alpha|; alpha 0.8, 0.5 and 1.25;
  - the first iterations, where keep is still +0.0 or has been x / tt exactly once: maxiter 1, 2, 3; and 50;
  - all-positive frames, which leave through the on-demand pass at iteration 1 and read what STATE1 wrote for the moved columns;
  - 4096 frames through the persistent launch of both shipped instances, fast and never-converging frames in turn: a wave's next
    frame starts from keep = +0.0, not from the x / tt of the frame before."""
import functools

import numpy as np
import pytest

from ldpc_testlib import MS_DEC, Oracle, adversarial_llr, assert_bits_equal, awgn_llr, pack_bits
from test_gpu_ms_m64_allrows import carry_rows
from test_gpu_ms_m64_carry import _all_rows_kept, _thirty_rows
from test_gpu_ms_m64_eqslot import _record_rows_last
from test_gpu_ms_m64_local import AOT_NAME, _every_shift_zero, _hand_written, _matrix, _shipped, _signs, local_columns
from test_gpu_ms_m64_resident import _code, _expect_equal_both_ways, _without_soft

gpu = pytest.mark.gpu   # the tests that decode; those that only look at the matrices and the inputs run anywhere

M = 64
FRAMES = 16
FILTER_ROWS = 2   # kMsM64FilterRows
KMAX = 32767.0    # kMaxVal


def _span_three_and_first_only():
    """6 x 8, every row carried.  Block column 0: local, rows 2 and 5 (span 3, the cap), behind the filter rows; 6: local, degree 3,
    rows 2-4; 3: local in the two filter rows; 1: rotated, one edge -- its only LDS operation is a FIRST store; the others rotated,
    degree 3."""
    return _matrix(6, 8, [(2, 0, 0), (5, 0, 0), (3, 1, 21), (0, 2, 5), (1, 2, 9), (4, 2, 60), (0, 3, 0), (1, 3, 0),
                          (1, 4, 33), (2, 4, 7), (3, 4, 1), (0, 5, 12), (4, 5, 3), (5, 5, 50), (2, 6, 0), (3, 6, 0), (4, 6, 0),
                          (0, 7, 40), (3, 7, 63), (5, 7, 17)])


CODES = {"every_column_local_2x4": _every_shift_zero,
         "hand_written_3x6": _hand_written,
         "every_row_carried_4x8": _all_rows_kept,
         "two_bit_words_9x36": lambda: _code(36, 33, rh=9),
         "record_rows_last_14x28": _record_rows_last,
         "no_row_carried_30x60": _thirty_rows,
         "span_three_and_first_only_6x8": _span_three_and_first_only,
         "shipped_16x32": _shipped}


def filter_rows(H):
    """ms_m64_filter_rows"""
    return min(FILTER_ROWS, H.shape[0])


def fill_columns(H):
    """ms_m64_fill_col(k, KR, FR): a local column, every row of it carried, none of them a filter row"""
    kr, fr = carry_rows(H), filter_rows(H)
    out = []
    for k in local_columns(H):
        rows = np.flatnonzero(H[:, k] >= 0)
        if rows[-1] < kr and rows[0] >= fr:
            out.append(k)
    return out


def first_store_columns(H):
    """block columns that go through LDS, with their first block row: that edge is a plain store in STATE1"""
    loc = local_columns(H)
    return [k for k in range(H.shape[1]) if k not in loc and (H[:, k] >= 0).any()]


def test_the_matrices_hold_what_they_are_meant_to_exercise():
    got = {case: (make().shape, carry_rows(make()), len(local_columns(make())), fill_columns(make())) for case, make in CODES.items()}
    assert got["every_column_local_2x4"] == ((2, 4), 2, 4, [])                       # RH <= FR
    assert got["hand_written_3x6"][:3] == ((3, 6), 3, 2) and got["hand_written_3x6"][3] == []   # degree 1 and 3, both in a filter row
    H = _all_rows_kept()
    assert got["every_row_carried_4x8"][:2] == ((4, 8), 4) and fill_columns(H) and set(fill_columns(H)) < set(local_columns(H))
    shape, kr, nloc, fill = got["two_bit_words_9x36"]
    assert (shape, kr, nloc) == ((9, 36), 9, 33) and len(fill) > 0 and len(fill) < 33   # two words, moved and unmoved columns in both orders
    H = _record_rows_last()
    kr = carry_rows(H)
    assert H.shape == (14, 28) and 2 < kr < 14, kr
    # the dual diagonal: column kr - 1 has an edge in the last carried row and one in the first row with a record, and stays;
    # its neighbours below move
    assert kr - 1 in local_columns(H) and H[kr - 1, kr - 1] == 0 and H[kr, kr - 1] == 0 and kr - 1 not in fill_columns(H)
    assert kr - 2 in fill_columns(H) and kr - 3 in fill_columns(H), (kr, fill_columns(H))
    assert got["no_row_carried_30x60"][1] == 0 and got["no_row_carried_30x60"][3] == []
    H = _span_three_and_first_only()
    assert carry_rows(H) == 6 and local_columns(H) == [0, 3, 6] and fill_columns(H) == [0, 6]
    assert np.flatnonzero(H[:, 0] >= 0).tolist() == [2, 5] and int((H[:, 1] >= 0).sum()) == 1 and H[3, 1] > 0
    H = _shipped()
    assert carry_rows(H) == 15 and local_columns(H) == list(range(15)) and fill_columns(H) == list(range(2, 14))


def _extremes(H, seed):
    """FRAMES frames at 2 dB with +-0.0, +-1e300 and |y| at, just below and just above 32 767 on the local columns and on the columns
    that go through LDS (each has a first-row edge): the whole column on the first eight... frames, every other lane after that"""
    Hi = np.asarray(H, dtype=np.int32)
    y = awgn_llr(Hi, M, 2.0, seed, FRAMES, burn_codeword=False)
    below, above = np.nextafter(KMAX, 0.0), np.nextafter(KMAX, np.inf)
    vals = [0.0, -0.0, 1e300, -1e300, KMAX, -KMAX, below, -above]
    cols = local_columns(H), first_store_columns(H)
    for f, val in enumerate(vals):
        for k in cols[f % 2] + cols[1 - f % 2][::3]:
            y[f, k * M:(k + 1) * M] = val                      # the whole column
            y[f + 8, k * M + (f % 2):(k + 1) * M:2] = -val     # every other lane of it, the other sign
    return np.ascontiguousarray(y)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """name -> LLRs [FRAMES, N]; computed once per case"""
    H = CODES[case]()
    no = list(CODES).index(case)
    Hi = np.asarray(H, dtype=np.int32)
    out = {"awgn 0 dB": awgn_llr(Hi, M, 0.0, 3310 + no, FRAMES, burn_codeword=False),
           "awgn 2 dB": awgn_llr(Hi, M, 2.0, 3320 + no, FRAMES, burn_codeword=False),
           "adversarial": np.ascontiguousarray(adversarial_llr(H, M, 330 + no)[0]),
           "extremes on local and first-row columns": _extremes(H, 3330 + no),
           "all positive": np.abs(awgn_llr(Hi, M, 2.0, 3340 + no, FRAMES, burn_codeword=False)) + 0.5}
    for v in out.values():
        assert v.shape[1] == H.shape[1] * M
        v.setflags(write=False)
    return out


def test_the_inputs_hold_what_they_are_meant_to_exercise():
    for case in CODES:
        H = CODES[case]()
        ins = _inputs(case)
        assert all(np.isfinite(v).all() and 1 <= v.shape[0] <= 256 for v in ins.values()), case
        assert (Oracle(H, M).decode(MS_DEC, ins["all positive"], 50, 0)[1] == 1).all(), case
        ex = ins["extremes on local and first-row columns"]
        seen = set()
        for k in local_columns(H) + first_store_columns(H):
            col = ex[:, k * M:(k + 1) * M]
            seen |= {(float(abs(v)), bool(np.signbit(v))) for v in col[:8, 0]} | {(float(abs(v)), bool(np.signbit(v))) for v in col[8:, 1]}
        for mag in (0.0, 1e300, KMAX, np.nextafter(KMAX, 0.0), np.nextafter(KMAX, np.inf)):
            assert any(m == mag for m, _ in seen), (case, mag)
        assert (0.0, True) in seen and (0.0, False) in seen, case


def _expect_equal_at_alpha(dec, oracle, llr, maxiter, alpha, what, torch):
    """_expect_equal_both_ways at a normalisation factor other than the default"""
    d_ref, it_ref, _ = oracle.decode(MS_DEC, llr, maxiter, 0, alpha=alpha)
    s_ref, _, _ = oracle.decode(MS_DEC, llr, maxiter, 1, alpha=alpha)
    x = torch.from_numpy(np.array(llr)).cuda()
    for want_soft in (False, True):
        hard, iters, soft = dec.decode(x, maxiter, alpha=alpha, want_soft=want_soft)
        torch.cuda.synchronize()
        assert _without_soft(dec) == (0 if want_soft else 1), (what, want_soft)
        assert np.array_equal(iters.cpu().numpy(), it_ref), (what, want_soft, iters.cpu().numpy(), it_ref)
        assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref)), (what, want_soft)
        if want_soft:
            assert_bits_equal(soft.cpu().numpy(), s_ref, "soft values, " + what)
    return it_ref


@gpu
@pytest.mark.parametrize("case", list(CODES))
def test_ms_m64_with_state1_filled_equals_the_oracle_with_and_without_soft_values(case):
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H = CODES[case]()
    oracle = Oracle(H, M)
    seen = []
    with ldpc_lib_amd.LdpcHip(MS_DEC, H, M) as dec:   # one context: each hiprtc instance is compiled once
        if case == "shipped_16x32":
            assert dec.kernel_name == AOT_NAME, dec.kernel_name
        else:
            assert "ms_m64_body" in dec.kernel_name and "hiprtc" in dec.kernel_name, dec.kernel_name
        for name, llr in _inputs(case).items():
            for maxiter in (1, 2, 3, 50):
                it = _expect_equal_both_ways(dec, oracle, llr, maxiter, f"{case}, {name}, maxiter {maxiter}", torch)
                seen.append(it)
                print(case, name, "maxiter", maxiter, "iterations", it.tolist())
        for alpha in (0.5, 1.25):   # one pass each
            for name in ("awgn 2 dB", "extremes on local and first-row columns"):
                seen.append(_expect_equal_at_alpha(dec, oracle, _inputs(case)[name], 50, alpha, f"{case}, {name}, alpha {alpha}", torch))
        assert dec.last_launch() == dec.kernel_name
    seen = np.concatenate(seen)
    assert (seen > 0).any() and (seen < 0).any(), "both exits of the iteration loop"


@gpu
def test_a_persistent_wave_of_the_shipped_instances_starts_its_next_frame_from_zero_keep():
    """4096 frames, twice the 2048 resident waves of an MI355X: frames that converge at iteration 1 in turn with frames that never
    do.  After a never-converging frame keep holds x and tt of its last iteration; after a fast one, of its first."""
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H = _shipped()
    N = H.shape[1] * M
    both = np.concatenate([_inputs("shipped_16x32")["all positive"][:FRAMES // 2], 3.0 * _signs(3399, (FRAMES // 2, N))])
    oracle = Oracle(H, M)
    d_ref, it_ref, _ = oracle.decode(MS_DEC, both, 50, 0)
    s_ref, _, _ = oracle.decode(MS_DEC, both, 50, 1)
    assert (it_ref[:FRAMES // 2] == 1).all() and (it_ref[FRAMES // 2:] == -50).all(), it_ref
    idx = np.random.RandomState(3398).randint(0, FRAMES // 2, size=4096)
    idx[1::2] += FRAMES // 2   # even places: a frame that converges at once, odd places: one that never does
    x = torch.from_numpy(both[idx]).cuda()
    with ldpc_lib_amd.LdpcHip(MS_DEC, H, M) as dec:
        assert dec.kernel_name == AOT_NAME, dec.kernel_name
        for want_soft in (False, True):
            hard, iters, soft = dec.decode(x, 50, want_soft=want_soft)
            torch.cuda.synchronize()
            assert dec.last_launch() == AOT_NAME and _without_soft(dec) == (0 if want_soft else 1), (dec.last_launch(), want_soft)
            bad = np.flatnonzero(iters.cpu().numpy() != it_ref[idx])
            assert not bad.size, (want_soft, [(int(f), int(idx[f])) for f in bad[:8]])
            assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref)[idx]), want_soft
            if want_soft:
                assert_bits_equal(soft.cpu().numpy(), s_ref[idx], "soft values")
