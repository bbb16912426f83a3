"""GPU: ms_m64_body forms the syndrome of its first block rows only, and the rest on demand.

Block rows [0, FR) -- the FILTER ROWS, ms_m64_filter_rows of ldpc_spec.hpp, restated below -- form their syndrome word inside STATE3
as every row did.  When one of their checks fails the iteration is not converged and nothing else is looked at.  Only when they
all pass does the wave look at the checks of rows [FR, RH): a cold pass that takes the signs of a block column as one lane mask (a
ballot over the high dword of the lane's own image slot, or over the column's bit of the bit word in the instance without soft
values), rotates it per edge on the scalar unit and leaves at the first group of block rows with a failing check.  What can go
wrong, and what this file aims at:

  - the rule's ends: a 2 x 4 with RH <= FR (no pass at all), codes with many rows past the filter;
  - every source of a sign: a rotated and an unrotated edge of a column that goes through LDS, a local column of degree 1 and 3,
    33 local columns (two bit words), in rows past FR -- through both instances in one context, with and without soft_out in turn;
  - rows that carry values and rows that keep records behind the filter (14 x 28), a code that carries no row (30 x 60);
  - frames that enter the pass: all-positive frames converge at iteration 1 THROUGH the pass; FILTER-BLIND frames -- every filter
    row satisfied, a later row not -- with the wrong variables so strong that the frame enters the pass in every iteration up to
    maxiter, and so weak that it converges in between;
  - the rotation's direction and the column -> mask bookkeeping: a wrong bit anywhere stops a frame early or never, and the signed
    iteration count says so;
  - 4096 frames through the persistent launch of both shipped instances, all-positive and filter-blind never-converging frames in
    turn: a wave's next frame starts from nothing of the one before.

Everything is compared with the CPU oracle bit for bit: hard decisions, signed iteration counts, soft values where requested."""
import functools

import numpy as np
import pytest

from ldpc_testlib import MS_DEC, Oracle, adversarial_llr, assert_bits_equal, awgn_llr, pack_bits
from test_gpu_ms_m64_carry import _thirty_rows
from test_gpu_ms_m64_eqslot import _record_rows_last, carried_rows
from test_gpu_ms_m64_local import AOT_NAME, _every_shift_zero, _hand_written, _shipped, local_columns
from test_gpu_ms_m64_resident import _code, _expect_equal_both_ways, _without_soft, local_bits

gpu = pytest.mark.gpu   # the tests that decode; those that only look at the matrices and the inputs run anywhere

M = 64
FRAMES = 16
FILTER_ROWS = 2   # kMsM64FilterRows
EXIT_ROWS = 4     # kMsM64ExitRows: the pass can leave after every group of so many block rows
BIG = 8.0         # the magnitude of a filter-blind frame's right variables


def filter_rows(H):
    """ms_m64_filter_rows: the same count for every code, all rows of a code that has no more"""
    return min(FILTER_ROWS, H.shape[0])


def blind_columns(H, groups=0):
    """block columns without an edge in a filter row, nor in the first `groups` exit groups of the pass"""
    rows = filter_rows(H) + groups * EXIT_ROWS
    return [k for k in range(H.shape[1]) if (H[:rows, k] < 0).all() and (H[:, k] >= 0).any()]


CODES = {"no_pass_2x4": _every_shift_zero,
         "hand_written_3x6": _hand_written,
         "two_bit_words_9x36": lambda: _code(36, 33, rh=9),
         "record_rows_last_14x28": _record_rows_last,
         "no_row_carried_30x60": _thirty_rows,
         "shipped_16x32": _shipped}
# every block column of these has an edge in a filter row: no frame can be filter-blind
NOT_BLIND = ("no_pass_2x4", "hand_written_3x6")
# most of its columns have one edge, so it has codewords of weight 2: the decoder answers a variable that cannot move by moving its
# neighbour, and what the oracle says about a filter-blind frame's iterations is compared but not prescribed
TINY_CODEWORDS = ("two_bit_words_9x36",)


def syndrome(H, y):
    """[frames, RH, M] of 0 / 1: what the first iteration's vote sees, from H and the signs of y alone (the c2v values start at
    zero, so the soft values of iteration 1 are the channel values).  Check n of block row j meets variable (n + c) mod M of a
    block column with shift c."""
    rh, nh = H.shape
    neg = (np.asarray(y) < 0).reshape(-1, nh, M)
    s = np.zeros((neg.shape[0], rh, M), dtype=np.uint8)
    for j in range(rh):
        for k in np.flatnonzero(H[j] >= 0):
            s[:, j] ^= np.roll(neg[:, k], -int(H[j, k]), axis=1)
    return s


def _blind(H, seed):
    """FRAMES filter-blind frames: +BIG everywhere (the all-zero codeword), a few variables of blind columns with the wrong sign --
    on the even frames by a magnitude no message ever outweighs, on the odd ones by one the first messages already do.  Every
    fourth frame takes them from columns that the first exit group of the pass does not see either, where the code has such: the
    pass goes through its first exit, forms the masks of a later group and leaves there."""
    rng = np.random.RandomState(seed)
    nh = H.shape[1]
    y = np.full((FRAMES, nh * M), BIG)
    for f in range(FRAMES):
        cols = (f % 4 == 0 and blind_columns(H, 1)) or blind_columns(H)
        for k in rng.choice(cols, size=min(len(cols), 1 + f % 3), replace=False):
            lanes = rng.choice(M, size=1 + (f // 2) % 4, replace=False)
            y[f, k * M + lanes] = -1e9 if f % 2 == 0 else -BIG / 16
    return y


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """name -> LLRs [<= 256, N]; computed once per case"""
    H = CODES[case]()
    no = list(CODES).index(case)
    Hi = np.asarray(H, dtype=np.int32)
    N = H.shape[1] * M
    out = {"awgn 0 dB": awgn_llr(Hi, M, 0.0, 3210 + no, FRAMES, burn_codeword=False),
           "awgn 2 dB": awgn_llr(Hi, M, 2.0, 3220 + no, FRAMES, burn_codeword=False),
           "adversarial": np.ascontiguousarray(adversarial_llr(H, M, 320 + no)[0]),
           "all positive": np.abs(awgn_llr(Hi, M, 2.0, 3230 + no, FRAMES, burn_codeword=False)) + 0.5}
    if case not in NOT_BLIND:
        out["filter-blind"] = _blind(H, 3240 + no)
    for v in out.values():
        assert v.shape[1] == N
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(case, name, maxiter):
    """the oracle's signed iteration counts, once per (case, input, maxiter)"""
    it = Oracle(CODES[case](), M).decode(MS_DEC, _inputs(case)[name], maxiter, 0)[1]
    it.setflags(write=False)
    return it


def test_the_matrices_hold_what_they_are_meant_to_exercise():
    got = {case: (H.shape, filter_rows(H), len(blind_columns(H))) for case, H in ((c, make()) for c, make in CODES.items())}
    assert {c: g[:2] for c, g in got.items()} == {"no_pass_2x4": ((2, 4), 2), "hand_written_3x6": ((3, 6), 2), "two_bit_words_9x36": ((9, 36), 2),
                                                  "record_rows_last_14x28": ((14, 28), 2), "no_row_carried_30x60": ((30, 60), 2),
                                                  "shipped_16x32": ((16, 32), 2)}, got
    for case, (_, _, blind) in got.items():
        assert (blind == 0) == (case in NOT_BLIND), (case, blind)
    assert sum(1 for case in CODES if case not in NOT_BLIND + TINY_CODEWORDS) >= 3 and "shipped_16x32" not in NOT_BLIND + TINY_CODEWORDS
    # rows past the filter of the hand-written code: a rotated and an unrotated edge through LDS, a local column of degree 3 and of degree 1
    H = _hand_written()
    assert filter_rows(H) == 2 and H[2, 0] == 5 and H[2, 2] == 40 and H[2, 3] == 0 and local_columns(H) == [3, 5] and H[1, 5] == 0
    H = CODES["two_bit_words_9x36"]()
    assert max(w for w, _ in local_bits(H).values()) == 1
    assert {w for k, (w, _) in local_bits(H).items() if (H[2:, k] >= 0).any()} == {0, 1}   # both words are read behind the filter
    assert any(H[j, k] > 0 for j in range(2, 9) for k in range(36))                        # and a rotated edge
    H = _record_rows_last()
    assert 2 < carried_rows(H) < 14             # carried rows and rows with a record behind the filter
    assert carried_rows(_thirty_rows()) == 0


def test_the_inputs_hold_what_they_are_meant_to_exercise():
    for case in CODES:
        H = CODES[case]()
        fr = filter_rows(H)
        ins = _inputs(case)
        assert all(np.isfinite(v).all() and v.shape[1] == H.shape[1] * M and 1 <= v.shape[0] <= 256 for v in ins.values()), case
        assert not syndrome(H, ins["all positive"]).any(), case
        assert (_reference(case, "all positive", 50) == 1).all(), case   # through the pass, where there is one
        if case in NOT_BLIND:
            assert "filter-blind" not in ins
            continue
        s = syndrome(H, ins["filter-blind"])
        assert not s[:, :fr].any(), case
        assert s[:, fr:].reshape(FRAMES, -1).any(axis=1).all(), case
        if H.shape[0] > fr + EXIT_ROWS:   # among the frames that never converge: the first exit of the pass taken, and passed
            first, later = s[0::2, fr:fr + EXIT_ROWS].reshape(FRAMES // 2, -1).any(axis=1), s[0::2, fr + EXIT_ROWS:].reshape(FRAMES // 2, -1).any(axis=1)
            assert first.any() and (~first & later).any(), (case, first, later)
        for maxiter in (1, 2, 3, 50) if case not in TINY_CODEWORDS else ():
            it = _reference(case, "filter-blind", maxiter)
            assert (np.abs(it[0::2]) == maxiter).all() and (it[0::2] < 0).all(), (case, maxiter, it)   # the pass in every iteration
            if maxiter >= 3:
                assert ((it[1::2] >= 2) & (it[1::2] < maxiter)).all(), (case, maxiter, it)
            else:   # too few iterations for an iteration in between: they converge at the second, if there is one
                assert (it[1::2] == (2 if maxiter == 2 else -1)).all(), (case, maxiter, it)


@gpu
@pytest.mark.parametrize("case", list(CODES))
def test_ms_m64_with_the_syndrome_on_demand_equals_the_oracle_with_and_without_soft_values(case):
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H = CODES[case]()
    oracle = Oracle(H, M)
    seen = []
    with ldpc_lib_amd.LdpcHip(MS_DEC, H, M) as dec:
        if case == "shipped_16x32":
            assert dec.kernel_name == AOT_NAME, dec.kernel_name
        else:
            assert "ms_m64_body" in dec.kernel_name and "hiprtc" in dec.kernel_name, dec.kernel_name
        for name, llr in _inputs(case).items():
            for maxiter in (1, 2, 3, 50):
                it = _expect_equal_both_ways(dec, oracle, llr, maxiter, f"{case}, {name}, maxiter {maxiter}", torch)
                seen.append(it)
                print(case, name, "maxiter", maxiter, "iterations", it.tolist())
        assert dec.last_launch() == dec.kernel_name
    seen = np.concatenate(seen)
    assert (seen > 0).any() and (seen < 0).any(), "both exits of the iteration loop"


@gpu
def test_a_persistent_wave_of_the_shipped_instances_enters_the_pass_anew_in_its_next_frame():
    """4096 frames, twice the 2048 resident waves of an MI355X: all-positive frames, which leave through the pass at iteration 1, in
    turn with filter-blind frames that never converge and enter the pass in all 50 iterations.  A wave's next frame must start
    from nothing of the one before: no lane mask, no bit word, no vote."""
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H = _shipped()
    both = np.concatenate([_inputs("shipped_16x32")["all positive"][:FRAMES // 2], _inputs("shipped_16x32")["filter-blind"][0::2]])
    oracle = Oracle(H, M)
    d_ref, it_ref, _ = oracle.decode(MS_DEC, both, 50, 0)
    s_ref, _, _ = oracle.decode(MS_DEC, both, 50, 1)
    assert (it_ref[:FRAMES // 2] == 1).all() and (it_ref[FRAMES // 2:] == -50).all(), it_ref
    idx = np.random.RandomState(3299).randint(0, FRAMES // 2, size=4096)
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
