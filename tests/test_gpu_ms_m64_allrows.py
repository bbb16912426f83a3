"""GPU: STATE2 of ms_m64_body streams its channel loads over the block columns that are not local, and the body carries the block
rows that the registers freed by that allow.

Until now STATE2 issued the loads of 16 block columns at once and 8 more at each group of 8, local columns counted; behind a run of
local columns that bounded nothing.  Now the loads run over the non-local columns only (ms_m64_nonlocal_col of ldpc_spec.hpp):
the first min(DEPTH, count) together, then two at every second column, DEPTH ahead.  The registers no longer in flight go to carried
rows (ms_m64_carry_rows, restated as carry_rows below), while STATE3 of the widest row still fits (state3_regs).  What can go
wrong, and what this file aims at:

  - the stream's ends: no non-local column at all (an empty STATE2), 1, DEPTH - 1, DEPTH, DEPTH + 1 and 2 DEPTH + 1 of them, odd
    and even counts (the pairs), local columns in front of and between them (the n-th non-local column is not column n);
  - a code of 20 x 40 (more block columns than the old schedule's window of 24);
  - rows that had a record and are carried now: a 14 x 28, and a second 14 x 28 whose first row with a record is 8 wide and shares a local
    column with the last carried row; a 30 x 60 that carries no row under either rule; the shipped code (ahead-of-time instance,
    rows 0-14 of 16 carried);
  - AWGN at 0 and 2 dB and the adversarial LLRs of ldpc_testlib, maxiter 1, 2, 3 and 50, frames that stop at once and frames that
    never do;
  - several frames per wave of the persistent launch on the shipped instance.

Everything is compared with the CPU oracle bit for bit: hard decisions, signed iteration counts, soft values."""
import numpy as np
import pytest

from ldpc_testlib import MS_DEC, Oracle, adversarial_llr, assert_bits_equal, awgn_llr, pack_bits, random_qc_code
from test_gpu_ms_m64_carry import _expect_equal, _signs, _thirty_rows, _twenty_rows
from test_gpu_ms_m64_eqslot import AOT_NAME, _record_rows_last, _shipped, carried_rows
from test_gpu_ms_m64_local import _every_shift_zero, _matrix, local_columns

gpu = pytest.mark.gpu   # the tests that decode; those that only look at the matrices run anywhere

M = 64
FRAMES = 16
DEPTH = 8            # kMsM64YDepth
STATE3_REGS = 244    # kMsM64State3Regs


def nonlocal_columns(H):
    """ms_m64_nonlocal_col of ldpc_spec.hpp, restated: the block columns STATE2 loads, in ascending order"""
    loc = local_columns(H)
    return [k for k in range(H.shape[1]) if k not in loc]


def y_in_flight_r23(H):
    """ms_m64_y_in_flight_r23: the old schedule had the columns below k0 + 24 loaded when it reached k0 = 0, 8, 16, ..."""
    nl = set(nonlocal_columns(H))
    return max(sum(1 for k in range(k0, min(k0 + 24, H.shape[1])) if k in nl) for k0 in range(0, H.shape[1], 8))


def _keep_rows(H, budget):
    """ms_m64_keep_rows: whole rows in ascending order, 2 registers per edge that goes through LDS less the 5 of the record"""
    loc = local_columns(H)
    nl = [int((H[j] >= 0).sum()) - sum(1 for k in loc if H[j, k] >= 0) for j in range(H.shape[0])]
    edges = rows = 0
    while rows < H.shape[0] and 2 * (edges + nl[rows]) - 5 * (rows + 1) <= budget:
        edges += nl[rows]
        rows += 1
    return rows


def _keep_budget(H):
    """ms_m64_keep_budget (see carried_rows of test_gpu_ms_m64_eqslot.py)"""
    rh, nh = H.shape
    others = 5 * rh + 2 * min(nh, 24) + 2 * int((H >= 0).sum(axis=1).max())
    return max(2 * 68 - 5 * 13 - max(others - (5 * 16 + 2 * 24 + 2 * 8), 0), 0)


def state3_regs(H, rows):
    """ms_m64_state3_regs: 2 per edge of ANY kind in a carried row, 5 per record, v2c values and prefix minima of the widest row"""
    w = [int(x) for x in (H >= 0).sum(axis=1)]
    return 2 * sum(w[:rows]) + 5 * (H.shape[0] - rows) + 4 * max(w) - 2


def carry_rows(H, depth=DEPTH):
    """ms_m64_carry_rows: round 20's rows, then those that two registers per channel value no longer in flight pay for, while
    STATE3 fits"""
    base = _keep_rows(H, _keep_budget(H))
    assert base == carried_rows(H)
    back = max(y_in_flight_r23(H) - min(depth, len(nonlocal_columns(H))), 0)
    more = _keep_rows(H, _keep_budget(H) + 2 * back) if base > 0 else 0   # a code that carried no row still carries none
    rows = base
    while rows < more and state3_regs(H, rows + 1) <= STATE3_REGS:
        rows += 1
    return rows


def _stream_code(count):
    """3 x (count + 3): `count` rotated block columns, number i in block rows i mod 3 and (i + 1) mod 3, behind a local column in
    front (block rows 0-1), around a second one in their middle (block rows 1-2) and in front of a third (block row 0 alone)."""
    entries, k, mid = [(0, 0, 0), (1, 0, 0)], 1, count // 2
    for i in range(count + 1):
        if i == mid:
            entries += [(1, k, 0), (2, k, 0)]
            k += 1
        if i < count:
            entries += [(i % 3, k, (7 * i + 3) % 63 + 1), ((i + 1) % 3, k, (11 * i + 5) % 63 + 1)]
            k += 1
    return _matrix(3, count + 3, entries + [(0, k, 0)])


def _rows_carried_now_14x28():
    """14 x 28 of the usual protograph shape, 114 edges: rows 9-13 kept their record under round 20's rule"""
    return _record_rows_last()


def _eight_wide_boundary_14x28():
    """14 x 28 of the usual protograph shape whose first row with a record is 8 wide; the dual diagonal's column has an edge in it
    and one in the last carried row"""
    return random_qc_code(np.random.RandomState(BOUNDARY_SEED), 14, 28, M, [5, 6, 4])


BOUNDARY_SEED = 2663

CODES = {"no_column_streamed_2x4": _every_shift_zero,
         "one_column_streamed": lambda: _stream_code(1),
         "depth_less_one_streamed": lambda: _stream_code(DEPTH - 1),
         "depth_streamed": lambda: _stream_code(DEPTH),
         "depth_and_one_streamed": lambda: _stream_code(DEPTH + 1),
         "twice_depth_and_one_streamed": lambda: _stream_code(2 * DEPTH + 1),
         "twenty_rows_20x40": _twenty_rows,
         "rows_carried_now_14x28": _rows_carried_now_14x28,
         "eight_wide_boundary_14x28": _eight_wide_boundary_14x28,
         "no_row_carried_30x60": _thirty_rows,
         "shipped_16x32": _shipped}


def test_the_matrices_hold_what_they_are_meant_to_exercise():
    assert nonlocal_columns(_every_shift_zero()) == [] and carry_rows(_every_shift_zero()) == 2
    for count in (1, DEPTH - 1, DEPTH, DEPTH + 1, 2 * DEPTH + 1):
        H = _stream_code(count)
        nl = nonlocal_columns(H)
        assert len(nl) == count and len(local_columns(H)) == 3 and 0 in local_columns(H), count
        assert nl != list(range(count)) and int((H >= 0).sum(axis=1).max()) <= 16, count
        assert carry_rows(H) == 3, count
    H = _twenty_rows()
    assert H.shape == (20, 40) and len(nonlocal_columns(H)) == 21 and carried_rows(H) == 6 and carry_rows(H) == 10   # NH above the old window of 24
    H = _rows_carried_now_14x28()
    assert carried_rows(H) == 9 and carry_rows(H) > 9, carry_rows(H)
    H = _eight_wide_boundary_14x28()
    kr = carry_rows(H)
    assert carried_rows(H) < kr < 14 and int((H[kr] >= 0).sum()) == 8, (carried_rows(H), kr)
    assert kr - 1 in local_columns(H) and H[kr - 1, kr - 1] == 0 and H[kr, kr - 1] == 0   # a local column with an edge on each side
    assert carried_rows(_thirty_rows()) == 0 and carry_rows(_thirty_rows()) == 0
    H = _shipped()
    assert len(nonlocal_columns(H)) == 17 and nonlocal_columns(H)[0] == 15 and y_in_flight_r23(H) == 17
    assert carried_rows(H) == 13 and carry_rows(H) == 15
    assert (state3_regs(H, 15), state3_regs(H, 16)) == (243, 254)


def _inputs(H, no):
    """name -> LLRs"""
    Hi = np.asarray(H, dtype=np.int32)
    rh, nh = H.shape
    N = nh * M
    # the Es/N0 of a rate-1/2 code at Eb/N0 = 12 dB (a code of lower rate gets the difference on top): the first iteration's hard
    # decisions are a codeword; random signs on one magnitude: no iteration's are
    fast = awgn_llr(Hi, M, 12.0 + max(0.0, 10.0 * np.log10(0.5 * nh / max(nh - rh, 1))), 2530 + no, FRAMES // 2, burn_codeword=False)
    return {"awgn 0 dB": awgn_llr(Hi, M, 0.0, 2510 + no, FRAMES, burn_codeword=False),
            "awgn 2 dB": awgn_llr(Hi, M, 2.0, 2520 + no, FRAMES, burn_codeword=False),
            "adversarial": adversarial_llr(H, M, 80 + no)[0],
            "both exits": np.concatenate([fast, 3.0 * _signs(2540 + no, (FRAMES // 2, N))])}


def test_the_inputs_hold_what_they_are_meant_to_exercise():
    for no, (case, make) in enumerate(CODES.items()):
        H = make()
        for name, llr in _inputs(H, no).items():
            assert llr.shape[1] == H.shape[1] * M and 1 <= llr.shape[0] <= 256 and np.isfinite(llr).all(), (case, name)


@gpu
@pytest.mark.parametrize("case", list(CODES))
def test_ms_m64_with_streamed_channel_loads_equals_the_oracle(case):
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
                if name == "both exits" and maxiter == 50 and case != "no_column_streamed_2x4":
                    assert (it[:FRAMES // 2] >= 1).all() and (it[:FRAMES // 2] <= 2).sum() >= 6 and (it[FRAMES // 2:] == -50).all(), it


@gpu
def test_a_persistent_wave_of_the_shipped_instance_alternates_fast_and_never_converging_frames():
    """4096 frames, twice the 2048 resident waves of an MI355X: frames that converge at once alternate with frames that never do,
    so a wave starts a frame with the carried values of rows 13 and 14 and the channel values in flight of a frame that stopped at
    another iteration."""
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H = _shipped()
    both = _inputs(H, list(CODES).index("shipped_16x32"))["both exits"]
    oracle = Oracle(H, M)
    d_ref, it_ref, _ = oracle.decode(MS_DEC, both, 50, 0)
    s_ref, _, _ = oracle.decode(MS_DEC, both, 50, 1)
    assert ((it_ref[:FRAMES // 2] >= 1) & (it_ref[:FRAMES // 2] <= 2)).all() and (it_ref[FRAMES // 2:] == -50).all(), it_ref
    idx = np.random.RandomState(2599).randint(0, FRAMES // 2, size=4096)
    idx[1::2] += FRAMES // 2   # even places: a frame that converges at once, odd places: one that never does
    with ldpc_lib_amd.LdpcHip(MS_DEC, H, M) as dec:
        assert dec.kernel_name == AOT_NAME, dec.kernel_name
        hard, iters, soft = dec.decode(torch.from_numpy(both[idx]).cuda(), 50, want_soft=True)
        torch.cuda.synchronize()
        assert dec.last_launch() == AOT_NAME, dec.last_launch()
    bad = np.flatnonzero(iters.cpu().numpy() != it_ref[idx])
    assert not bad.size, [(int(f), int(idx[f])) for f in bad[:8]]
    assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref)[idx])
    assert_bits_equal(soft.cpu().numpy(), s_ref[idx], "soft values")
