"""CPU: ms_m64_body carries the decoded check-to-variable values of its first block rows and finds the min1 slot by value equality.

(a) The argument next to `keep` in ms_m64_body, as executable text.  STATE3 of a block row ends with the two smallest magnitudes
    nm1 <= nm2 of the row, clamped at K = 32767.  A row with a record stores the slot npos of nm1 (the last slot whose strict
    compare v < nm1 held, or 0) and the next iteration decodes  mag[s] = (s == npos) ? nm2 : nm1.  A carried row stores no slot:
    mag[s] = (|tt[s]| == nm1) ? nm2 : nm1  while the row's |tt| are still in registers.  Both decodes are restated here with an
    fmin / fmax that drop NaNs and a strict <, and compared byte for byte: exhaustively for row widths 1-4 over eleven values
    around everything the argument names (+0.0, the smallest denormal, neighbours of 1.0 and of K, K itself, 1e300, inf, NaN), and
    on a seeded random sweep of widths 1-16 over the same values, where ties of every order are the rule.

(b) The cross-compiled shipped instance and the hand-written 3 x 6 of test_gpu_ms_m64_local.py, built as
    tests/test_ms_m64_local_cpu.py builds them: no spilled VGPR, no scratch, at most 256 VGPRs, the number of ds_add_f64
    unchanged (65 and 5), and the header's count of carried rows is the one test_gpu_ms_m64_eqslot.py restates."""
import itertools
import re

import numpy as np
import pytest

from test_gpu_ms_m64_eqslot import carried_rows
from test_gpu_ms_m64_local import CODES
from test_ms_m64_local_cpu import _atomics_expected, _code_struct, _compile, _metadata, needs_hipcc

K = 32767.0
VALUES = np.array([0.0, 5e-324, 1.0, np.nextafter(1.0, 2.0), 2.0, np.nextafter(K, 0.0), K, np.nextafter(K, np.inf), 1e300, np.inf,
                   np.nan])


def _two_smallest(v):
    """STATE3's min loop over the rows of v [rows, width]: (nm1, nm2, npos).  np.fmin / np.fmax return the other operand when one is
    a NaN, as v_min_f64 / v_max_f64 do; < is false on a NaN."""
    n, w = v.shape
    nm1 = np.fmin(v[:, 0], K)              # slot 0: from nm1 = nm2 = K only nm1 moves
    nm2 = np.full(n, K)
    npos = np.zeros(n, dtype=np.int64)
    for s in range(1, w):
        with np.errstate(invalid="ignore"):
            c1 = v[:, s] < nm1
        nm2 = np.fmin(np.fmax(v[:, s], nm1), nm2)
        npos = np.where(c1, s, npos)
        nm1 = np.fmin(v[:, s], nm1)
    return nm1, nm2, npos


def _decode_by_slot(v):
    nm1, nm2, npos = _two_smallest(v)
    return np.where(np.arange(v.shape[1])[None, :] == npos[:, None], nm2[:, None], nm1[:, None])


def _decode_by_equality(v):
    nm1, nm2, _ = _two_smallest(v)
    with np.errstate(invalid="ignore"):
        e = v == nm1[:, None]              # ordered equality: false on a NaN
    return np.where(e, nm2[:, None], nm1[:, None])


def _assert_same_bytes(v):
    a, b = np.ascontiguousarray(_decode_by_slot(v)), np.ascontiguousarray(_decode_by_equality(v))
    bad = np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)).any(axis=1))
    assert not bad.size, (v[bad[0]], a[bad[0]], b[bad[0]])
    assert a.tobytes() == b.tobytes()
    assert not np.isnan(a).any() and (a <= K).all()   # the magnitudes a record may hold


def test_the_restated_min_and_max_drop_nans():
    assert np.fmin(np.nan, 1.0) == 1.0 and np.fmax(np.nan, 1.0) == 1.0 and np.fmin(2.0, np.nan) == 2.0
    nm1, nm2, npos = _two_smallest(np.array([[np.nan, 3.0, 2.0, 2.0, np.nan]]))
    assert (nm1[0], nm2[0], npos[0]) == (2.0, 2.0, 2)   # strict <: the first of two equal minima keeps the slot


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_decode_by_equality_is_decode_by_slot_exhaustively(width):
    v = np.array(list(itertools.product(VALUES, repeat=width)))
    assert v.shape == (11 ** width, width)
    _assert_same_bytes(v)


def test_decode_by_equality_is_decode_by_slot_on_a_random_sweep():
    rng = np.random.RandomState(2001)
    rows = 0
    for width in range(1, 17):
        v = VALUES[rng.randint(0, VALUES.size, size=(12500, width))]
        _assert_same_bytes(v)
        rows += v.shape[0]
    assert rows == 200000


@needs_hipcc
@pytest.mark.parametrize("case", ["shipped_16x32", "hand_written_3x6"])
def test_carried_rows_fit_the_registers_and_change_no_atomic(case, tmp_path):
    H = CODES[case]()
    name = "ldpc_spec::CodeAppendixCM64" if case == "shipped_16x32" else "Code"
    rule = (f"static_assert(ldpc_spec::ms_m64_keep_rows<{name}>(ldpc_spec::ms_m64_keep_budget<{name}>()) == {carried_rows(H)}, "
            "\"carried block rows\");\n")
    asm = _compile(tmp_path, ("" if case == "shipped_16x32" else _code_struct(H)) + rule, name, H)
    got = {k: _metadata(asm, k) for k in (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size")}
    adds = len(re.findall(r"^\s+ds_add_f64\s", asm, re.M))
    print(got, "ds_add_f64", adds)
    assert got[".vgpr_spill_count"] == 0, got
    assert got[".private_segment_fixed_size"] == 0, got
    assert got[".vgpr_count"] <= 256, got
    assert adds == _atomics_expected(H) == {"shipped_16x32": 65, "hand_written_3x6": 5}[case], adds
