"""CPU: the carried block rows of ms_m64_body form their check-to-variable magnitudes from prefix and suffix minima.

(a) The argument next to `keep` in ms_m64_body, as executable text.  The magnitude of the c2v value on slot s of a row is
    min(K, min over s' != s of v[s']), K = 32767, v = |v2c|.  Three ways to get it are restated here with an fmin that drops NaNs
    (np.fmin, as v_min_f64 does) and compared byte for byte:
      - by slot: the record's decode (s == npos) ? nm2 : nm1 of test_ms_m64_eqslot_cpu.py;
      - by prefix and suffix minima, exactly as the body builds them: pf[0] = fmin(v_0, K), pf[s] = fmin(v_s, pf[s - 1]) up to
        s = RW - 2, then descending s with suf = K: mag[RW - 1] = pf[RW - 2], mag[s] = fmin(pf[s - 1], suf), mag[0] = suf,
        suf = fmin(v_s, suf) after every slot s > 0; a row of width 1 gives K;
      - the reference's rule: val clamped with `> K`, `if (val < min1) ... else if (val < min2)`, decode by pos.
    The first two agree on every NaN-free row (exhaustively for widths 1-4 over ten values, and on a seeded sweep of 200 000 rows of
    width 1-16).  The last two agree on every row, NaN included (exhaustively for widths 1-4 over eleven values): a NaN moves
    nothing in the reference and is dropped by every fmin here.  (The min / max chain of the rows with a record turns a NaN into a
    copy of the running min1 instead; no decoder input holds a NaN)

(b) The cross-compiled shipped instance, the hand-written 3 x 6 of test_gpu_ms_m64_local.py and the 3 x 16 with a row of weight
    16 of test_gpu_ms_m64_carry.py, built as tests/test_ms_m64_local_cpu.py builds them: no spilled VGPR, no scratch, at most 256
    VGPRs, the number of ds_add_f64 unchanged, and -- every carried row of the shipped instance takes the new form -- no
    v_cmp_eq_f64 left in its kernel."""
import itertools
import re

import numpy as np
import pytest

from test_gpu_ms_m64_carry import _slot_matrix
from test_gpu_ms_m64_eqslot import carried_rows
from test_gpu_ms_m64_local import CODES
from test_gpu_ms_m64_prefix import prefix_rows
from test_ms_m64_eqslot_cpu import VALUES, K, _decode_by_slot, _two_smallest
from test_ms_m64_local_cpu import _atomics_expected, _code_struct, _compile, _metadata, needs_hipcc

NAN_FREE = VALUES[~np.isnan(VALUES)]


def _decode_by_prefix_suffix(v):
    """the magnitudes of a carried row as ms_m64_body forms them, v [rows, width]"""
    n, w = v.shape
    mag = np.empty((n, w))
    if w == 1:
        mag[:, 0] = K
        return mag
    pf = np.empty((n, w - 1))
    pf[:, 0] = np.fmin(v[:, 0], K)
    for s in range(1, w - 1):
        pf[:, s] = np.fmin(v[:, s], pf[:, s - 1])
    suf = np.full(n, K)
    for s in range(w - 1, -1, -1):
        if s == w - 1:
            mag[:, s] = pf[:, w - 2]
        elif s == 0:
            mag[:, s] = suf
        else:
            mag[:, s] = np.fmin(pf[:, s - 1], suf)
        if s > 0:
            suf = np.fmin(v[:, s], suf)
    return mag


def _decode_by_reference_rule(v):
    """decoders.cpp: val = (val > K) ? K : val;  if (val < min1) { pos = k; min2 = min1; min1 = val; } else if (val < min2)
    min2 = val;  from min1 = min2 = K, pos = 0; the next iteration reads (pos == k) ? min2 : min1.  Every compare is false on a NaN."""
    n, w = v.shape
    min1, min2, pos = np.full(n, K), np.full(n, K), np.zeros(n, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for k in range(w):
            val = np.where(v[:, k] > K, K, v[:, k])
            a = val < min1
            b = ~a & (val < min2)
            min2 = np.where(a, min1, np.where(b, val, min2))
            min1 = np.where(a, val, min1)
            pos = np.where(a, k, pos)
    return np.where(np.arange(w)[None, :] == pos[:, None], min2[:, None], min1[:, None])


def _assert_same_bytes(a, b, v):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    bad = np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)).any(axis=1))
    assert not bad.size, (v[bad[0]], a[bad[0]], b[bad[0]])
    assert a.tobytes() == b.tobytes()
    assert not np.isnan(a).any() and (a <= K).all() and not np.signbit(a).any()   # what a carried value's magnitude may be


def test_the_values_are_those_of_the_equality_argument():
    assert VALUES.size == 11 and NAN_FREE.size == 10 and np.isnan(VALUES).sum() == 1
    assert np.fmin(np.nan, K) == K and np.fmin(1.0, np.nan) == 1.0
    nm1, nm2, _ = _two_smallest(np.array([[3.0, 1.0, 2.0]]))
    assert (nm1[0], nm2[0]) == (1.0, 2.0)
    assert _decode_by_prefix_suffix(np.array([[3.0, 1.0, 2.0]])).tolist() == [[1.0, 2.0, 1.0]]
    assert _decode_by_prefix_suffix(np.array([[0.5]])).tolist() == [[K]]
    assert _decode_by_prefix_suffix(np.array([[0.5, 7.0]])).tolist() == [[7.0, 0.5]]


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_prefix_suffix_is_decode_by_slot_exhaustively_without_nan(width):
    v = np.array(list(itertools.product(NAN_FREE, repeat=width)))
    assert v.shape == (10 ** width, width)
    _assert_same_bytes(_decode_by_slot(v), _decode_by_prefix_suffix(v), v)


def test_prefix_suffix_is_decode_by_slot_on_a_random_sweep_without_nan():
    rng = np.random.RandomState(2301)
    rows = 0
    for width in range(1, 17):
        v = NAN_FREE[rng.randint(0, NAN_FREE.size, size=(12500, width))]
        _assert_same_bytes(_decode_by_slot(v), _decode_by_prefix_suffix(v), v)
        rows += v.shape[0]
    assert rows == 200000


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_prefix_suffix_is_the_reference_rule_exhaustively_nan_included(width):
    v = np.array(list(itertools.product(VALUES, repeat=width)))
    assert v.shape == (11 ** width, width) and np.isnan(v).any()
    _assert_same_bytes(_decode_by_prefix_suffix(v), _decode_by_reference_rule(v), v)


def test_the_record_form_differs_from_the_reference_on_a_nan_row():
    """what the docstring says of rows with a record, so that the statement stays true: from width 2 on, a NaN slot makes the
    min / max chain copy the running min1 into min2"""
    v = np.array([[1.0, np.nan, 3.0]])
    assert _decode_by_slot(v).tolist() == [[1.0, 1.0, 1.0]]
    assert _decode_by_reference_rule(v).tolist() == [[3.0, 1.0, 1.0]] == _decode_by_prefix_suffix(v).tolist()


SHAPES = {"shipped_16x32": CODES["shipped_16x32"], "hand_written_3x6": CODES["hand_written_3x6"], "row_of_weight_16_3x16": _slot_matrix}


@needs_hipcc
@pytest.mark.parametrize("case", list(SHAPES))
def test_prefix_rows_fit_the_registers_and_change_no_atomic(case, tmp_path):
    H = SHAPES[case]()
    if case == "row_of_weight_16_3x16":
        assert [int(x) for x in (H >= 0).sum(axis=1)] == [16, 8, 1]
    name = "ldpc_spec::CodeAppendixCM64" if case == "shipped_16x32" else "Code"
    kr, kp = carried_rows(H), prefix_rows(H)
    rule = (f"static_assert(ldpc_spec::ms_m64_keep_rows<{name}>(ldpc_spec::ms_m64_keep_budget<{name}>()) == {kr}, \"carried block rows\");\n"
            f"static_assert(ldpc_spec::ms_m64_prefix_rows<1 << 30>({kr}) == {kp}, \"rows by prefix / suffix minima\");\n")
    asm = _compile(tmp_path, ("" if case == "shipped_16x32" else _code_struct(H)) + rule, name, H)
    got = {k: _metadata(asm, k) for k in (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size")}
    adds = len(re.findall(r"^\s+ds_add_f64\s", asm, re.M))
    eqs = len(re.findall(r"^\s+v_cmp_eq_f64", asm, re.M))
    print(got, "ds_add_f64", adds, "v_cmp_eq_f64", eqs)
    assert got[".vgpr_spill_count"] == 0, got
    assert got[".private_segment_fixed_size"] == 0, got
    assert got[".vgpr_count"] <= 256, got
    assert adds == _atomics_expected(H) == {"shipped_16x32": 65, "hand_written_3x6": 5, "row_of_weight_16_3x16": 9}[case], adds
    if case == "shipped_16x32":
        assert (kr, kp) == (13, 13)
        assert eqs == 0, eqs   # KP == KR: no carried row selects by value equality any more
