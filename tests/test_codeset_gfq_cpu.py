"""GF(q) code sets (C codes over GF(q) of one shape in one launch) without a GPU: the exported entry points, the host-side record
table against a numpy restatement (tests/codeset_gfq_sets.py:record), and every refusal of the builder with the code it names."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from codeset_gfq_sets import cw2_mixture_set, mixed_4x8, record, shipped_set
from ldpc_testlib import ROOT

NEW_SYMBOLS = ["ldpc_hip_open_codes_gfq", "ldpc_hip_codes_gfq_table_host", "ldpc_hip_decode_codes_gfq_dev", "ldpc_hip_count_errors_codes_gfq_dev",
               "ldpc_hip_simulate_codes_gfq", "ldpc_hip_simulate_codes_gfq_stop"]
EINVAL, EUNSUPPORTED = -1, -2
E = -1


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


def three_patterns():
    """Three 3 x 5 codes over GF(8) at M = 7 that differ in pattern, edge count (8, 10, 15), row and column weights; shifts at both
    ends of [0, M) and beyond it (reduced mod M), a coefficient that is only there at an empty circulant."""
    hb = np.array([[[0, 6, E, E, 3], [E, 1, 2, E, E], [5, E, E, 0, 6]],
                   [[1, 1, E, 4, E], [E, 0, 13, E, 7], [2, E, 5, 5, 3]],
                   [[0, 1, 2, 3, 4], [6, 5, 4, 3, 2], [0, 0, 0, 0, 0]]], dtype=np.int16)
    hc = np.array([[[1, 7, 0, 9, 3], [E, 1, 2, E, E], [5, E, E, 4, 6]],
                   [[1, 1, E, 4, E], [E, 2, 3, E, 7], [2, E, 5, 5, 3]],
                   [[7, 1, 2, 3, 4], [6, 5, 4, 3, 2], [1, 1, 1, 1, 1]]], dtype=np.int16)
    return 3, 7, hb, hc


def table_np(hb, hc, M):
    off, tab = [], []
    for b, c in zip(hb, hc):
        off.append(len(tab))
        tab += record(b, c, M).tolist()
    return np.array(off, dtype=np.int32), np.array(tab, dtype=np.int32)


def test_symbols_header_and_class(L):
    lib = L.load_library()
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"#define\s+LDPC_HIP_ABI_VERSION\s+4\b", header) and lib.ldpc_hip_abi_version() == 4
    assert lib.ldpc_hip_codes(None) == 0 and lib.ldpc_hip_gfq_q(None) == 0
    for method in ("decode", "count_errors", "simulate", "simulate_until", "profile", "profile_read", "close"):
        assert callable(getattr(L.LdpcHipCodesGfq, method))
    assert "LdpcHipCodesGfq" in L.__all__ and "codes_gfq_table" in L.__all__


def test_table_of_three_patterns(L):
    q_bits, M, hb, hc = three_patterns()
    off, tab = L.codes_gfq_table(q_bits, hb, hc, M)
    want_off, want_tab = table_np(hb, hc, M)
    assert np.array_equal(off, want_off) and np.array_equal(tab, want_tab)
    assert [int(tab[o]) for o in off] == [8, 10, 15]
    assert [int(tab[o + 1]) for o in off] == [0, 1, 0], "only code 1 has weight 2 in every block column"


def test_table_of_a_cw2_mixture(L):
    """One all-column-weight-2 code and one mixed code in a set: cw2 is per code, e_rl = coefficient - 1."""
    hb, hc = cw2_mixture_set(33, 16)
    hb, hc = hb[:2], hc[:2]
    off, tab = L.codes_gfq_table(4, hb, hc, 33)
    want_off, want_tab = table_np(hb, hc, 33)
    assert np.array_equal(off, want_off) and np.array_equal(tab, want_tab)
    assert [int(tab[o + 1]) for o in off] == [1, 0]
    rh, nh = hb.shape[1:]
    for c, o in enumerate(off):
        E_ = int(tab[o])
        assert E_ == int((hb[c] >= 0).sum())
        e_rl = tab[o + 2 + rh + 1 + nh + 1 + 2 * E_:][:E_]
        assert np.array_equal(e_rl, hc[c][hb[c] >= 0] - 1)
    assert int(tab[off[0]]) != int(tab[off[1]]), "the two kinds of code differ in edge count too"
    # shipped(M, q) and a set of candidates of it
    hb, hc = shipped_set(8, 16)
    off, tab = L.codes_gfq_table(4, hb, hc, 8)
    want_off, want_tab = table_np(hb, hc, 8)
    assert np.array_equal(off, want_off) and np.array_equal(tab, want_tab)


def test_sizes_only_and_capacity(L):
    lib = L.load_library()
    q_bits, M, hb, hc = three_patterns()
    _, want = table_np(hb, hc, M)
    n = C.c_longlong(-1)
    assert lib.ldpc_hip_codes_gfq_table_host(q_bits, 3, 5, M, hb.ctypes.data, hc.ctypes.data, 3, None, None, 0, C.byref(n)) == 0
    assert n.value == len(want)
    off = np.empty(3, dtype=np.int32)
    tab = np.full(len(want), -7, dtype=np.int32)
    assert lib.ldpc_hip_codes_gfq_table_host(q_bits, 3, 5, M, hb.ctypes.data, hc.ctypes.data, 3, off.ctypes.data, tab.ctypes.data, len(want) - 1, None) == EINVAL
    assert "room for" in lib.ldpc_hip_last_error().decode() and (tab == -7).all()
    assert lib.ldpc_hip_codes_gfq_table_host(q_bits, 3, 5, M, hb.ctypes.data, hc.ctypes.data, 3, off.ctypes.data, tab.ctypes.data, len(want), None) == 0
    assert np.array_equal(tab, want)


def _rc(lib, q_bits, hb, hc, M, C_=None, shape=None):
    hb = np.ascontiguousarray(hb, dtype=np.int16)
    hc = np.ascontiguousarray(hc, dtype=np.int16)
    rh, nh = shape or hb.shape[1:]
    n = C.c_longlong(-1)
    rc = lib.ldpc_hip_codes_gfq_table_host(q_bits, rh, nh, M, hb.ctypes.data, hc.ctypes.data, hb.shape[0] if C_ is None else C_, None, None, 0, C.byref(n))
    return rc, lib.ldpc_hip_last_error().decode()


def test_builder_refusals(L):
    lib = L.load_library()
    q_bits, M, hb, hc = three_patterns()
    assert _rc(lib, q_bits, hb, hc, M)[0] == 0
    # what ldpc_hip_open_gfq refuses per code: LDPC_HIP_EUNSUPPORTED, with the code and the row or position
    for qb in (1, 0, -2, 11):
        rc, msg = _rc(lib, qb, hb, hc, M)
        assert rc == EUNSUPPORTED and "q" in msg, (qb, msg)
    assert _rc(lib, 2, hb, np.where(hc > 0, 1 + hc % 3, hc), M)[0] == 0 and _rc(lib, 10, hb, hc, M)[0] == 0
    bad = hb.copy(); bad[1, 1, :] = E; bad[1, 1, 2] = 3                                              # block row 1 of code 1 has weight 1
    rc, msg = _rc(lib, q_bits, bad, hc, M)
    assert rc == EUNSUPPORTED and "code 1" in msg and "row 1" in msg and "weight 1" in msg, msg
    bad = hb.copy(); bad[2, 0, :] = E                                                                # ... and weight 0
    rc, msg = _rc(lib, q_bits, bad, hc, M)
    assert rc == EUNSUPPORTED and "code 2" in msg and "row 0" in msg and "weight 0" in msg, msg
    wide_b = np.zeros((2, 2, 1025), dtype=np.int16)                                                  # row weight 1025, in code 1 only
    wide_b[0, :, 1024] = E
    rc, msg = _rc(lib, q_bits, wide_b, np.ones_like(wide_b), 1)
    assert rc == EUNSUPPORTED and "code 1" in msg and "row 0" in msg and "1024" in msg, msg
    wide_b[1, :, 1024] = E
    assert _rc(lib, q_bits, wide_b, np.ones_like(wide_b), 1)[0] == 0                                 # weight 1024 is served
    bad = hc.copy(); bad[2, 1, 3] = 0                                                                # coefficient 0 on a circulant of code 2
    rc, msg = _rc(lib, q_bits, hb, bad, M)
    assert rc == EUNSUPPORTED and "code 2" in msg and "(1, 3)" in msg and "coefficient 0" in msg, msg
    assert hc[0, 0, 2] == 0 and hb[0, 0, 2] == E                                                     # ... at an empty one it is not read
    # LDPC_HIP_EINVAL
    for Cn in (0, -3):
        rc, msg = _rc(lib, q_bits, hb, hc, M, C_=Cn)
        assert rc == EINVAL and "C = %d" % Cn in msg
    for shape, m in (((0, 5), M), ((3, 0), M), ((-1, 5), M), ((3, 5), 0), ((3, 5), -7)):
        assert _rc(lib, q_bits, hb, hc, m, shape=shape)[0] == EINVAL, (shape, m)
    for v in (-2, -300):
        bad = hb.copy(); bad[1, 2, 4] = v                                                            # a shift below -1, in code 1
        rc, msg = _rc(lib, q_bits, bad, hc, M)
        assert rc == EINVAL and "code 1" in msg and "(2, 4)" in msg and "below -1" in msg, msg
    for v in (8, -1):
        bad = hc.copy(); bad[1, 0, 0] = v                                                            # not an element of GF(8)
        rc, msg = _rc(lib, q_bits, hb, bad, M)
        assert rc == EINVAL and "code 1" in msg and "(0, 0)" in msg, msg
    n = C.c_longlong()
    assert lib.ldpc_hip_codes_gfq_table_host(q_bits, 3, 5, M, None, hc.ctypes.data, 3, None, None, 0, C.byref(n)) == EINVAL
    assert lib.ldpc_hip_codes_gfq_table_host(q_bits, 3, 5, M, hb.ctypes.data, None, 3, None, None, 0, C.byref(n)) == EINVAL
    # no limit on M, rh or nh beyond the single-code decoder's: shapes the binary sets refuse
    big_b, big_c = mixed_4x8(1000, 16)
    assert _rc(lib, 4, big_b[None], big_c[None], 1000)[0] == 0
    tall = np.zeros((1, 20, 40), dtype=np.int16)
    assert _rc(lib, 4, tall, tall + 1, 3)[0] == 0


def test_entry_points_refuse_a_null_context(L):
    lib = L.load_library()
    cnt = (C.c_ulonglong * 5)()
    st = (C.c_ulonglong * 4)()
    assert lib.ldpc_hip_decode_codes_gfq_dev(None, None, 1, 4, 10, None, None, None, None) == EINVAL
    assert lib.ldpc_hip_count_errors_codes_gfq_dev(None, None, None, 4, None, None, None) == EINVAL
    assert lib.ldpc_hip_simulate_codes_gfq(None, 2.0, 10, 1, 0, 4, cnt, None) == EINVAL
    assert lib.ldpc_hip_simulate_codes_gfq_stop(None, 2.0, 10, 1, 0, 12, 100, 0.05, 64, 64, st) == EINVAL
    assert "GF(q) code-set context" in lib.ldpc_hip_last_error().decode()
