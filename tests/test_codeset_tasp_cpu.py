"""TDMP sum-product code sets (decoder 7, ldpc_hip_open_codes_tdmp) without a GPU: the host-side graph table and TDMP's limits in
ldpc_hip_codes_table_host, the exported entry point, and the properties the GPU tests (test_gpu_codeset_tasp.py) need of their
inputs: row weights, pairwise different codes, the LDS bound, and an SNR at which the oracle converges on some frames only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import codeset_tasp_sets as S
from ldpc_testlib import ROOT, TASP_DEC, load_base_matrix, relift
from test_codeset_cpu import SETS, table_np

EINVAL, EUNSUPPORTED = -1, -2
E = -1


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


def _rc(lib, codes, M):
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    n = C.c_longlong(-1)
    rc = lib.ldpc_hip_codes_table_host(TASP_DEC, codes.shape[1], codes.shape[2], M, codes.ctypes.data, codes.shape[0], None, None, 0, C.byref(n))
    return rc, lib.ldpc_hip_last_error().decode()


def test_error_codes_match_the_header():
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+LDPC_HIP_EINVAL\s+\(?-1\)?", header) and re.search(r"#define\s+LDPC_HIP_EUNSUPPORTED\s+\(?-2\)?", header)


@pytest.mark.parametrize("name", ["single row", "three 2x4"])
def test_table_builder(L, name):
    M, codes = SETS[name]
    off, tab = L.codes_table(TASP_DEC, np.array(codes, dtype=np.int16), M)
    want_off, want_tab = table_np(codes)
    assert np.array_equal(off, want_off)
    assert np.array_equal(tab, want_tab)


def test_table_builder_on_the_gpu_sets(L):
    for case in S.CASES:
        codes = S.code_set(case)
        off, tab = L.codes_table(TASP_DEC, codes, case[0])
        want_off, want_tab = table_np(codes)
        assert np.array_equal(off, want_off) and np.array_equal(tab, want_tab), case


def test_builder_refusals(L):
    lib = L.load_library()
    ok = np.array(SETS["three 2x4"][1], dtype=np.int16)
    assert _rc(lib, ok, 5)[0] == 0
    bad = ok.copy(); bad[1, 0, 2:] = -1; bad[1, 1, 2:] = [3, 4]         # weight 1 in row 0 of code 1 (every column still used)
    assert ((bad[1] >= 0).sum(axis=1) == [2, 4]).all()
    bad[1, 0, 1] = -1
    rc, msg = _rc(lib, bad, 5)
    assert rc == EINVAL and "code 1" in msg and "row 0" in msg and "weight 1" in msg, msg
    rc, msg = _rc(lib, np.array(SETS["two 3x5 M=100"][1], dtype=np.int16), 100)   # its code 0 has a weight-1 row 1
    assert rc == EINVAL and "code 0" in msg and "row 1" in msg, msg
    assert _rc(lib, np.zeros((2, 2, 17), dtype=np.int16), 2)[0] == EINVAL          # row weight 17
    assert _rc(lib, np.zeros((2, 2, 16), dtype=np.int16), 2)[0] == 0
    assert _rc(lib, np.zeros((1, 17, 18), dtype=np.int16), 2)[0] == EINVAL         # rh = 17
    assert _rc(lib, np.zeros((1, 16, 16), dtype=np.int16), 2)[0] == 0
    assert _rc(lib, np.zeros((1, 2, 4), dtype=np.int16), 513)[0] == EINVAL         # M = 513
    assert _rc(lib, np.zeros((1, 2, 4), dtype=np.int16), 512)[0] == 0
    bad = ok.copy(); bad[2, :, 2] = -1                                               # an empty block column
    rc, msg = _rc(lib, bad, 5)
    assert rc == EINVAL and "code 2" in msg and "column 2" in msg
    # nothing is held per block column in registers: nh = 40 with rh = 4
    wide = -np.ones((1, 4, 40), dtype=np.int16)
    for k in range(40):
        wide[0, k % 4, k] = k % 7
    assert ((wide[0] >= 0).sum(axis=1) == 10).all() and _rc(lib, wide, 7)[0] == 0
    assert lib.ldpc_hip_codes_table_host(3, 4, 40, 7, wide.ctypes.data, 1, None, None, 0, None) == EINVAL   # MS_DEC keeps its nh <= 32


def test_lds_bound(L):
    lib = L.load_library()
    base = load_base_matrix()
    assert int((base >= 0).sum()) == 112
    # the shipped search shape fits with one workgroup per CU
    H = np.where(base >= 0, relift(base, 126) % 126, -1).astype(np.int16)[None]
    assert S.lds_bytes(H, 126) == 145168 and _rc(lib, H, 126)[0] == 0
    # the same base matrix at M = 256 does not: 8 * (8192 + 112 * 256) + 16 bytes
    H = np.where(base >= 0, relift(base, 256) % 256, -1).astype(np.int16)[None]
    rc, msg = _rc(lib, H, 256)
    assert S.lds_bytes(H, 256) == 294928 and rc == EUNSUPPORTED and "294928" in msg, msg
    # the bound itself at 16 x 32, M = 126: 8 * (4032 + ne * 126) + 16 <= 163840 <=> ne <= 130; the largest code of a set decides
    def grown(ne):
        G = np.where(base >= 0, relift(base, 126) % 126, -1).astype(np.int16)
        for j, k in zip(*np.nonzero(G < 0)):
            if (G >= 0).sum() < ne and (G[j] >= 0).sum() < 16:
                G[j, k] = (j + k) % 126
        assert (G >= 0).sum() == ne
        return G
    small = grown(112)
    assert S.lds_bytes([grown(130)], 126) == 163312 and _rc(lib, np.stack([small, grown(130)]), 126)[0] == 0
    for pair in ([small, grown(131)], [grown(131), small]):
        rc, msg = _rc(lib, np.stack(pair), 126)
        assert rc == EUNSUPPORTED and "164320" in msg, msg


def test_symbol_header_and_binding(L):
    lib = L.load_library()
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        header = f.read()
    assert hasattr(lib, "ldpc_hip_open_codes_tdmp")
    assert re.search(r"\bint\s+ldpc_hip_open_codes_tdmp\s*\(int rh, int nh, int M, const int16_t \*hd, int C, int device, ldpc_hip_ctx \*\*out\)", header)
    assert re.search(r"#define\s+LDPC_HIP_ABI_VERSION\s+4\b", header) and lib.ldpc_hip_abi_version() == 4
    h = C.c_void_p(123)
    assert lib.ldpc_hip_open_codes_tdmp(2, 4, 5, None, 1, 0, C.byref(h)) == EINVAL and not h.value     # refused before any device call
    assert lib.ldpc_hip_open_codes_tdmp(2, 4, 5, None, 1, 0, None) == EINVAL


@pytest.mark.parametrize("case", list(S.CASES), ids=S.CASE_IDS)
def test_gpu_inputs_have_the_required_properties(case):
    """What test_gpu_codeset_tasp.py relies on, asserted here so that nothing is searched at GPU time."""
    M, rh, nh = case
    r = S.reference(case)
    codes = r["codes"]
    assert codes.shape == (S.NCODES, rh, nh)
    w = (codes >= 0).sum(axis=2)
    assert w.min() >= 2 and w.max() <= 16 and ((codes >= 0).sum(axis=1) >= 1).all()
    assert len({(H >= 0).tobytes() for H in codes}) == S.NCODES and len({tuple(x) for x in w}) == S.NCODES
    assert S.lds_bytes(codes, M) <= S.LDS_LIMIT
    for layout in ("shared", "percode"):
        its = np.array([x[1] for x in r["ref"][layout]])
        assert (its > 0).any() and (its < 0).any(), (case, layout, r["snr"], its)
        assert ((its == -S.MAXITER) | ((its >= 0) & (its <= S.MAXITER))).all()


def test_other_gpu_inputs():
    for B in (1, 4):
        M, codes, llr = S.boundary_set(B)
        assert ((codes >= 0).sum(axis=2) >= 2).all() and S.lds_bytes(codes, M) <= S.LDS_LIMIT
        its = [S.oracle_tdmp(codes[c], M, llr[c], S.MAXITER)[1] for c in range(3)]
        assert (its[1] == 0).all() and (its[0] < 0).all() and (its[2] < 0).all(), its      # a codeword at the input returns 0
    codes, llr = S.maxiter_one_set()
    assert set(np.unique([S.oracle_tdmp(codes[c], 20, llr, 1)[1] for c in range(S.NCODES)])) == {-1, 1}
    codes = S.simulate_set()
    assert ((codes >= 0).sum(axis=2) >= 2).all() and len({(H >= 0).tobytes() for H in codes}) == S.SIM["C"]
    M, codes = S.driver_set()
    assert ((codes >= 0).sum(axis=2) >= 2).all()
