"""Code sets (C codes of one shape in one launch) without a GPU: the exported entry points, the host-side graph table against a
numpy restatement on hand-written code sets, the builder's refusals, and the C example against the header."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ldpc_testlib import LMS_DEC, MS_DEC, ROOT, SP_DEC

NEW_SYMBOLS = ["ldpc_hip_open_codes", "ldpc_hip_codes", "ldpc_hip_decode_codes_dev", "ldpc_hip_count_errors_codes_dev", "ldpc_hip_simulate_codes",
               "ldpc_hip_codes_table_host"]
EINVAL = -1


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


def table_np(codes):
    """The table as include/ldpc_hip.h describes it: per code row_start[rh + 1] relative to the code's own edges, then the edges
    (block column << 16) | shift with rows, then columns ascending; offsets[c] = where code c starts."""
    off, tab = [], []
    for H in np.asarray(codes):
        off.append(len(tab))
        edges, row_start = [], []
        for row in H:
            row_start.append(len(edges))
            edges += [(k << 16) | int(v) for k, v in enumerate(row) if v >= 0]
        tab += row_start + [len(edges)] + edges
    return np.array(off, dtype=np.int32), np.array(tab, dtype=np.int32)


E = -1
SETS = {
    # one code, one block row of full weight
    "single row": (3, [[[0, 1, 2, 0]]]),
    # three codes that differ in empty blocks, edge count and row weights
    "three 2x4": (5, [[[0, E, 1, 4], [E, 0, 2, E]],
                      [[0, 3, E, E], [4, 0, 1, 2]],
                      [[2, 2, 2, 2], [0, 1, 3, 4]]]),
    # multi-wave lifting, shifts at both ends of [0, M), a weight-1 row
    "two 3x5 M=100": (100, [[[99, E, E, 0, 50], [E, 0, E, E, E], [1, E, 99, E, 7]],
                            [[0, 0, 0, E, E], [E, 98, E, 3, E], [E, E, 5, 5, 99]]]),
}


def test_symbols_header_and_class(L):
    lib = L.load_library()
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"#define\s+LDPC_HIP_ABI_VERSION\s+4\b", header) and lib.ldpc_hip_abi_version() == 4
    assert lib.ldpc_hip_codes(None) == 0
    for method in ("decode", "count_errors", "simulate", "close"):
        assert callable(getattr(L.LdpcHipCodes, method))
    assert "LdpcHipCodes" in L.__all__


@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("dec", [MS_DEC, LMS_DEC])
def test_table_builder(L, name, dec):
    M, codes = SETS[name]
    off, tab = L.codes_table(dec, np.array(codes, dtype=np.int16), M)
    want_off, want_tab = table_np(codes)
    assert np.array_equal(off, want_off)
    assert np.array_equal(tab, want_tab)


def _rc(lib, dec, codes, M, C_=None):
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    n = C.c_longlong(-1)
    rc = lib.ldpc_hip_codes_table_host(dec, codes.shape[1], codes.shape[2], M, codes.ctypes.data, codes.shape[0] if C_ is None else C_, None, None, 0,
                                       C.byref(n))
    return rc, lib.ldpc_hip_last_error().decode()


def test_builder_refusals(L):
    lib = L.load_library()
    ok = np.array(SETS["three 2x4"][1], dtype=np.int16)
    assert _rc(lib, MS_DEC, ok, 5)[0] == 0
    for dec in (SP_DEC, 0, 4, 9, 6):
        rc, msg = _rc(lib, dec, ok, 5)
        assert rc == EINVAL and "decoder id" in msg
    for Cn in (0, -3):
        assert _rc(lib, MS_DEC, ok, 5, C_=Cn)[0] == EINVAL
    assert _rc(lib, MS_DEC, np.zeros((1, 2, 4), dtype=np.int16), 513)[0] == EINVAL                  # M > 512
    assert _rc(lib, LMS_DEC, np.zeros((1, 2, 4), dtype=np.int16), 512)[0] == 0
    assert _rc(lib, LMS_DEC, np.zeros((1, 65, 66), dtype=np.int16), 2)[0] == EINVAL                 # rh > 64
    assert _rc(lib, LMS_DEC, np.zeros((1, 17, 18), dtype=np.int16), 2)[0] == EINVAL                 # the kernels' own bound: 16 block rows
    assert _rc(lib, MS_DEC, np.zeros((2, 2, 17), dtype=np.int16), 2)[0] == EINVAL                   # row weight 17
    assert _rc(lib, MS_DEC, np.zeros((2, 2, 16), dtype=np.int16), 2)[0] == 0
    bad = ok.copy(); bad[1, 0, :] = -1                                                               # an all-empty row, in code 1
    rc, msg = _rc(lib, MS_DEC, bad, 5)
    assert rc == EINVAL and "code 1" in msg and "row 0" in msg
    bad = ok.copy(); bad[2, :, 2] = -1                                                               # an all-empty column, in code 2
    rc, msg = _rc(lib, MS_DEC, bad, 5)
    assert rc == EINVAL and "code 2" in msg and "column 2" in msg
    for v in (5, -2, 300):                                                                           # a shift outside [-1, M)
        bad = ok.copy(); bad[0, 0, 0] = v
        assert _rc(lib, MS_DEC, bad, 5)[0] == EINVAL
    # a table that does not fit the caller's buffer
    off = np.empty(3, dtype=np.int32)
    tab = np.empty(4, dtype=np.int32)
    assert lib.ldpc_hip_codes_table_host(MS_DEC, 2, 4, 5, ok.ctypes.data, 3, off.ctypes.data, tab.ctypes.data, 4, None) == EINVAL


def test_codes_entry_points_refuse_a_null_context(L):
    lib = L.load_library()
    cnt = (C.c_ulonglong * 5)()
    assert lib.ldpc_hip_decode_codes_dev(None, None, 1, 4, 10, 0.8, None, None, None, None) == EINVAL
    assert lib.ldpc_hip_count_errors_codes_dev(None, None, None, 4, None, None, None) == EINVAL
    assert lib.ldpc_hip_simulate_codes(None, 2.0, 0, 10, 0.8, 1, 0, 4, cnt, None) == EINVAL


def test_c_example_builds_against_the_header(tmp_path):
    exe = tmp_path / "simulate_codes"
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "simulate_codes.c"),
                           "-o", str(exe), "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    assert exe.exists()
    # the example's protograph is one the builder accepts
    src = open(os.path.join(ROOT, "examples", "simulate_codes.c")).read()
    body = re.search(r"mask\[RH \* NH\] = \{(.*?)\};", src, re.S).group(1)
    mask = np.array([int(v) for v in re.findall(r"\d", body)]).reshape(4, 8)
    import ldpc_lib_amd
    off, tab = ldpc_lib_amd.codes_table(MS_DEC, np.where(mask > 0, 0, -1).astype(np.int16)[None], 64)
    assert off.tolist() == [0] and len(tab) == 5 + mask.sum()
