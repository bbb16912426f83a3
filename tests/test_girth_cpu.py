"""Girth / ACE trace without a GPU: the numpy restatement (tests/girth_model.py) against the compiled reference's recorded results
(tests/golden/girth/, tools/make_girth_goldens.py); the graph ldpc_hip_girth_graph_host builds against the model's; upstream's reduction
(ldpc_hip_trace_matrix_host) against the goldens and the M = 126 anchor; every LDPC_HIP_EINVAL of ldpc_hip_girth_codes, which it finds
before any device call; the exports and the ABI version."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import girth_model as gm
from ldpc_testlib import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_girth_goldens  # noqa: E402

EINVAL, EUNSUPPORTED = -1, -2
GOLDENS = gm.load_goldens()


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


def test_golden_cases_are_the_tools_and_are_small_data():
    cases = make_girth_goldens.cases()
    assert set(GOLDENS) == set(cases)
    for name, (codes, M, gmax, gtarget, min_ace, max_spec) in cases.items():
        g = GOLDENS[name]
        assert np.array_equal(g["codes"], np.asarray(codes)) and (g["M"], g["gmax"], g["gtarget"]) == (M, gmax, gtarget), name
        assert g["min_ace"] == (None if min_ace is None else list(min_ace)) and g["max_spec"] == (None if max_spec is None else list(max_spec)), name
        assert g["S"].shape == g["SA"].shape == (len(g["codes"]), gmax) and g["ret"].shape == (len(g["codes"]),), name
        assert os.path.getsize(os.path.join(gm.GIRTH_GOLDEN_DIR, name + ".json")) < 8192, name


def test_golden_cases_cover_what_they_are_for():
    girth = {n: [gm.trace_matrix(s, a)[0] for s, a in zip(g["S"], g["SA"])] for n, g in GOLDENS.items()}
    assert girth["no_cycle"] == [21] and not GOLDENS["no_cycle"]["S"].any() and not GOLDENS["no_cycle"]["SA"].any()
    assert girth["four_cycles"] == [4] and girth["appc_m126"] == [6]
    weights = (GOLDENS["column_weights"]["codes"][0] >= 0).sum(axis=0)
    assert 0 in weights and 1 in weights
    # the anchors: S and SA at d = 3, 5, 7, 9, 11
    assert GOLDENS["appc_m126"]["S"][0, 3:12:2].tolist() == [0, 33, 1068, 25947, 688199]
    assert GOLDENS["appc_m126"]["SA"][0, 3:12:2].tolist() == [0, 7, 21, 13, 14]
    assert GOLDENS["appc_m64"]["S"][0, 3:12:2].tolist() == [7, 79, 2090, 50793, 0]
    assert GOLDENS["appc_m64"]["SA"][0, 3:12:2].tolist() == [17, 7, 21, 13, 0]
    # bounds: a failure at the first and at the second non-zero entry leaves return value 0 and nothing behind that entry
    full = np.count_nonzero(GOLDENS["gf16_m8"]["SA"][0])
    for name, entries in (("bounds_spec_fails_first", 1), ("bounds_spec_fails_second", 2), ("bounds_ace_fails_second", 2), ("bounds_both_fail_second", 2),
                          ("bounds_neither", 1)):
        assert GOLDENS[name]["ret"].tolist() == [0] and np.count_nonzero(GOLDENS[name]["SA"][0]) == entries < full, name
    for name in ("bounds_spec_only_passes", "bounds_ace_only_passes", "bounds_either_passes_by_ace", "bounds_either_passes_by_spec"):
        assert GOLDENS[name]["ret"].tolist() == [1] and np.array_equal(GOLDENS[name]["S"], GOLDENS["gf16_m8"]["S"]), name
    assert np.count_nonzero(GOLDENS["appc_m5_gtarget1"]["S"][0]) == 1 < np.count_nonzero(GOLDENS["appc_m5"]["S"][0])
    one = GOLDENS["set_one_mask"]
    assert len(one["codes"]) == 6 and len({(c >= 0).tobytes() for c in one["codes"]}) == 1
    assert len(set(girth["set_one_mask"])) >= 3 and set(one["ret"].tolist()) == {0, 1}
    assert len({int(np.flatnonzero(a).max()) for a in one["SA"]}) >= 3, "stopping depths"
    two = GOLDENS["set_two_masks"]
    assert len({int((c >= 0).sum()) for c in two["codes"]}) == 2, "two edge counts"
    # the rows of B: M beyond one workgroup's lanes, within and beyond the LDS of a CU
    assert 1024 < GOLDENS["small_m1100"]["M"] and 12 * 1100 * 6 <= 160 * 1024 < 12 * 2400 * 6
    assert int((GOLDENS["small_m2400"]["codes"][0] >= 0).sum()) == 12


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_model_equals_golden(name):
    g = GOLDENS[name]
    for c, hd in enumerate(g["codes"]):
        S, SA, ret, peak = gm.trace(hd, g["M"], g["gmax"], g["gtarget"], g["min_ace"], g["max_spec"])
        assert np.array_equal(S, g["S"][c]) and np.array_equal(SA, g["SA"][c]) and ret == g["ret"][c], (name, c)
        assert peak < 2 ** 31, "a golden case must not overflow upstream's int"


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_graph_host_equals_the_models_graph(L, name):
    g = GOLDENS[name]
    for hd in g["codes"]:
        E, begin, pred = L.girth_graph(hd, g["M"])
        mE, mbegin, mpred = gm.graph(hd, g["M"])
        assert E == mE == int((hd >= 0).sum())
        assert np.array_equal(begin, mbegin) and np.array_equal(pred, mpred)
        for J in range(E):
            assert np.all(np.diff(pred[begin[J]:begin[J + 1], 0]) > 0), "ascending j"


def test_graph_host_sizing_mode_and_checks(L):
    lib = L.load_library()
    hd = GOLDENS["small_m7"]["codes"][0]
    E, n = C.c_int(-1), C.c_longlong(-1)
    assert lib.ldpc_hip_girth_graph_host(3, 6, 7, hd.ctypes.data, C.byref(E), None, None, C.byref(n)) == 0
    assert (E.value, n.value) == (12, len(gm.graph(hd, 7)[2]))
    assert lib.ldpc_hip_girth_graph_host(3, 6, 5, hd.ctypes.data, C.byref(E), None, None, C.byref(n)) == EINVAL   # shift 5, 6 >= M
    assert lib.ldpc_hip_girth_graph_host(3, 6, 7, None, C.byref(E), None, None, C.byref(n)) == EINVAL


def test_trace_matrix_host_equals_goldens_and_the_anchor(L):
    for name, g in GOLDENS.items():
        for S, SA in zip(g["S"], g["SA"]):
            assert L.trace_matrix(S, SA) == gm.trace_matrix(S, SA), name
    g = GOLDENS["appc_m126"]
    assert L.trace_matrix(g["S"][0], g["SA"][0]) == (6, [7, 21, 13, 14], [33, 1068, 25947, 688199])
    g = GOLDENS["no_cycle"]
    assert L.trace_matrix(g["S"][0], g["SA"][0]) == (21, [0, 0, 0, 0], [0, 0, 0, 0])
    g = GOLDENS["small_m7_gmax8"]
    assert L.trace_matrix(g["S"][0], g["SA"][0])[0] == 4
    lib = L.load_library()
    S = np.zeros(20, dtype=np.int32)
    out, girth = np.zeros(4, dtype=np.int32), C.c_int()
    assert lib.ldpc_hip_trace_matrix_host(S.ctypes.data, S.ctypes.data, 21, C.byref(girth), out.ctypes.data, out.ctypes.data) == EINVAL
    assert lib.ldpc_hip_trace_matrix_host(None, S.ctypes.data, 20, C.byref(girth), out.ctypes.data, out.ctypes.data) == EINVAL


def test_girth_codes_refuses_bad_arguments_before_any_device_call(L):
    """Every LDPC_HIP_EINVAL of the header, on a machine that may have no GPU: a call that reached the device would fail differently
    there (LDPC_HIP_EHIP), and the outputs stay untouched."""
    lib = L.load_library()
    hd = np.ascontiguousarray(GOLDENS["small_m7"]["codes"])
    S = np.full((1, 20), 77, dtype=np.int32)
    SA, st = S.copy(), np.full(1, 77, dtype=np.int32)

    def call(rh=3, nh=6, M=7, hd=hd, Cn=1, gmax=20, gtarget=4, S=S, SA=SA, st=st):
        return lib.ldpc_hip_girth_codes(rh, nh, M, None if hd is None else hd.ctypes.data, Cn, gmax, gtarget, None, None, 0,
                                        None if S is None else S.ctypes.data, None if SA is None else SA.ctypes.data,
                                        None if st is None else st.ctypes.data)

    wide = np.full((1, 1, 1001), -1, dtype=np.int16)
    low, high = hd.copy(), hd.copy()
    low[0, 1, 1] = -2
    high[0, 2, 5] = 7
    cases = {"C = 0": dict(Cn=0), "C < 0": dict(Cn=-3), "gmax 3": dict(gmax=3), "gmax 21": dict(gmax=21), "gtarget 0": dict(gtarget=0),
             "nh 1001": dict(rh=1, nh=1001, hd=wide), "shift -2": dict(hd=low), "shift M": dict(hd=high), "M 0": dict(M=0), "M < 0": dict(M=-7),
             "S NULL": dict(S=None), "SA NULL": dict(SA=None), "status NULL": dict(st=None), "hd NULL": dict(hd=None), "rh 0": dict(rh=0)}
    for what, kw in cases.items():
        assert call(**kw) == EINVAL, what
        assert "ldpc_hip_girth_codes" in lib.ldpc_hip_last_error().decode(), what
    assert "code 0, block row 2, block column 5: shift 7" in (call(hd=high), lib.ldpc_hip_last_error().decode())[1]
    assert (S == 77).all() and (SA == 77).all() and (st == 77).all()
    with pytest.raises(L.LdpcHipError, match="gmax = 2"):
        L.girth_codes(hd, 7, gmax=2)


def test_girth_codes_names_the_bytes_of_a_code_that_does_not_fit(L):
    """12 * E^2 * M bytes beyond 4 GiB: LDPC_HIP_EUNSUPPORTED, also found without a device."""
    hd = np.zeros((1, 8, 16), dtype=np.int16)   # E = 128
    with pytest.raises(L.LdpcHipError, match=r"%d bytes.*\(code -2\)" % (12 * 128 * 128 * 30000)):
        L.girth_codes(hd, 30000)


def test_exports_and_abi_version(L):
    lib = L.load_library()
    assert lib.ldpc_hip_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    assert re.search(r"#define LDPC_HIP_ABI_VERSION 4\b", header)
    for name in ("ldpc_hip_girth_codes", "ldpc_hip_girth_graph_host", "ldpc_hip_trace_matrix_host"):
        assert hasattr(lib, name) and re.search(r"\bint %s\(" % name, header), name
    for name in ("girth_codes", "girth_graph", "trace_matrix"):
        assert callable(getattr(L, name))


def test_ldpc_sim_takes_the_girth_flag(tmp_path):
    """The flag is consumed wherever it stands and leaves the positional arguments alone: the jsonx utility, which needs no GPU, still
    sees its three.  (The usage text is pinned by an older test and does not list the flag; the header comment and INTEGRATION.md do.)"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = os.path.join(ROOT, "ldpc-lib_amd", "ldpc_sim")
    (tmp_path / "in.jsonx").write_text("{ a = { girth = 6 } }")
    run = subprocess.run([exe, "--girth", "jsonx", str(tmp_path / "in.jsonx"), str(tmp_path / "out.jsonx")], capture_output=True, text=True)
    assert run.returncode == 0 and "girth = 6" in (tmp_path / "out.jsonx").read_text(), run.stderr


def test_cpp_layer_header_compiles_on_its_own(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "ldpc/girth.h"\n#include "ldpc/bp_simulation.h"\n'
                   "int f(ldpc::Matrix const &H) { std::vector<int> a, s; return ldpc::trace_matrix(H, 8, 4, a, s); }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])
