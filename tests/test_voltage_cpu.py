"""The voltage check and the bank search without a GPU: the numpy restatement (tests/voltage_model.py) against every golden of the
compiled upstream sources (tests/golden/voltage/, tools/make_voltage_goldens.py); that the goldens are the tool's cases and hold what
they are for; every refusal of ldpc_hip_check_voltages and ldpc_hip_label_bank, which they find before any device call; the exports;
the C++ header; the host code of the check that needs no device under the address and undefined-behaviour sanitizers as a stand-alone
program."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import voltage_model as vm
from ldpc_testlib import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_voltage_goldens as mvg  # noqa: E402

EINVAL, EUNSUPPORTED = -1, -2
GOLDENS = mvg.goldens()   # the tool's cases joined with upstream's results; asserts that the files belong to these inputs
CHECKS = sorted(n for n, g in GOLDENS.items() if g["kind"] == "check")
BANKS = sorted(n for n, g in GOLDENS.items() if g["kind"] == "bank")


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


def test_golden_cases_are_the_tools_and_are_small_data():
    checks, banks = mvg.check_cases(), mvg.bank_cases()
    assert set(CHECKS) == set(checks) and set(BANKS) == set(banks)
    assert sorted(os.listdir(vm.VOLTAGE_GOLDEN_DIR)) == ["bank.json", "check.json"]
    assert sorted([*vm.load_golden("check"), *vm.load_golden("bank")]) == sorted(GOLDENS)
    for name, (proto, g, mm, V, Cf) in checks.items():
        assert len(GOLDENS[name]["results"]) == len(V), name
    for name in banks:
        gold = GOLDENS[name]
        assert gold["max_attempts"] <= 100000 and len(gold["fingerprint"]) == 8 and len(gold["accepted"]) == len(gold["min_ok"]), name
    assert os.path.getsize(vm.golden_path("check")) + os.path.getsize(vm.golden_path("bank")) < 32 * 1024


def test_golden_cases_cover_what_they_are_for():
    results = [(g, r) for n in CHECKS for g in [GOLDENS[n]] for r in g["results"]]
    assert {mvg.status_of(r) for _, r in results} == {0, 1, 2}
    assert any(mvg.status_of(r) == 0 and g["max_modulo"] >= 2 and r["min_ok"] == g["max_modulo"] + 1 for g, r in results)
    assert any(mvg.status_of(r) == 0 and r["failed"] == mvg.digest([]) for g, r in results)
    assert {len(GOLDENS[n]["voltages"]) for n in CHECKS} == {1, 63, 64, 65, 200}
    assert {GOLDENS[n]["max_modulo"] for n in CHECKS} == {1, 2, 3, 63, 64, 65, 127, 128, 1000, 65535}
    assert [GOLDENS["small_g%d_k%d_v%d_m%d" % c]["eqs"] for c in ((6, 1, 2, 1), (8, 64, 31, 3), (10, 200, 31, 64))] == [3, 11, 20]
    for name in ("small_coef_g10_k65_v31_m64_c15", "small_coef_g10_k64_v7_m128_c3"):   # the g = 10 cases carry status 1 and status 2
        assert {mvg.status_of(r) for r in GOLDENS[name]["results"]} == {0, 1, 2}
    assert all(r.get("died", "global_divisor_table is called with the argument 0") == "global_divisor_table is called with the argument 0" for _, r in results)
    assert (GOLDENS["k23_g14_m127"]["eqs"], GOLDENS["k23_g14_m127"]["tree_girth"]) == (9, 12)
    assert GOLDENS["same_columns_m64"]["eqs"] == 0 and all(r == {"first_failed": -1, "min_ok": 2, "max_nonok": 1, "failed": mvg.digest([])}
                                                           for r in GOLDENS["same_columns_m64"]["results"])
    ship = GOLDENS["appc_g6_m1000"]
    assert ship["eqs"] == 343 and ship["voltages"][0] == mvg.shipped_labelling().tolist()
    assert (ship["results"][0]["min_ok"], ship["results"][0]["max_nonok"], ship["results"][0]["failed"][0]) == (79, 215, 140)
    assert GOLDENS["appc_g8_m127"]["eqs"] == 5200 and GOLDENS["appc_g8_m127"]["results"][0] == {"first_failed": 0}
    for name in CHECKS:   # the all-zero labelling and the one with a single non-zero edge
        V = np.array(GOLDENS[name]["voltages"])
        if len(V) >= 63:
            assert any((v == 0).all() for v in V[:3]) and any((v != 0).sum() == 1 for v in V[:3]), name
    for name in BANKS:
        assert len(GOLDENS[name]["accepted"]) >= 2, name
    plain, exact = GOLDENS["bank_small_g8_t31"], GOLDENS["bank_small_g8_t31_exact62"]
    assert plain["accepted"] != exact["accepted"], "the exact modulo rejects an attempt"
    assert GOLDENS["bank_appc_g6_t126"]["attempts_tested"] == 3000 and len(GOLDENS["bank_appc_g6_t126"]["accepted"]) == 420   # 14 %
    assert GOLDENS["bank_k23_g14_t50"]["tree_girth"] == 12


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_model_equals_golden(L, name):
    mvg.check_model(name, GOLDENS[name])


def test_check_voltages_refuses_bad_arguments_before_any_device_call(L):
    """Every LDPC_HIP_EINVAL / LDPC_HIP_EUNSUPPORTED of the header on a machine that may have no GPU: a call that reached the device
    would fail differently there (LDPC_HIP_EHIP); the outputs stay untouched."""
    lib = L.load_library()
    proto = np.ascontiguousarray(mvg.SMALL, dtype=np.int16)
    V = np.ones((2, 12), dtype=np.int32)
    out = [np.full(2, 77, dtype=np.int32) for _ in range(4)]
    failed = np.full((2, 2), 77, dtype=np.uint64)
    tg, ne = C.c_int(77), C.c_int(77)

    def call(rh=3, nh=6, proto=proto, g=8, mm=100, V=V, Cf=None, K=2, status=out[0], min_ok=out[1], max_nonok=out[2], max_abs=out[3]):
        def ptr(a):
            return None if a is None else a.ctypes.data
        return lib.ldpc_hip_check_voltages(rh, nh, ptr(proto), g, mm, ptr(V), ptr(Cf), K, 0, ptr(status), ptr(min_ok), ptr(max_nonok), ptr(max_abs),
                                           ptr(failed), C.byref(tg), C.byref(ne))

    negative = proto.copy()
    negative[1, 2] = -1
    low, high = V.copy(), V.copy()
    low[1, 3], high[0, 11] = -1, 32768
    einval = {"rh 0": dict(rh=0), "nh < 0": dict(nh=-6), "proto NULL": dict(proto=None), "negative entry": dict(proto=negative),
              "no edge": dict(proto=np.zeros((3, 6), dtype=np.int16)), "girth 3": dict(g=3), "max_modulo 0": dict(mm=0), "max_modulo < 0": dict(mm=-4),
              "K 0": dict(K=0), "K < 0": dict(K=-1), "voltages NULL": dict(V=None), "status NULL": dict(status=None), "min_ok NULL": dict(min_ok=None),
              "max_nonok NULL": dict(max_nonok=None), "max_abs_sum NULL": dict(max_abs=None), "voltage -1": dict(V=low), "voltage 32768": dict(V=high),
              "coefficient -1": dict(Cf=low), "coefficient 32768": dict(Cf=high)}
    for what, kw in einval.items():
        assert call(**kw) == EINVAL, what
        assert "ldpc_hip_check_voltages" in lib.ldpc_hip_last_error().decode(), what
    assert "labelling 1, edge 3: voltage -1" in (call(V=low), lib.ldpc_hip_last_error().decode())[1]
    assert "labelling 0, edge 11: coefficient 32768" in (call(Cf=high), lib.ldpc_hip_last_error().decode())[1]
    assert call(mm=65536) == EUNSUPPORTED and "max_modulo = 65536, at most 65535" in lib.ldpc_hip_last_error().decode()
    assert call(g=66) == EUNSUPPORTED and "target_girth = 66, at most 64" in lib.ldpc_hip_last_error().decode()
    wide = np.ones((1, 4097), dtype=np.int16)
    assert call(rh=1, nh=4097, proto=wide, V=np.ones((2, 4097), dtype=np.int32)) == EUNSUPPORTED
    assert "4097 edges, at most 4096" in lib.ldpc_hip_last_error().decode()
    dense = np.ones((6, 12), dtype=np.int16)
    assert call(rh=6, nh=12, proto=dense, g=12, V=np.ones((2, 72), dtype=np.int32)) == EUNSUPPORTED
    assert re.search(r"more than (1048576 equations|4194304 paths)", lib.ldpc_hip_last_error().decode())
    assert all((o == 77).all() for o in out) and (failed == 77).all() and (tg.value, ne.value) == (77, 77)
    with pytest.raises(L.LdpcHipError, match=r"max_modulo = 70000.*\(code -2\)"):
        L.check_voltages(proto, 8, V, 70000)


def test_label_bank_refuses_bad_arguments_before_any_device_call(L):
    lib = L.load_library()
    proto = np.ascontiguousarray(mvg.SMALL, dtype=np.int16)
    state = np.arange(624, dtype=np.uint32)
    hd = np.full((2, 3, 6), 77, dtype=np.int16)
    min_ok = np.full(2, 77, dtype=np.int32)
    index = np.full(2, 77, dtype=np.int64)
    out = np.full(624, 77, dtype=np.uint32)
    found, tg, pos_out, tested = C.c_int(77), C.c_int(77), C.c_int(77), C.c_longlong(77)

    def call(rh=3, nh=6, proto=proto, g=8, T=31, exact=0, A=100, want=2, state=state, pos=0, hd=hd, min_ok=min_ok, index=index, found=found, tested=tested,
             tg=tg, out=out, pos_out=pos_out):
        def ptr(a):
            return None if a is None else a.ctypes.data

        def ref(v):
            return None if v is None else C.byref(v)
        return lib.ldpc_hip_label_bank(rh, nh, ptr(proto), g, T, exact, A, want, ptr(state), pos, 0, ptr(hd), ptr(min_ok), ptr(index), ref(found), ref(tested),
                                       ref(tg), ptr(out), ref(pos_out))

    negative = proto.copy()
    negative[1, 2] = -1
    cases = {"rh 0": dict(rh=0), "proto NULL": dict(proto=None), "negative entry": dict(proto=negative), "no edge": dict(proto=np.zeros((3, 6), dtype=np.int16)),
             "girth 3": dict(g=3), "T 1": dict(T=1), "T 32768": dict(T=32768), "exact below T": dict(exact=30), "exact 1": dict(exact=1),
             "exact < 0": dict(exact=-62), "exact 65536": dict(exact=65536), "A 0": dict(A=0), "want 0": dict(want=0), "state NULL": dict(state=None),
             "pos -1": dict(pos=-1), "pos 625": dict(pos=625), "hd NULL": dict(hd=None), "min_ok NULL": dict(min_ok=None), "index NULL": dict(index=None),
             "found NULL": dict(found=None), "tested NULL": dict(tested=None), "tree_girth NULL": dict(tg=None), "state_out NULL": dict(out=None),
             "pos_out NULL": dict(pos_out=None)}
    for what, kw in cases.items():
        assert call(**kw) == EINVAL, what
        assert "ldpc_hip_label_bank" in lib.ldpc_hip_last_error().decode(), what
    assert "exact_modulo = 30, must be 0 or T = 31 .. 65535" in (call(exact=30), lib.ldpc_hip_last_error().decode())[1]
    assert call(g=66) == EUNSUPPORTED
    assert (hd == 77).all() and (min_ok == 77).all() and (index == 77).all() and (out == 77).all()
    assert (found.value, tg.value, pos_out.value, tested.value) == (77, 77, 77, 77)
    with pytest.raises(L.LdpcHipError, match=r"T = 40000"):
        L.label_bank(proto, 8, 40000, 10, state, 0)


def test_exports_and_abi_version(L):
    lib = L.load_library()
    assert lib.ldpc_hip_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    assert re.search(r"#define LDPC_HIP_ABI_VERSION 4\b", header)
    for name in ("ldpc_hip_check_voltages", "ldpc_hip_label_bank"):
        assert hasattr(lib, name) and re.search(r"\bint %s\(" % name, header), name
    for name in ("check_voltages", "label_bank", "failed_moduli"):
        assert callable(getattr(L, name)) and name in L.__all__
    assert L.failed_moduli(np.array([0b1010, 1], dtype=np.uint64)).tolist() == [1, 3, 64]


def test_cpp_layer_header_compiles_on_its_own(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "ldpc/equations.h"\n#include "ldpc/bp_simulation.h"\n'
                   "bool f(ldpc::Matrix const &P, std::vector<int> const &v, std::vector<std::vector<int>> const &V) {\n"
                   "    ldpc::voltage_check_result r = ldpc::check_voltages(P, 8, v, 126);\n"
                   "    return r.check_modulo(126) && ldpc::check_voltages(P, 8, V, 126).size() && ldpc::check_voltages_and_coefs(P, 8, v, 126, v, 16).check_modulo(3)\n"
                   "        && ldpc::check_voltages_and_coefs(P, 8, V, 126, V, 16).size();\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_device_free_host_code_under_sanitizers(tmp_path):
    """tests/cpp/voltage_sanitize.cpp: what ldpc_hip_check_voltages computes on the host before and between its device calls --
    first_bad_value and piece_size of csrc/ldpc_voltage.hpp -- and failed_set of include/ldpc/equations.h, compiled with
    -fsanitize=address,undefined as a program of its own.  (The API's allocations, copies and launches need HIP and are not run
    under a sanitizer.)  Pieces tile the batch for the forced sizes the GPU tests use, for the byte limit and for the cap on a launch."""
    exe = str(tmp_path / "voltage_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "ldpc-lib_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "voltage_sanitize.cpp"), "-o", exe])

    def run(V, has_coef, has_failed, mm, forced, members, piece_bytes=256 << 20, piece_max=1 << 20):
        V = np.asarray(V)
        bits = np.zeros(mm // 64 + 1, dtype=np.uint64)
        for m in members:
            bits[m >> 6] |= np.uint64(1) << np.uint64(m & 63)
        words = [*V.shape, int(has_coef), int(has_failed), mm, forced, piece_bytes, piece_max, *V.reshape(-1).tolist(), *["%x" % int(w) for w in bits]]
        out = subprocess.run([exe], input=" ".join(str(w) for w in words), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        bad, pieces, got = (line.split()[1:] for line in out.stdout.strip().split("\n"))
        assert [int(v) for v in got] == sorted(members)
        return int(bad[0]), [int(v) for v in pieces]

    g = GOLDENS["small_g10_k200_v31_m64"]
    model = mvg.check_model("small_g10_k200_v31_m64", g)
    members = next(m["failed"] for m in model if m["status"] == 0)
    assert run(g["voltages"], 0, 1, 64, 0, members) == (-1, [0, 200])
    assert run(g["voltages"], 0, 1, 64, 1, [])[1] == list(range(201))
    assert run(g["voltages"], 1, 0, 64, 65, [1, 64]) == (-1, [0, 65, 130, 195, 200])
    assert run(g["voltages"], 0, 1, 65535, 10 ** 9, [1, 2, 63, 64, 65, 65535])[1] == [0, 200]
    V = np.array(g["voltages"])
    V[7, 3] = 32768
    assert run(V, 0, 0, 1, 0, [1])[0] == 7 * 12 + 3
    V[0, 0] = -1
    assert run(V, 0, 0, 127, 3, [127])[0] == 0
    # the byte limit: 12 voltages, a bitmap of two words and 16 bytes of results are 80 bytes per labelling, 160 with coefficients and
    # without the bitmap 112; the cap on a launch holds for a forced size too; a limit below one labelling still gives pieces of one
    V = np.array(g["voltages"])
    assert run(V, 0, 1, 64, 0, [], piece_bytes=1000)[1] == [*range(0, 200, 12), 200]
    assert run(V, 1, 0, 64, 0, [], piece_bytes=1000)[1] == [*range(0, 200, 8), 200]
    assert run(V, 0, 1, 64, 0, [], piece_max=50)[1] == [0, 50, 100, 150, 200]
    assert run(V, 0, 1, 64, 70, [], piece_max=50)[1] == [0, 50, 100, 150, 200]
    assert run(V, 0, 1, 64, 0, [], piece_bytes=10)[1] == list(range(201))
