"""Exact replay on code sets without a GPU: the exported entry points against the header, the binding's methods, the refusals that need
no device, the C example and the `--code-sets` flag of ldpc_sim."""
import ctypes as C
import os
import re
import subprocess

import pytest

from ldpc_testlib import ROOT

EINVAL = -1
SYMBOLS = ["ldpc_hip_mt_set_state_codes", "ldpc_hip_mt_get_state_codes", "ldpc_hip_mt_advance_codes", "ldpc_hip_mt_simulate_codes",
           "ldpc_hip_mt_simulate_codes_stop"]


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


def test_symbols_are_exported_and_declared(L):
    lib = L.load_library()
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS + ["ldpc_hip_frames_codes_host"]:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"#define\s+LDPC_HIP_ABI_VERSION\s+4\b", header) and lib.ldpc_hip_abi_version() == 4


def test_binding_methods_exist(L):
    for name in ("mt_set_state", "mt_get_state", "mt_advance", "mt_simulate", "mt_simulate_until"):
        assert callable(getattr(L.LdpcHipCodes, name)), name
    assert callable(L.host.bp_simulation_codes) and L.bp_simulation_codes is L.host.bp_simulation_codes
    compat = C.CDLL(os.path.join(ROOT, "ldpc-lib_amd", "libldpc_compat.so"))
    assert hasattr(compat, "ldpc_bp_simulation_codes_exact")


def test_null_and_negative_arguments_are_refused(L):
    lib = L.load_library()
    words = (C.c_uint32 * 624)()
    pos = C.c_int(77)
    state = (C.c_ulonglong * 6)(*[7] * 6)
    cnt = (C.c_ulonglong * 5)(*[7] * 5)
    calls = [
        lambda: lib.ldpc_hip_mt_set_state_codes(None, words, 0),
        lambda: lib.ldpc_hip_mt_set_state_codes(None, None, -1),
        lambda: lib.ldpc_hip_mt_get_state_codes(None, words, C.byref(pos)),
        lambda: lib.ldpc_hip_mt_advance_codes(None, 2.0, 0, 10),
        lambda: lib.ldpc_hip_mt_advance_codes(None, 2.0, 0, -1),
        lambda: lib.ldpc_hip_mt_simulate_codes(None, 2.0, 0, 10, 0.8, 5, cnt, None, None),
        lambda: lib.ldpc_hip_mt_simulate_codes(None, 2.0, 0, 10, 0.8, -5, None, None, None),
        lambda: lib.ldpc_hip_mt_simulate_codes_stop(None, 2.0, 0, 10, 0.8, 25, 1000, 0.05, 64, 64, state),
        lambda: lib.ldpc_hip_mt_simulate_codes_stop(None, 2.0, 0, -1, 0.8, 25, 1000, 0.05, 0, -64, None),
        lambda: lib.ldpc_hip_frames_codes_host(None, None, 5, 10, 0.8, cnt, None, None),
    ]
    for i, call in enumerate(calls):
        assert call() == EINVAL, i
        assert "code-set context" in lib.ldpc_hip_last_error().decode(), i
    assert list(state) == [7] * 6 and list(cnt) == [7] * 5 and pos.value == 77


def test_c_example_builds_against_the_header(tmp_path):
    exe = tmp_path / "simulate_codes_exact"
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "simulate_codes_exact.c"),
                           "-o", str(exe), "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    assert exe.exists()
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 2 and "<seed>" in run.stderr


def test_ldpc_sim_names_the_flag_in_its_usage():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    run = subprocess.run([os.path.join(ROOT, "ldpc-lib_amd", "ldpc_sim")], capture_output=True, text=True)
    assert run.returncode == 1 and "[--code-sets]" in run.stderr
    # the flag is taken from any position and leaves the positional arguments alone: a wrong verb still ends in the usage
    run = subprocess.run([os.path.join(ROOT, "ldpc-lib_amd", "ldpc_sim"), "--code-sets", "simulate", "a", "b"], capture_output=True, text=True)
    assert run.returncode == 1 and "usage:" in run.stderr
