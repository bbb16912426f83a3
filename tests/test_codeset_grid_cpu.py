"""The SNR grid on code sets (ldpc_hip_*_codes_grid*), what needs no GPU: the symbols, their declarations, the Python
methods, the refusals that come before any device call, and the two C++ templates against the header."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from codeset_grid_sets import MAX_POINTS
from ldpc_testlib import ROOT

EINVAL = -1
ENTRIES = ("ldpc_hip_simulate_codes_grid", "ldpc_hip_simulate_codes_grid_stop", "ldpc_hip_mt_simulate_codes_grid", "ldpc_hip_mt_simulate_codes_grid_stop")


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


def test_symbols_are_exported_and_declared(L):
    lib = L.load_library()
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        header = f.read()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(ldpc_hip_ctx \*ctx, const double \*snr_db, int P," % name, header), name
        assert getattr(lib, name).argtypes is not None, name
    assert re.search(r"#define LDPC_HIP_ABI_VERSION 4\b", header)


def test_python_methods(L):
    want = {"simulate_grid": ("snr_db", "maxiter", "seed", "first_frame", "frames"),
            "simulate_grid_until": ("snr_db", "maxiter", "seed", "n_frame_errors", "n_experiments", "reference_frame_error"),
            "mt_simulate_grid": ("snr_db", "maxiter", "frames"),
            "mt_simulate_grid_until": ("snr_db", "maxiter", "n_frame_errors", "n_experiments", "reference_frame_error")}
    for name, first in want.items():
        params = list(inspect.signature(getattr(L.LdpcHipCodes, name)).parameters)
        assert tuple(params[1:1 + len(first)]) == first, (name, params)
        assert "punctured_blocks" in params and "alpha" in params, name
    assert "records" in inspect.signature(L.LdpcHipCodes.mt_simulate_grid).parameters
    assert "records" in inspect.signature(L.LdpcHipCodes.simulate_grid).parameters


def test_refusals_without_a_device(L):
    lib = L.load_library()
    snr = np.array([1.0, 2.0], dtype=np.float64)
    ref = np.array([0.1, 0.1], dtype=np.float64)
    cnt = np.full((2, 4, 5), 7, dtype=np.uint64)
    state = np.full((2, 4, 6), 7, dtype=np.uint64)
    for P in (0, -1, 1, 2, MAX_POINTS, MAX_POINTS + 1):
        calls = [lib.ldpc_hip_simulate_codes_grid(None, snr.ctypes.data, P, 0, 20, 0.8, 1, 0, 8, cnt.ctypes.data, None),
                 lib.ldpc_hip_simulate_codes_grid_stop(None, snr.ctypes.data, P, 0, 20, 0.8, 1, 0, 12, 100, ref.ctypes.data, 64, 64, state.ctypes.data),
                 lib.ldpc_hip_mt_simulate_codes_grid(None, snr.ctypes.data, P, 0, 20, 0.8, 8, cnt.ctypes.data, None, None),
                 lib.ldpc_hip_mt_simulate_codes_grid_stop(None, snr.ctypes.data, P, 0, 20, 0.8, 12, 100, ref.ctypes.data, 64, 64, state.ctypes.data)]
        assert calls == [EINVAL] * 4, (P, calls)
        msg = lib.ldpc_hip_last_error().decode()
        assert "ldpc_hip_mt_simulate_codes_grid_stop" in msg, msg
        if 1 <= P <= MAX_POINTS:   # a grid that is one: a null context is no binary code-set context
            assert "code-set context" in msg, msg
        else:                      # the grid itself is refused first, by its size
            assert "P = %d" % P in msg and "1 .. %d" % MAX_POINTS in msg, msg
    for call in (lambda: lib.ldpc_hip_simulate_codes_grid(None, None, 2, 0, 20, 0.8, 1, 0, 8, cnt.ctypes.data, None),
                 lambda: lib.ldpc_hip_mt_simulate_codes_grid_stop(None, None, 2, 0, 20, 0.8, 12, 100, ref.ctypes.data, 64, 64, state.ctypes.data)):
        assert call() == EINVAL and "snr_db" in lib.ldpc_hip_last_error().decode()
    assert (cnt == 7).all() and (state == 7).all(), "a refused call leaves its outputs alone"


def test_cpp_templates_compile_against_the_header(tmp_path):
    src = tmp_path / "grid_tu.cpp"
    src.write_text("""#include <utility>
#include <vector>
#include "ldpc/bp_simulation.h"
#include "ldpc/decoders.h"
using Grid = std::vector<std::vector<std::pair<double, double>>>;
Grid philox(std::vector<ldpc::Matrix> const &codes, std::vector<double> const &snrs, std::vector<double> const &refs,
            std::vector<std::vector<ldpc::SimCounters>> *cnt) {
    return ldpc::bp_simulation_codes_grid_t<ldpc::Matrix, ldpc::OwnRngEnv>(codes, 32, 20, 12, 300LL, snrs, refs, 3, 0, 0, 0, 0, 9ULL, 0, cnt);
}
Grid exact(std::vector<ldpc::Matrix> const &codes, std::vector<double> const &snrs, std::vector<double> const &refs,
           std::vector<std::vector<ldpc::SimCounters>> *cnt) {
    return ldpc::bp_simulation_codes_grid_exact_t<ldpc::Matrix, ldpc::OwnRngEnv>(codes, 32, 20, 12, 300LL, snrs, refs, 3, 0, 0, 0, 0, 0, cnt, 64, 256, 0, 1);
}
Grid standalone(std::vector<ldpc::Matrix> const &codes, std::vector<double> const &snrs, std::vector<double> const &refs) {
    Grid a = ldpc::bp_simulation_codes_grid(codes, 32, 20, 12, 300, snrs, refs, 3, 0, 0, 0, 0, 9ULL);
    Grid b = ldpc::bp_simulation_codes_grid_exact(codes, 32, 20, 12, 300, snrs, refs, 3, 0, 0, 0, 0);
    a.insert(a.end(), b.begin(), b.end());
    return a;
}
""")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O0", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])
