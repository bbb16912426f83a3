"""The device stopping rule of code sets without a GPU: the exported entry point against the header, its refusal of a null context,
the C example, host.replay_stop_rule on hand-made records with the answers written out, and the batch schedule the GPU test
computes frames_decoded from."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from codeset_stop_sets import CASES, code_set, frames_launched, schedule, stop_piece
from ldpc_testlib import ROOT

EINVAL = -1
ERR = 1 << 30   # bit 30 of a record: the frame has a wrong bit


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


def test_symbol_header_and_methods(L):
    lib = L.load_library()
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        header = f.read()
    assert hasattr(lib, "ldpc_hip_simulate_codes_stop")
    assert re.search(r"\bint\s+ldpc_hip_simulate_codes_stop\s*\(", header)
    assert re.search(r"#define\s+LDPC_HIP_ABI_VERSION\s+4\b", header) and lib.ldpc_hip_abi_version() == 4
    assert callable(L.LdpcHipCodes.simulate_until)
    assert L.host.replay_stop_rule is L.replay_stop_rule and "replay_stop_rule" in L.__all__


def test_null_context_is_refused(L):
    lib = L.load_library()
    state = (C.c_ulonglong * 4)(7, 7, 7, 7)
    assert lib.ldpc_hip_simulate_codes_stop(None, 2.0, 0, 10, 0.8, 1, 0, 25, 1000, 0.05, 64, 64, state) == EINVAL
    assert "code-set context" in lib.ldpc_hip_last_error().decode()
    assert list(state) == [7, 7, 7, 7]


def test_c_example_builds_against_the_header(tmp_path):
    exe = tmp_path / "simulate_codes_stop"
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "simulate_codes_stop.c"),
                           "-o", str(exe), "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    assert exe.exists()


def records(n, errors):
    """n clean records with errors {frame index: wrong information bits}."""
    r = np.zeros(n, dtype=np.int32)
    for i, bits in errors.items():
        r[i] = ERR | bits
    return r


# name -> (records, n_frame_errors, n_experiments, reference_frame_error, (experiment, nse, nde))
REPLAY = {
    # the third error is frame 64, the last of a 64-frame batch; the error in frame 65 is not reached.  An error frame may have all
    # its wrong bits in the parity part: the record is bit 30 alone
    "n_frame_errors on a batch boundary": (records(128, {10: 3, 20: 0, 63: 5, 64: 9}), 3, 1000, 1.0, (64, 8, 3)),
    # experiment <= n_experiments admits frame n_experiments + 1 = 6 (an error frame here) and no more
    "experiment > n_experiments": (records(10, {5: 2, 6: 4}), 100, 5, 1.0, (6, 2, 1)),
    # 9 / 9 > 0.125 as well, but the rule asks for 10 error frames
    "FER rule at the 10th error, not the 9th": (records(20, {i: 1 for i in range(20)}), 100, 1000, 0.05, (10, 10, 10)),
    # 10 / 32 == 2.5 * 0.125 exactly (both are 0.3125): no stop; the 11th error ends the run by n_frame_errors
    "FER quotient equal to the bound": (records(64, {**{i: 1 for i in range(9)}, 31: 1, 40: 1, 41: 7}), 11, 1000, 0.125, (41, 11, 11)),
    # one frame earlier the quotient is 10 / 31 > 0.3125
    "FER quotient just above the bound": (records(64, {**{i: 1 for i in range(9)}, 30: 1, 40: 1}), 11, 1000, 0.125, (31, 10, 10)),
    # 2.5 * 0 = 0: any 10th error stops
    "reference_frame_error 0": (records(1200, {100 * i + 99: 2 for i in range(12)}), 50, 5000, 0.0, (1000, 20, 10)),
    # frame 20 is the 10th error (n_frame_errors), fires the FER rule and is frame n_experiments + 1
    "all stops on one frame": (records(40, {**{i: 3 for i in range(9)}, 19: 4, 20: 1}), 10, 19, 0.05, (20, 31, 10)),
    "no error at all": (records(200, {}), 5, 99, 0.05, (100, 0, 0)),
    # fewer records than the rule would consume
    "records run out": (records(7, {6: 1}), 5, 99, 0.05, (7, 1, 1)),
    "n_frame_errors 0": (records(7, {0: 1}), 0, 99, 0.05, (0, 0, 0)),
    "n_experiments 0": (records(7, {0: 1, 1: 1}), 5, 0, 0.05, (1, 1, 1)),
}


@pytest.mark.parametrize("name", sorted(REPLAY))
def test_replay_stop_rule(L, name):
    rec, nfe, nexp, ref, want = REPLAY[name]
    got = L.host.replay_stop_rule(rec, nfe, nexp, ref)
    assert got == want and all(type(v) is int for v in got)
    assert L.host.replay_stop_rule(list(rec), nfe, nexp, ref) == want   # any sequence of integers


def test_replay_agrees_with_the_batch_walk_of_bp_simulation(L):
    """replay_stopping_rule (the batched walk bp_simulation uses for one code) and replay_stop_rule give the same counters."""
    rng = np.random.RandomState(3)
    for trial in range(50):
        n = 400
        rec = np.where(rng.rand(n) < rng.choice([0.01, 0.05, 0.3]), ERR | rng.randint(0, 50, n), 0).astype(np.int32)
        nfe, nexp, ref = int(rng.randint(1, 30)), int(rng.randint(0, 500)), float(rng.choice([0.0, 0.01, 0.05, 1.0]))
        state = dict(nse=0, nde=0, nue=0, experiment=0)
        for lo in range(0, n, 64):
            if L.replay_stopping_rule(rec[lo:lo + 64], np.ones(len(rec[lo:lo + 64]), dtype=np.int32), state, nfe, nexp, ref):
                break
        assert L.host.replay_stop_rule(rec, nfe, nexp, ref) == (state["experiment"], state["nse"], state["nde"]), trial


def test_schedule():
    assert schedule(1500, 64, 64) == [(i, 64) for i in range(23)] + [(23, 29)]
    assert schedule(1500, 1024, 65536) == [(0, 1024), (1, 477)]
    assert schedule(5000, 64, 1024) == [(0, 64), (1, 256), (2, 1024), (3, 1024), (4, 1024), (5, 1024), (6, 585)]
    assert schedule(0, 64, 64) == [(0, 1)]
    assert schedule(99, 64, 64, piece=48) == [(0, 48), (0, 16), (1, 36)]
    pieces = schedule(1500, 64, 64)
    assert stop_piece(1, pieces) == 0 and stop_piece(64, pieces) == 0 and stop_piece(65, pieces) == 1 and stop_piece(1501, pieces) == 23
    assert frames_launched(64, pieces) == 64 and frames_launched(65, pieces) == 128 and frames_launched(1501, pieces) == 1501


def test_code_sets_are_accepted(L):
    """Every set of the GPU test passes the table builder for its decoder, and its code 0 is the all-weight-1 matrix."""
    for name, (dec, M, *_rest) in CASES.items():
        codes = code_set(M)
        assert 3 <= len(codes) <= 5
        assert ((codes[0] >= 0).sum(axis=0) == 1).all() and ((codes[0] >= 0).sum(axis=1) == 2).all(), name
        off, tab = L.codes_table(dec, codes, M)
        assert len(off) == len(codes)
