"""The stopping rule of a code set on the device (LdpcHipCodes.simulate_until / ldpc_hip_simulate_codes_stop): experiment, nse and
nde per code as exact integers against host.replay_stop_rule over the records of the existing route (simulate(records=True)), for
the three decoders at three liftings; invariance under the batch schedule, the pieces, first_frame and puncturing; frames_decoded
and the launch count against the schedule (stopped codes are skipped); edges, refusals and the C++ harness on both of its routes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from codeset_stop_sets import CASES, MAXITER, code_set, frames_launched, schedule, stop_piece
from ldpc_testlib import MS_DEC, ROOT

pytestmark = pytest.mark.gpu

EINVAL = -1
BATCH = 64


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


_REF = {}


def reference(L, name, first_frame=0, punct=0):
    """Once per (case, first_frame, punctured blocks): the records of n_experiments + 1 frames of every code through the existing
    route, and the sequential rule over each row."""
    key = (name, first_frame, punct)
    if key not in _REF:
        dec, M, snr, seed, nfe, nexp, ref_fer = CASES[name]
        codes = code_set(M)
        with L.LdpcHipCodes(dec, codes, M) as cs:
            _, info = cs.simulate(snr, MAXITER, seed, first_frame, nexp + 1, punctured_blocks=punct, records=True)
        _REF[key] = np.array([L.host.replay_stop_rule(row, nfe, nexp, ref_fer) for row in info], dtype=np.uint64)
    return _REF[key]


def stop_batches(want, nexp, first_batch=BATCH, max_batch=BATCH):
    """The batch in which every code stops, from the reference."""
    pieces = schedule(nexp, first_batch, max_batch)
    return [pieces[stop_piece(int(e), pieces)][0] for e in want[:, 0]]


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_sequential_rule(L, torch, name, monkeypatch):
    dec, M, snr, seed, nfe, nexp, ref_fer = CASES[name]
    want = reference(L, name)
    batches = stop_batches(want, nexp)
    print(name, "reference (experiment, nse, nde):", want.tolist(), "stop batches of 64:", batches)
    assert len(set(batches)) >= (3 if name == "ms_M32" else 2), "a set whose codes all stop together shows nothing"
    assert batches[0] == min(batches) and batches.count(batches[0]) == 1, "code 0 stops first and alone: slot 0 is code 1 afterwards"
    codes = code_set(M)
    with L.LdpcHipCodes(dec, codes, M) as cs:
        cs.profile(True)
        got = cs.simulate_until(snr, MAXITER, seed, nfe, nexp, ref_fer, first_batch=BATCH, max_batch=BATCH)
        _, launches = cs.profile_read()
        cs.profile(False)
        wide = cs.simulate_until(snr, MAXITER, seed, nfe, nexp, ref_fer, first_batch=1024, max_batch=65536)
        default = cs.simulate_until(snr, MAXITER, seed, nfe, nexp, ref_fer)
        ramp = cs.simulate_until(snr, MAXITER, seed, nfe, nexp, ref_fer, first_batch=3, max_batch=200)
        monkeypatch.setenv("LDPC_HIP_CODES_PIECE", "48")
        cut = cs.simulate_until(snr, MAXITER, seed, nfe, nexp, ref_fer, first_batch=BATCH, max_batch=BATCH)
        cut_wide = cs.simulate_until(snr, MAXITER, seed, nfe, nexp, ref_fer, first_batch=1024, max_batch=65536)
        monkeypatch.delenv("LDPC_HIP_CODES_PIECE")
    print(name, "device:", got.tolist())
    assert got.dtype == np.uint64 and got.shape == (len(codes), 4)
    for what, res in (("64/64", got), ("1024/65536", wide), ("default", default), ("3/200", ramp), ("pieces of 48", cut), ("pieces of 48, 1024/65536", cut_wide)):
        assert np.array_equal(res[:, :3], want), (what, res.tolist(), want.tolist())
    # skipping: every frame launched for a code, from the schedule
    for what, res, pieces in (("64/64", got, schedule(nexp, BATCH, BATCH)), ("1024/65536", wide, schedule(nexp, 1024, 65536)),
                              ("default", default, schedule(nexp, 1024, 65536)), ("3/200", ramp, schedule(nexp, 3, 200)),
                              ("pieces of 48", cut, schedule(nexp, BATCH, BATCH, piece=48)),
                              ("pieces of 48, 1024/65536", cut_wide, schedule(nexp, 1024, 65536, piece=48))):
        assert res[:, 3].tolist() == [frames_launched(int(e), pieces) for e in want[:, 0]], (what, res.tolist())
    fd = got[:, 3].astype(np.int64)
    assert fd.tolist() == [min(BATCH * (b + 1), nexp + 1) for b in batches]      # whole batches up to the stop batch
    assert fd.sum() < len(codes) * fd.max()
    assert launches == max(batches) + 1, "one decode launch per piece in which a code was running"


def test_first_frame(L, torch):
    name = "ms_M32"
    dec, M, snr, seed, nfe, nexp, ref_fer = CASES[name]
    want = reference(L, name, first_frame=1000)
    assert not np.array_equal(want, reference(L, name)), "other noise, other counters"
    with L.LdpcHipCodes(dec, code_set(M), M) as cs:
        got = cs.simulate_until(snr, MAXITER, seed, nfe, nexp, ref_fer, first_frame=1000, first_batch=BATCH, max_batch=BATCH)
    assert np.array_equal(got[:, :3], want), (got.tolist(), want.tolist())


def test_punctured_block(L, torch):
    name = "lms_M20"
    dec, M, snr, seed, nfe, nexp, ref_fer = CASES[name]
    want = reference(L, name, punct=1)
    assert not np.array_equal(want, reference(L, name))
    with L.LdpcHipCodes(dec, code_set(M), M) as cs:
        got = cs.simulate_until(snr, MAXITER, seed, nfe, nexp, ref_fer, first_batch=BATCH, max_batch=BATCH, punctured_blocks=1)
    assert np.array_equal(got[:, :3], want), (got.tolist(), want.tolist())


def test_edges(L, torch):
    name = "ms_M32"
    dec, M, snr, seed, nfe, nexp, ref_fer = CASES[name]
    codes = code_set(M)
    with L.LdpcHipCodes(dec, codes, M) as cs:
        cs.profile(True)
        for a, b in ((0, nexp), (-3, nexp), (nfe, -1)):   # :591 fails before the first frame
            assert not cs.simulate_until(snr, MAXITER, seed, a, b, ref_fer).any()
        assert cs.profile_read()[1] == 0, "nothing is launched"
        one = cs.simulate_until(snr, MAXITER, seed, nfe, 0, ref_fer)
        assert cs.profile_read()[1] == 1
        _, info = cs.simulate(snr, MAXITER, seed, 0, 1, records=True)
    assert one[:, 0].tolist() == [1] * len(codes) and one[:, 3].tolist() == [1] * len(codes)
    assert one[:, 1].tolist() == (info[:, 0] & ((1 << 30) - 1)).tolist() and one[:, 2].tolist() == (info[:, 0] != 0).astype(int).tolist()
    # a set of one code: the medium code alone gives its row of the set's result
    want = reference(L, name)
    with L.LdpcHipCodes(dec, codes[1:2], M) as cs:
        alone = cs.simulate_until(snr, MAXITER, seed, nfe, nexp, ref_fer, first_batch=BATCH, max_batch=BATCH)
    assert alone.shape == (1, 4) and np.array_equal(alone[0, :3], want[1])
    assert alone[0, 3] == frames_launched(int(want[1, 0]), schedule(nexp, BATCH, BATCH))


def test_refusals(L, torch):
    lib = L.load_library()
    codes = code_set(32)
    state = (C.c_ulonglong * (4 * len(codes)))(*([5] * (4 * len(codes))))

    def call(h, maxiter=10, first_batch=64, max_batch=64, st=state, first_frame=0, punct=0):
        return lib.ldpc_hip_simulate_codes_stop(h, 4.0, punct, maxiter, 0.8, 1, first_frame, 12, 100, 0.05, first_batch, max_batch, st)

    with L.LdpcHipCodes(MS_DEC, codes, 32) as cs, L.LdpcHip(MS_DEC, codes[1], 32) as lone:
        cs.profile(True)
        assert call(lone.h) == EINVAL and "code-set context" in lib.ldpc_hip_last_error().decode()
        assert call(cs.h, st=None) == EINVAL
        assert call(cs.h, first_batch=0) == EINVAL and call(cs.h, first_batch=-4) == EINVAL
        assert call(cs.h, first_batch=65, max_batch=64) == EINVAL
        assert call(cs.h, maxiter=0) == EINVAL and call(cs.h, maxiter=-1) == EINVAL
        assert call(cs.h, first_frame=-1) == EINVAL and call(cs.h, punct=8) == EINVAL
        assert cs.profile_read()[1] == 0 and list(state) == [5] * len(state), "a refused call launches nothing and leaves state alone"
        assert call(cs.h) == 0 and list(state)[0] > 0   # and the context still works


def test_cpp_harness_takes_both_routes(L, torch, tmp_path):
    """ldpc::bp_simulation_codes with show_process = 0 (the rule on the device) and = 1 (the records replayed on the host) on the
    same set: the same return values and counters."""
    L.load_library()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = str(tmp_path / "codes_stop_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "codes_stop_driver.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_compat", "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    for name in ("ms_M32", "tdmp_M20"):
        dec, M, snr, seed, nfe, nexp, ref_fer = CASES[name]
        codes = code_set(M)
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(np.array([len(codes), codes.shape[1], codes.shape[2], M, dec, MAXITER, nfe, nexp, BATCH, seed], dtype=np.int32).tobytes())
            f.write(np.array([snr, ref_fer], dtype=np.float64).tobytes())
            f.write(codes.tobytes())
        out = subprocess.check_output([exe, str(tmp_path / "in.bin")], timeout=120).decode().split("\n")
        rows = {(w[0], int(w[1])): w[2:] for w in (line.split() for line in out if line.startswith(("device ", "host ")))}
        assert len(rows) == 2 * len(codes), out
        assert any(line.startswith("code=") for line in out), "show_process = 1 prints a line per error frame"
        want = reference(L, name)
        for c in range(len(codes)):
            assert rows["device", c] == rows["host", c], (name, c, rows["device", c], rows["host", c])
            assert [int(v) for v in rows["device", c][2:]] == [int(want[c, 1]), int(want[c, 2]), int(want[c, 0])], (name, c)
