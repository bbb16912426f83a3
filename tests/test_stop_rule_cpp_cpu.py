"""ldpc::replay_stop_rule of include/ldpc/bp_simulation.h, the one replay of upstream's stopping rule behind every C++ harness, against
host.replay_stop_rule: tests/cpp/stop_rule_driver.cpp feeds it records in batches of 1, 7 and 64 frames; the counters are compared as
integers and must not depend on the batch size."""
import os
import subprocess

import numpy as np
import pytest

from ldpc_testlib import ROOT
from test_codeset_stop_cpu import ERR, REPLAY

BATCHES = (1, 7, 64)


def random_records(seed):
    """300 records, about 5 % error frames with up to 49 wrong information bits."""
    rng = np.random.RandomState(seed)
    return np.where(rng.rand(300) < 0.05, ERR | rng.randint(0, 50, 300), 0).astype(np.int32)


def cases():
    """name -> (records, n_frame_errors, n_experiments, reference_frame_error)"""
    out = {name: case[:4] for name, case in REPLAY.items()}
    for seed in range(30):
        rec = random_records(seed)
        # by turns: the 10th error frame at a reference rate it exceeds, a count of error frames the records hold, a frame limit
        # inside the records; the two limits not under test are out of reach, so that the named exit is the one that fires
        nfe, nexp, ref = ((1000, 1000, 0.01), (int(1 + seed % 9), 1000, 1.0), (1000, 37 + seed, 1.0))[seed % 3]
        out["random %d" % seed] = (rec, nfe, nexp, ref)
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import ldpc_lib_amd
    ldpc_lib_amd.load_library()
    exe = str(tmp_path_factory.mktemp("stop_rule") / "stop_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "stop_rule_driver.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    return exe


def run(driver, tmp_path, rec, iters, nfe, nexp, ref, batch):
    path = tmp_path / "records.txt"
    with open(path, "w") as f:
        f.write("%d %d %r %d %d\n" % (nfe, nexp, ref, batch, len(rec)))
        f.write("\n".join("%d %d" % (r, i) for r, i in zip(rec, iters)) + "\n")
    return tuple(int(v) for v in subprocess.check_output([driver, str(path)], text=True).split())


def test_replay_against_the_python_rule(driver, tmp_path):
    from ldpc_lib_amd import host
    exits = {"nde": [], "experiment": [], "fer": []}
    for name, (rec, nfe, nexp, ref) in cases().items():
        rec = np.asarray(rec, dtype=np.int32)
        iters = np.random.RandomState(len(name)).randint(-50, 51, len(rec))   # < 0: the decoder gave up, >= 0: an undetected error
        experiment, nse, nde = host.replay_stop_rule(rec, nfe, nexp, ref)
        bad = rec[:experiment] != 0
        want = (experiment, nse, nde, int((bad & (iters[:experiment] >= 0)).sum()), int(np.abs(iters[:experiment]).sum()))
        for batch in BATCHES:
            got = run(driver, tmp_path, rec, iters, nfe, nexp, ref, batch)
            print(name, "batch", batch, "got", got, "want", want)
            assert got[:5] == want, (name, batch)
            assert got[5] == (experiment - batch * ((experiment - 1) // batch) if experiment else 0), (name, batch)
        # which exit ended the run, and where in a batch of 64 (0 = on its last frame)
        if experiment < len(rec):
            if nde >= nfe > 0:
                exits["nde"].append(experiment % 64)
            elif experiment > nexp >= 0:
                exits["experiment"].append(experiment % 64)
            elif nde >= 10 and nde / experiment > 2.5 * ref:
                exits["fer"].append(experiment % 64)
    assert all(exits.values()), exits                               # each of the three exits fires
    assert any(pos != 0 for v in exits.values() for pos in v)       # ... one of them in the middle of a batch
