"""Exact replay of upstream's q-ary frame loop, the part that needs no GPU: the additive C-ABI and its refusals on a null context, the
defined message, the harness model's set-up against the compiled upstream where oracle/_ref exists, and the golden sets under
tests/golden/gfq_exact/ (tools/make_gfq_exact_goldens.py): their input conditions, and their records regenerated from the model."""
import ctypes as C
import glob
import os
import re
import sys

import numpy as np
import pytest

import gfq_harness_model as hm
from gfq_chain_ref import chain_ref_available, ref_left2right
from gfq_ref import GfqReference, gfq_ref_available
from ldpc_testlib import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_gfq_exact_goldens as maker  # noqa: E402

NEW_SYMBOLS = ("ldpc_hip_gfq_upstream_message", "ldpc_hip_gfq_set_codeword", "ldpc_hip_mt_set_state_gfq", "ldpc_hip_mt_get_state_gfq",
               "ldpc_hip_mt_advance_gfq", "ldpc_hip_mt_frames_gfq", "ldpc_hip_frames_gfq_noise_host",
               "ldpc_hip_codes_gfq_set_codewords", "ldpc_hip_mt_set_state_codes_gfq", "ldpc_hip_mt_get_state_codes_gfq", "ldpc_hip_mt_advance_codes_gfq",
               "ldpc_hip_mt_simulate_codes_gfq", "ldpc_hip_mt_simulate_codes_gfq_stop", "ldpc_hip_frames_codes_gfq_noise_host")


def _lib():
    import ldpc_lib_amd
    return ldpc_lib_amd.load_library()


def test_header_declares_and_library_exports_the_new_entries():
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        header = f.read()
    lib = _lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
    assert "{6, 11, 0, 4, 2, 1, 2, 5}" in header and "& (q - 1)" in header   # the defined message is written down where callers read
    assert lib.ldpc_hip_abi_version() == 4


@pytest.mark.parametrize("q_bits", [2, 4, 6])
@pytest.mark.parametrize("K", [3, 8, 32])
def test_upstream_message(q_bits, K):
    import ldpc_lib_amd
    msg = ldpc_lib_amd.gfq_upstream_message(q_bits, K)
    want = [v & ((1 << q_bits) - 1) for v in (6, 11, 0, 4, 2, 1, 2, 5)][:K] + [0] * max(K - 8, 0)
    assert msg.dtype == np.int16 and msg.tolist() == want
    assert np.array_equal(msg, hm.upstream_message(q_bits, K))
    if q_bits == 2:
        assert msg[:3].tolist() == [2, 3, 0]   # 6 and 11 do not exist in GF(4)


def test_upstream_message_bad_arguments():
    lib = _lib()
    buf = np.zeros(8, dtype=np.int16)
    for q_bits, K, ptr in ((1, 8, buf.ctypes.data), (11, 8, buf.ctypes.data), (4, -1, buf.ctypes.data), (4, 8, None)):
        assert lib.ldpc_hip_gfq_upstream_message(q_bits, K, ptr) == -1
    assert lib.ldpc_hip_gfq_upstream_message(4, 0, None) == 0
    assert not buf.any()


def test_every_new_entry_point_refuses_a_null_context():
    lib = _lib()
    st = np.zeros(624, dtype=np.uint32)
    pos = C.c_int()
    rec = np.zeros(4, dtype=np.int32)
    noise = np.zeros(64, dtype=np.float64)
    cnt = np.zeros(6, dtype=np.uint64)
    calls = {
        "ldpc_hip_gfq_set_codeword": (None, None),
        "ldpc_hip_mt_set_state_gfq": (None, st.ctypes.data, 624),
        "ldpc_hip_mt_get_state_gfq": (None, st.ctypes.data, C.byref(pos)),
        "ldpc_hip_mt_advance_gfq": (None, 1),
        "ldpc_hip_mt_frames_gfq": (None, 2.0, 0, 10, 1, rec.ctypes.data, rec.ctypes.data),
        "ldpc_hip_frames_gfq_noise_host": (None, noise.ctypes.data, 2.0, 0, 10, 1, rec.ctypes.data, rec.ctypes.data),
        "ldpc_hip_codes_gfq_set_codewords": (None, None),
        "ldpc_hip_mt_set_state_codes_gfq": (None, st.ctypes.data, 624),
        "ldpc_hip_mt_get_state_codes_gfq": (None, st.ctypes.data, C.byref(pos)),
        "ldpc_hip_mt_advance_codes_gfq": (None, 1),
        "ldpc_hip_mt_simulate_codes_gfq": (None, 2.0, 0, 10, 1, cnt.ctypes.data, rec.ctypes.data, rec.ctypes.data),
        "ldpc_hip_mt_simulate_codes_gfq_stop": (None, 2.0, 0, 10, 5, 100, 0.1, 16, 64, cnt.ctypes.data),
        "ldpc_hip_frames_codes_gfq_noise_host": (None, noise.ctypes.data, 2.0, 0, 10, 1, cnt.ctypes.data, rec.ctypes.data, rec.ctypes.data),
    }
    assert set(calls) | {"ldpc_hip_gfq_upstream_message"} == set(NEW_SYMBOLS)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -1, name
        assert (b"not a GF(q) code-set context" if "codes" in name else b"not a GF(q) context") in lib.ldpc_hip_last_error(), name


def test_inverse_left2right():
    rng = np.random.RandomState(4)
    for shape in ((2, 4), (3, 6), (4, 8), (3, 3)):
        m = rng.randint(-1, 60, shape)
        assert np.array_equal(hm.cm.left2right(hm.inverse_left2right(m)), m)


def test_golden_sets_exist_and_meet_the_conditions_on_the_inputs():
    names = {os.path.basename(p)[:-4] for p in glob.glob(os.path.join(hm.EXACT_GOLDEN_DIR, "*.npz"))}
    assert names == set(hm.CASES)
    sets = {n: hm.load(n) for n in names}
    maker.check_inputs(sets)
    for n, g in sets.items():
        assert os.path.getsize(os.path.join(hm.EXACT_GOLDEN_DIR, n + ".npz")) < 16 * 1024
        p = hm.CASES[n]
        assert 64 <= len(g["frame_info"]) == p["frames"] <= 512
        H, coef = hm.harness_inputs(n)
        assert np.array_equal(g["H"], H) and np.array_equal(g["coef"], coef)
    s1, s2, s3 = sets["s1_gf16_m8_enc"], sets["s2_gf4_m5_enc"], sets["s3_gf64_m7_enc"]
    assert (int(s1["q_bits"]), s1["hb"].shape, int(s1["M"])) == (4, (4, 8), 8) and ((s1["hb"] >= 0).sum(axis=0) == 2).all()
    assert (int(s2["q_bits"]), s2["hb"].shape, int(s2["M"])) == (2, (3, 6), 5)
    assert (int(s3["q_bits"]), s3["hb"].shape, int(s3["M"])) == (6, (3, 6), 7)


@pytest.mark.parametrize("name", sorted(hm.CASES))
def test_goldens_reproduce_from_the_model(name):
    """With oracle/_ref the decoder inside the loop is the compiled upstream, without it the numpy model: the records are the same."""
    g = hm.load(name)
    got = hm.run_case(name)
    for key in ("hb", "hc", "coef_back", "word", "frame_info", "iters", "counters", "stop_state"):
        assert np.array_equal(got[key], g[key]), key
    assert got["ber_fer"].tobytes() == g["ber_fer"].tobytes() and got["ending"] == str(g["ending"])
    assert float(got["max_lh"]) == float(g["max_lh"]) < 512
    # the stopping rule of the model is the one the library's host layer replays
    import ldpc_lib_amd
    assert ldpc_lib_amd.replay_stop_rule(g["frame_info"], int(g["stop"][0]), int(g["stop"][1]), float(g["stop"][2])) == tuple(int(v) for v in g["stop_state"])


@pytest.mark.skipif(not (gfq_ref_available() and chain_ref_available()), reason="oracle/_ref (the compiled upstream reference) is absent")
@pytest.mark.parametrize("name", sorted(hm.CASES))
def test_model_setup_equals_the_compiled_reference(name):
    """bp_simulation.cpp:348-399: decod_init with ncols2convert on the matrices as given, the rewritten hc, left2right of both."""
    p = hm.CASES[name]
    H, coef = hm.harness_inputs(name)
    ref = GfqReference(p["q_bits"], H, coef, p["M"], p["n2c"])
    back = ref.coefficients()
    ref.close()
    hb, hc, coef_back = hm.setup(p["q_bits"], H, coef, p["n2c"])
    assert np.array_equal(coef_back, back)
    assert np.array_equal(hb, ref_left2right(H)) and np.array_equal(hc, ref_left2right(back))
    assert (p["n2c"] > 0) == (not np.array_equal(back, coef))



def test_ldpc_sim_usage_is_unchanged():
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    res = subprocess.run([os.path.join(ROOT, "ldpc-lib_amd", "ldpc_sim")], capture_output=True, text=True)
    assert res.returncode == 1
    assert res.stderr == ("usage: ldpc_sim simulation <scenario file name> <result file name> [--throughput [--random-codewords N]] [--code-sets] "
                          "[--device N | --devices 0,1,.. | --devices all]\n"
                          "       ldpc_sim jsonx <in.jsonx> <out.jsonx>        re-emit in canonical form\n"
                          "       ldpc_sim jsonx-get <in.jsonx> <path/to/field>  print one value (falls back to 'defaults' records)\n")
