"""Exact replay on code sets (ldpc_hip_mt_*_codes, LdpcHipCodes.mt_*, ldpc::bp_simulation_codes_exact, `ldpc_sim --code-sets`):
upstream's own mt19937 / polar-method noise drawn once and decoded by every code of a set.  Per code everything is compared with
tolerance 0 against the single-code exact route (LdpcHip.mt_frames, host.bp_simulation(exact_seed=)) from the same generator state
and, for the decoders it restates, against the sequential CPU oracle (oracle/harness_oracle.cpp).

One refusal of the entry points is not exercised: LDPC_HIP_EUNSUPPORTED for a frame longer than one generation round (2^27 samples).
No set can be opened that long -- M <= 512 and every set kernel's LDS image bound N to a few ten thousand (ldpc_codeset_api.hpp,
codeset_build) -- so the check of the shared mt_frame_proto cannot be reached through a set context."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from codeset_gfq_sets import weak_first_set
from codeset_sp_sets import appendix_c
from codeset_stop_sets import MAXITER, NH, RH, code_set, frames_launched, schedule
from ldpc_testlib import LMS_DEC, MS_DEC, ROOT, SimResult, c_int_p, oracle_lib

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -2
SP_DEC, ASP_DEC, IMS_DEC, IASP_DEC, TASP_DEC, LCHE_DEC = 1, 2, 4, 5, 7, 9
DECS = {"ms": MS_DEC, "lms": LMS_DEC, "tdmp": TASP_DEC, "iasp": IASP_DEC, "lche": LCHE_DEC, "ims": IMS_DEC, "sp": SP_DEC, "asp": ASP_DEC}
ORACLE_DECS = (MS_DEC, LMS_DEC, TASP_DEC, IMS_DEC, SP_DEC, ASP_DEC)   # what orc_bp_simulation restates
SEED = 9
# the three ways a run ends: name -> SNR [dB], n_frame_errors, n_experiments, reference_frame_error
ENDINGS = {"frame_errors": (2.5, 7, 300, 1.0), "fer_rule": (1.1, 10**9, 300, 0.02), "experiments": (4.0, 10**9, 300, 1.0)}


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module", autouse=True)
def table_tier(L):
    """The single-code contexts of the comparisons open on the table-driven / shape-unlimited tier (identical bits, no hiprtc)."""
    lib = L.load_library()
    before = lib.ldpc_hip_set_jit_mode(0)
    yield
    lib.ldpc_hip_set_jit_mode(before)


def entry_state(L, M, seed=SEED, rh=RH, nh=NH):
    """std::mt19937(seed) after the codeword draws of bp_simulation.cpp:512: where the first frame's noise starts"""
    return L.mt19937_state(seed, (nh - rh) * M)


def next_word(L, state, pos):
    """the generator's next tempered output"""
    bg = np.random.MT19937()
    s = bg.state
    s["state"]["key"] = np.array(state, dtype=np.uint32)
    s["state"]["pos"] = int(pos)
    bg.state = s
    return int(bg.random_raw(1)[0])


def host_rule(L, info, iters, nfe, nexp, ref):
    """experiment, nse, nde, nue, sum |iters| of the sequential rule over one code's ordered records"""
    st = {"nse": 0, "nde": 0, "nue": 0, "experiment": 0}
    L.replay_stopping_rule(info, iters, st, nfe, nexp, ref)
    return [st["experiment"], st["nse"], st["nde"], st["nue"], int(np.abs(iters[:st["experiment"]].astype(np.int64)).sum())]


_ORACLE = {}


def oracle_run(H, M, dec, snr, nfe, nexp, ref, punct=0, seed=SEED, maxiter=MAXITER):
    key = (H.tobytes(), M, dec, snr, nfe, nexp, ref, punct, seed, maxiter)
    if key not in _ORACLE:
        res = SimResult()
        Hc = np.ascontiguousarray(H, dtype=np.int32)
        assert oracle_lib().orc_bp_simulation(H.shape[0], H.shape[1], Hc.ctypes.data_as(c_int_p), M, maxiter, nfe, nexp, snr, ref, dec, 0, punct, seed,
                                              C.byref(res), None) == 0
        _ORACLE[key] = ([res.experiment, res.nse, res.nde, res.nue, res.sum_abs_iter], res.ber, res.fer, res.rng_next)
    return _ORACLE[key]


def single_route(L, H, M, dec, snr, nfe, nexp, ref, punct=0):
    """The single-code exact route: (five counters, BER, FER, next word of the generator)"""
    ber, fer, st = L.bp_simulation(H, M, MAXITER, nfe, nexp, snr, ref, decoder_type=dec, punctured_blocks=punct, exact_seed=SEED, batch=128,
                                   return_state=True)
    return [st["experiment"], st["nse"], st["nde"], st["nue"], st["sum_abs_iters"]], ber, fer, next_word(L, *st["generator"])


# ---- 1. records ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dec", list(DECS.values()), ids=list(DECS))
def test_records_equal_the_single_code_route(L, torch, dec):
    B, snr = 37, 3.0
    for M in (20, 32, 64, 126):   # three frames per wave, two, one, two waves per frame
        codes = code_set(M)
        st = entry_state(L, M)
        with L.LdpcHipCodes(dec, codes, M) as cs:
            cs.mt_set_state(*st)
            cnt, info, its = cs.mt_simulate(snr, MAXITER, B, records=True)
            after = cs.mt_get_state()
        assert info.shape == its.shape == (len(codes), B) and cnt.shape == (len(codes), 5)
        for c, H in enumerate(codes):
            with L.LdpcHip(dec, H, M) as one:
                one.mt_set_state(*st)
                want_info, want_its = one.mt_frames(snr, MAXITER, B)
                want_after = one.mt_get_state()
            assert np.array_equal(info[c], want_info), (M, c, info[c].tolist(), want_info.tolist())
            assert np.array_equal(its[c], want_its), (M, c, its[c].tolist(), want_its.tolist())
            assert np.array_equal(after[0], want_after[0]) and after[1] == want_after[1], (M, c)
            err = want_info != 0
            assert cnt[c].tolist() == [int((want_info[err] & ((1 << 30) - 1)).sum()), int(err.sum()), int((err & (want_its >= 0)).sum()), B,
                                       int(np.abs(want_its).sum())], (M, c)
        assert (info != 0).any() and (info == 0).any(), "a set without error frames, or with nothing else, shows little"


# ---- 2. the rule on the device ------------------------------------------------------------------------------------------------------
_RECORDS = {}


def records_reference(L, dec, M, snr, nexp, punct=0):
    """Once per case: the ordered records of n_experiments + 1 frames of every code"""
    key = (dec, M, snr, nexp, punct)
    if key not in _RECORDS:
        with L.LdpcHipCodes(dec, code_set(M), M) as cs:
            cs.mt_set_state(*entry_state(L, M))
            _, info, its = cs.mt_simulate(snr, MAXITER, nexp + 1, punctured_blocks=punct, records=True)
        _RECORDS[key] = (info, its)
    return _RECORDS[key]


@pytest.mark.parametrize("ending", list(ENDINGS))
@pytest.mark.parametrize("dec", list(DECS.values()), ids=list(DECS))
def test_rule_on_the_device(L, torch, dec, ending):
    M = 32
    snr, nfe, nexp, ref = ENDINGS[ending]
    codes = code_set(M)
    info, its = records_reference(L, dec, M, snr, nexp)
    want = np.array([host_rule(L, info[c], its[c], nfe, nexp, ref) for c in range(len(codes))], dtype=np.uint64)
    with L.LdpcHipCodes(dec, codes, M) as cs:
        cs.mt_set_state(*entry_state(L, M))
        got = cs.mt_simulate_until(snr, MAXITER, nfe, nexp, ref, first_batch=64, max_batch=64)
    print(ending, "device:", got.tolist())
    assert got.dtype == np.uint64 and got.shape == (len(codes), 6)
    assert np.array_equal(got[:, :5], want), (got.tolist(), want.tolist())
    if ending == "frame_errors":
        assert want[0, 2] == nfe and want[0, 0] == want[:, 0].min() and (want[1:, 0] > want[0, 0]).all(), "the weak code stops first, on its error frames"
    if ending == "fer_rule":
        assert (want[:, 2] >= 10).all() and (want[:, 0] < nexp + 1).all(), "every code ends on the FER rule"
    if ending == "experiments":
        assert (want[:, 0] == nexp + 1).all()
    for c, H in enumerate(codes):
        info_len = (NH - RH) * M
        ber, fer = int(got[c, 1]) / int(got[c, 0]) / info_len, int(got[c, 2]) / int(got[c, 0])
        if dec in ORACLE_DECS:
            cnt, ober, ofer, _ = oracle_run(H, M, dec, snr, nfe, nexp, ref)
        else:
            cnt, ober, ofer, _ = single_route(L, H, M, dec, snr, nfe, nexp, ref)
        assert got[c, :5].tolist() == cnt and ber == ober and fer == ofer, (c, got[c].tolist(), cnt)


# ---- 3. invariance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dec,M", [(MS_DEC, 32), (TASP_DEC, 20)], ids=["ms_M32", "tdmp_M20"])
def test_schedule_and_pieces_do_not_matter(L, torch, monkeypatch, dec, M):
    snr, nfe, nexp, ref = ENDINGS["frame_errors"]
    codes = code_set(M)
    info, its = records_reference(L, dec, M, snr, nexp)
    want = np.array([host_rule(L, info[c], its[c], nfe, nexp, ref) for c in range(len(codes))], dtype=np.uint64)
    assert len(set(want[:, 0].tolist())) >= 2, "a set whose codes all stop together shows nothing"
    with L.LdpcHipCodes(dec, codes, M) as cs:
        for piece in (None, 7):
            if piece:
                monkeypatch.setenv("LDPC_HIP_CODES_PIECE", str(piece))
            for first_batch in (1, 64, 256):
                for max_batch in (256, 1024):
                    cs.mt_set_state(*entry_state(L, M))
                    got = cs.mt_simulate_until(snr, MAXITER, nfe, nexp, ref, first_batch=first_batch, max_batch=max_batch)
                    assert np.array_equal(got[:, :5], want), (piece, first_batch, max_batch, got.tolist(), want.tolist())
                    pieces = schedule(nexp, first_batch, max_batch, **({"piece": piece} if piece else {}))
                    assert got[:, 5].tolist() == [frames_launched(int(e), pieces) for e in want[:, 0]], (piece, first_batch, max_batch, got.tolist())
        monkeypatch.delenv("LDPC_HIP_CODES_PIECE")


# ---- 4. the generator ---------------------------------------------------------------------------------------------------------------
def test_generator_before_and_after(L, torch):
    dec, M = MS_DEC, 32
    snr, nfe, nexp, ref = ENDINGS["frame_errors"]
    codes = code_set(M)
    st = entry_state(L, M)
    with L.LdpcHipCodes(dec, codes, M) as cs, L.LdpcHip(dec, codes[1], M) as one:
        cs.mt_set_state(*st)
        got = cs.mt_simulate_until(snr, MAXITER, nfe, nexp, ref, first_batch=64, max_batch=256)
        back = cs.mt_get_state()
        assert np.array_equal(back[0], st[0]) and back[1] == st[1], "the run puts the generator back where it found it"
        for c, H in enumerate(codes):   # ... and mt_advance takes it to the end of code c's run
            cs.mt_set_state(*st)
            cs.mt_advance(snr, int(got[c, 0]))
            assert next_word(L, *cs.mt_get_state()) == oracle_run(H, M, dec, snr, nfe, nexp, ref)[3], c
        # mt_simulate of B frames ends where a single context that draws and drops B frames ends
        for B in (1, 37, 1000):
            cs.mt_set_state(*st)
            one.mt_set_state(*st)
            cs.mt_simulate(snr, MAXITER, B)
            one.mt_llr(snr, B, skip=True)
            a, b = cs.mt_get_state(), one.mt_get_state()
            assert np.array_equal(a[0], b[0]) and a[1] == b[1], B
        # nothing to do: no frame is consumed (:591 fails before the first frame)
        cs.mt_set_state(*st)
        for a, b in ((0, nexp), (-3, nexp), (nfe, -1)):
            assert not cs.mt_simulate_until(snr, MAXITER, a, b, ref).any()
        back = cs.mt_get_state()
        assert np.array_equal(back[0], st[0]) and back[1] == st[1]


# ---- 5. puncturing ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dec", [LMS_DEC, TASP_DEC], ids=["lms_0p5", "tdmp_0p0"])
def test_two_punctured_blocks(L, torch, dec):
    M, punct = 32, 2
    snr, nfe, nexp, ref = 4.5, 7, 300, 1.0
    codes = code_set(M)
    with L.LdpcHipCodes(dec, codes, M) as cs:
        cs.mt_set_state(*entry_state(L, M))
        got = cs.mt_simulate_until(snr, MAXITER, nfe, nexp, ref, first_batch=64, max_batch=256, punctured_blocks=punct)
        cs.mt_set_state(*entry_state(L, M))
        plain = cs.mt_simulate_until(snr, MAXITER, nfe, nexp, ref, first_batch=64, max_batch=256)
    assert not np.array_equal(got[:, :5], plain[:, :5]), "other positions erased, other counters"
    for c, H in enumerate(codes):
        cnt, _, _, _ = single_route(L, H, M, dec, snr, nfe, nexp, ref, punct=punct)
        assert got[c, :5].tolist() == cnt, (c, got[c].tolist(), cnt)


# ---- 6. anchors ---------------------------------------------------------------------------------------------------------------------
def shifted(H, M, k):
    """Another code on the same pattern: a shift per circulant that is no relabelling of rows or columns"""
    i, j = np.indices(H.shape)
    return np.where(H >= 0, (H.astype(np.int32) + k * (i * j + 1)) % M, -1).astype(np.int16)


@pytest.mark.parametrize("dec,M,snr,maxiter,nfe,nexp,anchor", [(MS_DEC, 64, 2.0, 50, 10**9, 4000, (170, 4001)), (TASP_DEC, 126, 1.7, 15, 50, 10**8, (50, 821))],
                         ids=["cfg2_170_of_4001", "tdmp_50_of_821"])
def test_anchors(L, torch, dec, M, snr, maxiter, nfe, nexp, anchor):
    H = appendix_c(M)[0]
    codes = np.array([shifted(H, M, 5), H, shifted(H, M, 11)], dtype=np.int16)
    with L.LdpcHipCodes(dec, codes, M) as cs:
        cs.mt_set_state(*entry_state(L, M, seed=1, rh=16, nh=32))
        got = cs.mt_simulate_until(snr, maxiter, nfe, nexp, 1.0)
    print("anchor run:", got.tolist())
    assert (int(got[1, 2]), int(got[1, 0])) == anchor
    assert got[0, :5].tolist() != got[1, :5].tolist() and got[2, :5].tolist() != got[1, :5].tolist(), "the neighbours are other codes"


# ---- 7. the C++ layer ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def compat(L):
    L.load_library()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    lib = C.CDLL(os.path.join(ROOT, "ldpc-lib_amd", "libldpc_compat.so"))
    lib.ldpc_bp_simulation_codes_exact.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                                   C.c_int, C.c_int, C.c_uint, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]
    return lib


@pytest.mark.parametrize("show", [0, 1])
@pytest.mark.parametrize("noise", ["device", "host"])
def test_cpp_layer(L, torch, compat, monkeypatch, noise, show):
    dec, M = MS_DEC, 32
    snr, nfe, nexp, ref = 2.5, 7, 300, 0.05
    monkeypatch.setenv("LDPC_HIP_EXACT_NOISE", noise)
    codes = code_set(M)
    flat = np.ascontiguousarray(codes, dtype=np.int32)
    for leave_at in (0, -1):
        out = np.zeros((len(codes), 7), dtype=np.float64)
        nxt = C.c_uint()
        assert compat.ldpc_bp_simulation_codes_exact(len(codes), RH, NH, flat.ctypes.data, M, MAXITER, nfe, nexp, snr, ref, dec, 0, show, SEED, 0, 64, 256,
                                                     leave_at, out.ctypes.data, C.addressof(nxt)) == 0
        for c, H in enumerate(codes):
            cnt, ber, fer, _ = oracle_run(H, M, dec, snr, nfe, nexp, ref)
            assert [int(out[c, 5]), int(out[c, 2]), int(out[c, 3]), int(out[c, 4]), int(out[c, 6])] == cnt, (leave_at, c, out[c].tolist(), cnt)
            assert out[c, 0] == ber and out[c, 1] == fer
        assert nxt.value == oracle_run(codes[leave_at], M, dec, snr, nfe, nexp, ref)[3], leave_at
    assert oracle_run(codes[0], M, dec, snr, nfe, nexp, ref)[3] != oracle_run(codes[-1], M, dec, snr, nfe, nexp, ref)[3]


# ---- 8. ldpc_sim --------------------------------------------------------------------------------------------------------------------
def code_record(H, dec, M, snrs):
    rows = "\n".join("        " + " ".join("%4d" % v for v in row) for row in H)
    return """    {
      _SNRs = array { %s }
      _decoder_type = %d
      _iterations = %d
      _lifting = %d
      _q_mod = 2
      _marking = "skip"
      _punctured_blocks = 0
      code = matrix (%d %d) {
%s
      }
      girth = 6
    }""" % (" ".join(str(s) for s in snrs), dec, MAXITER, M, H.shape[0], H.shape[1], rows)


def test_ldpc_sim_code_sets(L, torch, tmp_path):
    M = 32
    codes = code_set(M)
    # three codes of one group, and one with another decoder that runs alone as it always did
    records = [code_record(codes[c], MS_DEC, M, (2.0, 3.0)) for c in (1, 2, 3)] + [code_record(codes[1], LMS_DEC, M, (2.0, 3.0))]
    scenario = tmp_path / "scenario.jsonx"
    scenario.write_text("""{
  settings = {
    random_seed = 3
    num_codewords = 300
    error_blocks = 1000000
    error_minimization = { name = "FER" threshold = 1 good_code_multiple = 1.25 }
    modulation_type = 0
    permutation_type = 0
    permutation_block = 128
    permutation_inter = 1
  }
  results = array {
%s
  }
}""" % "\n".join(records))
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = os.path.join(ROOT, "ldpc-lib_amd", "ldpc_sim")
    env = dict(os.environ, LDPC_HIP_JIT="0")
    plain = subprocess.run([exe, "simulation", str(scenario), str(tmp_path / "plain.jsonx")], capture_output=True, text=True, timeout=120, env=env)
    sets = subprocess.run([exe, "simulation", str(scenario), str(tmp_path / "sets.jsonx"), "--code-sets"], capture_output=True, text=True, timeout=120, env=env)
    assert plain.returncode == 0 and sets.returncode == 0, (plain.stderr, sets.stderr)
    assert "set of 3 codes" in sets.stdout and "set of" not in plain.stdout

    def without_time(path):
        text = path.read_text()
        assert len(re.findall(r"\btime = \S+", text)) == 4
        return re.sub(r"\btime = \S+", "time = -", text)

    a, b = without_time(tmp_path / "plain.jsonx"), without_time(tmp_path / "sets.jsonx")
    assert a == b
    fer = subprocess.check_output([exe, "jsonx-get", str(tmp_path / "sets.jsonx"), "results/0/simulation_logs/0/FER"], text=True)
    assert any(float(x) > 0 for x in fer.replace("array {", "").replace("}", "").split()), "error-free points compare nothing"


# ---- 9. refusals and cross-use ------------------------------------------------------------------------------------------------------
def test_refusals_and_cross_use(L, torch):
    lib = L.load_library()
    M = 32
    codes = code_set(M)
    st, pos = entry_state(L, M)
    words = np.ascontiguousarray(st, dtype=np.uint32)
    out_words = np.empty(624, dtype=np.uint32)
    out_pos = C.c_int()
    cnt = np.zeros((len(codes), 5), dtype=np.uint64)
    state = np.full((len(codes), 6), 5, dtype=np.uint64)
    info = np.empty(8, dtype=np.int32)

    def codes_entries(h, set_state=True):
        return ([lib.ldpc_hip_mt_set_state_codes(h, words.ctypes.data, pos)] if set_state else []) + [
                lib.ldpc_hip_mt_get_state_codes(h, out_words.ctypes.data, C.byref(out_pos)),
                lib.ldpc_hip_mt_advance_codes(h, 3.0, 0, 5),
                lib.ldpc_hip_mt_simulate_codes(h, 3.0, 0, MAXITER, 0.8, 5, cnt.ctypes.data, None, None),
                lib.ldpc_hip_mt_simulate_codes_stop(h, 3.0, 0, MAXITER, 0.8, 7, 100, 0.05, 64, 64, state.ctypes.data)]

    hb, hc = weak_first_set()
    with L.LdpcHip(MS_DEC, codes[1], M) as lone, L.LdpcHipGfq(4, hb[1], hc[1], 8) as gfq, L.LdpcHipCodesGfq(4, hb, hc, 8) as gfq_set:
        for ctx in (lone, gfq, gfq_set):
            assert codes_entries(ctx.h) == [EINVAL] * 5, type(ctx).__name__
            assert "code-set context" in lib.ldpc_hip_last_error().decode()
    assert (state == 5).all() and not cnt.any()
    with L.LdpcHipCodes(MS_DEC, codes, M) as cs:
        # the single-code entry points stay closed to a set
        assert lib.ldpc_hip_mt_set_state(cs.h, words.ctypes.data, pos) == EINVAL and "code-set context" in lib.ldpc_hip_last_error().decode()
        assert lib.ldpc_hip_mt_get_state(cs.h, out_words.ctypes.data, C.byref(out_pos)) == EINVAL
        assert lib.ldpc_hip_mt_llr_dev(cs.h, 3.0, 0, 0, 4, None, None) == EINVAL
        assert lib.ldpc_hip_mt_frames(cs.h, 3.0, 0, 0, MAXITER, 0.8, 8, info.ctypes.data, info.ctypes.data) == EINVAL
        assert lib.ldpc_hip_mt_normal_dev(cs.h, 4, None, None) == EINVAL
        # no generator state yet
        assert codes_entries(cs.h, set_state=False) == [EINVAL] * 4 and "no state" in lib.ldpc_hip_last_error().decode()
        assert (state == 5).all()
        cs.mt_set_state(st, pos)
        cs.profile(True)
        # arguments
        assert lib.ldpc_hip_mt_set_state_codes(cs.h, None, 0) == EINVAL and lib.ldpc_hip_mt_set_state_codes(cs.h, words.ctypes.data, 625) == EINVAL
        assert lib.ldpc_hip_mt_get_state_codes(cs.h, None, C.byref(out_pos)) == EINVAL
        assert lib.ldpc_hip_mt_advance_codes(cs.h, 3.0, 0, -1) == EINVAL and lib.ldpc_hip_mt_advance_codes(cs.h, 3.0, NH, 1) == EINVAL
        assert lib.ldpc_hip_mt_simulate_codes(cs.h, 3.0, 0, MAXITER, 0.8, 5, None, None, None) == EINVAL
        assert lib.ldpc_hip_mt_simulate_codes(cs.h, 3.0, 0, 0, 0.8, 5, cnt.ctypes.data, None, None) == EINVAL
        assert lib.ldpc_hip_mt_simulate_codes(cs.h, 3.0, -1, MAXITER, 0.8, 5, cnt.ctypes.data, None, None) == EINVAL

        def stop(maxiter=MAXITER, first_batch=64, max_batch=64, st_ptr=state.ctypes.data, punct=0):
            return lib.ldpc_hip_mt_simulate_codes_stop(cs.h, 3.0, punct, maxiter, 0.8, 7, 100, 0.05, first_batch, max_batch, st_ptr)

        assert stop(st_ptr=None) == EINVAL and stop(first_batch=0) == EINVAL and stop(first_batch=65) == EINVAL
        assert stop(maxiter=0) == EINVAL and stop(punct=NH) == EINVAL
        assert cs.profile_read()[1] == 0 and (state == 5).all(), "a refused call launches nothing and leaves state alone"
        back = cs.mt_get_state()
        assert np.array_equal(back[0], words) and back[1] == pos, "... and the generator too"
        assert stop() == 0 and state[0, 0] > 0   # and the context still works
