"""TDMP sum-product code sets on the GPU (tasp_layered_codes_kernel, LdpcHipCodes(TASP_DEC, ...) / ldpc_hip_open_codes_tdmp): bit for
bit against the CPU oracle and against a single-code LdpcHip context per matrix (JIT off: tasp_global_kernel) in every lifting
regime and both LLR layouts, code boundaries inside the grid, maxiter = 1, non-finite LLRs, the shared-noise simulation with and
without punctured blocks and its split invariance, the C++ stopping-rule harness, refusals.  The inputs and their properties are
those of codeset_tasp_sets.py, asserted on the CPU in test_codeset_tasp_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import codeset_tasp_sets as S
from ldpc_testlib import ROOT, TASP_DEC, assert_bits_equal, load_base_matrix, pack_bits, relift

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -2
MAXITER, NCODES = S.MAXITER, S.NCODES


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
    """No hiprtc in this file: the single-code TDMP contexts run tasp_global_kernel (or an ahead-of-time instance), whose bits are
    those of every other tier."""
    lib = L.load_library()
    before = lib.ldpc_hip_set_jit_mode(0)
    yield
    lib.ldpc_hip_set_jit_mode(before)


def _np(hard, iters, soft):
    return hard.cpu().numpy().view(np.uint32), iters.cpu().numpy(), soft.cpu().numpy()


@pytest.mark.parametrize("layout", ["shared", "percode"])
@pytest.mark.parametrize("case", list(S.CASES), ids=S.CASE_IDS)
def test_parity(L, torch, case, layout):
    M, rh, nh = case
    r = S.reference(case)
    codes, ref = r["codes"], r["ref"][layout]
    llr = r["shared"] if layout == "shared" else r["percode"]
    x = torch.from_numpy(np.ascontiguousarray(llr)).cuda()
    with L.LdpcHipCodes(TASP_DEC, codes, M) as cs:
        assert cs.C == NCODES and cs.lib.ldpc_hip_codes(cs.h) == NCODES and cs.decoder_id == TASP_DEC
        assert cs.kernel_name == "tasp_layered_codes_kernel" + ("<multiwave>" if M > 64 else "")
        hard, iters, soft = cs.decode(x, MAXITER, shared=layout == "shared", want_soft=True)
        torch.cuda.synchronize()
        assert cs.lib.ldpc_hip_last_launch(cs.h).decode() == cs.kernel_name
    hard, iters, soft = _np(hard, iters, soft)
    assert_bits_equal(x.cpu().numpy(), llr, "the input is not modified")
    for c in range(NCODES):
        d_ref, it_ref, s_ref = ref[c]
        assert np.array_equal(iters[c], it_ref), (c, iters[c], it_ref)
        assert np.array_equal(hard[c], pack_bits(d_ref)), c
        assert_bits_equal(soft[c], s_ref, f"a-posteriori probabilities of code {c}")
        with L.LdpcHip(TASP_DEC, codes[c], M) as one:   # and the single-code context on the same matrix
            h1, i1, s1 = one.decode(x if layout == "shared" else x[c], MAXITER, want_soft=True)
            torch.cuda.synchronize()
        assert np.array_equal(iters[c], i1.cpu().numpy()) and np.array_equal(hard[c], h1.cpu().numpy().view(np.uint32)), c
        assert_bits_equal(soft[c], s1.cpu().numpy(), f"a-posteriori probabilities of code {c} against LdpcHip")


@pytest.mark.parametrize("B", [1, 4])
def test_code_boundaries(L, torch, B):
    """M = 20 packs three frames into a wave, so with B = 1 and B = 4 the last wave of each code is partly filled.  Code 1 is a codeword
    at the input and returns 0 without an iteration; codes 0 and 2, its neighbours in the grid, are noisy and never converge: no
    frame's result depends on the other frames of its wave or on the next code."""
    M, codes, llr = S.boundary_set(B)
    ref = [S.oracle_tdmp(codes[c], M, llr[c], MAXITER) for c in range(3)]
    assert (ref[1][1] == 0).all() and (ref[0][1] < 0).all() and (ref[2][1] < 0).all(), [r[1] for r in ref]
    with L.LdpcHipCodes(TASP_DEC, codes, M) as cs:
        hard, iters, soft = cs.decode(torch.from_numpy(llr).cuda(), MAXITER, shared=False, want_soft=True)
        torch.cuda.synchronize()
    hard, iters, soft = _np(hard, iters, soft)
    for c in range(3):
        assert np.array_equal(iters[c], ref[c][1]), c
        assert np.array_equal(hard[c], pack_bits(ref[c][0])), c
        assert_bits_equal(soft[c], ref[c][2], f"code {c}")


def test_maxiter_one(L, torch):
    codes, llr = S.maxiter_one_set()
    ref = [S.oracle_tdmp(codes[c], 20, llr, 1) for c in range(NCODES)]
    its = np.array([x[1] for x in ref])
    assert set(np.unique(its)) == {-1, 1}, its
    with L.LdpcHipCodes(TASP_DEC, codes, 20) as cs:
        hard, iters, soft = _np(*cs.decode(torch.from_numpy(llr).cuda(), 1, want_soft=True))
    for c in range(NCODES):
        assert np.array_equal(iters[c], ref[c][1]) and np.array_equal(hard[c], pack_bits(ref[c][0])), c
        assert_bits_equal(soft[c], ref[c][2], f"code {c}")


@pytest.mark.parametrize("case", [(20, 4, 8), (100, 3, 6)], ids=["M20", "M100"])
def test_non_finite_llrs(L, torch, case):
    """One frame with a NaN, a +Inf and a -Inf LLR (and its finite neighbours in the wave) against the single-code context."""
    M, rh, nh = case
    r = S.reference(case)
    codes = r["codes"]
    llr = r["shared"][:4].copy()
    llr[1, 3], llr[1, M + 1], llr[1, 2 * M] = np.nan, np.inf, -np.inf
    x = torch.from_numpy(llr).cuda()
    with L.LdpcHipCodes(TASP_DEC, codes, M) as cs:
        hard, iters, soft = _np(*cs.decode(x, MAXITER, want_soft=True))
    for c in range(NCODES):
        with L.LdpcHip(TASP_DEC, codes[c], M) as one:
            h1, i1, s1 = _np(*one.decode(x, MAXITER, want_soft=True))
        assert np.array_equal(iters[c], i1) and np.array_equal(hard[c], h1), (c, iters[c], i1)
        assert_bits_equal(soft[c], s1, f"code {c}", nan_ok=True)
        for b in (0, 2, 3):   # the finite frames next to it are those of the parity test
            assert iters[c, b] == r["ref"]["shared"][c][1][b]
            assert_bits_equal(soft[c, b], r["ref"]["shared"][c][2][b], f"code {c}, frame {b}")


@pytest.mark.parametrize("punct", [0, 1])
def test_simulate(L, torch, punct, monkeypatch):
    """simulate_codes = C single-code simulations over the same noise: counters and ordered records, however the frames are split.
    With a punctured block the channel value of the punctured positions must be TDMP's 0.0, not the LLR decoders' 0.5."""
    M, Cn, B, first, snr, seed = (S.SIM[k] for k in ("M", "C", "B", "first", "snr", "seed"))
    codes = S.simulate_set()
    with L.LdpcHipCodes(TASP_DEC, codes, M) as cs:
        cnt, info = cs.simulate(snr, MAXITER, seed, first, B, punctured_blocks=punct, records=True)
        a = cs.simulate(snr, MAXITER, seed, first, 150, punctured_blocks=punct, records=True)
        b = cs.simulate(snr, MAXITER, seed, first + 150, 150, punctured_blocks=punct, records=True)
        monkeypatch.setenv("LDPC_HIP_CODES_PIECE", "64")      # and in pieces of 64 frames inside one call
        c = cs.simulate(snr, MAXITER, seed, first, B, punctured_blocks=punct, records=True)
        monkeypatch.delenv("LDPC_HIP_CODES_PIECE")
        only = cs.simulate(snr, MAXITER, seed, first, B, punctured_blocks=punct)
        # the device entry points on the same frames
        with L.LdpcHip(TASP_DEC, codes[0], M) as one0:
            x = one0.awgn_llr(snr, seed, first, B, punctured_blocks=punct)
            if punct:
                assert bool((x[:, -M:] == 0.0).all())
            hard, iters, _ = cs.decode(x, MAXITER)
            dcnt, dinfo = cs.count_errors(hard, iters, want_frame_info=True)
            torch.cuda.synchronize()
    assert np.array_equal(a[0] + b[0], cnt) and np.array_equal(np.concatenate([a[1], b[1]], axis=1), info)
    assert np.array_equal(c[0], cnt) and np.array_equal(c[1], info) and np.array_equal(only, cnt)
    assert np.array_equal(dcnt.cpu().numpy().astype(np.uint64), cnt) and np.array_equal(dinfo.cpu().numpy(), info)
    assert (cnt[:, 3] == B).all() and 0 < cnt[:, 1].sum() < Cn * B, cnt
    for q in range(Cn):
        with L.LdpcHip(TASP_DEC, codes[q], M) as one:
            s = one.simulate(snr, MAXITER, seed, first, B, punctured_blocks=punct)
            x = one.awgn_llr(snr, seed, first, B, punctured_blocks=punct)
            h1, i1, _ = one.decode(x, MAXITER)
            _, inf1 = one.count_errors(h1, i1, want_frame_info=True, first_frame=first)
            torch.cuda.synchronize()
        assert [s["nse"], s["nde"], s["nue"], s["frames"], s["sum_abs_iters"]] == cnt[q].tolist(), (q, s, cnt[q])
        assert np.array_equal(inf1.cpu().numpy(), info[q]), q


def test_stopping_rule_from_cpp(L, torch, tmp_path):
    """ldpc::bp_simulation_codes with decoder 7 on three codes of very different strength = three ldpc::bp_simulation_throughput_t
    calls with the same seed; batches of 64 frames, and the codes stop in three different batches."""
    L.load_library()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = str(tmp_path / "codes_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "codes_driver.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_compat", "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    M, codes = S.driver_set()
    rh, nh, batch = codes.shape[1], codes.shape[2], 64
    nfe, nexp, snr, ref_fer = 6, 1500, 3.0, 1.0
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([3, rh, nh, M, TASP_DEC, MAXITER, nfe, nexp, batch, 9], dtype=np.int32).tobytes())
        f.write(np.array([snr, ref_fer], dtype=np.float64).tobytes())
        f.write(codes.tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "in.bin")], env=dict(os.environ, LDPC_HIP_JIT="0"), timeout=120).decode().split("\n")
    rows = {(w[0], int(w[1])): w[2:] for w in (line.split() for line in out if line)}
    assert len(rows) == 6, out
    stop_batch = set()
    for c in range(3):
        assert rows["set", c] == rows["one", c], (c, rows["set", c], rows["one", c])
        experiment = int(rows["set", c][4])
        assert 0 < experiment <= nexp + 1
        stop_batch.add((experiment - 1) // batch)
    assert len(stop_batch) == 3, rows


def test_refusals_and_cross_use(L, torch):
    lib = L.load_library()
    ok = S.boundary_set(1)[1][:2]

    def open_rc(fn, codes, M, *dec):
        codes = np.ascontiguousarray(codes, dtype=np.int16)
        h = C.c_void_p()
        rc = fn(*dec, codes.shape[1], codes.shape[2], M, codes.ctypes.data, codes.shape[0], 0, C.byref(h))
        assert (rc == 0) == bool(h.value)
        if h.value:
            lib.ldpc_hip_close(h)
        return rc

    assert open_rc(lib.ldpc_hip_open_codes, ok, 20, TASP_DEC) == EINVAL          # decoder 7 has its own entry point
    assert open_rc(lib.ldpc_hip_open_codes_tdmp, ok, 20) == 0
    bad = ok.copy(); bad[1, 2, :] = -1; bad[1, 2, 0] = 3                          # a weight-1 row
    assert open_rc(lib.ldpc_hip_open_codes_tdmp, bad, 20) == EINVAL
    msg = lib.ldpc_hip_last_error().decode()
    assert "code 1" in msg and "row 2" in msg, msg
    base = load_base_matrix()
    big = np.where(base >= 0, relift(base, 256) % 256, -1).astype(np.int16)[None]
    assert open_rc(lib.ldpc_hip_open_codes_tdmp, big, 256) == EUNSUPPORTED
    assert "294928" in lib.ldpc_hip_last_error().decode()

    B, N, W = 4, 8 * 20, 5
    x = torch.full((2, B, N), 9.0, dtype=torch.float64, device="cuda")
    hard = torch.full((2, B, W), 0x55, dtype=torch.int32, device="cuda")
    iters = torch.full((2, B), -77, dtype=torch.int32, device="cuda")
    cnt = (C.c_ulonglong * 10)()

    def untouched():
        torch.cuda.synchronize()
        return bool((hard == 0x55).all()) and bool((iters == -77).all())

    with L.LdpcHipCodes(TASP_DEC, ok, 20) as cs, L.LdpcHip(TASP_DEC, ok[0], 20) as one:
        for maxiter in (0, -5):
            assert lib.ldpc_hip_decode_codes_dev(cs.h, x.data_ptr(), 0, B, maxiter, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        # the single-code and GF(q) entry points on a TDMP set context
        assert lib.ldpc_hip_decode_dev(cs.h, x.data_ptr(), B, 10, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        c4, sit = (C.c_ulonglong * 4)(), C.c_ulonglong()
        assert lib.ldpc_hip_simulate(cs.h, 2.0, 0, 0, 10, 0.8, 1, 0, B, c4, C.byref(sit)) == EINVAL
        assert lib.ldpc_hip_decode_gfq_dev(cs.h, x.data_ptr(), B, 10, 0.0, None, iters.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_codes(cs.h) == 2 and lib.ldpc_hip_codes(one.h) == 0
        # the set entry points on a single-code TDMP context
        assert lib.ldpc_hip_decode_codes_dev(one.h, x.data_ptr(), 1, B, 10, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_count_errors_codes_dev(one.h, hard.data_ptr(), iters.data_ptr(), B, None, x.data_ptr(), None) == EINVAL
        assert lib.ldpc_hip_simulate_codes(one.h, 2.0, 0, 10, 0.8, 1, 0, B, cnt, None) == EINVAL
        assert untouched(), "a refused call must not launch anything"
        assert bool((x == 9.0).all())
        # and the context still works; alpha is ignored
        h2, i2, _ = cs.decode(x, 10, shared=False, alpha=0.8)
        h3, i3, _ = cs.decode(x, 10, shared=False, alpha=0.123)
        torch.cuda.synchronize()
        assert bool((i2 == 0).all()) and bool((h2 == 0).all()) and bool((i3 == 0).all()) and bool((h3 == 0).all())
