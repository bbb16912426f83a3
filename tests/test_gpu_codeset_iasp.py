"""IASP code sets on the GPU (iasp_codes_kernel, LdpcHipCodes(IASP_DEC, ...) / ldpc_hip_open_codes_iasp): return values and packed
hard words exactly and soft outputs bit for bit against the numpy restatement (iasp_model.IaspModel), against the compiled
reference's golden vectors and against a single-code LdpcHip context per matrix (JIT off), in every lifting regime and both LLR
layouts; the 30 x 60, M = 67 shape of upstream's input12L.jsonx; the all-weight-2 branch per code; code boundaries inside the grid;
maxiter = 1; non-finite LLRs; the shared-noise simulation and its split invariance; the stopping rule on the device and through
the C++ layer; refusals.  The inputs and their properties are those of codeset_iasp_sets.py, asserted on the CPU in
test_codeset_iasp_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import codeset_iasp_sets as S
from codeset_iasp_sets import IASP_DEC
from codeset_stop_sets import schedule, stop_piece
from ldpc_testlib import ROOT, assert_bits_equal

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
    """No hiprtc in this file: the single-code IASP contexts run iasp_global_kernel (or the ahead-of-time instance), whose bits are
    those of every other tier."""
    lib = L.load_library()
    before = lib.ldpc_hip_set_jit_mode(0)
    yield
    lib.ldpc_hip_set_jit_mode(before)


def _np(hard, iters, soft):
    return hard.cpu().numpy().view(np.uint32), iters.cpu().numpy(), soft.cpu().numpy()


def _name(M):
    return "iasp_codes_kernel" + ("<multiwave>" if M > 64 else "")


def _same(got, want, what):
    """got / want = (hard words, return values, soft outputs) of one code."""
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])
    assert np.array_equal(got[0], want[0]), what
    assert_bits_equal(got[2], want[2], what)


def _decode_set(L, torch, codes, M, llr, maxiter, shared=True):
    x = torch.from_numpy(np.ascontiguousarray(llr)).cuda()
    with L.LdpcHipCodes(IASP_DEC, codes, M) as cs:
        assert cs.kernel_name == _name(M) and cs.lib.ldpc_hip_codes(cs.h) == len(codes)
        out = cs.decode(x, maxiter, shared=shared, want_soft=True)
        torch.cuda.synchronize()
        assert cs.lib.ldpc_hip_last_launch(cs.h).decode() == cs.kernel_name
    hard, iters, soft = _np(*out)
    return [(hard[c], iters[c], soft[c]) for c in range(len(codes))]


def _decode_one(L, torch, H, M, llr, maxiter):
    with L.LdpcHip(IASP_DEC, H, M) as one:
        out = _np(*one.decode(torch.from_numpy(np.ascontiguousarray(llr)).cuda(), maxiter, want_soft=True))
    return out


@pytest.mark.parametrize("layout", ["shared", "percode"])
@pytest.mark.parametrize("case", list(S.CASES), ids=S.CASE_IDS)
def test_parity(L, torch, case, layout):
    M, rh, nh = case
    r = S.reference(case)
    codes, ref = r["codes"], r["ref"][layout]
    llr = r["shared"] if layout == "shared" else r["percode"]
    got = _decode_set(L, torch, codes, M, llr, MAXITER, shared=layout == "shared")
    for c in range(NCODES):
        _same(got[c], ref[c], f"code {c} against the model")
        _same(got[c], _decode_one(L, torch, codes[c], M, llr if layout == "shared" else llr[c], MAXITER), f"code {c} against LdpcHip")


def test_the_30x60_shape(L, torch):
    """upstream's input12L.jsonx: 30 x 60 base matrices at M = 67.  Code 0 against the compiled reference, the relabelled codes against
    the model."""
    g = S.golden_set(S.SHAPE_30x60, 5)
    codes, M = g["codes"], g["M"]
    assert codes.shape[1:] == (30, 60) and M == 67
    with L.LdpcHipCodes(IASP_DEC, codes, M) as cs:
        assert cs.kernel_name == "iasp_codes_kernel<multiwave>" and cs.rh == 30 and cs.R == 30 * 67
    got = _decode_set(L, torch, codes, M, g["llr"], g["maxiter"])
    _same(got[0], (g["hard"], g["iters"], g["soft"]), "code 0 against the compiled reference")
    for c in range(1, 5):
        _same(got[c], S.model(codes[c], M, g["llr"], g["maxiter"]), f"code {c} against the model")


@pytest.mark.parametrize("name", S.LIFTINGS)
def test_compiled_reference_at_other_liftings(L, torch, name):
    g = S.golden_set(name, 3)
    got = _decode_set(L, torch, g["codes"], g["M"], g["llr"], g["maxiter"])
    _same(got[0], (g["hard"], g["iters"], g["soft"]), "code 0 against the compiled reference")
    for c in (1, 2):
        _same(got[c], S.model(g["codes"][c], g["M"], g["llr"], g["maxiter"]), f"code {c} against the model")


@pytest.mark.parametrize("name", sorted(S.CW2))
def test_all_weight_two_branch_per_code(L, torch, name):
    """Codes 0 and 2 have block columns of weight 2 only (upstream's own branch), codes 1 and 3 not: the flag is the code's."""
    g = S.cw2_set(name)
    codes, M = g["codes"], g["M"]
    got = _decode_set(L, torch, codes, M, g["llr"], g["maxiter"])
    _same(got[0], (g["hard"], g["iters"], g["soft"]), "code 0 against the compiled reference")
    for c in (1, 2, 3):
        _same(got[c], S.model(codes[c], M, g["llr"], g["maxiter"]), f"code {c} against the model")
        _same(got[c], _decode_one(L, torch, codes[c], M, g["llr"], g["maxiter"]), f"code {c} against LdpcHip")


@pytest.mark.parametrize("B", [1, 4])
def test_code_boundaries(L, torch, B):
    """M = 20 packs three frames into a wave, so with B = 1 and B = 4 the last wave of each code is partly filled.  Code 1 is a codeword
    at the input and returns 0 with the input words as outputs; codes 0 and 2, its neighbours in the grid, never converge."""
    M, codes, llr = S.boundary_set(B)
    ref = [S.model(codes[c], M, llr[c], MAXITER) for c in range(3)]
    assert (ref[1][1] == 0).all() and (ref[0][1] < 0).all() and (ref[2][1] < 0).all(), [r[1] for r in ref]
    got = _decode_set(L, torch, codes, M, llr, MAXITER, shared=False)
    for c in range(3):
        _same(got[c], ref[c], f"code {c}")
    from iasp_model import channel_prior
    q = np.clip(np.trunc(channel_prior(llr[1]) * 4096 + 0.5), 1, 4095)
    assert_bits_equal(got[1][2], q * 16 / 65536.0, "a codeword at the input: the outputs are the input words")


def test_maxiter_one(L, torch):
    codes, llr = S.maxiter_one_set()
    ref = [S.model(codes[c], 20, llr, 1) for c in range(NCODES)]
    assert set(np.unique([x[1] for x in ref])) == {-1, 1}
    got = _decode_set(L, torch, codes, 20, llr, 1)
    for c in range(NCODES):
        _same(got[c], ref[c], f"code {c}")


@pytest.mark.parametrize("case", [(20, 4, 8), (100, 3, 6)], ids=["M20", "M100"])
def test_non_finite_llrs(L, torch, case):
    """+-Inf LLRs against the model and the single-code context; a NaN against the single-code context only (the numpy prior is
    NaN-free by its contract).  The finite frames of the wave are those of the parity test."""
    M, rh, nh = case
    r = S.reference(case)
    codes = r["codes"]
    inf = r["shared"][:4].copy()
    inf[1, M + 1], inf[1, 2 * M] = np.inf, -np.inf
    nan = inf.copy()
    nan[1, 3] = np.nan
    g_inf = _decode_set(L, torch, codes, M, inf, MAXITER)
    g_nan = _decode_set(L, torch, codes, M, nan, MAXITER)
    for c in range(NCODES):
        _same(g_inf[c], S.model(codes[c], M, inf, MAXITER), f"code {c}, Inf, against the model")
        _same(g_inf[c], _decode_one(L, torch, codes[c], M, inf, MAXITER), f"code {c}, Inf, against LdpcHip")
        _same(g_nan[c], _decode_one(L, torch, codes[c], M, nan, MAXITER), f"code {c}, NaN, against LdpcHip")
        ref = r["ref"]["shared"][c]
        for got in (g_inf[c], g_nan[c]):
            for b in (0, 2, 3):   # the finite frames next to it are those of the parity test
                _same(tuple(x[b] for x in got), tuple(x[b] for x in ref), f"code {c}, frame {b}")


@pytest.mark.parametrize("punct", [0, 1])
def test_simulate(L, torch, punct, monkeypatch):
    """simulate_codes = C single-code simulations over the same noise: counters and ordered records, however the frames are split.
    With a punctured block the channel value of the punctured positions must be IASP's 0.0, not the LLR decoders' 0.5."""
    M, Cn, B, first, snr, seed = (S.SIM[k] for k in ("M", "C", "B", "first", "snr", "seed"))
    codes = S.simulate_set()
    with L.LdpcHipCodes(IASP_DEC, codes, M) as cs:
        cnt, info = cs.simulate(snr, MAXITER, seed, first, B, punctured_blocks=punct, records=True)
        a = cs.simulate(snr, MAXITER, seed, first, 150, punctured_blocks=punct, records=True)
        b = cs.simulate(snr, MAXITER, seed, first + 150, 150, punctured_blocks=punct, records=True)
        monkeypatch.setenv("LDPC_HIP_CODES_PIECE", "64")      # and in pieces of 64 frames inside one call
        c = cs.simulate(snr, MAXITER, seed, first, B, punctured_blocks=punct, records=True)
        monkeypatch.delenv("LDPC_HIP_CODES_PIECE")
        only = cs.simulate(snr, MAXITER, seed, first, B, punctured_blocks=punct)
    assert np.array_equal(a[0] + b[0], cnt) and np.array_equal(np.concatenate([a[1], b[1]], axis=1), info)
    assert np.array_equal(c[0], cnt) and np.array_equal(c[1], info) and np.array_equal(only, cnt)
    assert (cnt[:, 3] == B).all() and 0 < cnt[:, 1].sum() < Cn * B, cnt
    for q in range(Cn):
        with L.LdpcHip(IASP_DEC, codes[q], M) as one:
            s = one.simulate(snr, MAXITER, seed, first, B, punctured_blocks=punct)
            x = one.awgn_llr(snr, seed, first, B, punctured_blocks=punct)
            if punct:
                assert bool((x[:, -M:] == 0.0).all())
            h1, i1, _ = one.decode(x, MAXITER)
            _, inf1 = one.count_errors(h1, i1, want_frame_info=True, first_frame=first)
            torch.cuda.synchronize()
        assert [s["nse"], s["nde"], s["nue"], s["frames"], s["sum_abs_iters"]] == cnt[q].tolist(), (q, s, cnt[q])
        assert np.array_equal(inf1.cpu().numpy(), info[q]), q


def _stop_reference(L):
    p = S.STOP
    with L.LdpcHipCodes(IASP_DEC, S.stop_set(), p["M"]) as cs:
        _, info = cs.simulate(p["snr"], MAXITER, p["seed"], 0, p["nexp"] + 1, records=True)
    return np.array([L.host.replay_stop_rule(row, p["nfe"], p["nexp"], p["ref_fer"]) for row in info], dtype=np.uint64)


def test_stopping_rule_on_the_device(L, torch, monkeypatch):
    """simulate_until on [weak, medium, strong]: experiment, nse and nde per code as exact integers against the sequential rule over
    the records of simulate; the weak code (no coding gain: ten error frames among the first dozen) stops in the first batch, so
    every later launch covers a subset of the codes."""
    p = S.STOP
    want = _stop_reference(L)
    pieces = schedule(p["nexp"], p["batch"], p["batch"])
    batches = [pieces[stop_piece(int(e), pieces)][0] for e in want[:, 0]]
    print("reference (experiment, nse, nde):", want.tolist(), "stop batches:", batches)
    assert batches[0] == 0 and max(batches) > 0, "subset launches: the weak code stops first, another one later"
    with L.LdpcHipCodes(IASP_DEC, S.stop_set(), p["M"]) as cs:
        cs.profile(True)
        got = cs.simulate_until(p["snr"], MAXITER, p["seed"], p["nfe"], p["nexp"], p["ref_fer"], first_batch=p["batch"], max_batch=p["batch"])
        _, launches = cs.profile_read()
        cs.profile(False)
        wide = cs.simulate_until(p["snr"], MAXITER, p["seed"], p["nfe"], p["nexp"], p["ref_fer"])
        monkeypatch.setenv("LDPC_HIP_CODES_PIECE", "48")
        cut = cs.simulate_until(p["snr"], MAXITER, p["seed"], p["nfe"], p["nexp"], p["ref_fer"], first_batch=p["batch"], max_batch=p["batch"])
        monkeypatch.delenv("LDPC_HIP_CODES_PIECE")
    for what, res in (("64/64", got), ("default", wide), ("pieces of 48", cut)):
        assert np.array_equal(res[:, :3], want), (what, res.tolist(), want.tolist())
    assert got[:, 3].tolist() == [min(p["batch"] * (b + 1), p["nexp"] + 1) for b in batches]
    assert launches == max(batches) + 1


def test_stopping_rule_from_cpp(L, torch, tmp_path):
    """ldpc::bp_simulation_codes with decoder 5 through both of its routes, show_process = 0 (the rule on the device) and = 1 (the
    records replayed on the host): the same counters, and those of the Python reference."""
    L.load_library()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = str(tmp_path / "codes_stop_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "codes_stop_driver.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_compat", "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    p = S.STOP
    codes = S.stop_set()
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(codes), codes.shape[1], codes.shape[2], p["M"], IASP_DEC, MAXITER, p["nfe"], p["nexp"], p["batch"], p["seed"]], dtype=np.int32).tobytes())
        f.write(np.array([p["snr"], p["ref_fer"]], dtype=np.float64).tobytes())
        f.write(codes.tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "in.bin")], env=dict(os.environ, LDPC_HIP_JIT="0"), timeout=120).decode().split("\n")
    rows = {(w[0], int(w[1])): w[2:] for w in (line.split() for line in out if line.startswith(("device ", "host ")))}
    assert len(rows) == 2 * len(codes), out
    want = _stop_reference(L)
    for c in range(len(codes)):
        assert rows["device", c] == rows["host", c], (c, rows["device", c], rows["host", c])
        assert [int(v) for v in rows["device", c][2:]] == [int(want[c, 1]), int(want[c, 2]), int(want[c, 0])], c


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

    assert open_rc(lib.ldpc_hip_open_codes, ok, 20, IASP_DEC) == EINVAL          # decoder 5 has its own entry point
    assert open_rc(lib.ldpc_hip_open_codes_iasp, ok, 20) == 0
    bad = ok.copy(); bad[1, 2, :] = -1; bad[1, 2, 0] = 3                          # a weight-1 row
    assert open_rc(lib.ldpc_hip_open_codes_iasp, bad, 20) == EINVAL
    msg = lib.ldpc_hip_last_error().decode()
    assert "code 1" in msg and "row 2" in msg, msg
    assert open_rc(lib.ldpc_hip_open_codes_iasp, S.big_image_set(), 512) == EUNSUPPORTED
    assert "180240" in lib.ldpc_hip_last_error().decode()

    B, N, W = 4, 8 * 20, 5
    x = torch.full((2, B, N), 9.0, dtype=torch.float64, device="cuda")
    hard = torch.full((2, B, W), 0x55, dtype=torch.int32, device="cuda")
    iters = torch.full((2, B), -77, dtype=torch.int32, device="cuda")
    cnt = (C.c_ulonglong * 10)()

    def untouched():
        torch.cuda.synchronize()
        return bool((hard == 0x55).all()) and bool((iters == -77).all())

    with L.LdpcHipCodes(IASP_DEC, ok, 20) as cs, L.LdpcHip(IASP_DEC, ok[0], 20) as one:
        for maxiter in (0, -5):
            assert lib.ldpc_hip_decode_codes_dev(cs.h, x.data_ptr(), 0, B, maxiter, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        # the single-code and GF(q) entry points on an IASP set context
        assert lib.ldpc_hip_decode_dev(cs.h, x.data_ptr(), B, 10, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        c4, sit = (C.c_ulonglong * 4)(), C.c_ulonglong()
        assert lib.ldpc_hip_simulate(cs.h, 2.0, 0, 0, 10, 0.8, 1, 0, B, c4, C.byref(sit)) == EINVAL
        assert lib.ldpc_hip_decode_gfq_dev(cs.h, x.data_ptr(), B, 10, 0.0, None, iters.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_decode_codes_gfq_dev(cs.h, x.data_ptr(), 1, B, 10, None, iters.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_codes(cs.h) == 2 and lib.ldpc_hip_codes(one.h) == 0
        # the set entry points on a single-code IASP context
        assert lib.ldpc_hip_decode_codes_dev(one.h, x.data_ptr(), 1, B, 10, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_count_errors_codes_dev(one.h, hard.data_ptr(), iters.data_ptr(), B, None, x.data_ptr(), None) == EINVAL
        assert lib.ldpc_hip_simulate_codes(one.h, 2.0, 0, 10, 0.8, 1, 0, B, cnt, None) == EINVAL
        assert untouched(), "a refused call must not launch anything"
        assert bool((x == 9.0).all())
        # and the context still works; alpha is not read
        h2, i2, _ = cs.decode(x, 10, shared=False, alpha=0.8)
        h3, i3, _ = cs.decode(x, 10, shared=False, alpha=0.123)
        torch.cuda.synchronize()
        assert bool((i2 == 0).all()) and bool((h2 == 0).all()) and bool((i3 == 0).all()) and bool((h3 == 0).all())
