"""Wide code sets on the GPU (ldpc_hip_open_codes_wide: ms_flood_wide_codes_kernel, lms_layered_wide_codes_kernel and
tasp_layered_codes_kernel without a block-row limit): return values, packed hard words and soft outputs EXACTLY against the CPU oracle
and against a single-code LdpcHip context per matrix (JIT off), at 17 and 30 block rows and 33 block columns, in every lifting regime
and both LLR layouts; alpha; the wide route against the register-resident set kernels where both fit; adversarial channel values;
code boundaries inside the grid; maxiter = 1 with each optional output left out; the shared-noise and the exact-replay simulation
with their stopping rules; the C++ layer; refusals.  The inputs and their properties are those of codeset_wide_sets.py, asserted on
the CPU in test_codeset_wide_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import codeset_wide_sets as S
from codeset_stop_sets import schedule, stop_piece
from codeset_wide_sets import DECS, LMS_DEC, MS_DEC, TASP_DEC
from ldpc_testlib import ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -2
MAXITER = S.MAXITER
DEC_PARAM = pytest.mark.parametrize("dec", DECS, ids=[S.DEC_IDS[d] for d in DECS])


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
    """No hiprtc in this file: the single-code contexts run the table-driven or the shape-unlimited tier, whose bits are those of
    every other tier."""
    lib = L.load_library()
    before = lib.ldpc_hip_set_jit_mode(0)
    yield
    lib.ldpc_hip_set_jit_mode(before)


def _np(hard, iters, soft):
    return hard.cpu().numpy().view(np.uint32), iters.cpu().numpy(), soft.cpu().numpy()


def _same(got, want, what):
    """got / want = (hard words, return values, soft outputs) of one code."""
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])
    assert np.array_equal(got[0], want[0]), what
    assert_bits_equal(got[2], want[2], what)


def _set_decode(cs, torch, llr, maxiter, shared=True, alpha=0.8):
    llr = np.ascontiguousarray(llr)
    x = torch.from_numpy(llr.copy()).cuda()
    out = cs.decode(x, maxiter, alpha=alpha, shared=shared, want_soft=True)
    torch.cuda.synchronize()
    assert cs.lib.ldpc_hip_last_launch(cs.h).decode() == cs.kernel_name
    assert_bits_equal(x.cpu().numpy(), llr, "the input is not modified")
    hard, iters, soft = _np(*out)
    return [(hard[c], iters[c], soft[c]) for c in range(cs.C)]


def _decode_wide(L, torch, dec, codes, M, llr, maxiter, shared=True, alpha=0.8):
    with L.LdpcHipCodes(dec, codes, M, wide=True) as cs:
        assert cs.kernel_name == S.kernel_name(dec, M) and cs.lib.ldpc_hip_codes(cs.h) == len(codes) and cs.decoder_id == dec
        assert (cs.rh, cs.nh) == codes.shape[1:] and cs.R == codes.shape[1] * M and cs.N == codes.shape[2] * M
        return _set_decode(cs, torch, llr, maxiter, shared, alpha)


def _decode_one(L, torch, dec, H, M, llr, maxiter, alpha=0.8):
    with L.LdpcHip(dec, H, M) as one:
        out = _np(*one.decode(torch.from_numpy(np.ascontiguousarray(llr)).cuda(), maxiter, alpha=alpha, want_soft=True))
    return out


@pytest.mark.parametrize("alpha", [-0.8, -0.0, 0.0])
def test_alpha_that_is_not_above_zero_is_refused(L, torch, alpha):
    """ms_flood_wide_codes_kernel starts from y + 0.0 as ms_flood_codes_kernel does: where upstream's y + acc * alpha is -0.0 (y is and
    the product is too, which takes a negative alpha, or a zero one and acc < 0) it returns +0.0.  Upstream's bits or an error: the
    wide route refuses, and names alpha."""
    r = S.reference("rows17_M20", MS_DEC)
    M, codes, llr = r["M"], r["codes"], r["shared"]
    with L.LdpcHipCodes(MS_DEC, codes, M, wide=True) as cs:
        assert cs.kernel_name == S.kernel_name(MS_DEC, M)
        with pytest.raises(L.LdpcHipError, match="alpha = -?0.* is not above zero"):
            _set_decode(cs, torch, llr, MAXITER, alpha=alpha)
        got = _set_decode(cs, torch, llr, MAXITER)
    for c in range(len(codes)):
        _same(got[c], r["ref"]["shared"][c], f"code {c} against the oracle, after the refusal")


@pytest.mark.parametrize("layout", ["shared", "percode"])
@pytest.mark.parametrize("name,dec", S.PARITY, ids=S.PARITY_IDS)
def test_parity(L, torch, name, dec, layout):
    r = S.reference(name, dec)
    M, codes, ref = r["M"], r["codes"], r["ref"][layout]
    llr = r[layout]
    got = _decode_wide(L, torch, dec, codes, M, llr, MAXITER, shared=layout == "shared")
    for c in range(len(codes)):
        _same(got[c], ref[c], f"code {c} against the oracle")
        _same(got[c], _decode_one(L, torch, dec, codes[c], M, llr if layout == "shared" else llr[c], MAXITER), f"code {c} against LdpcHip")
    if S.is_wide(dec, *codes.shape[1:]) and layout == "shared":     # the binding takes the wide route by itself
        with L.LdpcHipCodes(dec, codes, M) as cs:
            assert cs.kernel_name == S.kernel_name(dec, M)
            again = _set_decode(cs, torch, llr, MAXITER)
        for c in range(len(codes)):
            _same(again[c], got[c], f"code {c}, route chosen by the binding")


@pytest.mark.parametrize("alpha", [0.5, 1.0])
def test_alpha_is_honoured(L, torch, alpha):
    r = S.reference("rows17_M20", MS_DEC)
    M, codes, llr = r["M"], r["codes"], r["shared"]
    ref = [S.oracle(MS_DEC, codes[c], M, llr, MAXITER, alpha=alpha) for c in range(len(codes))]
    assert any(not np.array_equal(ref[c][2], r["ref"]["shared"][c][2]) for c in range(len(codes))), "alpha must matter on this set"
    got = _decode_wide(L, torch, MS_DEC, codes, M, llr, MAXITER, alpha=alpha)
    for c in range(len(codes)):
        _same(got[c], ref[c], f"code {c} against the oracle, alpha {alpha}")
        _same(got[c], _decode_one(L, torch, MS_DEC, codes[c], M, llr, MAXITER, alpha=alpha), f"code {c} against LdpcHip, alpha {alpha}")


@pytest.mark.parametrize("layout", ["shared", "percode"])
@pytest.mark.parametrize("name", S.NARROW)
@DEC_PARAM
def test_narrow_against_wide(L, torch, dec, name, layout):
    """Where both routes accept the shape, the wide context and the register-resident set context give identical outputs."""
    r = S.reference(name, dec)
    M, codes, llr = r["M"], r["codes"], r[layout]
    wide = _decode_wide(L, torch, dec, codes, M, llr, MAXITER, shared=layout == "shared")
    with L.LdpcHipCodes(dec, codes, M) as cs:
        assert cs.kernel_name == S.NARROW_KERNEL[dec] + ("<multiwave>" if M > 64 else "")
        narrow = _set_decode(cs, torch, llr, MAXITER, shared=layout == "shared")
    for c in range(len(codes)):
        _same(wide[c], narrow[c], f"code {c}, wide against narrow")
        _same(wide[c], r["ref"][layout][c], f"code {c} against the oracle")


@DEC_PARAM
def test_adversarial_frames(L, torch, dec):
    """adversarial_llr's finite frames (ties, clamps at 32767, -0.0, subnormals, ...) on the 17 x 34 set: every frame against LdpcHip
    per code and against the oracle."""
    M, codes, llr, labels = S.adversarial_set()
    got = _decode_wide(L, torch, dec, codes, M, llr, MAXITER)
    for c in range(len(codes)):
        one = _decode_one(L, torch, dec, codes[c], M, llr, MAXITER)
        ref = S.oracle(dec, codes[c], M, llr, MAXITER)
        for f, label in enumerate(labels):
            _same(tuple(x[f] for x in got[c]), tuple(x[f] for x in one), f"code {c}, frame {f} ({label}) against LdpcHip")
            _same(tuple(x[f] for x in got[c]), tuple(x[f] for x in ref), f"code {c}, frame {f} ({label}) against the oracle")


@pytest.mark.parametrize("B", [1, 4])
@DEC_PARAM
def test_code_boundaries(L, torch, dec, B):
    """M = 20 packs three frames into a wave, so with B = 1 and B = 4 the last wave of each code is partly filled.  Code 1 sees a
    codeword (min-sum and layered min-sum return 1, TDMP 0); codes 0 and 2, its neighbours in the grid, never converge: no frame's
    result depends on its wave-mates or on the next code."""
    M, codes, llr = S.boundary_set(B)
    ref = [S.oracle(dec, codes[c], M, llr[c], MAXITER) for c in range(3)]
    middle = 0 if dec == TASP_DEC else 1
    assert (ref[1][1] == middle).all() and (ref[0][1] == -MAXITER).all() and (ref[2][1] == -MAXITER).all(), [r[1] for r in ref]
    got = _decode_wide(L, torch, dec, codes, M, llr, MAXITER, shared=False)
    for c in range(3):
        _same(got[c], ref[c], f"code {c}")
    assert (got[1][0] == 0).all()


@DEC_PARAM
def test_maxiter_one_and_optional_outputs(L, torch, dec):
    """maxiter = 1, and each of the three outputs left out in turn: the other two are what they are with all three."""
    M, codes, llr = S.maxiter_one_set(dec)
    Cn, B, N = len(codes), len(llr), llr.shape[1]
    ref = [S.oracle(dec, codes[c], M, llr, 1) for c in range(Cn)]
    assert set(np.unique([x[1] for x in ref])) == {-1, 1}
    x = torch.from_numpy(llr).cuda()
    with L.LdpcHipCodes(dec, codes, M, wide=True) as cs:
        full = _set_decode(cs, torch, llr, 1)
        for c in range(Cn):
            _same(full[c], ref[c], f"code {c}")
        W = cs.hard_words
        for leave in ("hard", "iters", "soft"):
            hard = torch.full((Cn, B, W), 0x55, dtype=torch.int32, device="cuda")
            iters = torch.full((Cn, B), -77, dtype=torch.int32, device="cuda")
            soft = torch.full((Cn, B, N), 7.0, dtype=torch.float64, device="cuda")
            rc = cs.lib.ldpc_hip_decode_codes_dev(cs.h, x.data_ptr(), 1, B, 1, 0.8, None if leave == "hard" else hard.data_ptr(),
                                                  None if leave == "iters" else iters.data_ptr(), None if leave == "soft" else soft.data_ptr(), None)
            assert rc == 0, cs.lib.ldpc_hip_last_error().decode()
            torch.cuda.synchronize()
            h, i, s = _np(hard, iters, soft)
            assert (h == 0x55).all() if leave == "hard" else all(np.array_equal(h[c], full[c][0]) for c in range(Cn)), leave
            assert (i == -77).all() if leave == "iters" else all(np.array_equal(i[c], full[c][1]) for c in range(Cn)), leave
            if leave == "soft":
                assert (s == 7.0).all()
            else:
                assert_bits_equal(s, np.array([full[c][2] for c in range(Cn)]), f"soft without {leave}")


# ---- Monte-Carlo on the 17 x 34 set at M = 20, three codes
@pytest.mark.parametrize("punct", [0, 1])
@DEC_PARAM
def test_simulate(L, torch, dec, punct, monkeypatch):
    """simulate_codes = C single-code simulations over the same noise: counters and ordered records, however the frames are split."""
    Cn, B, first, snr, seed = (S.SIM[k] for k in ("C", "B", "first", "snr", "seed"))
    M, codes = S.simulate_set()
    with L.LdpcHipCodes(dec, codes, M, wide=True) as cs:
        cnt, info = cs.simulate(snr, MAXITER, seed, first, B, punctured_blocks=punct, records=True)
        a = cs.simulate(snr, MAXITER, seed, first, 150, punctured_blocks=punct, records=True)
        b = cs.simulate(snr, MAXITER, seed, first + 150, 150, punctured_blocks=punct, records=True)
        monkeypatch.setenv("LDPC_HIP_CODES_PIECE", "64")      # and in pieces of 64 frames inside one call
        c = cs.simulate(snr, MAXITER, seed, first, B, punctured_blocks=punct, records=True)
        monkeypatch.delenv("LDPC_HIP_CODES_PIECE")
        assert cs.lib.ldpc_hip_last_launch(cs.h).decode() == S.kernel_name(dec, M)
    assert np.array_equal(a[0] + b[0], cnt) and np.array_equal(np.concatenate([a[1], b[1]], axis=1), info)
    assert np.array_equal(c[0], cnt) and np.array_equal(c[1], info)
    assert (cnt[:, 3] == B).all() and 0 < cnt[:, 1].sum() < Cn * B, cnt
    for q in range(Cn):
        with L.LdpcHip(dec, codes[q], M) as one:
            s = one.simulate(snr, MAXITER, seed, first, B, punctured_blocks=punct)
        assert [s["nse"], s["nde"], s["nue"], s["frames"], s["sum_abs_iters"]] == cnt[q].tolist(), (q, s, cnt[q])


@DEC_PARAM
def test_stopping_rule_on_the_device(L, torch, dec, monkeypatch):
    """simulate_until: experiment, nse and nde per code as exact integers against the sequential rule replayed on the host over the
    records of simulate, for batches of 64, the default schedule and pieces of 48 frames."""
    p = S.STOP
    M, codes = S.simulate_set()
    with L.LdpcHipCodes(dec, codes, M, wide=True) as cs:
        _, info = cs.simulate(p["snr"], MAXITER, p["seed"], 0, p["nexp"] + 1, records=True)
        want = np.array([L.host.replay_stop_rule(row, p["nfe"], p["nexp"], p["ref_fer"]) for row in info], dtype=np.uint64)
        pieces = schedule(p["nexp"], p["batch"], p["batch"])
        batches = [pieces[stop_piece(int(e), pieces)][0] for e in want[:, 0]]
        print("reference (experiment, nse, nde):", want.tolist(), "stop batches:", batches)
        got = cs.simulate_until(p["snr"], MAXITER, p["seed"], p["nfe"], p["nexp"], p["ref_fer"], first_batch=p["batch"], max_batch=p["batch"])
        default = cs.simulate_until(p["snr"], MAXITER, p["seed"], p["nfe"], p["nexp"], p["ref_fer"])
        monkeypatch.setenv("LDPC_HIP_CODES_PIECE", "48")
        cut = cs.simulate_until(p["snr"], MAXITER, p["seed"], p["nfe"], p["nexp"], p["ref_fer"], first_batch=p["batch"], max_batch=p["batch"])
        monkeypatch.delenv("LDPC_HIP_CODES_PIECE")
    for what, res in (("64/64", got), ("default", default), ("pieces of 48", cut)):
        assert np.array_equal(res[:, :3], want), (what, res.tolist(), want.tolist())
    assert got[:, 3].tolist() == [min(p["batch"] * (b + 1), p["nexp"] + 1) for b in batches]
    assert (want[:, 2] > 0).all(), "every code meets error frames"


@DEC_PARAM
def test_exact_replay(L, torch, dec):
    """mt_simulate_codes and mt_simulate_codes_stop against ldpc_hip_mt_frames per code from the same generator state."""
    M, codes = S.simulate_set()
    B, snr, nfe, nexp, ref = 150, S.STOP["snr"], 7, 149, 1.0
    st = L.mt19937_state(12345, 17 * M)
    with L.LdpcHipCodes(dec, codes, M, wide=True) as cs:
        cs.mt_set_state(*st)
        cnt, info, its = cs.mt_simulate(snr, MAXITER, B, records=True)
        after = cs.mt_get_state()
        cs.mt_set_state(*st)
        until = cs.mt_simulate_until(snr, MAXITER, nfe, nexp, ref, first_batch=64, max_batch=64)
    assert (info != 0).any() and (info == 0).any()
    for c, H in enumerate(codes):
        with L.LdpcHip(dec, H, M) as one:
            one.mt_set_state(*st)
            want_info, want_its = one.mt_frames(snr, MAXITER, B)
            want_after = one.mt_get_state()
        assert np.array_equal(info[c], want_info) and np.array_equal(its[c], want_its), c
        assert np.array_equal(after[0], want_after[0]) and after[1] == want_after[1], c
        err = want_info != 0
        assert cnt[c].tolist() == [int((want_info[err] & ((1 << 30) - 1)).sum()), int(err.sum()), int((err & (want_its >= 0)).sum()), B,
                                   int(np.abs(want_its).sum())], c
        k = {"nse": 0, "nde": 0, "nue": 0, "experiment": 0}
        L.replay_stopping_rule(want_info, want_its, k, nfe, nexp, ref)
        assert until[c, :5].tolist() == [k["experiment"], k["nse"], k["nde"], k["nue"], int(np.abs(want_its[:k["experiment"]].astype(np.int64)).sum())], c


# ---- the C++ layer
@pytest.mark.parametrize("dec,snr", [(MS_DEC, 2.0), (TASP_DEC, 1.0), (LMS_DEC, 1.5)], ids=["MS", "TDMP", "LMS"])
def test_cpp_layer(L, torch, tmp_path, dec, snr):
    """ldpc::bp_simulation_codes on a 17 x 34 set = one ldpc::bp_simulation_throughput_t per matrix (tests/cpp/codes_driver.cpp), and
    ldpc::bp_simulation_codes_exact = one exact single-code run (bp_simulation_t's route) per matrix."""
    L.load_library()
    M, codes = S.simulate_set()
    nfe, nexp, ref, batch, seed = 6, 300, 1.0, 64, 9
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = str(tmp_path / "codes_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "codes_driver.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_compat", "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(codes), 17, 34, M, dec, MAXITER, nfe, nexp, batch, seed], dtype=np.int32).tobytes())
        f.write(np.array([snr, ref], dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(codes, dtype=np.int16).tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "in.bin")], env=dict(os.environ, LDPC_HIP_JIT="0"), timeout=120).decode().split("\n")
    rows = {(w[0], int(w[1])): w[2:] for w in (line.split() for line in out if line.startswith(("set ", "one ")))}
    assert len(rows) == 2 * len(codes), out
    for c in range(len(codes)):
        assert rows["set", c] == rows["one", c], (c, rows["set", c], rows["one", c])
    assert any(int(rows["set", c][3]) > 0 for c in range(len(codes))), "error frames"
    # the exact replay
    compat = C.CDLL(os.path.join(ROOT, "ldpc-lib_amd", "libldpc_compat.so"))
    compat.ldpc_bp_simulation_codes_exact.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                                      C.c_int, C.c_int, C.c_uint, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]
    flat = np.ascontiguousarray(codes, dtype=np.int32)
    res = np.zeros((len(codes), 7), dtype=np.float64)
    nxt = C.c_uint()
    assert compat.ldpc_bp_simulation_codes_exact(len(codes), 17, 34, flat.ctypes.data, M, MAXITER, nfe, nexp, snr, ref, dec, 0, 0, 12345, 0, 64, 256, 0,
                                                 res.ctypes.data, C.addressof(nxt)) == 0
    for c, H in enumerate(codes):
        ber, fer, st = L.bp_simulation(H, M, MAXITER, nfe, nexp, snr, ref, decoder_type=dec, exact_seed=12345, batch=128, return_state=True)
        assert [int(res[c, 5]), int(res[c, 2]), int(res[c, 3]), int(res[c, 4]), int(res[c, 6])] == \
            [st["experiment"], st["nse"], st["nde"], st["nue"], st["sum_abs_iters"]], (c, res[c].tolist(), st)
        assert res[c, 0] == ber and res[c, 1] == fer, c


def test_refusals_and_cross_use(L, torch):
    lib = L.load_library()
    M, codes = S.simulate_set()
    ok = codes[:2]

    def open_rc(dec, codes, M):
        codes = np.ascontiguousarray(codes, dtype=np.int16)
        h = C.c_void_p()
        rc = lib.ldpc_hip_open_codes_wide(dec, codes.shape[1], codes.shape[2], M, codes.ctypes.data, codes.shape[0], 0, C.byref(h))
        assert (rc == 0) == bool(h.value)
        if h.value:
            lib.ldpc_hip_close(h)
        return rc

    for dec in (4, 5, 9):
        assert open_rc(dec, ok, M) == EINVAL and "decoder id" in lib.ldpc_hip_last_error().decode()
    for dec in DECS:
        assert open_rc(dec, ok, M) == 0
        bad = ok.copy(); bad[1, 16, :] = -1                                         # an empty block row
        assert open_rc(dec, bad, M) == EINVAL
        msg = lib.ldpc_hip_last_error().decode()
        assert "code 1" in msg and "row 16" in msg, msg
        assert open_rc(dec, S.dense_set(17, 34, 512), 512) == EUNSUPPORTED and "bytes" in lib.ldpc_hip_last_error().decode()
    h = C.c_void_p()                                                                  # the old entry points keep their limit
    assert lib.ldpc_hip_open_codes(MS_DEC, 17, 34, M, ok.ctypes.data, 2, 0, C.byref(h)) == EINVAL and not h.value
    assert lib.ldpc_hip_open_codes_tdmp(17, 34, M, ok.ctypes.data, 2, 0, C.byref(h)) == EINVAL and not h.value

    B, N, W = 4, 34 * M, (34 * M + 31) // 32
    x = torch.full((2, B, N), 9.0, dtype=torch.float64, device="cuda")
    hard = torch.full((2, B, W), 0x55, dtype=torch.int32, device="cuda")
    iters = torch.full((2, B), -77, dtype=torch.int32, device="cuda")
    cnt = (C.c_ulonglong * 10)()

    def untouched():
        torch.cuda.synchronize()
        return bool((hard == 0x55).all()) and bool((iters == -77).all())

    with L.LdpcHipCodes(MS_DEC, ok, M, wide=True) as cs, L.LdpcHip(MS_DEC, ok[0], M) as one:
        for maxiter in (0, -5):
            assert lib.ldpc_hip_decode_codes_dev(cs.h, x.data_ptr(), 0, B, maxiter, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
            assert lib.ldpc_hip_simulate_codes(cs.h, 2.0, 0, maxiter, 0.8, 1, 0, B, cnt, None) == EINVAL
        for punct in (34, 35):                                                    # punctured_blocks >= nh
            assert lib.ldpc_hip_simulate_codes(cs.h, 2.0, punct, 10, 0.8, 1, 0, B, cnt, None) == EINVAL
        # the single-code and GF(q) entry points on a wide set context
        assert lib.ldpc_hip_decode_dev(cs.h, x.data_ptr(), B, 10, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        c4, sit = (C.c_ulonglong * 4)(), C.c_ulonglong()
        assert lib.ldpc_hip_simulate(cs.h, 2.0, 0, 0, 10, 0.8, 1, 0, B, c4, C.byref(sit)) == EINVAL
        assert lib.ldpc_hip_decode_gfq_dev(cs.h, x.data_ptr(), B, 10, 0.0, None, iters.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_decode_codes_gfq_dev(cs.h, x.data_ptr(), 1, B, 10, None, iters.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_codes(cs.h) == 2 and lib.ldpc_hip_codes(one.h) == 0
        # the set entry points on a single-code context
        assert lib.ldpc_hip_decode_codes_dev(one.h, x.data_ptr(), 1, B, 10, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_count_errors_codes_dev(one.h, hard.data_ptr(), iters.data_ptr(), B, None, x.data_ptr(), None) == EINVAL
        assert lib.ldpc_hip_simulate_codes(one.h, 2.0, 0, 10, 0.8, 1, 0, B, cnt, None) == EINVAL
        assert untouched(), "a refused call must not launch anything"
        assert bool((x == 9.0).all())
        # and the context still works: a codeword at the input returns 1
        h2, i2, _ = cs.decode(x, 10, shared=False)
        torch.cuda.synchronize()
        assert bool((i2 == 1).all()) and bool((h2 == 0).all())
