"""Integer min-sum code sets on the GPU (ims_quantise_kernel + ims_flood_codes_kernel, LdpcHipCodes(IMS_DEC, ...) /
ldpc_hip_open_codes_ims): return values, packed hard words and soft outputs EXACTLY against the CPU oracle (orc_imin_sum) and against
a single-code LdpcHip context per matrix (JIT off), in every lifting regime and both LLR layouts; the quantiser and data-path word
lengths and alpha; the compiled reference's golden vector; more than 16 block rows and 32 block columns; rows of weight 1 next to
rows of weight 16; adversarial channel values; code boundaries inside the grid; maxiter = 1; the shared-noise simulation and its
split invariance; the stopping rule on the device and through the C++ layer; refusals.  The inputs and their properties are those
of codeset_ims_sets.py, asserted on the CPU in test_codeset_ims_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import codeset_ims_sets as S
from codeset_ims_sets import IMS_DEC
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
    """No hiprtc in this file: the single-code IMS contexts run ims_flood_kernel, ims_global_kernel or the ahead-of-time instance,
    whose bits are those of every other tier."""
    lib = L.load_library()
    before = lib.ldpc_hip_set_jit_mode(0)
    yield
    lib.ldpc_hip_set_jit_mode(before)


def _np(hard, iters, soft):
    return hard.cpu().numpy().view(np.uint32), iters.cpu().numpy(), soft.cpu().numpy()


def _name(M):
    return "ims_flood_codes_kernel" + ("<multiwave>" if M > 64 else "")


def _same(got, want, what):
    """got / want = (hard words, return values, soft outputs) of one code."""
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])
    assert np.array_equal(got[0], want[0]), what
    assert_bits_equal(got[2], want[2], what)


def _set_decode(cs, torch, llr, maxiter, shared=True, params=S.DEFAULTS):
    llr = np.ascontiguousarray(llr)
    x = torch.from_numpy(llr.copy()).cuda()
    cs.set_ims_params(*params[1:])
    out = cs.decode(x, maxiter, alpha=params[0], shared=shared, want_soft=True)
    torch.cuda.synchronize()
    assert cs.lib.ldpc_hip_last_launch(cs.h).decode() == cs.kernel_name
    assert_bits_equal(x.cpu().numpy(), llr, "the input is not modified")
    hard, iters, soft = _np(*out)
    return [(hard[c], iters[c], soft[c]) for c in range(cs.C)]


def _decode_set(L, torch, codes, M, llr, maxiter, shared=True, params=S.DEFAULTS):
    with L.LdpcHipCodes(IMS_DEC, codes, M) as cs:
        assert cs.kernel_name == _name(M) and cs.lib.ldpc_hip_codes(cs.h) == len(codes) and cs.decoder_id == IMS_DEC
        assert (cs.rh, cs.nh) == codes.shape[1:] and cs.R == codes.shape[1] * M and cs.N == codes.shape[2] * M
        return _set_decode(cs, torch, llr, maxiter, shared, params)


def _decode_one(L, torch, H, M, llr, maxiter, params=S.DEFAULTS):
    with L.LdpcHip(IMS_DEC, H, M) as one:
        one.set_ims_params(*params[1:])
        out = _np(*one.decode(torch.from_numpy(np.ascontiguousarray(llr)).cuda(), maxiter, alpha=params[0], want_soft=True))
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
        _same(got[c], ref[c], f"code {c} against the oracle")
        _same(got[c], _decode_one(L, torch, codes[c], M, llr if layout == "shared" else llr[c], MAXITER), f"code {c} against LdpcHip")


@pytest.mark.parametrize("params", S.PARAM_SETS, ids=S.PARAM_IDS)
@pytest.mark.parametrize("case", S.PARAM_CASES, ids=["M32", "M100"])
def test_parameters(L, torch, case, params):
    """alpha, thr, qbits and dbits are read: defaults, then the parameter set, then the defaults again on ONE context.  The first and
    the third result are equal (and the oracle's), the second is the oracle's and LdpcHip's with these parameters."""
    M = case[0]
    r = S.reference(case)
    codes, llr = r["codes"], r["shared"]
    with L.LdpcHipCodes(IMS_DEC, codes, M) as cs:
        first = _set_decode(cs, torch, llr, MAXITER)
        second = _set_decode(cs, torch, llr, MAXITER, params=params)
        third = _set_decode(cs, torch, llr, MAXITER)
    ref = S.param_reference(case, params)
    for c in range(NCODES):
        _same(first[c], r["ref"]["shared"][c], f"code {c}, defaults")
        _same(third[c], first[c], f"code {c}, defaults again")
        _same(second[c], ref[c], f"code {c} against the oracle, {params}")
        _same(second[c], _decode_one(L, torch, codes[c], M, llr, MAXITER, params), f"code {c} against LdpcHip, {params}")


def test_compiled_reference_as_code_0(L, torch):
    """Code 0 against the compiled reference's golden vector (16 frames of return values and hard words, 4 of soft values), the two
    relabelled codes against the oracle."""
    g = S.golden_set()
    codes, M = g["codes"], g["M"]
    got = _decode_set(L, torch, codes, M, g["llr"], g["maxiter"])
    assert np.array_equal(got[0][1], g["iters"]) and np.array_equal(got[0][0], g["hard"])
    assert_bits_equal(got[0][2][:len(g["soft"])], g["soft"], "code 0 against the compiled reference")
    for c in range(1, len(codes)):
        _same(got[c], S.oracle(codes[c], M, g["llr"], g["maxiter"]), f"code {c} against the oracle")


@pytest.mark.parametrize("which", ["30x60_M67", "rows17", "mixed_weights"])
def test_shapes_only_this_kernel_reaches(L, torch, which):
    """30 x 60 at M = 67 and 17 x 34 (the register-resident set kernels hold 16 block rows, flooding min-sum 32 block columns), and
    codes that mix rows of weight 1 and of weight 16."""
    M, codes, llr = {"30x60_M67": S.big_set, "rows17": S.rows17_set, "mixed_weights": S.mixed_weight_set}[which]()
    got = _decode_set(L, torch, codes, M, llr, MAXITER)
    for c in range(NCODES):
        _same(got[c], S.oracle(codes[c], M, llr, MAXITER), f"code {c} against the oracle")
        _same(got[c], _decode_one(L, torch, codes[c], M, llr, MAXITER), f"code {c} against LdpcHip")


@pytest.mark.parametrize("case", S.ADVERSARIAL_CASES, ids=["M20", "M100"])
def test_adversarial_frames(L, torch, case):
    """adversarial_llr's families (en = 0, en = inf, quantiser rounding boundaries, ties, clamps; all finite): every frame against
    LdpcHip per code and against the oracle, to which test_gpu_adversarial.py holds the single-code integer kernels on every frame."""
    M = case[0]
    codes, llr, labels = S.adversarial_set(case)
    got = _decode_set(L, torch, codes, M, llr, MAXITER)
    for c in range(NCODES):
        one = _decode_one(L, torch, codes[c], M, llr, MAXITER)
        ref = S.oracle(codes[c], M, llr, MAXITER)
        for f, label in enumerate(labels):
            _same(tuple(x[f] for x in got[c]), tuple(x[f] for x in one), f"code {c}, frame {f} ({label}) against LdpcHip")
            _same(tuple(x[f] for x in got[c]), tuple(x[f] for x in ref), f"code {c}, frame {f} ({label}) against the oracle")


@pytest.mark.parametrize("B", [1, 4])
def test_code_boundaries(L, torch, B):
    """M = 20 packs three frames into a wave, so with B = 1 and B = 4 the last wave of each code is partly filled.  Code 1 sees a
    codeword and returns 1 (integer min-sum has no return value 0); codes 0 and 2, its neighbours in the grid, never converge: no
    frame's result depends on its wave-mates or on the next code."""
    M, codes, llr = S.boundary_set(B)
    ref = [S.oracle(codes[c], M, llr[c], MAXITER) for c in range(3)]
    assert (ref[1][1] == 1).all() and (ref[0][1] == -MAXITER).all() and (ref[2][1] == -MAXITER).all(), [r[1] for r in ref]
    got = _decode_set(L, torch, codes, M, llr, MAXITER, shared=False)
    for c in range(3):
        _same(got[c], ref[c], f"code {c}")
    assert (got[1][0] == 0).all()


def test_maxiter_one(L, torch):
    codes, llr = S.maxiter_one_set()
    ref = [S.oracle(codes[c], 20, llr, 1) for c in range(NCODES)]
    assert set(np.unique([x[1] for x in ref])) == {-1, 1}
    got = _decode_set(L, torch, codes, 20, llr, 1)
    for c in range(NCODES):
        _same(got[c], ref[c], f"code {c}")


@pytest.mark.parametrize("punct", [0, 1])
def test_simulate(L, torch, punct, monkeypatch):
    """simulate_codes = C single-code simulations over the same noise: counters and ordered records, however the frames are split.
    With a punctured block the channel value of the punctured positions is the 0.5 of the LLR decoders."""
    M, Cn, B, first, snr, seed = (S.SIM[k] for k in ("M", "C", "B", "first", "snr", "seed"))
    codes = S.simulate_set()
    with L.LdpcHipCodes(IMS_DEC, codes, M) as cs:
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
        with L.LdpcHip(IMS_DEC, codes[q], M) as one:
            s = one.simulate(snr, MAXITER, seed, first, B, punctured_blocks=punct)
            x = one.awgn_llr(snr, seed, first, B, punctured_blocks=punct)
            if punct:
                assert bool((x[:, -M:] == 0.5).all())
            h1, i1, _ = one.decode(x, MAXITER)
            _, inf1 = one.count_errors(h1, i1, want_frame_info=True, first_frame=first)
            torch.cuda.synchronize()
        assert [s["nse"], s["nde"], s["nue"], s["frames"], s["sum_abs_iters"]] == cnt[q].tolist(), (q, s, cnt[q])
        assert np.array_equal(inf1.cpu().numpy(), info[q]), q


def _stop_reference(L):
    p = S.STOP
    with L.LdpcHipCodes(IMS_DEC, S.stop_set(), p["M"]) as cs:
        _, info = cs.simulate(p["snr"], MAXITER, p["seed"], 0, p["nexp"] + 1, records=True)
    return np.array([L.host.replay_stop_rule(row, p["nfe"], p["nexp"], p["ref_fer"]) for row in info], dtype=np.uint64)


def test_stopping_rule_on_the_device(L, torch, monkeypatch):
    """simulate_until on [weak, medium, strong]: experiment, nse and nde per code as exact integers against the sequential rule over
    the records of simulate; the weak code stops in the first batch, so every later launch covers a subset of the codes and slot 0 is
    no longer code 0 (while the quantiser still runs once per piece)."""
    p = S.STOP
    want = _stop_reference(L)
    pieces = schedule(p["nexp"], p["batch"], p["batch"])
    batches = [pieces[stop_piece(int(e), pieces)][0] for e in want[:, 0]]
    print("reference (experiment, nse, nde):", want.tolist(), "stop batches:", batches)
    assert batches[0] == 0 and max(batches) > 0, "subset launches: the weak code stops first, another one later"
    with L.LdpcHipCodes(IMS_DEC, S.stop_set(), p["M"]) as cs:
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


def test_cpp_layer(L, torch, tmp_path):
    """ldpc::bp_simulation_codes with decoder 4 through the stopping-rule driver on both routes, show_process = 0 (the rule on the
    device) and = 1 (the records replayed on the host): the same counters, and those of the Python reference."""
    L.load_library()
    p = S.STOP
    codes = S.stop_set()
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(codes), codes.shape[1], codes.shape[2], p["M"], IMS_DEC, MAXITER, p["nfe"], p["nexp"], p["batch"], p["seed"]], dtype=np.int32).tobytes())
        f.write(np.array([p["snr"], p["ref_fer"]], dtype=np.float64).tobytes())
        f.write(codes.tobytes())
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = str(tmp_path / "codes_stop_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "codes_stop_driver.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_compat", "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    want = _stop_reference(L)
    out = subprocess.check_output([exe, str(tmp_path / "in.bin")], env=dict(os.environ, LDPC_HIP_JIT="0"), timeout=120).decode().split("\n")
    rows = {(w[0], int(w[1])): w[2:] for w in (line.split() for line in out if line.startswith(("device ", "host ")))}
    assert len(rows) == 2 * len(codes), out
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

    assert open_rc(lib.ldpc_hip_open_codes, ok, 20, IMS_DEC) == EINVAL           # decoder 4 has its own entry point
    assert "decoder id" in lib.ldpc_hip_last_error().decode()
    assert open_rc(lib.ldpc_hip_open_codes_ims, ok, 20) == 0
    bad = ok.copy(); bad[1, 2, :] = -1                                            # an empty block row
    assert open_rc(lib.ldpc_hip_open_codes_ims, bad, 20) == EINVAL
    msg = lib.ldpc_hip_last_error().decode()
    assert "code 1" in msg and "row 2" in msg, msg
    assert open_rc(lib.ldpc_hip_open_codes_ims, S.dense_set(20, 40, 512), 512) == EUNSUPPORTED
    assert "163856" in lib.ldpc_hip_last_error().decode()

    B, N, W = 4, 8 * 20, 5
    x = torch.full((2, B, N), 9.0, dtype=torch.float64, device="cuda")
    hard = torch.full((2, B, W), 0x55, dtype=torch.int32, device="cuda")
    iters = torch.full((2, B), -77, dtype=torch.int32, device="cuda")
    cnt = (C.c_ulonglong * 10)()

    def untouched():
        torch.cuda.synchronize()
        return bool((hard == 0x55).all()) and bool((iters == -77).all())

    with L.LdpcHipCodes(IMS_DEC, ok, 20) as cs, L.LdpcHip(IMS_DEC, ok[0], 20) as one:
        for maxiter in (0, -5):
            assert lib.ldpc_hip_decode_codes_dev(cs.h, x.data_ptr(), 0, B, maxiter, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
            assert lib.ldpc_hip_simulate_codes(cs.h, 2.0, 0, maxiter, 0.8, 1, 0, B, cnt, None) == EINVAL
        for punct in (8, 9):                                                      # punctured_blocks >= nh
            assert lib.ldpc_hip_simulate_codes(cs.h, 2.0, punct, 10, 0.8, 1, 0, B, cnt, None) == EINVAL
        for bad_params in ((0.0, 6, 8), (1.4, 1, 8), (1.4, 16, 8), (1.4, 6, 16)):  # the accepted ranges are those of a single-code context
            assert lib.ldpc_hip_set_ims_params(cs.h, C.c_double(bad_params[0]), bad_params[1], bad_params[2]) == EINVAL
        # the single-code and GF(q) entry points on an IMS set context
        assert lib.ldpc_hip_decode_dev(cs.h, x.data_ptr(), B, 10, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        c4, sit = (C.c_ulonglong * 4)(), C.c_ulonglong()
        assert lib.ldpc_hip_simulate(cs.h, 2.0, 0, 0, 10, 0.8, 1, 0, B, c4, C.byref(sit)) == EINVAL
        assert lib.ldpc_hip_decode_gfq_dev(cs.h, x.data_ptr(), B, 10, 0.0, None, iters.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_decode_codes_gfq_dev(cs.h, x.data_ptr(), 1, B, 10, None, iters.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_codes(cs.h) == 2 and lib.ldpc_hip_codes(one.h) == 0
        # the set entry points on a single-code IMS context
        assert lib.ldpc_hip_decode_codes_dev(one.h, x.data_ptr(), 1, B, 10, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_count_errors_codes_dev(one.h, hard.data_ptr(), iters.data_ptr(), B, None, x.data_ptr(), None) == EINVAL
        assert lib.ldpc_hip_simulate_codes(one.h, 2.0, 0, 10, 0.8, 1, 0, B, cnt, None) == EINVAL
        assert untouched(), "a refused call must not launch anything"
        assert bool((x == 9.0).all())
        # and the context still works: a codeword at the input returns 1
        h2, i2, _ = cs.decode(x, 10, shared=False)
        torch.cuda.synchronize()
        assert bool((i2 == 1).all()) and bool((h2 == 0).all())
