"""Flooding sum-product code sets on the GPU (sp_flood_codes_kernel, asp_flood_codes_kernel; LdpcHipCodes(SP_DEC | ASP_DEC, ...) /
ldpc_hip_open_codes_sp): return values and packed hard words exactly and soft outputs bit for bit against the CPU oracle
(orc_sum_prod, orc_sum_prod_gf2), against the compiled reference's golden vectors and against a single-code LdpcHip context per
matrix (JIT off), in every lifting regime and both LLR layouts; more than 16 block rows; rows of weight 1 next to rows of weight 16;
30 x 60 at M = 67; ASP's all-weight-2 branch per code; code boundaries inside the grid; maxiter = 1; optional outputs; the
shared-noise simulation with its punctured positions; the stopping rule on the device and through the C++ layer; refusals.  The
inputs and their properties are those of codeset_sp_sets.py, asserted on the CPU in test_codeset_sp_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import codeset_sp_sets as S
from codeset_sp_sets import ASP_DEC, DECS, SP_DEC
from codeset_stop_sets import schedule, stop_piece
from ldpc_testlib import ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -2
MAXITER, NCODES = S.MAXITER, S.NCODES
both = pytest.mark.parametrize("dec", DECS, ids=S.DEC_IDS)


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
    """No hiprtc in this file: the single-code contexts run the table-driven or the shape-unlimited tier (or an ahead-of-time
    instance), whose bits are those of every other tier."""
    lib = L.load_library()
    before = lib.ldpc_hip_set_jit_mode(0)
    yield
    lib.ldpc_hip_set_jit_mode(before)


def _np(hard, iters, soft):
    return hard.cpu().numpy().view(np.uint32), iters.cpu().numpy(), soft.cpu().numpy()


def _name(dec, M):
    return ("sp" if dec == SP_DEC else "asp") + "_flood_codes_kernel" + ("<multiwave>" if M > 64 else "")


def _same(got, want, what):
    """got / want = (hard words, return values, soft outputs) of one code."""
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])
    assert np.array_equal(got[0], want[0]), what
    assert_bits_equal(got[2], want[2], what)


def _decode_set(L, torch, dec, codes, M, llr, maxiter, shared=True):
    llr = np.ascontiguousarray(llr)
    x = torch.from_numpy(llr.copy()).cuda()
    with L.LdpcHipCodes(dec, codes, M) as cs:
        assert cs.kernel_name == _name(dec, M) and cs.lib.ldpc_hip_codes(cs.h) == len(codes) and cs.decoder_id == dec
        assert (cs.rh, cs.nh) == codes.shape[1:] and cs.N == codes.shape[2] * M and cs.R == codes.shape[1] * M
        out = cs.decode(x, maxiter, shared=shared, want_soft=True)
        torch.cuda.synchronize()
        assert cs.lib.ldpc_hip_last_launch(cs.h).decode() == cs.kernel_name
    assert_bits_equal(x.cpu().numpy(), llr, "the input is not modified")
    hard, iters, soft = _np(*out)
    return [(hard[c], iters[c], soft[c]) for c in range(len(codes))]


def _decode_one(L, torch, dec, H, M, llr, maxiter):
    with L.LdpcHip(dec, H, M) as one:
        out = _np(*one.decode(torch.from_numpy(np.ascontiguousarray(llr)).cuda(), maxiter, want_soft=True))
    return out


@both
@pytest.mark.parametrize("layout", ["shared", "percode"])
@pytest.mark.parametrize("case", list(S.CASES), ids=S.CASE_IDS)
def test_parity(L, torch, case, layout, dec):
    M, rh, nh = case
    r = S.reference(dec, case)
    codes, ref = r["codes"], r["ref"][layout]
    llr = r["shared"] if layout == "shared" else r["percode"]
    got = _decode_set(L, torch, dec, codes, M, llr, MAXITER, shared=layout == "shared")
    for c in range(NCODES):
        _same(got[c], ref[c], f"code {c} against the oracle")
        _same(got[c], _decode_one(L, torch, dec, codes[c], M, llr if layout == "shared" else llr[c], MAXITER), f"code {c} against LdpcHip")


@pytest.mark.parametrize("which,dec", [("rows17", SP_DEC), ("rows17", ASP_DEC), ("mixed_weights", SP_DEC), ("30x60", SP_DEC), ("30x60", ASP_DEC)])
def test_shapes_only_these_kernels_reach(L, torch, which, dec):
    """17 block rows, codes that mix rows of weight 1 and of weight 16 (SP), and 30 x 60 at M = 67 (two waves per block column, a
    159 184-byte image for SP)."""
    M, codes, llr = {"rows17": S.rows17_set, "mixed_weights": S.mixed_weight_set, "30x60": S.big_set}[which]()
    maxiter = S.BIG["maxiter"] if which == "30x60" else MAXITER
    got = _decode_set(L, torch, dec, codes, M, llr, maxiter)
    if which == "30x60":
        assert got[0][1].tolist() == S.BIG["want"]
    for c in range(NCODES):
        _same(got[c], S.oracle(dec, codes[c], M, llr, maxiter), f"code {c} against the oracle")
        _same(got[c], _decode_one(L, torch, dec, codes[c], M, llr, maxiter), f"code {c} against LdpcHip")


@pytest.mark.parametrize("name", S.GOLDENS)
def test_compiled_reference_as_code_0(L, torch, name):
    """Code 0 against the compiled reference's golden vectors (its soft values cover the first frames only), every code against the
    oracle and against LdpcHip."""
    g = S.golden_set(name)
    codes, M, dec = g["codes"], g["M"], g["dec"]
    got = _decode_set(L, torch, dec, codes, M, g["llr"], g["maxiter"])
    ns = len(g["soft"])
    assert np.array_equal(got[0][1], g["iters"]) and np.array_equal(got[0][0], g["hard"])
    assert_bits_equal(got[0][2][:ns], g["soft"], "code 0 against the compiled reference")
    for c in range(NCODES):
        _same(got[c], S.oracle(dec, codes[c], M, g["llr"], g["maxiter"]), f"code {c} against the oracle")
        _same(got[c], _decode_one(L, torch, dec, codes[c], M, g["llr"], g["maxiter"]), f"code {c} against LdpcHip")


@both
def test_all_weight_2_codes_among_general_ones(L, torch, dec):
    """ASP takes upstream's own branch per code; SP ignores the flag."""
    g = S.cw2_mixed_set()
    codes, M = g["codes"], g["M"]
    got = _decode_set(L, torch, dec, codes, M, g["llr"], g["maxiter"])
    if dec == ASP_DEC:
        assert np.array_equal(got[0][1], g["iters"]) and np.array_equal(got[0][0], g["hard"])
        assert_bits_equal(got[0][2][:len(g["soft"])], g["soft"], "code 0 against the compiled reference")
    for c in range(NCODES):
        _same(got[c], S.oracle(dec, codes[c], M, g["llr"], g["maxiter"]), f"code {c} against the oracle")
        _same(got[c], _decode_one(L, torch, dec, codes[c], M, g["llr"], g["maxiter"]), f"code {c} against LdpcHip")


@both
@pytest.mark.parametrize("B", [1, 4])
def test_code_boundaries(L, torch, B, dec):
    """M = 20 packs three frames into a workgroup, so with B = 1 and B = 4 the last workgroup of each code is partly filled.  Code 1 is
    a codeword at the input and returns 0 with the input transform as its soft output; codes 0 and 2, its neighbours in the grid,
    never converge: no frame's result depends on its neighbours or on the next code."""
    M, codes, llr = S.boundary_set(B)
    ref = [S.oracle(dec, codes[c], M, llr[c], MAXITER) for c in range(3)]
    assert (ref[1][1] == 0).all() and (ref[0][1] == -MAXITER).all() and (ref[2][1] == -MAXITER).all(), [r[1] for r in ref]
    got = _decode_set(L, torch, dec, codes, M, llr, MAXITER, shared=False)
    for c in range(3):
        _same(got[c], ref[c], f"code {c}")
    assert (got[1][0] == 0).all()


@both
def test_maxiter_one(L, torch, dec):
    codes, llr = S.maxiter_one_set()
    ref = [S.oracle(dec, codes[c], 20, llr, 1) for c in range(NCODES)]
    assert set(np.unique([x[1] for x in ref])) == {-1, 1}
    got = _decode_set(L, torch, dec, codes, 20, llr, 1)
    for c in range(NCODES):
        _same(got[c], ref[c], f"code {c}")


@both
@pytest.mark.parametrize("case", [(20, 4, 8), (100, 3, 6)], ids=["M20", "M100"])
def test_optional_outputs(L, torch, case, dec):
    """Each of d_hard, d_iters and d_soft left out in turn: the other two do not change (ASP writes d_soft during the iterations, SP
    forms it at the end)."""
    M = case[0]
    r = S.reference(dec, case)
    codes, ref = r["codes"], r["ref"]["shared"]
    x = torch.from_numpy(r["shared"]).cuda()
    B, N = r["shared"].shape
    with L.LdpcHipCodes(dec, codes, M) as cs:
        for skip in range(3):
            hard = torch.full((NCODES, B, cs.hard_words), 0x55, dtype=torch.int32, device="cuda")
            iters = torch.full((NCODES, B), -77, dtype=torch.int32, device="cuda")
            soft = torch.full((NCODES, B, N), 7.5, dtype=torch.float64, device="cuda")
            ptr = [None if skip == i else t.data_ptr() for i, t in enumerate((hard, iters, soft))]
            assert cs.lib.ldpc_hip_decode_codes_dev(cs.h, x.data_ptr(), 1, B, MAXITER, 0.8, ptr[0], ptr[1], ptr[2], None) == 0
            torch.cuda.synchronize()
            h, i, s = _np(hard, iters, soft)
            for c in range(NCODES):
                assert (h[c] == 0x55).all() if skip == 0 else np.array_equal(h[c], ref[c][0]), (skip, c)
                assert (i[c] == -77).all() if skip == 1 else np.array_equal(i[c], ref[c][1]), (skip, c)
                if skip == 2:
                    assert (s[c] == 7.5).all()
                else:
                    assert_bits_equal(s[c], ref[c][2], f"soft, code {c}, output {skip} left out")


def _stop_reference(L, dec):
    p = S.STOP
    with L.LdpcHipCodes(dec, S.stop_set(), p["M"]) as cs:
        _, info = cs.simulate(p["snr"], MAXITER, p["seed"], 0, p["nexp"] + 1, records=True)
    return np.array([L.host.replay_stop_rule(row, p["nfe"], p["nexp"], p["ref_fer"]) for row in info], dtype=np.uint64)


@both
def test_code_list(L, torch, monkeypatch, dec):
    """simulate_until on [weak, medium, strong]: experiment, nse and nde per code as exact integers against the sequential rule over
    the records of simulate; the weak code stops in the first batch, so every later launch covers a subset of the codes and slot 0 is
    no longer code 0."""
    p = S.STOP
    want = _stop_reference(L, dec)
    pieces = schedule(p["nexp"], p["batch"], p["batch"])
    batches = [pieces[stop_piece(int(e), pieces)][0] for e in want[:, 0]]
    print("reference (experiment, nse, nde):", want.tolist(), "stop batches:", batches)
    assert batches[0] == 0 and max(batches) > 0, "subset launches: the weak code stops first, another one later"
    with L.LdpcHipCodes(dec, S.stop_set(), p["M"]) as cs:
        got = cs.simulate_until(p["snr"], MAXITER, p["seed"], p["nfe"], p["nexp"], p["ref_fer"], first_batch=p["batch"], max_batch=p["batch"])
        wide = cs.simulate_until(p["snr"], MAXITER, p["seed"], p["nfe"], p["nexp"], p["ref_fer"])
        monkeypatch.setenv("LDPC_HIP_CODES_PIECE", "48")
        cut = cs.simulate_until(p["snr"], MAXITER, p["seed"], p["nfe"], p["nexp"], p["ref_fer"], first_batch=p["batch"], max_batch=p["batch"])
        monkeypatch.delenv("LDPC_HIP_CODES_PIECE")
    for what, res in (("64/64", got), ("default", wide), ("pieces of 48", cut)):
        assert np.array_equal(res[:, :3], want), (what, res.tolist(), want.tolist())
    assert got[:, 3].tolist() == [min(p["batch"] * (b + 1), p["nexp"] + 1) for b in batches]


@both
@pytest.mark.parametrize("punct", [0, 1])
def test_simulate(L, torch, punct, monkeypatch, dec):
    """simulate_codes = C single-code simulations over the same noise: counters and ordered records, however the frames are split.
    With a punctured block the channel value of the punctured positions must be 0.0 (out_type 1), not min-sum's 0.5."""
    M, Cn, B, first, snr, seed = (S.SIM[k] for k in ("M", "C", "B", "first", "snr", "seed"))
    codes = S.simulate_set()
    with L.LdpcHipCodes(dec, codes, M) as cs:
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
        with L.LdpcHip(dec, codes[q], M) as one:
            s = one.simulate(snr, MAXITER, seed, first, B, punctured_blocks=punct)
            x = one.awgn_llr(snr, seed, first, B, punctured_blocks=punct)
            if punct:
                assert bool((x[:, -M:] == 0.0).all())
            h1, i1, _ = one.decode(x, MAXITER)
            _, inf1 = one.count_errors(h1, i1, want_frame_info=True, first_frame=first)
            torch.cuda.synchronize()
        assert [s["nse"], s["nde"], s["nue"], s["frames"], s["sum_abs_iters"]] == cnt[q].tolist(), (q, s, cnt[q])
        assert np.array_equal(inf1.cpu().numpy(), info[q]), q


def _driver(tmp_path, name):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", name + ".cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_compat", "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    return exe


@both
def test_cpp_layer(L, torch, tmp_path, dec):
    """ldpc::bp_simulation_codes with decoder 1 and 2 through the code-set driver: the set against one
    ldpc::bp_simulation_throughput_t call per code, and those of the Python reference."""
    L.load_library()
    p = S.STOP
    codes = S.stop_set()
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(codes), codes.shape[1], codes.shape[2], p["M"], dec, MAXITER, p["nfe"], p["nexp"], p["batch"], p["seed"]], dtype=np.int32).tobytes())
        f.write(np.array([p["snr"], p["ref_fer"]], dtype=np.float64).tobytes())
        f.write(codes.tobytes())
    env = dict(os.environ, LDPC_HIP_JIT="0")
    want = _stop_reference(L, dec)
    out = subprocess.check_output([_driver(tmp_path, "codes_driver"), str(tmp_path / "in.bin")], env=env, timeout=120).decode().split("\n")
    rows = {(w[0], int(w[1])): w[2:] for w in (line.split() for line in out if line.startswith(("set ", "one ")))}
    assert len(rows) == 2 * len(codes), out
    for c in range(len(codes)):
        assert rows["set", c] == rows["one", c], (c, rows["set", c], rows["one", c])
        assert [int(v) for v in rows["set", c][2:]] == [int(want[c, 1]), int(want[c, 2]), int(want[c, 0])], c


@both
def test_refusals_and_cross_use(L, torch, dec):
    lib = L.load_library()
    ok = S.boundary_set(1)[1][:2]

    def open_rc(fn, codes, M, *dec_):
        codes = np.ascontiguousarray(codes, dtype=np.int16)
        h = C.c_void_p()
        rc = fn(*dec_, codes.shape[1], codes.shape[2], M, codes.ctypes.data, codes.shape[0], 0, C.byref(h))
        assert (rc == 0) == bool(h.value)
        if h.value:
            lib.ldpc_hip_close(h)
        return rc

    assert open_rc(lib.ldpc_hip_open_codes, ok, 20, dec) == EINVAL               # decoders 1 and 2 have their own entry point
    assert "decoder id" in lib.ldpc_hip_last_error().decode()
    assert open_rc(lib.ldpc_hip_open_codes_sp, ok, 20, 0) == EINVAL              # which Gallager BP does not share
    assert "decoder id" in lib.ldpc_hip_last_error().decode()
    assert open_rc(lib.ldpc_hip_open_codes_sp, ok, 20, dec) == 0
    bad = ok.copy(); bad[1, 2, :] = -1                                            # an empty block row
    assert open_rc(lib.ldpc_hip_open_codes_sp, bad, 20, dec) == EINVAL
    msg = lib.ldpc_hip_last_error().decode()
    assert "code 1" in msg and "row 2" in msg, msg
    big = S.appendix_c(512)
    assert open_rc(lib.ldpc_hip_open_codes_sp, big, 512, dec) == EUNSUPPORTED
    assert str(S.lds_bytes(dec, big, 512)) in lib.ldpc_hip_last_error().decode()

    B, N, W = 4, 8 * 20, 5
    x = torch.full((2, B, N), 9.0, dtype=torch.float64, device="cuda")
    hard = torch.full((2, B, W), 0x55, dtype=torch.int32, device="cuda")
    iters = torch.full((2, B), -77, dtype=torch.int32, device="cuda")
    cnt = (C.c_ulonglong * 10)()

    def untouched():
        torch.cuda.synchronize()
        return bool((hard == 0x55).all()) and bool((iters == -77).all())

    with L.LdpcHipCodes(dec, ok, 20) as cs, L.LdpcHip(dec, ok[0], 20) as one:
        for maxiter in (0, -5):
            assert lib.ldpc_hip_decode_codes_dev(cs.h, x.data_ptr(), 0, B, maxiter, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        # the single-code and GF(q) entry points on a set context
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
        # and the context still works; alpha is not read
        h2, i2, _ = cs.decode(x, 10, shared=False, alpha=0.8)
        h3, i3, _ = cs.decode(x, 10, shared=False, alpha=0.123)
        torch.cuda.synchronize()
        assert bool((i2 == 0).all()) and bool((h2 == 0).all()) and bool((i3 == 0).all()) and bool((h3 == 0).all())
