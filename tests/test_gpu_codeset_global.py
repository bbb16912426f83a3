"""The global-memory tier of a code set on the GPU (ldpc_hip_open_codes_global, LdpcHipCodes(tier=...)): every result compared with
tolerance 0 -- return values, packed hard bits, soft values, counters -- against the CPU references of codeset_global_sets.py, against
one LdpcHip per matrix, and against the set route that takes the same set today.  The tests of shapes beyond the limits (M = 513,
M = 4100, the 294 928-byte TDMP image) fail without the route."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import codeset_global_sets as S
from ldpc_testlib import ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu
IDS = [S.DEC_IDS[d] for d in S.DECS]


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
    """The single-code contexts open without hiprtc: their bits are those of every other tier."""
    lib = L.load_library()
    before = lib.ldpc_hip_set_jit_mode(0)
    yield
    lib.ldpc_hip_set_jit_mode(before)


def run_set(cs, torch, llr, maxiter=S.MAXITER, alpha=0.8):
    hard, iters, soft = cs.decode(torch.from_numpy(np.ascontiguousarray(llr)).cuda(), maxiter, alpha=alpha, shared=llr.ndim == 2, want_soft=True)
    torch.cuda.synchronize()
    return hard.cpu().numpy().view(np.uint32), iters.cpu().numpy(), soft.cpu().numpy()


def check_against(got, ref, what):
    hard, iters, soft = got
    for c, (rh, ri, rs) in enumerate(ref):
        assert np.array_equal(iters[c], ri), (what, c, iters[c], ri)
        assert np.array_equal(hard[c], rh), (what, c)
        assert_bits_equal(soft[c], rs, f"{what}, code {c}, soft", nan_ok=True)


def single(L, torch, dec, H, M, llr, maxiter=S.MAXITER, alpha=0.8, ims=None):
    with L.LdpcHip(dec, H, M, device=0) as one:
        if ims:
            one.set_ims_params(*ims)
        hard, iters, soft = one.decode(torch.from_numpy(np.ascontiguousarray(llr)).cuda(), maxiter, alpha=alpha, want_soft=True)
        torch.cuda.synchronize()
        return hard.cpu().numpy().view(np.uint32), iters.cpu().numpy(), soft.cpu().numpy()


@pytest.mark.parametrize("layout", ["shared", "percode"])
@pytest.mark.parametrize("M", S.LIFTINGS)
@pytest.mark.parametrize("dec", S.DECS, ids=IDS)
def test_parity(L, torch, dec, M, layout):
    r = S.reference(M, dec)
    with L.LdpcHipCodes(dec, r["codes"], M, tier="global") as cs:
        assert cs.kernel_name == S.KERNEL[dec] and cs.entry == "ldpc_hip_open_codes_global"
        got = run_set(cs, torch, r[layout])
    check_against(got, r["ref"][layout], f"{S.DEC_IDS[dec]} M={M} {layout} against the reference")
    ones = [single(L, torch, dec, H, M, r[layout] if layout == "shared" else r[layout][c]) for c, H in enumerate(r["codes"])]
    check_against(got, ones, f"{S.DEC_IDS[dec]} M={M} {layout} against LdpcHip")


@pytest.mark.parametrize("dec", S.DECS, ids=IDS)
def test_both_routes(L, torch, dec):
    """The same set on the route it takes today and on the global tier: decode, simulate, simulate_until (the weak code stops first, so
    later launches cover a subset) and mt_simulate_until (every field but frames_decoded; the generator afterwards)."""
    codes, M = S.both_routes_set(dec), 20
    llr = S.ladder_llr(codes[0], M, 4242 + dec)
    out = {}
    for tier in ("auto", "global"):
        with L.LdpcHipCodes(dec, codes, M, tier=tier) as cs:
            assert (cs.entry == "ldpc_hip_open_codes_global") == (tier == "global")
            res = dict(decode=run_set(cs, torch, llr))
            res["simulate"] = cs.simulate(S.SIM["snr"], S.MAXITER, S.SIM["seed"], S.SIM["first"], S.SIM["B"], records=True)
            res["until"] = cs.simulate_until(S.STOP["snr"], S.MAXITER, S.STOP["seed"], S.STOP["nfe"], S.STOP["nexp"], S.STOP["ref_fer"],
                                             first_batch=S.STOP["batch"], max_batch=4 * S.STOP["batch"])
            state = np.arange(624, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(dec)
            cs.mt_set_state(state, 624)
            res["mt_until"] = cs.mt_simulate_until(S.STOP["snr"], S.MAXITER, S.STOP["nfe"], S.STOP["nexp"], S.STOP["ref_fer"],
                                                   first_batch=S.STOP["batch"], max_batch=4 * S.STOP["batch"])
            res["mt_state"] = cs.mt_get_state()
            out[tier] = res
    a, g = out["auto"], out["global"]
    for x, y in zip(a["decode"][:2], g["decode"][:2]):
        assert np.array_equal(x, y)
    assert_bits_equal(g["decode"][2], a["decode"][2], "soft", nan_ok=True)
    assert np.array_equal(a["simulate"][0], g["simulate"][0]) and np.array_equal(a["simulate"][1], g["simulate"][1])
    assert np.array_equal(a["until"], g["until"]), (a["until"], g["until"])
    assert len(set(a["until"][:, 0].tolist())) > 1, "the codes stop at different frames"
    assert np.array_equal(a["mt_until"][:, :5], g["mt_until"][:, :5])
    assert np.array_equal(a["mt_state"][0], g["mt_state"][0]) and a["mt_state"][1] == g["mt_state"][1]


@pytest.mark.parametrize("how", ["global", "default"])
@pytest.mark.parametrize("dec", S.DECS, ids=IDS)
def test_lifting_513(L, torch, dec, how):
    codes, llr, ref = S.beyond_reference(513, dec)
    with L.LdpcHipCodes(dec, codes, 513, **({"tier": "global"} if how == "global" else {})) as cs:
        assert cs.kernel_name == S.KERNEL[dec] and cs.entry == "ldpc_hip_open_codes_global"
        check_against(run_set(cs, torch, llr), ref, f"{S.DEC_IDS[dec]} at M = 513")


@pytest.mark.parametrize("dec", [S.MS_DEC, S.TASP_DEC], ids=["MS", "TDMP"])
def test_lifting_4100(L, torch, dec):
    """N = 16 400: workgroups of 1024 threads."""
    codes, llr, ref = S.beyond_reference(4100, dec)
    with L.LdpcHipCodes(dec, codes, 4100) as cs:
        assert cs.kernel_name == S.KERNEL[dec] and cs.N == 16400
        check_against(run_set(cs, torch, llr), ref, f"{S.DEC_IDS[dec]} at M = 4100")


def test_appendix_c_m256_tdmp(L, torch):
    """The image of 294 928 bytes that ldpc_hip_open_codes_tdmp refuses: the default route falls through to the global tier."""
    codes, llr, ref = S.appendix_c_m256()
    with L.LdpcHipCodes(S.TASP_DEC, codes, 256) as cs:
        assert cs.kernel_name == S.KERNEL[S.TASP_DEC] and cs.entry == "ldpc_hip_open_codes_global"
        check_against(run_set(cs, torch, llr, maxiter=15), ref, "TDMP, Appendix C at M = 256")


@pytest.mark.parametrize("B,cap", [(50, "7"), (400, None)], ids=["7 workgroups, 3 x 50", "1024 workgroups, 3 x 400"])
@pytest.mark.parametrize("dec", S.DECS, ids=IDS)
def test_workgroups_walk_many_items(L, torch, dec, B, cap, monkeypatch):
    """LDPC_HIP_CODES_GLOBAL_GRID=7 over 150 items, and the default cap of 1024 under 1200 items: a workgroup moves from code to code
    (another ne, other weights, another cw2) and must read nothing of its previous item.  Equal to the reference, and with the cap
    set equal to the uncapped run."""
    codes, llr = S.walk_inputs(dec, B)
    with L.LdpcHipCodes(dec, codes, 5, tier="global") as cs:
        free = run_set(cs, torch, llr)
        if cap:
            monkeypatch.setenv("LDPC_HIP_CODES_GLOBAL_GRID", cap)
            capped = run_set(cs, torch, llr)
            for x, y in zip(capped[:2], free[:2]):
                assert np.array_equal(x, y)
            assert_bits_equal(capped[2], free[2], "soft", nan_ok=True)
    check_against(free, S.walk_reference(dec, B), f"{S.DEC_IDS[dec]}, 3 x {B}")


def test_alpha_and_ims_params(L, torch):
    codes = S.small_set(67, "B")
    llr = S.ladder_llr(codes[0], 67, 99)
    with L.LdpcHipCodes(S.MS_DEC, codes, 67, tier="global") as cs:
        check_against(run_set(cs, torch, llr, alpha=0.75), [S.oracle(S.MS_DEC, H, 67, llr, alpha=0.75) for H in codes], "MS, alpha 0.75")
    params = (0.8, 2.0, 5, 7)
    with L.LdpcHipCodes(S.IMS_DEC, codes, 67, tier="global") as cs:
        cs.set_ims_params(*params[1:])
        check_against(run_set(cs, torch, llr), [S.oracle(S.IMS_DEC, H, 67, llr, ims=params) for H in codes], "IMS, thr 2.0, 5 and 7 bits")


def test_alpha_that_is_not_above_zero(L, torch):
    """Upstream's c2v value keeps the sign of m * alpha (decoders.cpp:4719-4720) and its y + acc * alpha is -0.0 where y and the
    product are; ms_global_frame is that arithmetic as written (the set kernels of the other routes refuse such an alpha), and the
    integer decoder's (m * ialpha) >> 4 with ialpha = -12 is the arithmetic shift of a negative product."""
    codes = S.small_set(67, "B")
    llr = np.array(S.ladder_llr(codes[0], 67, 99))
    llr[0, 1] = -0.0; llr[1, ::7] = -0.0; llr[2, ::5] = 0.0
    for dec, alpha in ((S.MS_DEC, -0.8), (S.MS_DEC, -0.0), (S.MS_DEC, 0.0), (S.IMS_DEC, -0.8)):
        ref = [S.oracle(dec, H, 67, llr, alpha=alpha) for H in codes]
        assert any(not np.array_equal(a[2], b[2]) for a, b in zip(ref, [S.oracle(dec, H, 67, llr, alpha=0.8) for H in codes])), "alpha must matter"
        if dec == S.MS_DEC:
            assert any(np.signbit(a[2][a[2] == 0]).any() for a in ref), "soft values of -0.0"
        with L.LdpcHipCodes(dec, codes, 67, tier="global") as cs:
            assert cs.kernel_name == S.KERNEL[dec]
            check_against(run_set(cs, torch, llr, alpha=alpha), ref, f"{S.DEC_IDS[dec]}, alpha {alpha!r}")
    with L.LdpcHipCodes(S.MS_DEC, codes, 67, tier="global") as cs:
        with pytest.raises(L.LdpcHipError, match="alpha"):
            run_set(cs, torch, llr, alpha=float("nan"))


@pytest.mark.parametrize("dec", S.DECS, ids=IDS)
def test_nan_and_inf(L, torch, dec):
    """NaN and +-Inf channel values.  Every decoder against one LdpcHip per matrix; against the CPU oracle where that is compiled C with
    IEEE arithmetic (decoders 1, 2, 3, 7, 8).  The integer decoders convert a NaN to an integer, which C leaves undefined and the numpy
    restatements of decoders 5 and 9 do not model: for 4, 5 and 9 the single-code context is the reference."""
    codes = S.small_set(67, S.kind(dec))
    bad = S.ladder_llr(codes[0], 67, 99)
    bad[1, 5] = np.nan; bad[2, 7] = np.inf; bad[3, 11] = -np.inf; bad[4, ::3] = np.inf
    with L.LdpcHipCodes(dec, codes, 67, tier="global") as cs:
        got = run_set(cs, torch, bad)
    check_against(got, [single(L, torch, dec, H, 67, bad) for H in codes], f"{S.DEC_IDS[dec]}, NaN and Inf against LdpcHip")
    if dec in (S.SP_DEC, S.ASP_DEC, S.MS_DEC, S.TASP_DEC, S.LMS_DEC):
        check_against(got, [S.oracle(dec, H, 67, bad) for H in codes], f"{S.DEC_IDS[dec]}, NaN and Inf against the oracle")


@pytest.mark.parametrize("dec", [S.MS_DEC, S.TASP_DEC, S.IASP_DEC], ids=["MS", "TDMP", "IASP"])
def test_simulate_splits_and_punctured_blocks(L, torch, dec, monkeypatch):
    codes = S.small_set(67, S.kind(dec))
    with L.LdpcHipCodes(dec, codes, 67, tier="global") as cs:
        whole, info = cs.simulate(2.0, S.MAXITER, 5, 100, 90, punctured_blocks=2, records=True)
        monkeypatch.setenv("LDPC_HIP_CODES_PIECE", "13")
        parts = [cs.simulate(2.0, S.MAXITER, 5, 100 + f, n, punctured_blocks=2, records=True) for f, n in ((0, 40), (40, 50))]
        monkeypatch.delenv("LDPC_HIP_CODES_PIECE")
    assert np.array_equal(whole, parts[0][0] + parts[1][0]) and np.array_equal(info, np.concatenate([parts[0][1], parts[1][1]], axis=1))
    with L.LdpcHipCodes(dec, codes, 67) as old:   # the route the set takes today
        assert old.entry != "ldpc_hip_open_codes_global"
        old_cnt, old_info = old.simulate(2.0, S.MAXITER, 5, 100, 90, punctured_blocks=2, records=True)
    assert np.array_equal(whole, old_cnt) and np.array_equal(info, old_info)


@pytest.mark.parametrize("dec", S.DECS, ids=IDS)
def test_maxiter_one_and_optional_outputs(L, torch, dec):
    codes = S.small_set(64, S.kind(dec))
    llr = S.ladder_llr(codes[0], 64, 64 + dec)
    ref = [S.oracle(dec, H, 64, llr, maxiter=1) for H in codes]
    t = torch.from_numpy(llr).cuda()
    with L.LdpcHipCodes(dec, codes, 64, tier="global") as cs:
        check_against(run_set(cs, torch, llr, maxiter=1), ref, f"{S.DEC_IDS[dec]}, maxiter 1")
        for skip in range(3):
            hard = torch.full((3, len(llr), cs.hard_words), -1, dtype=torch.int32, device="cuda")
            iters = torch.full((3, len(llr)), -99, dtype=torch.int32, device="cuda")
            soft = torch.full((3, len(llr), cs.N), -7.0, dtype=torch.float64, device="cuda")
            ptr = [None if skip == q else x.data_ptr() for q, x in enumerate((hard, iters, soft))]
            rc = cs.lib.ldpc_hip_decode_codes_dev(cs.h, t.data_ptr(), 1, len(llr), 1, 0.8, ptr[0], ptr[1], ptr[2], None)
            torch.cuda.synchronize()
            assert rc == 0
            got = (hard.cpu().numpy().view(np.uint32), iters.cpu().numpy(), soft.cpu().numpy())
            for c, r in enumerate(ref):
                for q in range(3):
                    if q == skip:
                        assert (got[q][c] == (0xffffffff, -99, -7.0)[q]).all()
                    elif q == 2:
                        assert_bits_equal(got[q][c], r[q], "soft", nan_ok=True)
                    else:
                        assert np.array_equal(got[q][c], r[q])


@pytest.mark.parametrize("dec", [S.MS_DEC, S.IMS_DEC, S.TASP_DEC], ids=["MS", "IMS", "TDMP"])
def test_refused_calls_leave_everything_alone(L, torch, dec):
    """A refused call on a context of the route launches nothing and leaves outputs, counters, the [C][4] and [C][6] states and the
    generator as they were (sentinel-filled buffers, HIP-event launch count, generator read back)."""
    EINVAL = -1
    lib = L.load_library()
    M = 67
    codes = S.small_set(M, S.kind(dec))
    llr = torch.from_numpy(S.ladder_llr(codes[0], M, 7)).cuda()
    B = llr.shape[0]
    st, pos = L.mt19937_state(9, 4 * M)
    words = np.ascontiguousarray(st, dtype=np.uint32)
    with L.LdpcHipCodes(dec, codes, M, tier="global") as cs:
        cs.mt_set_state(st, pos)
        cs.profile(True)
        hard = torch.full((3, B, cs.hard_words), -1, dtype=torch.int32, device="cuda")
        iters = torch.full((3, B), -99, dtype=torch.int32, device="cuda")
        soft = torch.full((3, B, cs.N), -7.0, dtype=torch.float64, device="cuda")

        def decode(llr_ptr=llr.data_ptr(), frames=B, maxiter=S.MAXITER):
            return lib.ldpc_hip_decode_codes_dev(cs.h, llr_ptr, 1, frames, maxiter, 0.8, hard.data_ptr(), iters.data_ptr(), soft.data_ptr(), None)

        assert decode(maxiter=0) == EINVAL and lib.ldpc_hip_last_error().decode() == "ldpc_hip_decode_codes_dev: maxiter must be >= 1 (got 0)"
        assert decode(llr_ptr=None) == EINVAL and decode(frames=-1) == EINVAL
        torch.cuda.synchronize()
        assert (hard.cpu().numpy() == -1).all() and (iters.cpu().numpy() == -99).all() and (soft.cpu().numpy() == -7.0).all()
        cnt = np.full((3, 5), 5, dtype=np.uint64)
        info = np.full((3, 8), -99, dtype=np.int32)
        assert lib.ldpc_hip_simulate_codes(cs.h, 2.0, 0, 0, 0.8, 1, 0, 8, cnt.ctypes.data, info.ctypes.data) == EINVAL
        assert lib.ldpc_hip_simulate_codes(cs.h, 2.0, 8, S.MAXITER, 0.8, 1, 0, 8, cnt.ctypes.data, info.ctypes.data) == EINVAL
        assert lib.ldpc_hip_simulate_codes(cs.h, 2.0, 0, S.MAXITER, 0.8, 1, -1, 8, cnt.ctypes.data, info.ctypes.data) == EINVAL
        assert lib.ldpc_hip_simulate_codes(cs.h, 2.0, 0, S.MAXITER, 0.8, 1, 0, 8, None, info.ctypes.data) == EINVAL
        assert lib.ldpc_hip_frames_codes_host(cs.h, None, 8, S.MAXITER, 0.8, cnt.ctypes.data, info.ctypes.data, None) == EINVAL
        assert lib.ldpc_hip_mt_simulate_codes(cs.h, 2.0, 0, 0, 0.8, 8, cnt.ctypes.data, info.ctypes.data, None) == EINVAL
        assert lib.ldpc_hip_mt_simulate_codes(cs.h, 2.0, -1, S.MAXITER, 0.8, 8, cnt.ctypes.data, info.ctypes.data, None) == EINVAL
        assert (cnt == 5).all() and (info == -99).all()
        state4 = np.full((3, 4), 5, dtype=np.uint64)
        state6 = np.full((3, 6), 5, dtype=np.uint64)

        def stop(maxiter=S.MAXITER, first_batch=64, max_batch=64, punct=0, first_frame=0):
            return lib.ldpc_hip_simulate_codes_stop(cs.h, 2.0, punct, maxiter, 0.8, 1, first_frame, 7, 100, 0.05, first_batch, max_batch, state4.ctypes.data)

        def mt_stop(maxiter=S.MAXITER, first_batch=64, max_batch=64, punct=0):
            return lib.ldpc_hip_mt_simulate_codes_stop(cs.h, 2.0, punct, maxiter, 0.8, 7, 100, 0.05, first_batch, max_batch, state6.ctypes.data)

        assert stop(maxiter=0) == EINVAL and stop(first_batch=0) == EINVAL and stop(first_batch=65) == EINVAL and stop(punct=8) == EINVAL
        assert stop(first_frame=-1) == EINVAL
        assert mt_stop(maxiter=0) == EINVAL and mt_stop(first_batch=0) == EINVAL and mt_stop(first_batch=65) == EINVAL and mt_stop(punct=8) == EINVAL
        assert (state4 == 5).all() and (state6 == 5).all()
        assert lib.ldpc_hip_mt_advance_codes(cs.h, 2.0, 0, -1) == EINVAL and lib.ldpc_hip_mt_advance_codes(cs.h, 2.0, 8, 1) == EINVAL
        assert cs.profile_read()[1] == 0, "a refused call launches nothing"
        back = cs.mt_get_state()
        assert np.array_equal(back[0], words) and back[1] == pos, "the generator is where it was"
        # the single-code entry points stay closed to the set, and the context still works
        assert lib.ldpc_hip_decode_dev(cs.h, llr.data_ptr(), B, S.MAXITER, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        assert stop() == 0 and state4[0, 0] > 0 and mt_stop() == 0 and state6[0, 0] > 0 and decode() == 0
        torch.cuda.synchronize()
        assert (iters.cpu().numpy() != -99).all()


# ---- the layers above: ldpc::bp_simulation_codes(_exact) and ldpc_sim --code-sets on 2 x 4 codes at M = 513 ---------------------------
def test_cpp_layer_at_m513(L, torch, tmp_path):
    """open_code_set sends a lifting above 512 to ldpc_hip_open_codes_global.  bp_simulation_codes through the driver of
    test_gpu_codeset.py (its rows per code equal those of bp_simulation_throughput_t on that matrix alone); bp_simulation_codes_exact
    through the compat library against the sequential CPU oracle."""
    from test_gpu_codeset_exact import SEED, oracle_run
    L.load_library()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = str(tmp_path / "codes_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "codes_driver.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_compat", "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    M, codes = 513, S.beyond_set(513)
    snr, nfe, nexp, ref_fer, batch = 3.0, 8, 400, 1.0, 64
    for dec in (S.MS_DEC, S.TASP_DEC):
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(np.array([2, 2, 4, M, dec, S.MAXITER, nfe, nexp, batch, 9], dtype=np.int32).tobytes())
            f.write(np.array([snr, ref_fer], dtype=np.float64).tobytes())
            f.write(codes.tobytes())
        out = subprocess.check_output([exe, str(tmp_path / "in.bin")], env=dict(os.environ, LDPC_HIP_JIT="0"), timeout=120).decode().split("\n")
        rows = {(w[0], int(w[1])): w[2:] for w in (line.split() for line in out if line)}
        assert len(rows) == 4, out
        for c in range(2):
            assert rows["set", c] == rows["one", c], (dec, c, rows["set", c], rows["one", c])
            assert 0 < int(rows["set", c][4]) <= nexp + 1
    compat = C.CDLL(os.path.join(ROOT, "ldpc-lib_amd", "libldpc_compat.so"))
    compat.ldpc_bp_simulation_codes_exact.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                                      C.c_int, C.c_int, C.c_uint, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]
    flat = np.ascontiguousarray(codes, dtype=np.int32)
    for dec in (S.MS_DEC, S.TASP_DEC):
        out = np.zeros((2, 7), dtype=np.float64)
        nxt = C.c_uint()
        assert compat.ldpc_bp_simulation_codes_exact(2, 2, 4, flat.ctypes.data, M, S.MAXITER, nfe, nexp, snr, ref_fer, dec, 0, 0, SEED, 0, 64, 256, -1,
                                                     out.ctypes.data, C.addressof(nxt)) == 0
        for c, H in enumerate(codes):
            cnt, ber, fer, _ = oracle_run(H, M, dec, snr, nfe, nexp, ref_fer, maxiter=S.MAXITER)
            assert [int(out[c, 5]), int(out[c, 2]), int(out[c, 3]), int(out[c, 4]), int(out[c, 6])] == cnt, (dec, c, out[c].tolist(), cnt)
            assert out[c, 0] == ber and out[c, 1] == fer and cnt[2] > 0
        assert nxt.value == oracle_run(codes[-1], M, dec, snr, nfe, nexp, ref_fer, maxiter=S.MAXITER)[3]


def test_ldpc_sim_code_sets_at_m513(L, torch, tmp_path):
    """An M = 513 scenario with and without --code-sets: set_takes answers for the route open_code_set takes, the group is scored as one
    set, and the result file differs in `time` only."""
    from test_gpu_codeset_exact import code_record
    codes = S.beyond_set(513)
    records = [code_record(H, S.MS_DEC, 513, (2.0, 4.0)) for H in codes]
    scenario = tmp_path / "scenario.jsonx"
    scenario.write_text("""{
  settings = {
    random_seed = 3
    num_codewords = 200
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
    assert "set of 2 codes" in sets.stdout and "set of" not in plain.stdout

    def without_time(path):
        text = path.read_text()
        assert len(re.findall(r"\btime = \S+", text)) == 2
        return re.sub(r"\btime = \S+", "time = -", text)

    assert without_time(tmp_path / "plain.jsonx") == without_time(tmp_path / "sets.jsonx")
    fer = subprocess.check_output([exe, "jsonx-get", str(tmp_path / "sets.jsonx"), "results/0/simulation_logs/0/FER"], text=True)
    assert any(float(x) > 0 for x in fer.replace("array {", "").replace("}", "").split()), "error-free points compare nothing"
