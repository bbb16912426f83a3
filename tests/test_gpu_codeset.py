"""Code sets on the GPU: C codes of one shape x B frames in one launch (LdpcHipCodes / ldpc_hip_*_codes*), bit for bit against the CPU
oracle and against a single-code LdpcHip context per matrix: every lifting regime of the two kernels, both LLR layouts, code
boundaries inside the grid, alpha, the shared-noise simulation and its split invariance, the C++ stopping-rule harness, refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ldpc_testlib import (LMS_DEC, MS_DEC, ROOT, Oracle, _as_double_p, assert_bits_equal, awgn_llr, load_base_matrix, pack_bits, random_qc_code,
                          relift)

pytestmark = pytest.mark.gpu

EINVAL = -1
MAXITER = 20
NCODES, NFRAMES = 5, 7
# (M, rh, nh): smallest lifting; F = 12; F = 3 (64 not divisible); F = 2; F = 1; two waves with a partial last one; the Appendix-C base;
# eight waves
CASES = [(1, 4, 8), (5, 4, 8), (20, 4, 8), (32, 4, 8), (64, 4, 8), (100, 3, 6), (126, 16, 32), (512, 2, 4)]


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
    """The single-code contexts of this file open without hiprtc (one compile per matrix would take a second each): they run the
    table-driven and ahead-of-time kernels, whose bits are those of every other tier."""
    lib = L.load_library()
    before = lib.ldpc_hip_set_jit_mode(0)
    yield
    lib.ldpc_hip_set_jit_mode(before)


def _fix_columns(rng, H, M, keep_row):
    """Give every empty block column a circulant in a row other than keep_row."""
    rh = H.shape[0]
    for k in np.flatnonzero((H >= 0).sum(axis=0) == 0):
        j = (keep_row + 1 + rng.randint(0, rh - 1)) % rh
        H[j, k] = rng.randint(0, M)


def _thin(rng, H, count, keep_row=-1):
    """Remove up to `count` circulants outside keep_row, keeping two in every block row and one in every block column."""
    for _ in range(count):
        free = [(j, k) for j, k in zip(*np.nonzero(H >= 0)) if j != keep_row and (H[j] >= 0).sum() > 2 and (H[:, k] >= 0).sum() > 1]
        if free:
            H[free[rng.randint(len(free))]] = -1


def _code_set_differs(codes, nh):
    masks = {(H >= 0).tobytes() for H in codes}
    row_weights = {tuple((H >= 0).sum(axis=1)) for H in codes}
    edges = {int((H >= 0).sum()) for H in codes}
    for H in codes:   # what ldpc_hip_open_codes takes: no empty block row or column, row weights up to 16
        if not (((H >= 0).sum(axis=0) > 0).all() and ((H >= 0).sum(axis=1) > 0).all() and (H >= 0).sum(axis=1).max() <= 16):
            return False
    return (len(masks) == len(codes) and len(row_weights) == len(codes) and len(edges) >= 3 and 2 in (codes[1] >= 0).sum(axis=1) and
            min(8, nh) in (codes[2] >= 0).sum(axis=1))


def make_code_set(seed, rh, nh, M, ncodes=NCODES):
    """ncodes protographs of one shape that differ pairwise in their empty blocks and row weights and have at least three different
    edge counts.  Code 1 has a block row of weight 2 and code 2 one of weight min(8, nh); for 16 x 32 code 0 is the Appendix-C base
    matrix.  Deterministic: the first of the seeds seed, seed + 1000, ... whose draw has these properties."""
    for attempt in range(100):
        codes = _draw_code_set(np.random.RandomState(seed + 1000 * attempt), rh, nh, M, ncodes)
        if _code_set_differs(codes, nh):
            return codes
    raise AssertionError("no code set with the required differences")


def _draw_code_set(rng, rh, nh, M, ncodes):
    info_weights = ([3], [2, 3], [min(rh, 5)], [2], [3, 1, 2])
    codes = []
    for i in range(ncodes):
        if i == 0 and (rh, nh) == (16, 32):
            H = relift(load_base_matrix(), M)
        else:
            H = relift(random_qc_code(rng, rh, nh, 512, info_weights[i % len(info_weights)]), M)
        H = np.where(H >= 0, H % M, -1).astype(np.int16)
        if i == 1:                          # a weight-2 row
            j = rh - 1
            H[j, np.flatnonzero(H[j] >= 0)[2:]] = -1
            _fix_columns(rng, H, M, j)
        elif i == 2:                        # a weight-8 row (the full row where nh < 8)
            j, want = 0, min(8, nh)
            while (H[j] >= 0).sum() < want:
                H[j, rng.choice(np.flatnonzero(H[j] < 0))] = rng.randint(0, M)
            while (H[j] >= 0).sum() > want:
                H[j, rng.choice(np.flatnonzero(H[j, rh:] >= 0) + rh)] = -1
            _fix_columns(rng, H, M, j)
            _thin(rng, H, rng.randint(0, rh), keep_row=j)
        elif i > 2:
            _thin(rng, H, rng.randint(1, 2 * rh))
        codes.append(H)
    return np.array(codes, dtype=np.int16)


def oracle_decode(H, M, dec, llr, maxiter, alpha=0.8):
    """(hard decword [B, N], iters [B], soft [B, N]) of the CPU oracle; alpha only matters to MS_DEC."""
    o = Oracle(H, M)
    llr = np.ascontiguousarray(llr, dtype=np.float64)
    out = []
    for decision in (0, 1):
        d = np.empty_like(llr)
        it = np.empty(len(llr), dtype=np.int32)
        for b in range(len(llr)):
            y = llr[b].copy()
            if dec == MS_DEC:
                it[b] = o.lib.orc_min_sum(o.h, _as_double_p(y), _as_double_p(d[b]), maxiter, decision, alpha)
            else:
                it[b] = o.lib.orc_lmin_sum(o.h, _as_double_p(y), _as_double_p(d[b]), maxiter, decision)
        out.append((d, it))
    o.close()
    assert np.array_equal(out[0][1], out[1][1])
    return out[0][0], out[0][1], out[1][0]


_REF = {}
SNR_LADDER = (2.0, 1.0, 3.0, 0.0, 4.0, -1.0, 5.0, -2.0, 6.0, 1.5, 2.5, 0.5, 3.5)


def reference(case):
    """Per case, computed once on the CPU: the code set, the shared [B, N] and per-code [C, B, N] LLRs at an SNR at which -- for both
    decoders and both layouts -- the oracle converges on some (c, f) and does not on others, and the oracle's results."""
    if case in _REF:
        return _REF[case]
    M, rh, nh = case
    codes = make_code_set(100 + M, rh, nh, M)
    H0 = codes[0].astype(np.int32)
    for snr in SNR_LADDER:
        shared = awgn_llr(H0, M, snr, 300 + M, NFRAMES, burn_codeword=False)
        percode = awgn_llr(H0, M, snr, 400 + M, NCODES * NFRAMES, burn_codeword=False).reshape(NCODES, NFRAMES, -1)
        ref, mixed = {}, True
        for dec in (MS_DEC, LMS_DEC):
            for layout, llr in (("shared", None), ("percode", percode)):
                res = [oracle_decode(codes[c], M, dec, shared if llr is None else llr[c], MAXITER) for c in range(NCODES)]
                its = np.array([r[1] for r in res])
                mixed = mixed and (its > 0).any() and (its < 0).any()
                ref[dec, layout] = res
        if mixed:
            break
    _REF[case] = dict(codes=codes, snr=snr, shared=shared, percode=percode, ref=ref)
    return _REF[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "M%d_%dx%d" % c)
def test_code_sets_differ_as_required(case):
    M, rh, nh = case
    assert _code_set_differs(reference(case)["codes"], nh)


@pytest.mark.parametrize("layout", ["shared", "percode"])
@pytest.mark.parametrize("dec", [MS_DEC, LMS_DEC], ids=["ms", "lms"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "M%d_%dx%d" % c)
def test_parity(L, torch, case, dec, layout):
    M, rh, nh = case
    r = reference(case)
    codes, ref = r["codes"], r["ref"][dec, layout]
    its_ref = np.array([x[1] for x in ref])
    assert (its_ref > 0).any() and (its_ref < 0).any(), ("the oracle must converge on some frames and not on others", r["snr"], its_ref)
    llr = r["shared"] if layout == "shared" else r["percode"]
    x = torch.from_numpy(np.ascontiguousarray(llr)).cuda()
    with L.LdpcHipCodes(dec, codes, M) as cs:
        assert cs.C == NCODES and cs.lib.ldpc_hip_codes(cs.h) == NCODES
        assert cs.kernel_name == ("ms_flood_codes_kernel" if dec == MS_DEC else "lms_layered_codes_kernel") + ("<multiwave>" if M > 64 else "")
        hard, iters, soft = cs.decode(x, MAXITER, shared=layout == "shared", want_soft=True)
        torch.cuda.synchronize()
    hard, iters, soft = hard.cpu().numpy().view(np.uint32), iters.cpu().numpy(), soft.cpu().numpy()
    assert_bits_equal(x.cpu().numpy(), llr, "the input is not modified")
    for c in range(NCODES):
        d_ref, it_ref, s_ref = ref[c]
        assert np.array_equal(iters[c], it_ref), (c, iters[c], it_ref)
        assert np.array_equal(hard[c], pack_bits(d_ref)), c
        assert_bits_equal(soft[c], s_ref, f"soft values of code {c}")
        with L.LdpcHip(dec, codes[c], M) as one:   # and the single-code context on the same matrix
            xc = x if layout == "shared" else x[c]
            h1, i1, s1 = one.decode(xc, MAXITER, want_soft=True)
            torch.cuda.synchronize()
        assert np.array_equal(iters[c], i1.cpu().numpy()) and np.array_equal(hard[c], h1.cpu().numpy().view(np.uint32)), c
        assert_bits_equal(soft[c], s1.cpu().numpy(), f"soft values of code {c} against LdpcHip")


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("dec", [MS_DEC, LMS_DEC], ids=["ms", "lms"])
def test_code_boundaries(L, torch, dec, B):
    """M = 20 packs three frames into a wave.  Code 1 sees strongly positive LLRs and converges at once, its neighbours in the grid
    (codes 0 and 2, noisy frames) do not: no frame's result depends on the other frames of its wave or on the next code's."""
    M = 20
    codes = make_code_set(7, 4, 8, M, ncodes=3)
    H0 = codes[0].astype(np.int32)
    llr = awgn_llr(H0, M, -3.0, 55, 3 * B, burn_codeword=False).reshape(3, B, -1)
    llr[1] = 30.0 + np.arange(B * 8 * M).reshape(B, -1) % 7
    ref = [oracle_decode(codes[c], M, dec, llr[c], MAXITER) for c in range(3)]
    assert (ref[1][1] == 1).all() and (ref[0][1] < 0).all() and (ref[2][1] < 0).all(), [r[1] for r in ref]
    with L.LdpcHipCodes(dec, codes, M) as cs:
        hard, iters, soft = cs.decode(torch.from_numpy(llr).cuda(), MAXITER, shared=False, want_soft=True)
        torch.cuda.synchronize()
    for c in range(3):
        assert np.array_equal(iters[c].cpu().numpy(), ref[c][1]), c
        assert np.array_equal(hard[c].cpu().numpy().view(np.uint32), pack_bits(ref[c][0])), c
        assert_bits_equal(soft[c].cpu().numpy(), ref[c][2], f"code {c}")


def test_alpha_is_honoured(L, torch):
    case = (32, 4, 8)
    r = reference(case)
    codes, llr = r["codes"], r["shared"]
    ref = [oracle_decode(codes[c], 32, MS_DEC, llr, MAXITER, alpha=0.75) for c in range(NCODES)]
    assert any(not np.array_equal(ref[c][2], r["ref"][MS_DEC, "shared"][c][2]) for c in range(NCODES)), "alpha must matter on this set"
    with L.LdpcHipCodes(MS_DEC, codes, 32) as cs:
        hard, iters, soft = cs.decode(torch.from_numpy(llr).cuda(), MAXITER, alpha=0.75, want_soft=True)
        torch.cuda.synchronize()
    for c in range(NCODES):
        assert np.array_equal(iters[c].cpu().numpy(), ref[c][1])
        assert np.array_equal(hard[c].cpu().numpy().view(np.uint32), pack_bits(ref[c][0]))
        assert_bits_equal(soft[c].cpu().numpy(), ref[c][2])


@pytest.mark.parametrize("alpha", [-0.8, -0.0, 0.0])
def test_alpha_that_is_not_above_zero_is_refused(L, torch, alpha):
    """Upstream's c2v value is sign ? -(m * alpha) : m * alpha (decoders.cpp:4719-4720) and its soft value y + acc * alpha is -0.0 where
    y is and the product is too (a negative factor and acc = +0.0, a zero factor and acc < 0).  ms_flood_codes_kernel keeps the
    product's sign (ms_row_scan) but starts from y + 0.0, so it returns +0.0 there.  Upstream's bits or an error: this route refuses
    (the set kernels of the global tier take any alpha, test_gpu_codeset_global.py).  The refusal names alpha, comes from every entry
    that decodes, and leaves the context as it was."""
    case = (32, 4, 8)
    r = reference(case)
    codes, llr = r["codes"], r["shared"]
    with L.LdpcHipCodes(MS_DEC, codes, 32) as cs:
        assert cs.kernel_name == "ms_flood_codes_kernel", cs.kernel_name
        with pytest.raises(L.LdpcHipError, match="alpha = -?0.* is not above zero"):
            cs.decode(torch.from_numpy(llr).cuda(), MAXITER, alpha=alpha, want_soft=True)
        with pytest.raises(L.LdpcHipError, match="alpha = -?0.* is not above zero"):
            cs.simulate(2.0, MAXITER, 5, 0, 8, alpha=alpha)
        hard, iters, soft = cs.decode(torch.from_numpy(llr).cuda(), MAXITER, want_soft=True)
        torch.cuda.synchronize()
    ref = r["ref"][MS_DEC, "shared"]
    for c in range(NCODES):
        assert np.array_equal(iters[c].cpu().numpy(), ref[c][1])
        assert_bits_equal(soft[c].cpu().numpy(), ref[c][2])


@pytest.mark.parametrize("punct", [0, 1])
@pytest.mark.parametrize("dec", [MS_DEC, LMS_DEC], ids=["ms", "lms"])
def test_simulate(L, torch, dec, punct, monkeypatch):
    """simulate_codes = C single-code simulations over the same noise: counters and ordered records, however the frames are split."""
    M, Cn, B, first, snr, seed = 32, 4, 300, 1000, 1.5, 77
    codes = make_code_set(11, 4, 8, M, ncodes=Cn)
    with L.LdpcHipCodes(dec, codes, M) as cs:
        cnt, info = cs.simulate(snr, MAXITER, seed, first, B, punctured_blocks=punct, records=True)
        a = cs.simulate(snr, MAXITER, seed, first, 150, punctured_blocks=punct, records=True)
        b = cs.simulate(snr, MAXITER, seed, first + 150, 150, punctured_blocks=punct, records=True)
        monkeypatch.setenv("LDPC_HIP_CODES_PIECE", "64")      # and in pieces of 64 frames inside one call
        c = cs.simulate(snr, MAXITER, seed, first, B, punctured_blocks=punct, records=True)
        monkeypatch.delenv("LDPC_HIP_CODES_PIECE")
        only = cs.simulate(snr, MAXITER, seed, first, B, punctured_blocks=punct)
        # the device entry points on the same frames
        one0 = L.LdpcHip(dec, codes[0], M)
        x = one0.awgn_llr(snr, seed, first, B, punctured_blocks=punct)
        hard, iters, _ = cs.decode(x, MAXITER)
        dcnt, dinfo = cs.count_errors(hard, iters, want_frame_info=True)
        dcnt, _ = cs.count_errors(hard, iters, counters=dcnt)   # accumulates
        torch.cuda.synchronize()
        one0.close()
    assert np.array_equal(a[0] + b[0], cnt) and np.array_equal(np.concatenate([a[1], b[1]], axis=1), info)
    assert np.array_equal(c[0], cnt) and np.array_equal(c[1], info) and np.array_equal(only, cnt)
    assert np.array_equal(dcnt.cpu().numpy().astype(np.uint64), 2 * cnt) and np.array_equal(dinfo.cpu().numpy(), info)
    assert (cnt[:, 3] == B).all() and 0 < cnt[:, 1].sum() < Cn * B, cnt
    for q in range(Cn):
        with L.LdpcHip(dec, codes[q], M) as one:
            s = one.simulate(snr, MAXITER, seed, first, B, punctured_blocks=punct)
            x = one.awgn_llr(snr, seed, first, B, punctured_blocks=punct)
            h1, i1, _ = one.decode(x, MAXITER)
            _, inf1 = one.count_errors(h1, i1, want_frame_info=True, first_frame=first)
            torch.cuda.synchronize()
        assert [s["nse"], s["nde"], s["nue"], s["frames"], s["sum_abs_iters"]] == cnt[q].tolist(), q
        assert np.array_equal(inf1.cpu().numpy(), info[q]), q


def test_stopping_rule_from_cpp(L, torch, tmp_path):
    """ldpc::bp_simulation_codes on three codes of very different strength = three ldpc::bp_simulation_throughput_t calls with the
    same seed; batches of 64 frames, so the codes stop in different batches."""
    L.load_library()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = str(tmp_path / "codes_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "codes_driver.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_compat", "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    M, rh, nh, batch = 32, 4, 8, 64
    rng = np.random.RandomState(5)
    strong = random_qc_code(rng, rh, nh, M, [3])
    medium = random_qc_code(rng, rh, nh, M, [2])
    weak = -np.ones((rh, nh), dtype=np.int16)     # every block column of weight 1: no coding gain at all
    for k in range(nh):
        weak[k % rh, k] = k % M
    codes = np.array([medium, weak, strong], dtype=np.int16)
    for dec, nfe, nexp, snr, ref_fer in ((MS_DEC, 12, 1500, 4.0, 0.05), (LMS_DEC, 6, 1500, 4.0, 1.0)):
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(np.array([3, rh, nh, M, dec, MAXITER, nfe, nexp, batch, 9], dtype=np.int32).tobytes())
            f.write(np.array([snr, ref_fer], dtype=np.float64).tobytes())
            f.write(codes.tobytes())
        out = subprocess.check_output([exe, str(tmp_path / "in.bin")], env=dict(os.environ, LDPC_HIP_JIT="0"), timeout=120).decode().split("\n")
        rows = {(w[0], int(w[1])): w[2:] for w in (line.split() for line in out if line)}
        assert len(rows) == 6, out
        stop_batch = set()
        for c in range(3):
            assert rows["set", c] == rows["one", c], (dec, c, rows["set", c], rows["one", c])
            experiment = int(rows["set", c][4])
            assert 0 < experiment <= nexp + 1
            stop_batch.add((experiment - 1) // batch)
        assert len(stop_batch) == 3, (dec, rows)


def test_refusals_and_cross_use(L, torch):
    lib = L.load_library()
    ok = make_code_set(3, 4, 8, 20, ncodes=3)[:2]

    def open_rc(dec, codes, M, Cn=None):
        codes = np.ascontiguousarray(codes, dtype=np.int16)
        h = C.c_void_p()
        rc = lib.ldpc_hip_open_codes(dec, codes.shape[1], codes.shape[2], M, codes.ctypes.data, codes.shape[0] if Cn is None else Cn, 0, C.byref(h))
        assert (rc == 0) == bool(h.value)
        if h.value:
            lib.ldpc_hip_close(h)
        return rc

    assert open_rc(MS_DEC, ok, 20) == 0
    for dec in (0, 1, 2, 4, 5, 6, 7, 9):
        assert open_rc(dec, ok, 20) == EINVAL
    assert open_rc(MS_DEC, ok, 20, Cn=0) == EINVAL and open_rc(MS_DEC, ok, 20, Cn=-1) == EINVAL
    assert open_rc(LMS_DEC, np.zeros((1, 2, 4)), 513) == EINVAL
    assert open_rc(LMS_DEC, np.zeros((1, 65, 66)), 2) == EINVAL
    assert open_rc(MS_DEC, np.zeros((1, 2, 17)), 2) == EINVAL
    bad = ok.copy(); bad[1, 2, :] = -1
    assert open_rc(MS_DEC, bad, 20) == EINVAL
    bad = ok.copy(); bad[0, :, 5] = -1
    assert open_rc(MS_DEC, bad, 20) == EINVAL
    for v in (20, -2):
        bad = ok.copy(); bad[1, 0, 0] = v
        assert open_rc(LMS_DEC, bad, 20) == EINVAL
    assert "outside" in lib.ldpc_hip_last_error().decode()

    B, N, W = 4, 8 * 20, 5
    x = torch.ones((2, B, N), dtype=torch.float64, device="cuda")
    hard = torch.full((2, B, W), 0x55, dtype=torch.int32, device="cuda")
    iters = torch.full((2, B), -77, dtype=torch.int32, device="cuda")
    cnt = (C.c_ulonglong * 10)()

    def untouched():
        torch.cuda.synchronize()
        return bool((hard == 0x55).all()) and bool((iters == -77).all())

    with L.LdpcHipCodes(MS_DEC, ok, 20) as cs, L.LdpcHip(MS_DEC, ok[0], 20) as one, \
            L.LdpcHipGfq(4, np.where(ok[0] >= 0, ok[0] % 8, -1), np.where(ok[0] >= 0, 1 + ok[0] % 15, -1), 8) as gf:
        for maxiter in (0, -5):
            assert lib.ldpc_hip_decode_codes_dev(cs.h, x.data_ptr(), 0, B, maxiter, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
            assert lib.ldpc_hip_simulate_codes(cs.h, 2.0, 0, maxiter, 0.8, 1, 0, B, cnt, None) == EINVAL
        assert lib.ldpc_hip_simulate_codes(cs.h, 2.0, 8, 10, 0.8, 1, 0, B, cnt, None) == EINVAL          # punctured_blocks >= nh
        # the single-code, multi-device and GF(q) entry points on a code-set context
        assert lib.ldpc_hip_decode_dev(cs.h, x.data_ptr(), B, 10, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_count_errors_dev(cs.h, hard.data_ptr(), iters.data_ptr(), B, None, x.data_ptr(), None) == EINVAL
        c4, sit = (C.c_ulonglong * 4)(), C.c_ulonglong()
        assert lib.ldpc_hip_simulate(cs.h, 2.0, 0, 0, 10, 0.8, 1, 0, B, c4, C.byref(sit)) == EINVAL
        assert lib.ldpc_hip_awgn_llr_dev(cs.h, 2.0, 0, 0, 1, 0, B, x.data_ptr(), None) == EINVAL
        assert lib.ldpc_hip_decode_gfq_dev(cs.h, x.data_ptr(), B, 10, 0.0, None, iters.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_gfq_q(cs.h) == 0 and lib.ldpc_hip_codes(one.h) == 0 and lib.ldpc_hip_codes(gf.h) == 0
        # the code-set entry points on a binary and on a GF(q) context
        for h in (one.h, gf.h):
            assert lib.ldpc_hip_decode_codes_dev(h, x.data_ptr(), 1, B, 10, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
            assert lib.ldpc_hip_count_errors_codes_dev(h, hard.data_ptr(), iters.data_ptr(), B, None, x.data_ptr(), None) == EINVAL
            assert lib.ldpc_hip_simulate_codes(h, 2.0, 0, 10, 0.8, 1, 0, B, cnt, None) == EINVAL
        assert untouched(), "a refused call must not launch anything"
        assert bool((x == 1.0).all())
        # and the context still works
        h2, i2, _ = cs.decode(x, 10, shared=False)
        torch.cuda.synchronize()
        assert bool((i2 == 1).all()) and bool((h2 == 0).all())
