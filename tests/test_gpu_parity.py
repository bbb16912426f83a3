"""GPU parity tests (run with -m gpu on an MI355X).  Everything goes through the C-ABI library (libldpc_hip.so);
the oracle (oracle/) is only the checker."""
import glob
import os

import numpy as np
import pytest

from ldpc_testlib import (ASP_DEC, BP_DEC, GOLDEN_DIR, IMS_DEC, LMS_DEC, MS_DEC, SP_DEC, TASP_DEC, Oracle, assert_bits_equal, awgn_llr, bpsk_sigma, load_base_matrix, pack_bits,
                          philox_gauss_pairs, relift, syndrome_np, unpack_bits)

pytestmark = pytest.mark.gpu

DECODER_SETS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz"))
                      if os.path.basename(p).split("_")[0] in ("ms", "lms", "sp", "ims", "tasp", "asp", "bp"))

# Sum-product family and Gallager BP: their transcendentals -- exp() of the channel LLRs for SP / ASP / TDMP, 2 exp + 2 log per edge
# and iteration for BP -- are evaluated on the device with glibc's own algorithms (ldpc_spec::exp_glibc / log_glibc, the FMA build
# x86-64 hosts select at run time); every other operation is IEEE-exact and in the reference's order.  So these decoders are held
# to the same bar as min-sum: hard decisions, iteration counts and a-posteriori values bit for bit (tolerance 0) against the
# goldens of the compiled reference and against the live oracle.  The live oracle runs on THIS host's libm: on a host without FMA
# glibc selects its other exp / log build, which differs in the last ulp, and the soft-value comparisons then allow a few ulps
# (the golden vectors were produced on an FMA host).  Hard decisions and iteration counts are compared exactly everywhere.
_HOST_HAS_FMA = " fma" in open("/proc/cpuinfo").read()
SP_RTOL = 0.0 if _HOST_HAS_FMA else 4e-15
TASP_RTOL = 0.0 if _HOST_HAS_FMA else 4e-15
BP_RTOL, BP_ATOL = (0.0, 0.0) if _HOST_HAS_FMA else (1e-12, 1e-14)


def _close(got, want, rtol, atol=0.0, what=""):
    """Tolerance 0 (an FMA host) means bit for bit, the sign of zero included; otherwise the stated non-FMA tolerance."""
    if rtol == 0 and atol == 0:
        assert_bits_equal(got, want, what)
    else:
        np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=what)


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.mark.parametrize("name", DECODER_SETS)
def test_golden_vectors_host_api(L, name):
    g = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    H, M, dec_id, maxiter = g["H"], int(g["M"]), int(g["dec_id"]), int(g["maxiter"])
    alpha = float(g["alpha"]) if "alpha" in g else 0.8   # the min-sum sets recorded at another factor carry it
    with L.LdpcHip(dec_id, H, M) as dec:
        d0, it0, after = dec.decode_host(g["llr"], maxiter, decision=0, alpha=alpha)
        assert np.array_equal(it0, g["iters"]), (it0, g["iters"])
        assert np.array_equal(pack_bits(d0), g["hard"])
        ns = g["soft"].shape[0]
        d1, it1, _ = dec.decode_host(g["llr"][:ns], maxiter, decision=1, alpha=alpha)
        assert np.array_equal(it1, g["iters"][:ns])
        if dec_id == SP_DEC:
            _close(d1, g["soft"], SP_RTOL)
        elif dec_id == BP_DEC:
            _close(d1, g["soft"], BP_RTOL, BP_ATOL)   # a-posteriori LLRs
        elif dec_id == ASP_DEC:
            _close(d1, g["soft"], TASP_RTOL)   # a-posteriori P(bit=1)
            x = np.clip(g["llr"] * 0.5, -20.0, 20.0)  # the input is left holding the channel P(bit=1) (decoders.cpp:2351-2358)
            np.testing.assert_allclose(after, np.exp(-x) / (np.exp(x) + np.exp(-x)), rtol=1e-14)
        elif dec_id == TASP_DEC:
            assert_bits_equal(d1, g["soft"])    # `decision` is dead upstream: still the hard decisions
            x = np.clip(g["llr"] * 0.5, -20.0, 20.0)  # and the input is left holding P(bit=1) (decoders.cpp:2611-2618)
            np.testing.assert_allclose(after, np.exp(-x) / (np.exp(x) + np.exp(-x)), rtol=1e-14)
        else:
            assert_bits_equal(d1, g["soft"])  # bit-exact a-posteriori LLRs
            assert_bits_equal(after, g["llr"])  # MS/LMS leave their input intact


@pytest.mark.parametrize("dec_id,M,snrs,frames,maxiter", [
    (MS_DEC, 64, (0.5, 1.2, 1.6, 2.0, 3.0), 160, 50),
    (MS_DEC, 64, (1.4,), 300, 7),
    (LMS_DEC, 64, (0.8, 1.2, 1.6, 2.5), 160, 50),
    (SP_DEC, 64, (1.0, 1.5, 2.0), 100, 50),
    (MS_DEC, 16, (2.5,), 203, 50),      # F = 4 frames per wave, ragged last wave
    (MS_DEC, 7, (3.0,), 100, 30),       # F = 9, 63 of 64 lanes used
    (LMS_DEC, 24, (2.5,), 77, 50),      # F = 2, lanes 48..63 idle
    (MS_DEC, 100, (1.8,), 24, 50),      # 2 waves per frame, 28 idle lanes
    (LMS_DEC, 200, (1.5,), 12, 50),     # 4 waves per frame
    (SP_DEC, 33, (2.0,), 40, 25),
    (IMS_DEC, 64, (1.0, 2.0, 3.0), 150, 50),   # int16 min-sum: exact by construction after the quantiser
    (IMS_DEC, 20, (3.0,), 100, 50),
    (IMS_DEC, 126, (2.0,), 24, 50),            # ahead-of-time int8 instance, 2 waves per frame, 2 idle lanes
    (IMS_DEC, 100, (1.5, 2.5), 30, 50),        # hiprtc int8 instance, 28 idle lanes
    (IMS_DEC, 256, (1.8,), 12, 50),            # hiprtc int8 instance, 4 waves per frame
    (IMS_DEC, 512, (1.8,), 6, 50),             # LDS would not hold the doubled arrays: table-driven kernel
    (TASP_DEC, 64, (1.0, 1.7, 2.5), 600, 15),   # TDMP sum-product, ahead-of-time instance
    (TASP_DEC, 126, (1.2, 1.7, 2.4), 400, 15),   # the shipped scenario's lifting: 4 waves per frame (two lanes per check), 4 idle lanes
    (TASP_DEC, 40, (2.5,), 60, 30),             # hiprtc instance, two waves, the second one a quarter full
    (TASP_DEC, 200, (1.6,), 24, 15),            # hiprtc instance, 7 waves per frame (two lanes per check)
    (ASP_DEC, 64, (1.0, 1.6, 2.2), 300, 30),    # probability-domain flooding sum-product (decoder 2), ahead-of-time instance
    (ASP_DEC, 128, (1.7,), 20, 25),             # hiprtc instance, two 64-lane chunks per block row/column
    (ASP_DEC, 126, (1.7,), 16, 25),             # the lifting of the shipped scenarios: last chunk 62 lanes
    (ASP_DEC, 20, (3.0,), 60, 30),              # one partly idle chunk
    (BP_DEC, 64, (1.0, 1.6, 2.2), 300, 30),     # Gallager BP (decoder 0), ahead-of-time instance; failed frames chain into successors
    (BP_DEC, 128, (1.7,), 20, 25),              # hiprtc instance
    (BP_DEC, 126, (1.4, 1.7), 24, 25),          # the lifting of the shipped scenarios; failed frames chain
    (BP_DEC, 9, (2.5,), 80, 30),
    (SP_DEC, 126, (1.2, 1.7), 120, 30),          # code-specialised sum-product for a lifting that is not a multiple of 64
])
def test_random_batches_against_oracle(L, torch, dec_id, M, snrs, frames, maxiter):
    H = relift(load_base_matrix(), M)
    llr = np.concatenate([awgn_llr(H, M, s, 100 + i, frames // len(snrs) + 1) for i, s in enumerate(snrs)])[:frames]
    o = Oracle(H, M)
    d_ref, it_ref, _ = o.decode(dec_id, llr, maxiter, 0)
    with L.LdpcHip(dec_id, H, M) as dec:
        x = torch.from_numpy(llr).cuda()
        hard, iters, soft = dec.decode(x, maxiter, want_soft=True)
        torch.cuda.synchronize()
        assert np.array_equal(iters.cpu().numpy(), it_ref)
        assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref))
        assert_bits_equal(x.cpu().numpy(), llr)  # the device entry point never modifies its input
        s_ref, _, _ = (Oracle(H, M) if dec_id == BP_DEC else o).decode(dec_id, llr, maxiter, 1)  # BP: state carries between calls
        if dec_id == BP_DEC:
            _close(soft.cpu().numpy(), s_ref, BP_RTOL, BP_ATOL)
        elif dec_id in (SP_DEC, ASP_DEC, TASP_DEC):  # exp() on the device vs glibc: a-posteriori values to the stated tolerance
            _close(soft.cpu().numpy(), s_ref, SP_RTOL if dec_id == SP_DEC else TASP_RTOL)
        else:
            assert_bits_equal(soft.cpu().numpy(), s_ref)


def test_edge_case_inputs(L, torch):
    """zeros, negative zeros, huge magnitudes (MAX_VAL clamp, decoders.cpp:4730), B = 0 / 1, ragged waves."""
    H = relift(load_base_matrix(), 64)
    N = 32 * 64
    rng = np.random.RandomState(5)
    llr = awgn_llr(H, 64, 1.5, 9, 12)
    llr[0] = 0.0
    llr[1] = -0.0
    llr[2] = np.where(rng.rand(N) < 0.5, -0.0, 0.0)
    llr[3] *= 1e6                                   # every |v2c| clamps to 32767
    llr[4, ::7] = 0.0
    llr[5, ::5] = -0.0
    llr[6] = np.abs(llr[6])                         # already a codeword
    llr[7] = 1e-310 * np.sign(llr[7])               # denormals
    o = Oracle(H, 64)
    for dec_id in (MS_DEC, LMS_DEC):
        d_ref, it_ref, _ = o.decode(dec_id, llr, 50, 0)
        with L.LdpcHip(dec_id, H, 64) as dec:
            d, it, _ = dec.decode_host(llr, 50)
            assert np.array_equal(it, it_ref), (dec_id, it, it_ref)
            assert np.array_equal(d, d_ref)
            d1, it1, _ = dec.decode_host(llr[3], 50)   # B = 1, 1-D input
            assert it1 == it_ref[3] and np.array_equal(d1, d_ref[3])
            e = torch.empty((0, N), dtype=torch.float64, device="cuda")
            hard, iters, _ = dec.decode(e, 50)
            assert hard.shape[0] == 0 and iters.shape[0] == 0
    # sum-product: already-a-codeword returns 0 (decoders.cpp:1989-2002), |LLR| > 20 clamps (INPUT_LIMIT)
    llr_sp = awgn_llr(H, 64, 2.0, 3, 4)
    llr_sp[0] = np.abs(llr_sp[0]) + 0.1
    llr_sp[1] *= 3.0                                # some |LLR| > 20: INPUT_LIMIT clamp without saturating the whole frame
    d_ref, it_ref, after_ref = o.decode(SP_DEC, llr_sp, 50, 0)
    with L.LdpcHip(SP_DEC, H, 64) as dec:
        d, it, after = dec.decode_host(llr_sp, 50)
        assert it_ref[0] == 0 and np.array_equal(it, it_ref)
        assert np.array_equal(d, d_ref)
        _close(after, after_ref, SP_RTOL)  # upstream clobbers soft[] with the ratios


def test_maxiter_one_and_unsupported_shapes(L):
    H = relift(load_base_matrix(), 64)
    llr = awgn_llr(H, 64, 1.0, 4, 8)
    o = Oracle(H, 64)
    for dec_id in (MS_DEC, LMS_DEC, SP_DEC):
        d_ref, it_ref, _ = o.decode(dec_id, llr, 1, 0)
        with L.LdpcHip(dec_id, H, 64) as dec:
            d, it, _ = dec.decode_host(llr, 1)
            assert np.array_equal(it, it_ref) and np.array_equal(d, d_ref)
    with L.LdpcHip(MS_DEC, H, 64) as dec, pytest.raises(L.LdpcHipError):
        dec.decode_host(llr, 0)  # maxiter < 1 is rejected, not guessed at
    with L.LdpcHip(ASP_DEC, relift(load_base_matrix(), 256), 256) as dec:
        assert "asp_global_kernel" in dec.kernel_name              # per-edge state would not fit the 160 KiB LDS: the shape-unlimited tier takes it
    with pytest.raises(L.LdpcHipError):
        L.LdpcHip(6, H, 64)  # FHT_DEC (GF(q)) is out of scope: fails loudly, no fallback
    with L.LdpcHip(MS_DEC, np.zeros((70, 140), dtype=np.int16), 64) as dec:   # more block rows than any resident kernel holds:
        assert "ms_global_kernel" in dec.kernel_name                            # the shape-unlimited tier takes it (tests/test_gpu_shapes.py)
    with L.LdpcHip(BP_DEC, np.zeros((70, 140), dtype=np.int16), 64) as dec:
        assert "bp_global_kernel" in dec.kernel_name


def test_full_size_properties(L, torch):
    """BASELINE config #2 size (65536 frames of the (2048,1024) code): size-independent properties."""
    H = relift(load_base_matrix(), 64)
    B, N = 65536, 2048
    with L.LdpcHip(MS_DEC, H, 64) as dec:
        llr = dec.awgn_llr(2.0, seed=7, first_frame=0, B=B)
        hard, iters, _ = dec.decode(llr, 50)
        torch.cuda.synchronize()
        it = iters.cpu().numpy()
        bits = unpack_bits(hard.cpu().numpy(), N)
        conv = it > 0
        assert 0.9 < conv.mean() < 1.0                       # FER ~4 % at 2.0 dB
        # 1. every frame reported as converged satisfies all parity checks; none of the others does
        fail = syndrome_np(H, 64, bits)
        assert not fail[conv].any() and fail[~conv].all()
        assert (it[~conv] == -50).all() and it[conv].max() <= 50 and it[conv].min() >= 1
        # 2. batch-split invariance: any sub-batch decodes to the same words
        h2, i2, _ = dec.decode(llr[1000:1777].contiguous(), 50)
        assert torch.equal(h2, hard[1000:1777]) and torch.equal(i2, iters[1000:1777])
        # 3. idempotence: a decoded codeword fed back as a confident LLR is returned unchanged in one iteration
        sel = np.flatnonzero(conv)[:4096]
        cw = torch.from_numpy(bits[sel].astype(np.float64)).cuda()
        h3, i3, _ = dec.decode((1.0 - 2.0 * cw) * 8.0, 50)
        assert (i3 == 1).all() and torch.equal(h3, hard[torch.from_numpy(sel).cuda()])
        # 4. sample cross-check against the oracle at this size (first and last 24 frames)
        o = Oracle(H, 64)
        for sl in (slice(0, 24), slice(B - 24, B)):
            d_ref, it_ref, _ = o.decode(MS_DEC, llr[sl].cpu().numpy(), 50, 0)
            assert np.array_equal(it[sl], it_ref) and np.array_equal(bits[sl], d_ref.astype(np.uint8))
        # 5. linearity of the channel symmetry: negating the LLRs of a codeword's support flips the decoded bits
        c = bits[sel[0]].astype(np.float64)
        y = llr[:64].clone()
        y_flipped = y * torch.from_numpy(1.0 - 2.0 * c).cuda()
        ha, ia, _ = dec.decode(y, 50)
        hb, ib, _ = dec.decode(y_flipped, 50)
        cw_words = torch.from_numpy(pack_bits(c[None, :]).view(np.int32)).cuda()
        assert torch.equal(ia, ib) and torch.equal(ha ^ cw_words, hb)


@pytest.mark.parametrize("dec_id,M,snr,B,maxiter,modulation", [
    (SP_DEC, 64, 2.0, 32768, 50, 0),       # BASELINE config #3
    (LMS_DEC, 512, 1.6, 4096, 50, 0),      # BASELINE config #4, one GPU's shard
    (MS_DEC, 64, 5.0, 65536, 50, 2),       # BASELINE config #5: behind the 16-QAM soft demapper
    (IMS_DEC, 64, 3.0, 65536, 50, 0),      # f1
    (TASP_DEC, 126, 1.7, 16384, 15, 0),    # f2: the shipped scenario
])
def test_full_size_properties_of_the_other_configurations(L, torch, dec_id, M, snr, B, maxiter, modulation):
    """Size-independent properties at the BASELINE sizes: a frame is reported converged exactly when its hard decisions satisfy
    every parity check, return values stay in range, any sub-batch decodes to the same words, and the first / last frames of
    the batch equal the oracle."""
    H = relift(load_base_matrix(), M)
    N = 32 * M
    zero_is_converged = dec_id in (SP_DEC, TASP_DEC)           # these return 0 for an input that already is a codeword
    with L.LdpcHip(dec_id, H, M) as dec:
        llr = dec.awgn_llr(snr, seed=11, first_frame=0, B=B, modulation=modulation)
        hard, iters, _ = dec.decode(llr, maxiter)
        torch.cuda.synchronize()
        it = iters.cpu().numpy()
        bits = unpack_bits(hard.cpu().numpy(), N)
        conv = it >= 0 if zero_is_converged else it > 0
        assert 0.5 < conv.mean() <= 1.0
        fail = syndrome_np(H, M, bits)
        assert not fail[conv].any() and fail[~conv].all()
        assert (it[~conv] == -maxiter).all() and it.max() <= maxiter
        lo, hi = B // 3, B // 3 + 333
        h2, i2, _ = dec.decode(llr[lo:hi].contiguous(), maxiter)
        assert torch.equal(h2, hard[lo:hi]) and torch.equal(i2, iters[lo:hi])
        o = Oracle(H, M)
        for sl in (slice(0, 8), slice(B - 8, B)):
            d_ref, it_ref, _ = o.decode(dec_id, llr[sl].cpu().numpy(), maxiter, 0)
            assert np.array_equal(it[sl], it_ref) and np.array_equal(bits[sl], d_ref.astype(np.uint8))


def test_device_noise_counting_and_simulate(L, torch):
    H = relift(load_base_matrix(), 64)
    N, R = 2048, 1024
    with L.LdpcHip(MS_DEC, H, 64) as dec:
        B, first = 300, 123456789012
        llr = dec.awgn_llr(1.4, seed=(5 << 32) | 77, first_frame=first, B=B)
        # noise generator against its CPU twin (Philox stream is exact; Box-Muller differs by libm/ocml rounding)
        sigma = bpsk_sigma(H, 1.4)
        g = philox_gauss_pairs((5 << 32) | 77, first + np.arange(B), N // 2)
        ref = -2.0 * (sigma * g + 2.0 * 0.0 - 1.0) / (sigma * sigma)
        np.testing.assert_allclose(llr.cpu().numpy(), ref, rtol=1e-11, atol=1e-11)
        # frames are keyed by their global index: a shifted window reproduces the overlap
        llr2 = dec.awgn_llr(1.4, seed=(5 << 32) | 77, first_frame=first + 100, B=50)
        assert torch.equal(llr2, llr[100:150])
        # puncturing (bp_simulation.cpp:697-710): last M*blocks LLRs are 0.5 for LLR decoders
        llr3 = dec.awgn_llr(1.4, seed=1, first_frame=0, B=4, punctured_blocks=2)
        assert (llr3[:, N - 128:] == 0.5).all() and not (llr3[:, :N - 128] == 0.5).any()
        # error accounting against numpy
        hard, iters, _ = dec.decode(llr, 50)
        cnt, info = dec.count_errors(hard, iters, want_frame_info=True)
        torch.cuda.synchronize()
        bits = unpack_bits(hard.cpu().numpy(), N)
        it = iters.cpu().numpy()
        bad = bits.any(axis=1)
        exp = [int(bits[bad][:, R:].sum()), int(bad.sum()), int((bad & (it >= 0)).sum()), B, int(np.abs(it).sum())]
        assert cnt.cpu().tolist() == exp
        inf = info.cpu().numpy()
        assert np.array_equal((inf & (1 << 30)) != 0, bad) and np.array_equal(inf & 0xFFFFF, bits[:, R:].sum(axis=1))
        # fused simulate == composition, and independent of how the frame range is chunked
        s = dec.simulate(1.4, 50, seed=(5 << 32) | 77, first_frame=first, B=B)
        assert [s["nse"], s["nde"], s["nue"], s["frames"], s["sum_abs_iters"]] == exp
        a = dec.simulate(1.4, 50, seed=(5 << 32) | 77, first_frame=first, B=100)
        b = dec.simulate(1.4, 50, seed=(5 << 32) | 77, first_frame=first + 100, B=200)
        assert all(a[k] + b[k] == s[k] for k in s)


def test_host_bp_simulation_replays_the_sequential_rule(L, torch):
    """ldpc_lib_amd.bp_simulation (batched, GPU) == frame-by-frame loop with the oracle decoder over the same noise."""
    H = relift(load_base_matrix(), 64)
    n_exp, n_fe, ref_fer, snr, seed = 700, 12, 0.02, 1.3, 99
    ber, fer, st = L.bp_simulation(H, 64, 50, n_fe, n_exp, snr, ref_fer, decoder_type=MS_DEC, seed=seed, batch=256,
                                   return_state=True)
    with L.LdpcHip(MS_DEC, H, 64) as dec:
        llr = dec.awgn_llr(snr, seed, 0, st["experiment"] + 5).cpu().numpy()
    o = Oracle(H, 64)
    nse = nde = nue = exp = 0
    while nde < n_fe and exp <= n_exp:          # bp_simulation.cpp:591-823
        d, it, _ = o.decode(MS_DEC, llr[exp], 50, 0)
        exp += 1
        if d.any():
            nse += int(d[1024:].sum()); nde += 1; nue += it >= 0
            if nde >= 10 and nde / exp > 2.5 * ref_fer:
                break
    assert (st["nse"], st["nde"], st["nue"], st["experiment"]) == (nse, nde, nue, exp)
    assert ber == nse / exp / 1024 and fer == nde / exp


def test_qam_frontend(L, torch):
    from ldpc_lib_amd.binding import qam_demod
    g = np.load(os.path.join(GOLDEN_DIR, "qam_frontend.npz"))
    for Q in (16, 64, 256):
        for out_type in (0, 1):
            for s in ("0p35", "0p8", "2p5"):
                key = f"q{Q}_t{out_type}_s{s}"
                x = torch.from_numpy(g[key + "_x"].reshape(-1, 2)).cuda()
                out = qam_demod(x, Q, 26.0, float(s.replace("p", ".")), out_type).cpu().numpy().ravel()
                ref = g[key + "_llr"]
                nan = np.isnan(ref)
                assert np.array_equal(np.isnan(out), nan), key
                np.testing.assert_allclose(out[~nan], ref[~nan], rtol=1e-12, atol=1e-13, err_msg=key)
    key = "q4_t0_s0p8"
    x = torch.from_numpy(g[key + "_x"].reshape(-1, 2)).cuda()
    out = qam_demod(x, 4, 26.0, 0.8, 0).cpu().numpy().ravel()
    assert np.array_equal(out, g[key + "_llr"])
    # device chain for 16 / 64 / 256-QAM (all-zero codeword at the constellation corner, Philox noise, demap, negate) against
    # its CPU twin: numpy Philox + Box-Muller, the oracle's demapper.  N = 2048 is not a multiple of 6: the last 64-QAM symbol is
    # padded (bp_simulation.cpp:575) and only its first two LLRs exist.
    import ctypes as C
    from ldpc_testlib import _as_double_p, oracle_lib, philox_gauss_pairs
    H = relift(load_base_matrix(), 64)
    with L.LdpcHip(MS_DEC, H, 64) as dec:
        for mod, Q, m, snr in ((2, 16, 4, 6.0), (3, 64, 6, 10.0), (4, 256, 8, 14.0)):
            B, first, seed, N = 6, 987654321, (9 << 32) | 5, 2048
            llr = dec.awgn_llr(snr, seed=seed, first_frame=first, B=B, modulation=mod).cpu().numpy()
            ns = (N + m - 1) // m
            rate, halfmlog = 0.5, m // 2
            sigma = np.sqrt(10.0 ** (-snr / 10.0) / (2 * rate * halfmlog * 2) * (2.0 * (Q - 1.0) / 3.0))   # bp_simulation.cpp:447-449
            g = philox_gauss_pairs(seed, first + np.arange(B), ns, tag=1)
            x = np.ascontiguousarray(-(2 ** halfmlog - 1) + sigma * g)
            ref = np.zeros((B, ns * m))
            for b in range(B):
                oracle_lib().orc_qam_demodulate(Q, 26.0, float(sigma), _as_double_p(x[b]), ns, _as_double_p(ref[b]), 0)
            np.testing.assert_allclose(llr, -ref[:, :N], rtol=1e-9, atol=1e-9, err_msg=f"QAM-{Q}")
            assert (llr > 0).mean() > 0.85      # zeros were sent
    # 16-QAM chain: statistics of the LLRs of the all-zero codeword + decodes at a reasonable Eb/N0
    H = relift(load_base_matrix(), 64)
    with L.LdpcHip(MS_DEC, H, 64) as dec:
        llr = dec.awgn_llr(6.0, seed=3, first_frame=0, B=512, modulation=2)
        hard, iters, _ = dec.decode(llr, 50)
        assert (llr > 0).double().mean().item() > 0.9
        assert (iters > 0).double().mean().item() > 0.95


def _other_m64_code():
    """A different (2048,1024)-shaped code: same protograph, other circulant shifts (so not the ahead-of-time instance)."""
    H = relift(load_base_matrix(), 64)
    H2 = H.copy()
    H2[H > 0] = (H[H > 0] * 7 + 3) % 64
    return H2


@pytest.mark.parametrize("variant,expect", [("2", "hiprtc"), ("0", "m64_kernel<atomic>"), ("1", "m64_kernel<rmw>"), ("-1", "ms_flood_kernel")])
def test_every_min_sum_kernel_tier_is_bit_exact(L, torch, monkeypatch, variant, expect):
    """The code-specialised hiprtc instance (any base matrix), the table-driven M=64 kernel (atomic and read-add-write
    accumulation) and the generic kernel must all reproduce the oracle bit for bit."""
    monkeypatch.setenv("LDPC_HIP_MS_VARIANT", variant)
    H2 = _other_m64_code()
    llr = np.concatenate([awgn_llr(H2, 64, s, 40 + i, 40) for i, s in enumerate((1.0, 1.6, 2.4))])
    o = Oracle(H2, 64)
    d_ref, it_ref, _ = o.decode(MS_DEC, llr, 50, 0)
    s_ref, _, _ = o.decode(MS_DEC, llr, 50, 1)
    with L.LdpcHip(MS_DEC, H2, 64) as dec:
        assert expect in dec.kernel_name, dec.kernel_name
        hard, iters, soft = dec.decode(torch.from_numpy(llr).cuda(), 50, want_soft=True)
        torch.cuda.synchronize()
        assert np.array_equal(iters.cpu().numpy(), it_ref)
        assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref))
        assert_bits_equal(soft.cpu().numpy(), s_ref)


@pytest.mark.parametrize("chunk,expect", [("1", "ms_chunk_appendix_c_m126_kernel"), ("0", "ms_spec_appendix_c_m126_kernel")])
def test_both_min_sum_kernels_for_the_shipped_lifting_are_bit_exact(L, monkeypatch, chunk, expect):
    """M = 126 (upstream's shipped tailbite length): one wave owning two 64-lane chunks (default, no barriers) and two waves with
    workgroup barriers produce the reference's bits, iteration counts and soft values."""
    monkeypatch.setenv("LDPC_HIP_MS_CHUNK", chunk)
    g = np.load(os.path.join(GOLDEN_DIR, "ms_m126_1p7.npz"))
    with L.LdpcHip(MS_DEC, g["H"], 126) as dec:
        assert expect in dec.kernel_name
        d0, it0, _ = dec.decode_host(g["llr"], int(g["maxiter"]), decision=0)
        assert np.array_equal(it0, g["iters"]) and np.array_equal(pack_bits(d0), g["hard"])
        ns = g["soft"].shape[0]
        d1, _, _ = dec.decode_host(g["llr"][:ns], int(g["maxiter"]), decision=1)
        assert_bits_equal(d1, g["soft"])
    H = relift(load_base_matrix(), 126)
    llr = np.concatenate([awgn_llr(H, 126, s, 70 + i, 12) for i, s in enumerate((0.8, 1.6, 2.4))])
    d_ref, it_ref, _ = Oracle(H, 126).decode(MS_DEC, llr, 50, 0)
    with L.LdpcHip(MS_DEC, H, 126) as dec:
        d, it, _ = dec.decode_host(llr, 50)
        assert np.array_equal(it, it_ref) and np.array_equal(d, d_ref)


def test_small_liftings_share_a_wavefront(L, torch):
    """M <= 32: floor(64/M) frames per wavefront in the code-specialised min-sum, layered and integer min-sum kernels; frames of one wave
    converge at different iterations and each must stop exactly where upstream stops it.  Ragged batch (last wave partly
    empty), M = 27 leaves 10 lanes idle; M = 1 puts 64 frames on a wave; 33 <= M < 64 runs one frame per wave with idle lanes."""
    for dec_id, small, one in ((MS_DEC, "ms_small_body", "ms_body"), (LMS_DEC, "lms_small_body", "lms_body"), (IMS_DEC, "ims_small_body", "ims_body")):
        for M, frames, expect in ((32, 101, small), (27, 77, small), (8, 333, small), (5, 200, small), (1, 1000, small), (40, 50, one)):
            H = relift(load_base_matrix(), M)
            llr = np.concatenate([awgn_llr(H, M, s, 90 + i, frames // 3 + 1) for i, s in enumerate((2.0, 3.5, 6.0))])[:frames]
            d_ref, it_ref, _ = Oracle(H, M).decode(dec_id, llr, 40, 0)
            s_ref, _, _ = Oracle(H, M).decode(dec_id, llr, 40, 1)
            with L.LdpcHip(dec_id, H, M) as dec:
                assert expect in dec.kernel_name, dec.kernel_name
                hard, iters, soft = dec.decode(torch.from_numpy(llr).cuda(), 40, want_soft=True)
                torch.cuda.synchronize()
                assert np.array_equal(iters.cpu().numpy(), it_ref), (dec_id, M)
                assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref)), (dec_id, M)
                assert_bits_equal(soft.cpu().numpy(), s_ref), (dec_id, M)
            assert len(set(it_ref.tolist())) > 3      # the frames of a wave really do stop at different iterations


def test_flagship_code_uses_the_ahead_of_time_instance(L):
    with L.LdpcHip(MS_DEC, relift(load_base_matrix(), 64), 64) as dec:
        assert "ahead of time" in dec.kernel_name


# ---- the C++ source-compatible layer (include/ldpc/*.h, csrc/compat) -------------------------------------------------
def _compat_lib(L):
    import ctypes as C
    import subprocess
    L.load_library()  # torch + libldpc_hip.so first: one HIP runtime per process
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "ldpc-lib_amd", "csrc", "compat")])
    lib = C.CDLL(os.path.join(root, "ldpc-lib_amd", "libldpc_compat.so"))
    lib.ldpc_bp_simulation_exact.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                             C.c_double, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_void_p, C.c_void_p]
    return lib


@pytest.mark.parametrize("dec_id,M,snr,maxit,n_fe,n_exp,ref,mod,punct,seed", [
    (MS_DEC, 64, 2.0, 50, 10**9, 700, 1.0, 0, 0, 1),        # runs the whole budget: 701 frames (bp_simulation.cpp:591 `<=`)
    (MS_DEC, 64, 2.0, 50, 10**9, 4000, 1.0, 0, 0, 1),       # BASELINE.md section 2, cfg2, the headline configuration: 170 errored frames in 4001
    (MS_DEC, 64, 1.2, 50, 10**9, 5000, 0.02, 0, 0, 1),      # stops early on the FER rule (:820): generator roll-back
    (MS_DEC, 64, 1.4, 50, 7, 5000, 1.0, 0, 0, 3),           # stops on n_frame_errors
    (LMS_DEC, 126, 1.7, 50, 10**9, 150, 1.0, 0, 0, 1),
    (MS_DEC, 1, 4.0, 20, 10**9, 2000, 1.0, 0, 0, 1),        # BASELINE config #1 (32,16): FER 0.056 in BASELINE.md
    (MS_DEC, 64, 2.5, 50, 10**9, 300, 1.0, 1, 0, 5),        # QAM4 formula (:607-612)
    (MS_DEC, 64, 3.0, 50, 10**9, 200, 1.0, 0, 2, 5),        # two punctured blocks (:697-710)
    (TASP_DEC, 126, 1.7, 15, 50, 10**8, 1.0, 0, 0, 1),      # the shipped `search` scenario: 50 errored frames in 821
    (ASP_DEC, 64, 1.6, 30, 10**9, 250, 1.0, 0, 0, 2),       # probability-domain sum-product, out_type 1 puncturing value
    (BP_DEC, 64, 1.3, 30, 10**9, 250, 1.0, 0, 0, 2),        # Gallager BP: failed frames leave their syndrome to the next frame
])
def test_exact_replay_harness_equals_the_sequential_harness(L, dec_id, M, snr, maxit, n_fe, n_exp, ref, mod, punct, seed):
    """C++ bp_simulation on the GPU (batched, host mt19937 noise in upstream's draw order) == the sequential CPU
    restatement of upstream's frame loop: same counters, same BER/FER doubles, same generator state afterwards."""
    import ctypes as C
    from ldpc_testlib import SimResult, c_int_p, oracle_lib
    lib = _compat_lib(L)
    H = np.ascontiguousarray(relift(load_base_matrix(), M), dtype=np.int32)
    out = (C.c_double * 7)()
    nxt = C.c_uint()
    rc = lib.ldpc_bp_simulation_exact(16, 32, H.ctypes.data, M, maxit, n_fe, n_exp, snr, ref, dec_id, mod, punct, seed, 0,
                                      C.addressof(out), C.addressof(nxt))
    assert rc == 0
    res = SimResult()
    assert oracle_lib().orc_bp_simulation(16, 32, H.ctypes.data_as(c_int_p), M, maxit, n_fe, n_exp, snr, ref, dec_id, mod, punct,
                                          seed, C.byref(res), None) == 0
    assert (out[2], out[3], out[4], out[5], out[6]) == (res.nse, res.nde, res.nue, res.experiment, res.sum_abs_iter)
    assert out[0] == res.ber and out[1] == res.fer
    assert nxt.value == res.rng_next
    if dec_id == TASP_DEC:
        assert (res.nde, res.experiment) == (50, 821)       # FER 0.061 measured by the survey with the upstream binary
    if (dec_id, M, n_exp, seed) == (MS_DEC, 1, 2000, 1):
        assert res.nde == 112 and res.experiment == 2001   # the FER 0.056 the survey measured with the compiled upstream binary
    if (dec_id, M, n_exp, seed, snr) == (MS_DEC, 64, 4000, 1, 2.0):
        assert (res.nde, res.experiment) == (170, 4001)     # FER 0.0425 of BASELINE.md section 2 (cfg2), upstream binary, seed 1


DROPIN_CASES = [
    # dec, M, snr, maxit, n_fe, n_exp, ref, mod, ptype, pblock, pinter, punct, seed
    (MS_DEC, 64, 2.0, 50, 10**9, 4000, 1.0, 0, 0, 128, 1, 0, 1),     # cfg2 headline: 170 / 4001
    (MS_DEC, 64, 1.2, 50, 10**9, 5000, 0.02, 0, 0, 128, 1, 0, 1),    # early stop on the FER rule: generator roll-back on upstream's own object
    (TASP_DEC, 126, 1.7, 15, 50, 10**8, 1.0, 0, 0, 128, 1, 0, 1),    # the shipped `search` scenario: 50 / 821
    (LMS_DEC, 64, 1.6, 50, 10**9, 300, 1.0, 1, 3, 64, 1, 2, 9),      # QAM4 + block interleaver + two punctured blocks
]


@pytest.mark.parametrize("case", DROPIN_CASES)
def test_upstream_bp_simulation_symbol_runs_on_the_gpu(L, case):
    """oracle/_ref/dropin_driver = csrc/compat/bp_simulation_dropin.cpp + decoders_compat.cpp compiled against UPSTREAM'S OWN
    bp_simulation.h / data_structures.h / commons_portable.h / decoders.h (oracle/Makefile `ref`, built where the upstream tree
    is mounted) and linked into a program that calls the exact symbol main_simulation.cpp:500 binds.  Its BER / FER doubles and
    the generator state it leaves in upstream's `generator` object must equal the sequential harness restatement's."""
    import ctypes as C
    import subprocess
    from ldpc_testlib import SimResult, c_int_p, oracle_lib
    dec_id, M, snr, maxit, n_fe, n_exp, ref, mod, ptype, pblock, pinter, punct, seed = case
    exe = os.path.join(os.path.dirname(GOLDEN_DIR), "..", "oracle", "_ref", "dropin_driver")
    assert os.path.exists(exe), "oracle/_ref/dropin_driver missing: run `make -C oracle ref` where /root/reference is mounted"
    H = np.ascontiguousarray(relift(load_base_matrix(), M), dtype=np.int32)
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        hp = os.path.join(td, "H.txt")
        np.savetxt(hp, H, fmt="%d")
        out = subprocess.run([exe, hp, "16", "32", str(M), str(maxit), str(n_fe), str(n_exp), repr(snr), repr(ref), str(dec_id),
                              str(mod), str(ptype), str(pblock), str(pinter), str(punct), str(seed)],
                             check=True, capture_output=True, text=True, timeout=900).stdout
    got = dict(line.split() for line in out.strip().splitlines() if line[:3] in ("BER", "FER", "RNG", "MS_"))
    olib = oracle_lib()
    res = SimResult()
    if ptype == 0:
        assert olib.orc_bp_simulation(16, 32, H.ctypes.data_as(c_int_p), M, maxit, n_fe, n_exp, snr, ref, dec_id, mod, punct, seed,
                                      C.byref(res), None) == 0
    else:
        from ldpc_lib_amd.binding import build_interleaver
        direct, inv = build_interleaver(H, M, ptype, 1, pblock, pinter)
        inv = np.ascontiguousarray(inv, dtype=np.int32)
        olib.orc_bp_simulation_perm.argtypes = [C.c_int, C.c_int, c_int_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                                                C.c_int, C.c_uint, c_int_p, C.POINTER(SimResult), c_int_p]
        assert olib.orc_bp_simulation_perm(16, 32, H.ctypes.data_as(c_int_p), M, maxit, n_fe, n_exp, snr, ref, dec_id, mod, punct, seed,
                                           inv.ctypes.data_as(c_int_p), C.byref(res), None) == 0
    assert float.fromhex(got["BER"]) == res.ber and float.fromhex(got["FER"]) == res.fer
    assert int(got["RNG"]) == res.rng_next
    if case is DROPIN_CASES[0]:
        assert (res.nde, res.experiment) == (170, 4001) and float.fromhex(got["FER"]) == 170 / 4001
    if dec_id == TASP_DEC:
        assert (res.nde, res.experiment) == (50, 821)
    # (the decoders.h surface under upstream's DEC_STATE layout is compared with the golden vectors, decoder by decoder, in
    # test_decoders_h_call_surface[upstream_header]; here only: the call works in the same process as the harness)
    assert int(got["MS_ITERS"]) != 0 and 0 <= int(got["MS_ONES"]) <= 32 * M


@pytest.mark.parametrize("layout", ["own_header", "upstream_header"])
@pytest.mark.parametrize("name", ["ms_m64_1p2", "lms_m64_0p8", "sp_m64_2p0", "ms_m126_1p7", "ms_m1_4p0", "ims_m64_2p0", "tasp_m126_1p7",
                                  "asp_m64_1p2", "bp_m64_1p0_stale"])
def test_decoders_h_call_surface(L, tmp_path, name, layout):
    """decod_open / hd fill / decod_init / <decoder>(st, st->y, st->decword, ...) / decod_close from a C++ program, on the reference's
    golden vectors (return values, decword as hard bits and as soft values, what is left in y) -- built against include/ldpc/decoders.h
    ("own_header") and against UPSTREAM'S OWN decoders.h with its DEC_STATE layout ("upstream_header": oracle/_ref/compat_driver_upstream,
    csrc/compat/decoders_compat.cpp with -DLDPC_COMPAT_UPSTREAM_HEADERS -- the flavour a maintainer links)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if layout == "upstream_header":
        exe = os.path.join(root, "oracle", "_ref", "compat_driver_upstream")
        assert os.path.exists(exe), "oracle/_ref/compat_driver_upstream missing: run `make -C oracle ref` where /root/reference is mounted"
    else:
        _compat_lib(L)
        exe = str(tmp_path / "compat_driver")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                               os.path.join(root, "tests", "cpp", "compat_driver.cpp"), "-o", exe,
                               "-L", os.path.join(root, "ldpc-lib_amd"), "-lldpc_compat", "-lldpc_hip",
                               "-Wl,-rpath," + os.path.join(root, "ldpc-lib_amd")])
    g = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    H, M, dec_id, maxiter = g["H"], int(g["M"]), int(g["dec_id"]), int(g["maxiter"])
    for decision, nfr in ((0, g["llr"].shape[0]), (1, g["soft"].shape[0])):
        llr = g["llr"][:nfr]
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(np.array([dec_id, H.shape[0], H.shape[1], M, nfr, maxiter, decision], dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(H, dtype=np.int16).tobytes())
            f.write(np.ascontiguousarray(llr, dtype=np.float64).tobytes())
        subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
        raw = open(tmp_path / "out.bin", "rb").read()
        N = H.shape[1] * M
        iters = np.frombuffer(raw[:4 * nfr], dtype=np.int32)
        dec = np.frombuffer(raw[4 * nfr:4 * nfr + 8 * nfr * N], dtype=np.float64).reshape(nfr, N)
        after = np.frombuffer(raw[4 * nfr + 8 * nfr * N:], dtype=np.float64).reshape(nfr, N)
        assert np.array_equal(iters, g["iters"][:nfr])
        if decision == 0 or dec_id == TASP_DEC:
            assert np.array_equal(pack_bits(dec), g["hard"][:nfr])
        elif dec_id == BP_DEC:
            _close(dec, g["soft"], BP_RTOL, BP_ATOL)
        elif dec_id in (SP_DEC, ASP_DEC):
            _close(dec, g["soft"], SP_RTOL if dec_id == SP_DEC else TASP_RTOL)
        else:
            assert_bits_equal(dec, g["soft"])
        if dec_id not in (BP_DEC, SP_DEC, ASP_DEC, TASP_DEC):
            assert_bits_equal(after, llr)          # MS/LMS leave y intact (SURVEY 8b ownership)
        else:
            assert not np.array_equal(after, llr)      # SP clobbers its input like upstream (decoders.cpp:1950)


@pytest.mark.parametrize("thr,qbits,dbits,alpha,expect", [
    (1.4, 6, 8, 0.8, "ims_spec"),       # upstream defaults: int8 code-specialised kernel
    (1.4, 6, 8, 1.0, "ims_spec"),       # ialpha = 16, still int8
    (2.0, 7, 8, 0.75, "ims_spec"),
    (1.4, 6, 10, 0.8, "ims_flood"),     # 10-bit data: beyond int8 -> table-driven int32 kernel, same results as the oracle
    (1.4, 6, 8, 1.25, "ims_flood"),     # ialpha = 20 > 16
])
def test_integer_min_sum_parameters_pick_the_right_kernel(L, torch, thr, qbits, dbits, alpha, expect):
    import ctypes as C
    from ldpc_testlib import _as_double_p, oracle_lib
    H = relift(load_base_matrix(), 64)
    llr = np.concatenate([awgn_llr(H, 64, s, 40 + i, 30) for i, s in enumerate((1.2, 2.2, 3.0))])
    o = Oracle(H, 64)
    lib = oracle_lib()
    lib.orc_imin_sum.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int]
    want_it = np.zeros(len(llr), dtype=np.int32)
    want_soft = np.zeros_like(llr)
    for f in range(len(llr)):
        y = llr[f].copy()
        want_it[f] = lib.orc_imin_sum(o.h, _as_double_p(y), _as_double_p(want_soft[f]), 50, 1, alpha, thr, qbits, dbits)
    with L.LdpcHip(IMS_DEC, H, 64) as dec:
        dec.set_ims_params(thr, qbits, dbits)
        hard, iters, soft = dec.decode(torch.from_numpy(llr).cuda(), 50, alpha=alpha, want_soft=True)
        torch.cuda.synchronize()
        assert np.array_equal(iters.cpu().numpy(), want_it)
        assert_bits_equal(soft.cpu().numpy(), want_soft)
        assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits((want_soft < 0).astype(np.float64)))
        assert expect in dec.last_launch(), dec.last_launch()


def test_bp_frames_chain_through_the_uncleared_syndrome(L):
    """Upstream's bp_decod_qc_lm XORs its input check into the syndrome the previous call left behind (decoders.cpp:1742-1762,
    SURVEY Appendix B Q8): a codeword-at-the-input frame that follows a FAILED frame returns 1, not 0.  The golden set holds
    such frames (2, 6, 9) and controls (0, 10).  The chain must survive any split into calls, and switch off cleanly."""
    g = np.load(os.path.join(GOLDEN_DIR, "bp_m64_1p0_stale.npz"))
    H, M, maxiter, llr, want = g["H"], int(g["M"]), int(g["maxiter"]), g["llr"], g["iters"]
    assert [int(want[f]) for f in (0, 1, 2, 5, 6, 8, 9, 10)] == [0, -50, 1, -50, 1, -50, 1, 0]
    with L.LdpcHip(BP_DEC, H, M) as dec:
        parts = [dec.decode_host(llr[a:b], maxiter)[1] for a, b in ((0, 2), (2, 3), (3, 9), (9, 16))]   # every cut after a failed frame
        assert np.array_equal(np.concatenate(parts), want)
        dec.set_bp_chain(True, reset_carry=True)
        d, it, _ = dec.decode_host(llr, maxiter)
        assert np.array_equal(it, want) and np.array_equal(pack_bits(d), g["hard"])
        dec.set_bp_chain(False, reset_carry=True)     # every frame from a zero syndrome: only the chained frames change
        _, it0, _ = dec.decode_host(llr, maxiter)
        changed = np.nonzero(it0 != want)[0].tolist()
        assert changed == [2, 6, 9] and all(it0[f] == 0 for f in changed)


@pytest.mark.parametrize("M,frames", [(64, 96), (126, 24), (200, 12), (512, 6)])
def test_layered_min_sum_specialised_instances(L, torch, M, frames):
    """hiprtc instances of lms_body (power-of-two and other liftings, 1..8 waves per frame) against the oracle."""
    H = relift(load_base_matrix(), M)
    H2 = H.copy()
    H2[H > 0] = (H[H > 0] * 5 + 1) % M          # not the ahead-of-time matrices
    llr = np.concatenate([awgn_llr(H2, M, s, 60 + i, frames // 2) for i, s in enumerate((1.0, 2.0))])
    o = Oracle(H2, M)
    d_ref, it_ref, _ = o.decode(LMS_DEC, llr, 50, 0)
    s_ref, _, _ = o.decode(LMS_DEC, llr, 50, 1)
    with L.LdpcHip(LMS_DEC, H2, M) as dec:
        assert "hiprtc" in dec.kernel_name, dec.kernel_name
        hard, iters, soft = dec.decode(torch.from_numpy(llr).cuda(), 50, want_soft=True)
        torch.cuda.synchronize()
        assert np.array_equal(iters.cpu().numpy(), it_ref)
        assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref))
        assert_bits_equal(soft.cpu().numpy(), s_ref)
    for Maot in (64, 512):
        with L.LdpcHip(LMS_DEC, relift(load_base_matrix(), Maot), Maot) as dec:
            assert "ahead of time" in dec.kernel_name


def test_sum_product_specialised_instances(L, torch):
    """code-specialised sum-product: ahead-of-time instance for the example code, hiprtc instance for another code."""
    H = relift(load_base_matrix(), 64)
    with L.LdpcHip(SP_DEC, H, 64) as dec:
        assert "sp_spec" in dec.kernel_name and "ahead of time" in dec.kernel_name
    H2 = _other_m64_code()
    llr = np.concatenate([awgn_llr(H2, 64, s, 70 + i, 40) for i, s in enumerate((1.2, 2.2))])
    o = Oracle(H2, 64)
    d_ref, it_ref, _ = o.decode(SP_DEC, llr, 50, 0)
    s_ref, _, _ = o.decode(SP_DEC, llr, 50, 1)
    with L.LdpcHip(SP_DEC, H2, 64) as dec:
        assert "sp_body" in dec.kernel_name and "hiprtc" in dec.kernel_name, dec.kernel_name
        hard, iters, soft = dec.decode(torch.from_numpy(llr).cuda(), 50, want_soft=True)
        torch.cuda.synchronize()
        assert np.array_equal(iters.cpu().numpy(), it_ref)
        assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref))
        _close(soft.cpu().numpy(), s_ref, SP_RTOL)


def test_c_example_runs(L, tmp_path):
    """the plain-C example (examples/simulate.c) end to end: FER at 2.0 dB within the Monte-Carlo spread of upstream's 0.0425"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "simulate")
    subprocess.check_call(["gcc", "-O1", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "simulate.c"), "-o", exe,
                           "-L", os.path.join(root, "ldpc-lib_amd"), "-lldpc_hip", "-Wl,-rpath," + os.path.join(root, "ldpc-lib_amd")])
    out = subprocess.check_output([exe, os.path.join(GOLDEN_DIR, "h16x32_m126.txt"), "64", "3", "50", "2.0", "2.0", "1", "100000"]).decode()
    row = [ln for ln in out.splitlines() if not ln.startswith("#")][0].split()
    assert abs(float(row[1]) - 0.0425) < 0.004, out


def test_ldpc_sim_driver_reproduces_the_sequential_harness(L, tmp_path):
    """`ldpc_sim simulation`: jsonx scenario in, result records out; every (code, SNR) point must equal the
    sequential CPU restatement of upstream's bp_simulation on the same generator seed -- and the three points the survey
    measured with the compiled upstream binary (112, 13 and 124 errored frames in 2001)."""
    import ctypes as C
    import subprocess
    from ldpc_testlib import SimResult, c_int_p, oracle_lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    _compat_lib(L)
    exe = os.path.join(root, "ldpc-lib_amd", "ldpc_sim")
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "ldpc-lib_amd", "csrc", "compat")])
    out = str(tmp_path / "result.jsonx")
    subprocess.check_call([exe, "simulation", os.path.join(root, "examples", "simulation_appendix_c.jsonx"), out])
    def get(path):
        return subprocess.check_output([exe, "jsonx-get", out, path], text=True).strip()
    def numbers(path):
        return [float(x) for x in get(path).replace("array {", "").replace("}", "").split()]
    points = [(0, MS_DEC, 1, 20, [4.0], 112), (1, SP_DEC, 64, 50, [2.0], 13), (2, LMS_DEC, 512, 50, [1.6], 124), (3, MS_DEC, 64, 50, [2.0, 2.5], None)]
    for idx, dec_id, M, maxit, snrs, survey_nde in points:
        assert int(get(f"results/{idx}/_decoder_type")) == dec_id and int(get(f"results/{idx}/_lifting")) == M
        H = np.ascontiguousarray(relift(load_base_matrix(), M), dtype=np.int32)
        cells = [int(x) for x in get(f"results/{idx}/code").replace("matrix (16 32) {", "").replace("}", "").split()]
        assert np.array_equal(np.array(cells).reshape(16, 32), H)       # shifts reduced modulo the lifting (main_simulation.cpp:400-414)
        fer, ber = numbers(f"results/{idx}/simulation_logs/0/FER"), numbers(f"results/{idx}/simulation_logs/0/BER")
        for s, snr in enumerate(snrs):
            res = SimResult()
            assert oracle_lib().orc_bp_simulation(16, 32, H.ctypes.data_as(c_int_p), M, maxit, 1000000, 2000, snr, 1.0, dec_id, 0, 0, 1,
                                                  C.byref(res), None) == 0
            assert res.experiment == 2001
            assert fer[s] == res.fer and ber[s] == res.ber
            if survey_nde is not None:
                assert res.nde == survey_nde


@pytest.mark.parametrize("perm_type,block,inter", [(1, 128, 1), (2, 128, 1), (3, 300, 1), (4, 128, 16)])
def test_exact_replay_harness_with_interleavers(L, torch, perm_type, block, inter):
    """permutation_type 1-4: the harness applies upstream's inverse map between channel and decoder
    (bp_simulation.cpp:684); counters, BER/FER and generator state equal the sequential restatement fed with the map recorded
    from the compiled upstream interleaver.  Also the device gather itself against numpy."""
    import ctypes as C
    from ldpc_lib_amd.binding import build_interleaver, permute
    from ldpc_testlib import SimResult, c_int_p, oracle_lib
    lib = _compat_lib(L)
    M = 64
    H = np.ascontiguousarray(relift(load_base_matrix(), M), dtype=np.int32)
    direct, inverse = build_interleaver(H, M, perm_type, 1, block, inter)     # == upstream's (tests/test_host_cpu.py)
    out = (C.c_double * 7)()
    nxt = C.c_uint()
    lib.ldpc_bp_simulation_exact_perm.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_void_p, C.c_void_p]
    assert lib.ldpc_bp_simulation_exact_perm(16, 32, H.ctypes.data, M, 50, 10**9, 400, 1.6, 1.0, MS_DEC, 0, perm_type, block, inter, 0, 7, 0,
                                             C.addressof(out), C.addressof(nxt)) == 0
    res = SimResult()
    olib = oracle_lib()
    olib.orc_bp_simulation_perm.argtypes = [C.c_int, C.c_int, c_int_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                                            C.c_int, C.c_uint, c_int_p, C.c_void_p, C.c_void_p]
    inv = np.ascontiguousarray(inverse, dtype=np.int32)
    assert olib.orc_bp_simulation_perm(16, 32, H.ctypes.data_as(c_int_p), M, 50, 10**9, 400, 1.6, 1.0, MS_DEC, 0, 0, 7, inv.ctypes.data_as(c_int_p),
                                       C.addressof(res), None) == 0
    assert (out[2], out[3], out[4], out[5], out[6]) == (res.nse, res.nde, res.nue, res.experiment, res.sum_abs_iter)
    assert out[0] == res.ber and out[1] == res.fer and nxt.value == res.rng_next
    ident = SimResult()
    assert olib.orc_bp_simulation_perm(16, 32, H.ctypes.data_as(c_int_p), M, 50, 10**9, 400, 1.6, 1.0, MS_DEC, 0, 0, 7, None, C.addressof(ident), None) == 0
    assert ident.sum_abs_iter != res.sum_abs_iter      # the interleaver moved the noise around (same statistics, other frames)
    x = torch.randn(37, 2048, dtype=torch.float64, device="cuda")
    for m in (direct, inverse):
        y = permute(x, torch.from_numpy(m).cuda())
        assert torch.equal(y.cpu(), x.cpu()[:, torch.from_numpy(m.astype(np.int64))])
    assert torch.equal(permute(permute(x, torch.from_numpy(direct).cuda()), torch.from_numpy(inverse).cuda()), x)


@pytest.mark.parametrize("rh,nh,M,weights,seed", [
    (4, 8, 96, (3, 4, 2, 4), 1),          # small, dense rows (row weight up to 6), 2 waves' worth of lanes on one wave (chunk kernel)
    (12, 24, 81, (3, 3, 6, 2, 11, 3), 2),  # 802.11n-like shape, lifting that is not a multiple of anything convenient
    (8, 20, 128, (2, 3, 8, 3, 2), 3),      # power-of-two lifting above 64, high-rate
])
def test_every_decoder_on_random_protographs(L, torch, rh, nh, M, weights, seed):
    """Codes the ahead-of-time instances know nothing about: every decoder compiles its own instance with hiprtc (or runs the
    table kernel) and must reproduce the oracle -- bit for bit for MS / LMS / IMS, hard bits + iteration counts (soft values
    to the stated tolerances) for the sum-product family."""
    from ldpc_testlib import random_qc_code
    rng = np.random.RandomState(seed)
    H = random_qc_code(rng, rh, nh, M, weights)
    assert (H >= 0).sum(axis=1).max() <= 16     # rows heavier than 8 circulants send integer min-sum to the table kernel
    llr = np.concatenate([awgn_llr(H, M, s, 200 + i, 10) for i, s in enumerate((1.5, 3.0, 4.5))])
    for dec_id in (MS_DEC, LMS_DEC, IMS_DEC, SP_DEC, ASP_DEC, TASP_DEC, BP_DEC):
        o = Oracle(H, M)
        d_ref, it_ref, _ = o.decode(dec_id, llr, 25, 0)
        with L.LdpcHip(dec_id, H, M) as dec:
            x = torch.from_numpy(llr).cuda()
            hard, iters, soft = dec.decode(x, 25, want_soft=True)
            torch.cuda.synchronize()
            assert np.array_equal(iters.cpu().numpy(), it_ref), (dec_id, dec.kernel_name)
            assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref)), (dec_id, dec.kernel_name)
            s_ref, _, _ = Oracle(H, M).decode(dec_id, llr, 25, 1)
            if dec_id in (MS_DEC, LMS_DEC, IMS_DEC):
                assert_bits_equal(soft.cpu().numpy(), s_ref), (dec_id, dec.kernel_name)
            elif dec_id == BP_DEC:
                _close(soft.cpu().numpy(), s_ref, BP_RTOL, BP_ATOL)
            else:
                _close(soft.cpu().numpy(), s_ref, SP_RTOL if dec_id == SP_DEC else TASP_RTOL)


@pytest.mark.parametrize("M", [64, 126])
def test_non_zero_codewords_decode_like_the_zero_codeword(L, torch, M):
    """Upstream only ever sends the all-zero codeword (bp_simulation.cpp:568).  With the encoder the decoders can
    be checked on real codewords: flipping the signs of the channel LLRs by a codeword c must flip the decisions by c and
    leave the iteration counts alone.  For min-sum and layered min-sum that symmetry is EXACT in floating point (negation
    commutes with every operation they use), so it is asserted bit for bit.  Integer min-sum is not mirror symmetric (an
    a-posteriori value or message of exactly 0 -- frequent with 8-bit integers -- decides "0" whatever was sent) and the
    sum-product family works on probabilities (p <-> 1-p does not mirror exactly): those are checked on converged frames."""
    from ldpc_lib_amd.binding import encode
    from ldpc_testlib import syndrome_np
    H = relift(load_base_matrix(), M)
    rng = np.random.RandomState(M)
    B, K, N = 48, 16 * M, 32 * M
    cws = np.stack([encode(H, M, rng.randint(0, 2, K).astype(np.uint8)) for _ in range(B)])
    assert not syndrome_np(H, M, cws).any()
    y0 = np.concatenate([awgn_llr(H, M, s, 300 + i, B // 3) for i, s in enumerate((1.4, 2.0, 3.0))])
    y = y0 * (1.0 - 2.0 * cws)
    for dec_id in (MS_DEC, LMS_DEC, IMS_DEC, SP_DEC, ASP_DEC, TASP_DEC, BP_DEC):
        if dec_id in (ASP_DEC, BP_DEC) and M > 128:
            continue
        with L.LdpcHip(dec_id, H, M) as dec:
            if dec_id == BP_DEC:
                dec.set_bp_chain(False, True)
            d0, it0, _ = dec.decode_host(y0.copy(), 30)
            d1, it1, _ = dec.decode_host(y.copy(), 30)
        if dec_id in (MS_DEC, LMS_DEC):
            assert np.array_equal(it0, it1), dec_id
            assert np.array_equal(d1.astype(np.uint8), d0.astype(np.uint8) ^ cws), dec_id
        else:
            conv = (it0 > 0) & (it1 > 0)
            assert conv.sum() >= B // 3 and ((it0 > 0) != (it1 > 0)).sum() <= 2, dec_id
            wrong = (d1[conv].astype(np.uint8) != cws[conv]).any(axis=1)             # converged, but to another codeword (undetected error)
            assert wrong.sum() <= 2, dec_id
            assert np.array_equal(wrong, (d0[conv] != 0).any(axis=1)) or wrong.sum() <= 1, dec_id   # ... and the zero-codeword run agrees on which
            assert np.abs(it0[conv] - it1[conv]).max() <= 3, dec_id


def test_hiprtc_code_objects_can_be_cached_on_disk(L, tmp_path, monkeypatch):
    """LDPC_HIP_CACHE_DIR: the first open of an unseen code compiles and leaves one .hsaco per (decoder body, code); a fresh
    process picks it up instead of compiling (seconds -> milliseconds) and decodes the same bits."""
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = (
        "import sys, time, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import torch, ldpc_lib_amd as L\n"
        "from ldpc_testlib import MS_DEC, awgn_llr, load_base_matrix, relift\n"
        "H = relift(load_base_matrix(), 64).copy(); H[H > 0] = (H[H > 0] * 5 + 1) %% 64\n"
        "t0 = time.perf_counter(); dec = L.LdpcHip(MS_DEC, H, 64); t = time.perf_counter() - t0\n"
        "d, it, _ = dec.decode_host(awgn_llr(H, 64, 2.0, 3, 16), 50)\n"
        "print(dec.kernel_name, '|', t, '|', it.tolist(), '|', int(d.sum()))\n") % (root, os.path.join(root, "tests"))
    env = dict(os.environ, LDPC_HIP_CACHE_DIR=str(tmp_path))
    out1 = subprocess.check_output([sys.executable, "-c", prog], env=env, text=True).strip().split("\n")[-1].split("|")
    files = [f for f in os.listdir(tmp_path) if f.endswith(".hsaco")]
    assert "hiprtc" in out1[0] and len(files) == 1
    out2 = subprocess.check_output([sys.executable, "-c", prog], env=env, text=True).strip().split("\n")[-1].split("|")
    assert out2[2:] == out1[2:] and "hiprtc" in out2[0]
    assert float(out2[1]) < 0.5 * float(out1[1]) or float(out2[1]) < 0.3      # no compilation the second time
    assert [f for f in os.listdir(tmp_path) if f.endswith(".hsaco")] == files


@pytest.mark.parametrize("dec_id,first_tier", [(MS_DEC, "ms_flood_m64_kernel"), (TASP_DEC, "tasp_global_kernel"), (LMS_DEC, "lms_layered_kernel")])
def test_background_specialisation_changes_tier_in_flight(L, torch, tmp_path, monkeypatch, dec_id, first_tier):
    """LDPC_HIP_JIT=async (what ldpc::bp_simulation_t selects): ldpc_hip_open of an unseen code does not wait for hiprtc -- the
    context starts on its table-driven / shape-unlimited kernel and moves to the code-specialised instance once the background
    compile has delivered it; both tiers return the oracle's bits, a second context gets the instance from the process cache."""
    import time
    monkeypatch.setenv("LDPC_HIP_JIT", "async")
    monkeypatch.setenv("LDPC_HIP_CACHE_DIR", str(tmp_path))
    H = relift(load_base_matrix(), 64).copy()
    H[H > 0] = (H[H > 0] * 11 + 2 + dec_id) % 64          # a code no other test has compiled in this process
    maxit = 15 if dec_id == TASP_DEC else 50
    llr = awgn_llr(H, 64, 1.8, 31 + dec_id, 96)
    d_ref, it_ref, _ = Oracle(H, 64).decode(dec_id, llr, maxit, 0)
    x = torch.from_numpy(llr).cuda()
    t0 = time.perf_counter()
    with L.LdpcHip(dec_id, H, 64) as dec:
        t_open = time.perf_counter() - t0
        assert first_tier in dec.kernel_name, dec.kernel_name
        hard, iters, _ = dec.decode(x, maxit)
        assert first_tier in dec.last_launch() or "hiprtc" in dec.kernel_name
        assert np.array_equal(iters.cpu().numpy(), it_ref) and np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref))
        t1 = time.perf_counter()
        while "hiprtc" not in dec.kernel_name and time.perf_counter() - t1 < 180:
            time.sleep(0.2)
        assert "hiprtc" in dec.kernel_name, dec.kernel_name
        t_jit = time.perf_counter() - t1
        hard, iters, _ = dec.decode(x, maxit)
        assert "hiprtc" in dec.last_launch()
        assert np.array_equal(iters.cpu().numpy(), it_ref) and np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref))
    # (that ldpc_hip_open did not wait for the compile is what `first_tier in dec.kernel_name` right after it shows; no wall-clock
    # assertion: the first background job also loads hiprtc and its compiler, which takes a second on a cold box)
    del t_open, t_jit
    with L.LdpcHip(dec_id, H, 64) as dec:
        assert "hiprtc" in dec.kernel_name                            # process cache


def test_process_may_exit_while_a_background_compile_is_in_flight(L, tmp_path):
    """Regression (round 2, gpurun_out/s7: SIGSEGV at exit): a process that ends while the hiprtc worker still compiles must leave
    with its own exit code -- the worker's exit handler waits for the compile in flight while hiprtc's compiler is still alive.
    Three fresh processes: one exits right after ldpc_hip_open, one after a decode on the first tier, one leaves the context open."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np, torch
import ldpc_lib_amd as L
from ldpc_testlib import load_base_matrix, relift, awgn_llr, BP_DEC
mode = sys.argv[1]
H = relift(load_base_matrix(), 64).copy()
H[H > 0] = (H[H > 0] * 7 + 3 + len(mode)) % 64
torch.zeros(1).cuda()                                   # the HIP context exists before the open, so the open itself is quick
dec = L.LdpcHip(BP_DEC, H, 64)                          # bp_body: the longest compile of all bodies (tens of seconds)
if mode == "decode":
    dec.decode(torch.from_numpy(awgn_llr(H, 64, 2.0, 1, 16)).cuda(), 15)
    torch.cuda.synchronize()
inflight = "hiprtc" not in dec.kernel_name              # the instance is still being compiled
if mode != "leak":
    dec.close()
print("leaving", mode, "inflight" if inflight else "done", flush=True)
sys.exit(7)
"""
    seen_inflight = 0
    for mode in ("open", "decode", "leak"):
        env = dict(os.environ, LDPC_HIP_JIT="async", LDPC_HIP_CACHE_DIR=str(tmp_path / mode))
        p = subprocess.run([sys.executable, "-c", script.format(root=root), mode], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 7 and "leaving " + mode in p.stdout, (mode, p.returncode, p.stdout[-500:], p.stderr[-1500:])
        seen_inflight += "inflight" in p.stdout
    assert seen_inflight >= 2, "the compile was never in flight at exit: the test did not exercise what it is for"


def test_contexts_closed_before_their_compile_are_dropped(L, torch, tmp_path, monkeypatch):
    """A code search opens and closes a context per candidate: queued background compiles of closed contexts are skipped."""
    import time
    monkeypatch.setenv("LDPC_HIP_JIT", "async")
    monkeypatch.setenv("LDPC_HIP_CACHE_DIR", str(tmp_path))
    base = relift(load_base_matrix(), 64)
    t0 = time.perf_counter()
    for k in range(12):
        H = base.copy()
        H[H > 0] = (H[H > 0] * 13 + 5 + k) % 64
        with L.LdpcHip(MS_DEC, H, 64) as dec:
            s = dec.simulate(2.0, 50, seed=k, first_frame=0, B=2048)
            assert s["frames"] == 2048
    assert time.perf_counter() - t0 < 30.0          # 12 synchronous hiprtc compiles would take longer than this by themselves
    # at most the compiles that were already running when their context closed reach the cache directory
    time.sleep(0.5)
    assert len([f for f in os.listdir(tmp_path) if f.endswith(".hsaco")]) <= 12
