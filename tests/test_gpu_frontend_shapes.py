"""GPU: the kernels around the decoders (csrc/ldpc_frontend.hpp, csrc/ldpc_encode.hpp) away from the (2048, 1024) shape, each against
the plain CPU references of tests/frontend_twin.py or the oracle.

  code A  16 x 33, M = 9    N = 297 (odd: the scalar store branch, the BPSK tail guard)   R = 144 = 4 * 32 + 16   10 packed words
  code B  16 x 30, M = 7    N = 210 (even, no multiple of 4 or 8: padded last symbols)    R = 112 = 3 * 32 + 16    7 packed words
  code C  A's H,   M = 67   N = 2211                                                       R = 1072 = 33 * 32 + 16  70 packed words
  code D  3 x 7,   M = 5    N = 35                                                         R = 15 (mask inside word 0) 2 packed words
  code E  16 x 32, M = 64   the usual shape, only where the test is about a grid cap or about R being a multiple of 32

A and B are the base matrices of tests/golden/interleavers.npz, so the interleaver maps the twin uses are upstream's own recorded
ones while the device builds its maps from set_interleaver(mode, block, step).  One context per code serves the whole module.
"""
import numpy as np
import pytest

from frontend_twin import (SATURATION_CASES, T_CUT, chain_twin, code_a, code_b, code_c, code_d, count_twin, random_info_twin,
                           recorded_interleavers, saturation_reference)
from ldpc_testlib import (IMS_DEC, MS_DEC, SP_DEC, Oracle, _as_double_p, adversarial_llr, load_base_matrix, oracle_lib, pack_bits, relift,
                          syndrome_np)

pytestmark = pytest.mark.gpu

FIRST = 4_000_000_123                # beyond 2^31, and 1 modulo 3: (first_frame + f) % ncw differs from f % ncw
SNR_OF_MOD = (1.5, 2.0, 6.0, 10.0, 14.0)


def code_e():
    return relift(load_base_matrix(), 64), 64


CODES = {"A": code_a, "B": code_b, "C": code_c, "D": code_d, "E": code_e}
MAPS = {"A": ((16, 33), 9), "B": ((16, 30), 7)}


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def ctx(L, torch):
    """name -> open context, opened at first use and kept for the module: 'A' .. 'E' with min-sum, 'A/sp' and 'B/sp' with a
    probability-type decoder (punctured value 0)"""
    opened = {}

    def get(name):
        if name not in opened:
            H, M = CODES[name[0]]()
            opened[name] = L.LdpcHip(SP_DEC if name.endswith("/sp") else MS_DEC, H, M)
        dec = opened[name]
        dec.set_codewords(None)
        dec.set_interleaver(0)
        return dec
    yield get
    for dec in opened.values():
        dec.close()


def _nan(torch, B, N):
    return torch.full((B, N), float("nan"), dtype=torch.float64, device="cuda")


def _rows(seed, count, N):
    """random bit rows as sent words: the channel and the count store them as given, they need not satisfy H"""
    return np.random.RandomState(seed).randint(0, 2, size=(count, N)).astype(np.uint8)


# ---- a. channel against the twin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("code", ["A", "B"])
def test_channel_equals_the_twin_off_the_usual_shape(ctx, torch, code, mod):
    """Every modulation without an interleaver and with upstream's recorded maps of modes 1..4, 0 and 2 punctured blocks, three sent
    rows, first_frame beyond 2^31, LLR-type and probability-type punctured value.  The output starts as NaN: an element the kernel
    does not write fails the comparison."""
    H, M = CODES[code]()
    N = H.shape[1] * M
    maps, _ = recorded_interleavers(*MAPS[code])
    h = 1 if mod <= 1 else mod
    cws = _rows(100 + mod, 3, N)
    B, seed, snr = 5, (3 << 32) | 19, SNR_OF_MOD[mod]
    perms = [None] + [(mode,) + maps[(h, mode)] for mode in (1, 2, 3, 4)]
    for name, punct_val in ((code, 0.5), (code + "/sp", 0.0)):
        dec = ctx(name)
        assert dec.N == N
        dec.set_codewords(cws)
        for perm in perms:
            direct = inverse = None
            dec.set_interleaver(0)
            if perm is not None:
                mode, bs, st, direct, inverse = perm
                dec.set_interleaver(mode, bs, st)
            for punct in (0, 2):
                got = dec.channel_llr(snr, seed, FIRST, B, modulation=mod, punctured_blocks=punct, out=_nan(torch, B, N)).cpu().numpy()
                ref = chain_twin(H, M, cws, FIRST, B, seed, snr, mod, punct, direct, inverse, punct_val)
                np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-9, err_msg=f"{name} mod {mod} perm {perm and perm[:3]} punct {punct}")
                if punct:
                    assert (got[:, N - 2 * M:] == punct_val).all()


@pytest.mark.parametrize("mod", [0, 3])
def test_channel_of_the_all_zero_word_on_code_c(ctx, torch, mod):
    H, M = code_c()
    dec = ctx("C")
    N, B, seed = dec.N, 5, (3 << 32) | 19
    assert N == 2211
    got = dec.channel_llr(SNR_OF_MOD[mod], seed, FIRST, B, modulation=mod, out=_nan(torch, B, N)).cpu().numpy()
    ref = chain_twin(H, M, None, FIRST, B, seed, SNR_OF_MOD[mod], mod, 0, None, None, 0.5)
    np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-9)


# ---- b. saturating demapper --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod,snr", SATURATION_CASES)
def test_saturated_demapper_outputs_are_exactly_the_cut_off(ctx, torch, mod, snr):
    """At these Eb/N0 0.42, 0.50 and 0.56 of the reference LLRs are +T or -T (the p0 == 0 / p1 == 0 branches of llr_or_p): there the
    device value must be that value, not merely close to it."""
    cws, first, B, seed, ref = saturation_reference(mod, snr)
    share = (np.abs(ref) == T_CUT).mean()
    assert 0.2 <= share <= 0.8 and not np.isnan(ref).any(), share
    dec = ctx("A")
    dec.set_codewords(cws)
    got = dec.channel_llr(snr, seed, first, B, modulation=mod, out=_nan(torch, B, dec.N), T=T_CUT).cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-9)
    sat = np.abs(ref) == T_CUT
    assert np.array_equal(got[sat], ref[sat])
    assert np.array_equal(np.abs(got) == T_CUT, sat)


# ---- c. grid-stride wrap of the channel ----------------------------------------------------------------------------------------------
def test_channel_beyond_its_grid_cap(ctx, torch):
    """1030 BPSK frames of N = 2048 are 1030 * 1024 units, more than the 4096 * 256 lanes of the capped grid: the last six frames are
    written by the second trip of the grid-stride loop."""
    H, M = code_e()
    dec = ctx("E")
    N, B, seed, snr = 2048, 1030, (5 << 32) | 77, 1.4
    assert B * (N // 2) > 4096 * 256
    cws = _rows(7, 3, N)
    dec.set_codewords(cws)
    out = dec.channel_llr(snr, seed, FIRST, B, out=_nan(torch, B, N))
    ref = chain_twin(H, M, cws, FIRST, B, seed, snr, 0, 0, None, None, 0.5)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-11, atol=1e-11)
    tail = dec.channel_llr(snr, seed, FIRST + 1024, 6, out=_nan(torch, 6, N))
    assert torch.equal(tail, out[1024:])


# ---- d. error count on synthetic decisions -------------------------------------------------------------------------------------------
def _synthetic_errors(rng, B, N, R):
    """error masks [B, N] cycling: none, parity part only, bit R - 1, bit R, bit N - 1, random; iteration counts in [-50, 50] with
    zeros and negatives on errored frames"""
    err = np.zeros((B, N), dtype=np.uint8)
    for f in range(B):
        kind = f % 6
        if kind == 1:
            err[f, rng.randint(0, R, size=3)] = 1
        elif kind == 2:
            err[f, R - 1] = 1
        elif kind == 3:
            err[f, R] = 1
        elif kind == 4:
            err[f, N - 1] = 1
        elif kind == 5:
            err[f] = rng.rand(N) < 0.1
    iters = rng.randint(-50, 51, size=B).astype(np.int32)
    iters[1::12] = 0
    iters[2::12] = -7
    iters[5::18] = -50
    return err, iters


@pytest.mark.parametrize("code", ["A", "B", "C", "D", "E"])
def test_error_count_equals_the_twin_on_synthetic_decisions(ctx, torch, code):
    """No decoder runs: packed decisions with known errors against count_twin, counters and per-frame records, for the all-zero word
    and three sent rows, first_frame 0 and beyond 2^31, B from one frame to more than the 2048 * 4 frames of the capped grid.
    Code E has R = 1024, a multiple of 32: the word whose last bit is R - 1 is all parity."""
    dec = ctx(code)
    N, R = dec.N, dec.R
    assert dec.hard_words == (N + 31) // 32
    rng = np.random.RandomState(len(code) + N)
    big = 8192 + 7
    err, iters = _synthetic_errors(rng, big, N, R)
    cws = _rows(N, 3, N)
    for ncw in (0, 3):
        dec.set_codewords(cws if ncw else None)
        for first in (0, FIRST):
            sent = cws[(first + np.arange(big)) % 3] if ncw else None
            bits = err ^ sent if ncw else err
            words = pack_bits(bits)
            for B in (1, 3, 4, 5, big):
                if code == "C" and B == 5:
                    assert dec.hard_words == 70
                hard = torch.from_numpy(words[:B].view(np.int32).copy()).cuda()
                it = torch.from_numpy(iters[:B].copy()).cuda()
                want, want_info = count_twin(bits[:B], iters[:B], R, None if sent is None else sent[:B])
                cnt, info = dec.count_errors(hard, it, want_frame_info=True, first_frame=first)
                assert cnt.cpu().tolist() == want, (code, ncw, first, B)
                assert np.array_equal(info.cpu().numpy(), want_info), (code, ncw, first, B)
                if B in (5, big):
                    again, none = dec.count_errors(hard, it, counters=cnt, first_frame=first)      # accumulates, no records wanted
                    assert none is None and again is cnt and cnt.cpu().tolist() == [2 * v for v in want]
            assert want[1] > 0 and want[0] > 0 and want[2] < want[1]


# ---- e. codeword tables made on the device --------------------------------------------------------------------------------------------
def test_device_made_codeword_tables_equal_their_twins(ctx, torch):
    """set_random_codewords on code A (N = 297, K = 153: the second Philox group holds 25 bits): the byte table read back through the
    BPSK channel at 40 dB, the transmit-order table through an interleaver and 16-QAM (75 symbols, the last one padded), the packed
    table through count_errors -- against random_info_twin and the host encoder."""
    from ldpc_lib_amd.binding import encode
    H, M = code_a()
    maps, _ = recorded_interleavers(*MAPS["A"])
    dec = ctx("A")
    N, K, seed, ncw, first = dec.N, dec.N - dec.R, (9 << 32) | 5, 5, 4_000_000_002
    assert N % 2 == 1 and K % 128 == 25
    dec.set_random_codewords(seed, ncw)
    info = random_info_twin(seed, 0, ncw, K)
    table = np.stack([encode(H, M, row) for row in info])
    assert not syndrome_np(H, M, table).any() and table[:, N - 1].any() and not table[:, N - 1].all()
    sent = table[(first + np.arange(10)) % ncw]
    llr = dec.awgn_llr(40.0, 3, first, 10, out=_nan(torch, 10, N)).cpu().numpy()
    assert not np.isnan(llr).any()
    bits = (llr < 0).astype(np.uint8)
    assert np.array_equal(bits[:5], bits[5:])
    assert not syndrome_np(H, M, bits).any()
    assert np.array_equal(bits[:, dec.R:], info[(first + np.arange(10)) % ncw])
    assert np.array_equal(bits, sent)
    # transmit order through the direct map, back through the inverse scatter, ntx = 300 > N
    bs, st, _, _ = maps[(2, 3)]
    dec.set_interleaver(3, bs, st)
    llr = dec.awgn_llr(40.0, 3, first, 10, modulation=2, out=_nan(torch, 10, N)).cpu().numpy()
    assert not np.isnan(llr).any() and np.array_equal((llr < 0).astype(np.uint8), sent)
    # the packed table of the error count, last partial word included
    hard = torch.from_numpy(pack_bits(sent).view(np.int32).copy()).cuda()
    it = torch.from_numpy(np.arange(-4, 6, dtype=np.int32)).cuda()
    cnt, rec = dec.count_errors(hard, it, want_frame_info=True, first_frame=first)
    want, want_rec = count_twin(sent, np.arange(-4, 6), dec.R, sent)
    assert want == [0, 0, 0, 10, 25] and cnt.cpu().tolist() == want and np.array_equal(rec.cpu().numpy(), want_rec)
    dec.set_random_codewords(0, 0)


# ---- f. IMS quantiser scale off the tile grid -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,expect", [({}, "ims_small_body instance (hiprtc)"), ({"LDPC_HIP_FORCE_GLOBAL": "1"}, "ims_global_kernel")],
                         ids=["code-specialised", "shape-unlimited"])
def test_ims_scale_off_the_tile_grid(L, torch, monkeypatch, env, expect):
    """ims_coef_kernel walks [64 frames][64 values] tiles: N = 297 ends 41 values into its fifth tile, B = 70 six frames into its
    second block.  Both tiers that take their scale from it, bit for bit against the oracle."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    H, M = code_a()
    llr, _ = adversarial_llr(H, M, 11)
    llr = llr[np.arange(70) % len(llr)]
    d_ref, it_ref, _ = Oracle(H, M).decode(IMS_DEC, llr, 20, 0)
    with L.LdpcHip(IMS_DEC, H, M) as dec:
        assert dec.kernel_name == expect, dec.kernel_name
        hard, iters, _ = dec.decode(torch.from_numpy(llr).cuda(), 20)
        torch.cuda.synchronize()
        assert dec.last_launch() == expect, dec.last_launch()
        assert np.array_equal(iters.cpu().numpy(), it_ref)
        assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref))


# ---- g. pass boundary ------------------------------------------------------------------------------------------------------------------
def test_simulate_across_the_pass_boundary(ctx, torch):
    """sim_enqueue cuts a pass at 65536 frames: 65536 + 37 frames of code D in one call == channel, decode and count over the same
    range in one composed call == two calls split at the boundary."""
    from ldpc_lib_amd.binding import encode
    H, M = code_d()
    dec = ctx("D")
    B, snr, seed, maxiter = 65536 + 37, 3.0, (2 << 32) | 11, 20
    cws = np.stack([encode(H, M, row) for row in _rows(3, 3, dec.N - dec.R)])          # codewords: most frames decode to what was sent
    assert not syndrome_np(H, M, cws).any() and 65536 % 3
    dec.set_codewords(cws)
    llr = dec.channel_llr(snr, seed, FIRST, B)
    hard, iters, _ = dec.decode(llr, maxiter)
    cnt, _ = dec.count_errors(hard, iters, first_frame=FIRST)
    want = cnt.cpu().tolist()
    print("composed counters over the pass boundary:", want)
    assert want[3] == B and 0.01 * B < want[1] < 0.5 * B and want[2] < want[1]
    keys = ("nse", "nde", "nue", "frames", "sum_abs_iters")
    s = dec.simulate(snr, maxiter, seed, FIRST, B)
    assert [s[k] for k in keys] == want
    a = dec.simulate(snr, maxiter, seed, FIRST, 65536)
    b = dec.simulate(snr, maxiter, seed, FIRST + 65536, 37)
    assert [a[k] + b[k] for k in keys] == want


# ---- h. function-level kernels past their grid cap -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(1, 1), (1, 257), (3704, 297)])
def test_permute_equals_numpy_take(L, torch, B, N):
    from ldpc_lib_amd.binding import permute
    rng = np.random.RandomState(B + N)
    if B > 1:
        assert B * N >= 1_100_000 > 4096 * 256
    x = rng.randn(B, N)
    index_map = rng.permutation(N).astype(np.int32)
    got = permute(torch.from_numpy(x).cuda(), torch.from_numpy(index_map).cuda()).cpu().numpy()
    assert np.array_equal(got, np.take(x, index_map, axis=1))


@pytest.mark.parametrize("ns", [1, 257, 1_100_000])
def test_qam16_mapper_and_demapper_equal_the_oracle(L, torch, ns):
    from ldpc_lib_amd.binding import qam_demod, qam_modulate
    rng = np.random.RandomState(ns)
    bits = rng.randint(0, 2, size=(ns, 4)).astype(np.uint8)
    want = np.zeros((ns, 2))
    flat = np.ascontiguousarray(bits.ravel().astype(np.float64))
    oracle_lib().orc_qam_modulate(16, _as_double_p(flat), flat.size, _as_double_p(want.reshape(-1)))
    got = qam_modulate(torch.from_numpy(bits).cuda(), 16).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13)
    assert set(np.unique(want)) <= {-3.0, -1.0, 1.0, 3.0}
    x = np.ascontiguousarray(want + 0.8 * rng.randn(ns, 2))
    x[::1000] = 60.0                                   # beyond the cut-off from every level: 0 / 0
    ref = np.zeros((ns, 4))
    oracle_lib().orc_qam_demodulate(16, T_CUT, 0.8, _as_double_p(x.reshape(-1)), ns, _as_double_p(ref.reshape(-1)), 0)
    out = qam_demod(torch.from_numpy(x).cuda(), 16, T_CUT, 0.8, 0).cpu().numpy()
    nan = np.isnan(ref)
    assert nan[::1000].all() and not nan[1:1000].any()
    assert np.array_equal(np.isnan(out), nan)
    np.testing.assert_allclose(out[~nan], ref[~nan], rtol=1e-12, atol=1e-13)
