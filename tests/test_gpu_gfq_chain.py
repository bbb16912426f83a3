"""The GF(q) transmit chain on the GPU, exact equality everywhere: the device encoder against the golden sets of the compiled upstream
encode_NBQCLDPC and against the numpy model over q x M x (rh, nh) x scheme; its refusals; the q-ary channel against the scalar model's
golden sets (uint64 images) and its Philox noise under batch splits; symbol-error counting against the model; ldpc_hip_simulate_gfq
against the four primitives composed by hand.  NaN sign / payload is the one thing not compared (see tests/test_gpu_gfq.py)."""
import math
import os

import numpy as np
import pytest

import gfq_chain_model as cm
from gfq_model import GfqModel
from ldpc_testlib import assert_bits_equal

pytestmark = pytest.mark.gpu

ENC_GOLDENS = ("gf4_m1_w2", "gf16_m8_xox", "gf16_m8_oxo_n2c2", "gf64_m67_oxo", "gf256_m128_xox", "gf16_m67_w2", "gf16_m8_broken")
B_ENC = 37


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _golden(name):
    return np.load(os.path.join(cm.CHAIN_GOLDEN_DIR, name + ".npz"))


@pytest.fixture(scope="module")
def sim_code():
    g = _golden("chain_sim_gf16_m8")
    return g


@pytest.mark.parametrize("name", ENC_GOLDENS)
def test_encoder_equals_the_compiled_reference(L, torch, name):
    g = _golden("chain_enc_" + name)
    with L.LdpcHipGfq(int(g["q_bits"]), g["hb"], g["hc"], int(g["M"]), int(g["ncols2convert"])) as dec:
        assert dec.k == g["msg"].shape[1]
        cw, ok = dec.encode(g["msg"])                               # numpy in, numpy out
        assert np.array_equal(cw, g["codeword"]) and np.array_equal(ok, g["ok"])
        cw_d, ok_d = dec.encode(torch.from_numpy(g["msg"]).cuda())  # device tensors
        assert np.array_equal(cw_d.cpu().numpy(), g["codeword"]) and np.array_equal(ok_d.cpu().numpy(), g["ok"])
        with pytest.raises(ValueError):
            dec.encode(np.full((1, dec.k), dec.q, dtype=np.int16))


@pytest.mark.parametrize("rh,nh", [(2, 4), (3, 6), (4, 8)])
@pytest.mark.parametrize("M", [1, 8, 67, 128])
@pytest.mark.parametrize("q_bits", [2, 4, 6, 8])
def test_encoder_equals_the_model(L, torch, q_bits, M, rh, nh):
    rng = np.random.RandomState(1000 * q_bits + 10 * M + rh)
    q = 1 << q_bits
    for scheme in cm.SCHEMES if rh >= 3 else ("w2",):
        hb, hc = cm.make_code(rng, q_bits, rh, nh, M, scheme)
        K = (nh - rh) * M
        a = rng.randint(0, q, (B_ENC, K)).astype(np.int16)
        a[0] = 0
        b = rng.randint(0, q, (B_ENC, K)).astype(np.int16)
        with L.LdpcHipGfq(q_bits, hb, hc, M) as dec:
            cw_a, ok_a = dec.encode(a)
            cw_b, _ = dec.encode(b)
            cw_ab, _ = dec.encode(a ^ b)
        want, ok = cm.encode(q_bits, hb, hc, M, a)
        assert np.array_equal(cw_a, want) and np.array_equal(ok_a, ok) and ok.all(), scheme
        assert not cw_a[0].any()                                     # zero message -> zero word
        assert np.array_equal(cw_a ^ cw_b, cw_ab)                    # linear over GF(q)
        assert not cm.syndrome(q_bits, hb, hc, M, cw_a).any()        # the independent syndrome
        assert np.array_equal(cw_a[:, :K], a)                        # systematic


def test_broken_dual_diagonal_reports_bad_coding_with_upstreams_words(L, torch):
    rng = np.random.RandomState(5)
    hb, hc = cm.make_code(rng, 4, 4, 8, 8, "oxo", break_diagonal=True)
    msg = rng.randint(0, 16, (B_ENC, 32)).astype(np.int16)
    msg[3] = 0
    with L.LdpcHipGfq(4, hb, hc, 8) as dec:
        cw, ok = dec.encode(msg)
    want, ok_m = cm.encode(4, hb, hc, 8, msg)
    assert np.array_equal(cw, want) and np.array_equal(ok, ok_m)
    assert ok[3] == 1 and not ok.all()
    assert np.array_equal(cm.syndrome(4, hb, hc, 8, cw).any(axis=1), ok == 0)


def _refusal_cases():
    rng = np.random.RandomState(9)
    hb, hc = cm.make_code(rng, 4, 4, 8, 8, "xox")
    hb2, hc2 = cm.make_code(rng, 4, 2, 4, 8, "w2")
    cases = {}

    def case(name, rule, words, edit, base=(hb, hc), n2c=0):
        b, c = base[0].copy(), base[1].copy()
        edit(b, c)
        cases[name] = (b, c, n2c, rule, words)

    def set_(arr, i, j, v):
        arr[i, j] = v

    case("nh_le_rh", "nh <= rh", "nh = 4 <= rh = 4", lambda b, c: None, base=(hb[:, :4].copy(), np.where(hb[:, :4] >= 0, 3, -1).astype(np.int16)))
    case("coefficient", "coefficient", "1421", lambda b, c: set_(c, 0, 0, 1) or set_(b, 0, 0, 0), n2c=1)   # alog[15] = 0 after conversion
    cases["coefficient"][1][:, 0] = np.where(cases["coefficient"][0][:, 0] >= 0, 15, -1)
    case("wrong_weight", "wrong weight", "1493", lambda b, c: set_(b, 0, 4, -1) or set_(b, 2, 4, -1))
    case("empty_first", "empty (0, nh-rh)", "(0, nh-rh)", lambda b, c: set_(b, 0, 4, -1) or set_(b, 1, 4, 0) or set_(c, 1, 4, 3))
    case("empty_last", "empty (rh-1, nh-rh)", "(rh-1, nh-rh)", lambda b, c: set_(b, 3, 4, -1) or set_(b, 1, 4, 0) or set_(c, 1, 4, 3))
    case("empty_diagonal", "empty (j, nh-rh+1+j)", "(j, nh-rh+1+j) = (1, 6)", lambda b, c: set_(b, 1, 6, -1) or set_(b, 1, 0, 0) or set_(c, 1, 0, 1))
    case("w3_end_coefficients", "weight 3, end coefficients differ", "1477", lambda b, c: set_(c, 3, 4, c[0, 4] % 15 + 1))
    case("w2_equal", "weight 2, equal coefficients", "1461", lambda b, c: set_(c, 1, 2, c[0, 2]), base=(hb2, hc2))
    case("w2_shift", "weight 2, non-zero shifts", "1467", lambda b, c: set_(b, 1, 2, 3), base=(hb2, hc2))
    return cases


REFUSALS = _refusal_cases()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_encoder_refusals_name_the_rule_and_leave_the_decoder_usable(L, torch, name):
    hb, hc, n2c, rule, words = REFUSALS[name]
    with L.LdpcHipGfq(4, hb, hc, 8, n2c) as dec:
        with pytest.raises(cm.EncodeRefused) as model:
            cm.encode(4, hb, dec.coefficients(), 8, np.zeros((1, max(dec.k, 1)), dtype=np.int64)[:, :max(dec.k, 0) or 1])
        assert model.value.rule == rule
        for _ in range(2):   # decided once, cached
            with pytest.raises(L.LdpcHipError) as e:
                dec.encode(np.zeros((2, dec.k), dtype=np.int16))
            assert "code -2" in str(e.value) and words in str(e.value), str(e.value)
        with pytest.raises(L.LdpcHipError):
            dec.simulate(3.0, 5, 4, seed=1, random_messages=True)
        soft = dec.channel(sigma=0.2, seed=1, B=3)
        qhard, iters, _ = dec.decode(soft, 10)
        assert not qhard.cpu().numpy().any() and (iters.cpu().numpy() >= 0).all()
        assert dec.simulate(8.0, 10, 4, seed=1, random_messages=False)[3] == 4


def test_rh_below_two_is_refused_by_the_encoder(L, torch):
    hb = np.array([[0, 1, 0]], dtype=np.int16)
    hc = np.array([[1, 2, 3]], dtype=np.int16)
    with L.LdpcHipGfq(4, hb, hc, 8) as dec:
        with pytest.raises(L.LdpcHipError) as e:
            dec.encode(np.zeros((1, dec.k), dtype=np.int16))
        assert "code -2" in str(e.value) and "rh = 1" in str(e.value)


@pytest.mark.parametrize("tag", ["gf4", "gf16", "gf64", "overflow"])
def test_channel_with_given_noise_equals_the_model(L, torch, tag):
    g = _golden("chain_channel_" + tag)
    q_bits = int(g["q_bits"])
    hb, hc = cm.make_code(np.random.RandomState(1), q_bits, 4, 8, 8, "xox")
    with L.LdpcHipGfq(q_bits, hb, hc, 8) as dec:
        assert dec.N == 64
        if tag != "overflow":
            assert dec.sigma(2.7) == float(g["sigma"])
        soft = dec.channel(codeword=g["codeword"], noise=g["noise"], sigma=float(g["sigma"])).cpu().numpy()
    assert_bits_equal(soft, g["soft"], tag, nan_ok=True)
    assert bool(np.isnan(soft).any()) == (tag == "overflow")


@pytest.mark.parametrize("q_bits", [2, 4, 6, 8])
def test_channel_philox_noise_is_keyed_by_the_global_frame(L, torch, q_bits):
    hb, hc = cm.make_code(np.random.RandomState(2), q_bits, 3, 6, 5, "oxo")
    with L.LdpcHipGfq(q_bits, hb, hc, 5) as dec:
        sigma = dec.sigma(2.7)
        one = dec.channel(sigma=sigma, seed=11, first_frame=100, B=24)
        again = dec.channel(sigma=sigma, seed=11, first_frame=100, B=24)
        parts = torch.cat([dec.channel(sigma=sigma, seed=11, first_frame=100, B=7), dec.channel(sigma=sigma, seed=11, first_frame=107, B=17)])
        other = dec.channel(sigma=sigma, seed=12, first_frame=100, B=24)
        zero = dec.channel(codeword=np.zeros((24, dec.N), dtype=np.int16), sigma=sigma, seed=11, first_frame=100)
        assert torch.equal(one, again) and torch.equal(one, parts) and torch.equal(one, zero)
        assert not torch.equal(one, other) and not torch.equal(one[0], one[1])
        s = one.cpu().numpy()
        assert np.isfinite(s).all() and np.abs(s.sum(axis=1) - 1).max() < 1e-12
        # the all-zero word was sent: a symbol's most likely value is 0 exactly when all q_bits received bits are negative, which
        # has probability p = (1 - Q(1 / sigma)) ** q_bits (0.84, 0.70, 0.58, 0.49 for q_bits 2, 4, 6, 8 at 2.7 dB and rate 1/2);
        # the share over the n = 24 * N independent symbols lies within 5 standard deviations of p
        p = (1.0 - 0.5 * math.erfc(1.0 / sigma / math.sqrt(2.0))) ** q_bits
        n = 24 * dec.N
        share = (s.argmax(axis=1) == 0).mean()
        print(f"q_bits {q_bits}: share of symbols decided 0 = {share:.4f}, expected {p:.4f} +- {5 * math.sqrt(p * (1 - p) / n):.4f}")
        assert abs(share - p) < 5 * math.sqrt(p * (1 - p) / n)


def test_counting_equals_the_model(L, torch):
    rng = np.random.RandomState(3)
    hb, hc = cm.make_code(rng, 4, 3, 6, 11, "xox")
    with L.LdpcHipGfq(4, hb, hc, 11) as dec:
        N, R = dec.N, dec.R
        for B in (1, 300):
            cw = rng.randint(0, 16, (B, N)).astype(np.int16)
            qh = cw.copy()
            iters = rng.randint(-15, 15, B).astype(np.int32)
            for f in range(B):
                kind = f % 5   # none / parity only / information only / both / converged but wrong
                if kind in (1, 3):
                    qh[f, rng.randint(0, R)] ^= 1 + rng.randint(0, 15)
                if kind in (2, 3, 4):
                    qh[f, rng.randint(R, N, 3)] ^= 5
                if kind == 4:
                    iters[f] = abs(int(iters[f]))
            if B == 1:
                qh[0, R] ^= 1
            for codeword in (cw, None):
                q_in = qh if codeword is not None else qh ^ cw
                want, info = cm.count(q_in, codeword, iters, R)
                cnt, finfo = dec.count_errors(q_in, codeword, iters)
                assert cnt.cpu().tolist() == want and np.array_equal(finfo.cpu().numpy(), info)
                cnt2, _ = dec.count_errors(torch.from_numpy(q_in).cuda(), None if codeword is None else torch.from_numpy(codeword).cuda(),
                                           torch.from_numpy(iters).cuda(), counters=cnt)   # accumulation over two calls
                assert cnt2 is cnt and cnt.cpu().tolist() == [2 * v for v in want]
            if B == 300:
                assert want[1] > want[2] > 0 and want[0] > 0


def _by_hand(dec, torch, snr, maxiter, seed, first_frame, B, random_messages):
    cw = None
    if random_messages:
        msg = cm.messages(dec.q, dec.k, seed, first_frame, B)
        cw, ok = dec.encode(torch.from_numpy(msg).cuda())
        assert bool(ok.all())
    soft = dec.channel(codeword=cw, sigma=dec.sigma(snr), seed=seed, first_frame=first_frame, B=B)
    qhard, iters, _ = dec.decode(soft, maxiter)
    cnt, _ = dec.count_errors(qhard, cw, iters)
    return cnt.cpu().tolist()


@pytest.mark.parametrize("random_messages", [False, True])
def test_simulate_equals_the_primitives_composed_by_hand(L, torch, sim_code, monkeypatch, random_messages):
    g = sim_code
    with L.LdpcHipGfq(4, g["hb"], g["hc"], 8) as dec:
        for snr in (1.5, 4.0):
            want = _by_hand(dec, torch, snr, 15, 21, 1000, 48, random_messages)
            assert want[3] == 48
            assert dec.simulate(snr, 15, 48, seed=21, first_frame=1000, random_messages=random_messages) == want
            a = dec.simulate(snr, 15, 20, seed=21, first_frame=1000, random_messages=random_messages)
            b = dec.simulate(snr, 15, 28, seed=21, first_frame=1020, random_messages=random_messages)
            assert [x + y for x, y in zip(a, b)] == want
            for var, val in (("LDPC_HIP_GFQ_SLOTS", "1"), ("LDPC_HIP_GFQ_PIECE", "5")):
                monkeypatch.setenv(var, val)
                assert dec.simulate(snr, 15, 48, seed=21, first_frame=1000, random_messages=random_messages) == want
                monkeypatch.delenv(var)
        low = _by_hand(dec, torch, 1.5, 15, 21, 1000, 48, random_messages)
        assert low[1] > 0, "the low SNR point is there to exercise the error counters"


def test_chain_on_the_golden_noise_reports_the_models_iterations(L, torch, sim_code):
    g = sim_code
    with L.LdpcHipGfq(4, g["hb"], g["hc"], 8) as dec:
        cw, ok = dec.encode(torch.from_numpy(g["msg"]).cuda())
        assert bool(ok.all()) and np.array_equal(cw.cpu().numpy(), g["codeword"])
        soft = dec.channel(codeword=cw, noise=g["noise"], sigma=dec.sigma(float(g["snr"])))
        qhard, iters, _ = dec.decode(soft, int(g["maxiter"]))
        cnt, info = dec.count_errors(qhard, cw, iters)
        assert cnt.cpu().tolist() == [0, 0, 0, 32, int(g["iters_sum"])] and not info.cpu().numpy().any()
