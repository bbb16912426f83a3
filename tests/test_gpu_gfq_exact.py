"""Exact replay of upstream's q-ary frame loop on the GPU (ldpc_hip_mt_*_gfq, ldpc_hip_frames_gfq_noise_host, LdpcHipGfq.mt_*): the
per-frame records against the golden sets of tests/golden/gfq_exact/ (the harness model of tests/gfq_harness_model.py around the
compiled upstream decoder), for equality -- whole, cut into calls, in pieces, with few slots, after an advance, continued on a second
context, and from Gaussians the host drew; and the refusals, which launch nothing and leave word and generator alone."""
import ctypes as C

import numpy as np
import pytest

import gfq_harness_model as hm
from ldpc_testlib import MS_DEC, load_base_matrix, relift

pytestmark = pytest.mark.gpu

_GOLDEN = {}


def golden(name):
    if name not in _GOLDEN:
        _GOLDEN[name] = {k: v for k, v in hm.load(name).items()}
    return _GOLDEN[name]


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def opened(L, g, seed=None):
    """A context on the case's code with the case's word, the generator at std::mt19937(seed)."""
    dec = L.LdpcHipGfq(int(g["q_bits"]), g["hb"], g["hc"], int(g["M"]))
    dec.set_codeword(g["word"] if int(g["encoded"]) else None)
    dec.mt_set_state(*L.mt19937_state(int(g["seed"]) if seed is None else seed))
    return dec


def frames(dec, g, B):
    return dec.mt_frames(float(g["snr"]), int(g["maxiter"]), B, punctured_blocks=int(g["punctured_blocks"]))


def same(got, g, lo=0, hi=None):
    info, iters = got
    hi = len(g["frame_info"]) if hi is None else hi
    return np.array_equal(info, g["frame_info"][lo:hi]) and np.array_equal(iters, g["iters"][lo:hi])


@pytest.mark.parametrize("name", sorted(hm.CASES))
def test_records_equal_the_goldens(L, torch, name):
    g = golden(name)
    bad = g["frame_info"] != 0
    assert float(g["max_lh"]) < 512 and bad.any() and not bad.all()   # the conditions on the inputs
    B = len(g["frame_info"])
    with opened(L, g) as dec:
        assert dec.sigma(float(g["snr"])) == hm.sigma_of(dec.rh, dec.nh, float(g["snr"]), 0)
        got = frames(dec, g, B)
        assert same(got, g), (got[0][:8], g["frame_info"][:8], got[1][:8], g["iters"][:8])
        info, iters = got
        nse = int((info[info != 0] & ((1 << 30) - 1)).sum())
        assert [nse, int((info != 0).sum()), int(((info != 0) & (iters >= 0)).sum()), B, int(np.abs(iters).sum())] == g["counters"].tolist()


@pytest.mark.parametrize("name", sorted(hm.CASES))
def test_records_do_not_depend_on_calls_pieces_or_slots(L, torch, name, monkeypatch):
    g = golden(name)
    B = len(g["frame_info"])
    with opened(L, g) as dec:
        parts = [frames(dec, g, 1), frames(dec, g, 7), frames(dec, g, B - 8)]
        assert same((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])), g)
        end = dec.mt_get_state()
        for var, val in (("LDPC_HIP_GFQ_PIECE", "5"), ("LDPC_HIP_GFQ_SLOTS", "3")):
            monkeypatch.setenv(var, val)
            dec.mt_set_state(*L.mt19937_state(int(g["seed"])))
            assert same(frames(dec, g, B), g), var
            monkeypatch.delenv(var)
            st = dec.mt_get_state()
            assert np.array_equal(st[0], end[0]) and st[1] == end[1]


@pytest.mark.parametrize("name", ["s1_gf16_m8_enc", "s2_gf4_m5_enc", "s3_gf64_m7_enc"])
def test_advance_and_a_state_handed_to_a_second_context(L, torch, name):
    g = golden(name)
    B = len(g["frame_info"])
    k = 37
    with opened(L, g) as dec, opened(L, g, seed=999) as other:
        dec.mt_advance(k)
        assert same(frames(dec, g, 20), g, k, k + 20)
        other.mt_set_state(*dec.mt_get_state())
        assert same(frames(other, g, B - k - 20), g, k + 20, B)
        dec.mt_advance(0)
        assert same(frames(dec, g, B - k - 20), g, k + 20, B)


@pytest.mark.parametrize("name", sorted(hm.CASES))
def test_frames_from_the_hosts_gaussians(L, torch, name, monkeypatch):
    g = golden(name)
    B = len(g["frame_info"])
    with L.LdpcHipGfq(int(g["q_bits"]), g["hb"], g["hc"], int(g["M"])) as dec:   # no generator state is needed
        dec.set_codeword(g["word"])
        noise = hm.gaussians(int(g["seed"]), B, dec.N * dec.q_bits)
        assert same(dec.frames_from_noise(noise, float(g["snr"]), int(g["maxiter"]), int(g["punctured_blocks"])), g)
        monkeypatch.setenv("LDPC_HIP_GFQ_PIECE", "5")
        assert same(dec.frames_from_noise(noise[11:40], float(g["snr"]), int(g["maxiter"]), int(g["punctured_blocks"])), g, 11, 40)


def test_the_word_matters_and_can_be_taken_back(L, torch):
    """The encoded cases really depend on the word: with the all-zero word the same noise gives the records of a different run; and
    set_codeword(None) is the all-zero word again."""
    g = golden("s2_gf4_m5_enc")
    B = 64
    with opened(L, g) as dec:
        with_word = frames(dec, g, B)
        dec.set_codeword(None)
        dec.mt_set_state(*L.mt19937_state(int(g["seed"])))
        without = frames(dec, g, B)
        dec.set_codeword(np.zeros(dec.N, dtype=np.int16))
        dec.mt_set_state(*L.mt19937_state(int(g["seed"])))
        zeros = frames(dec, g, B)
    assert same(with_word, g, 0, B) and not np.array_equal(with_word[1], without[1])
    assert np.array_equal(without[0], zeros[0]) and np.array_equal(without[1], zeros[1])
    # the device encoder makes the word the model made
    with L.LdpcHipGfq(int(g["q_bits"]), g["hb"], g["hc"], int(g["M"])) as dec:
        cw, ok = dec.encode(L.gfq_upstream_message(dec.q_bits, dec.k)[None])
        assert ok[0] == 1 and np.array_equal(cw[0], g["word"])


def test_refusals_launch_nothing_and_leave_word_and_generator_alone(L, torch):
    g = golden("s1_gf16_m8_zero")
    lib = L.load_library()
    snr, maxiter = float(g["snr"]), int(g["maxiter"])
    rec = np.full(8, -7, dtype=np.int32)
    its = np.full(8, -7, dtype=np.int32)
    st = np.zeros(624, dtype=np.uint32)
    pos = C.c_int()
    noise = np.zeros((8, 64 * 4))

    def refused(rc, words):
        assert rc == -1 and words in lib.ldpc_hip_last_error().decode(), (rc, lib.ldpc_hip_last_error())
        assert (rec == -7).all() and (its == -7).all()

    with L.LdpcHipGfq(4, g["hb"], g["hc"], 8) as dec:
        dec.profile(True)
        # no generator state
        refused(lib.ldpc_hip_mt_frames_gfq(dec.h, snr, 0, maxiter, 8, rec.ctypes.data, its.ctypes.data), "no state")
        refused(lib.ldpc_hip_mt_advance_gfq(dec.h, 3), "no state")
        refused(lib.ldpc_hip_mt_get_state_gfq(dec.h, st.ctypes.data, C.byref(pos)), "no state")
        # bad arguments
        dec.mt_set_state(*L.mt19937_state(5))
        entry = dec.mt_get_state()
        refused(lib.ldpc_hip_mt_set_state_gfq(dec.h, None, 0), "bad argument")
        refused(lib.ldpc_hip_mt_set_state_gfq(dec.h, entry[0].ctypes.data, 625), "bad argument")
        refused(lib.ldpc_hip_mt_advance_gfq(dec.h, -1), "bad argument")
        refused(lib.ldpc_hip_mt_frames_gfq(dec.h, snr, 0, 0, 8, rec.ctypes.data, its.ctypes.data), "maxiter")
        refused(lib.ldpc_hip_mt_frames_gfq(dec.h, snr, 8, maxiter, 8, rec.ctypes.data, its.ctypes.data), "punctured_blocks")
        refused(lib.ldpc_hip_mt_frames_gfq(dec.h, snr, -1, maxiter, 8, rec.ctypes.data, its.ctypes.data), "punctured_blocks")
        refused(lib.ldpc_hip_mt_frames_gfq(dec.h, snr, 0, maxiter, -1, rec.ctypes.data, its.ctypes.data), "bad argument")
        refused(lib.ldpc_hip_mt_frames_gfq(dec.h, snr, 0, maxiter, 8, None, its.ctypes.data), "bad argument")
        refused(lib.ldpc_hip_frames_gfq_noise_host(dec.h, None, snr, 0, maxiter, 8, rec.ctypes.data, its.ctypes.data), "bad argument")
        refused(lib.ldpc_hip_frames_gfq_noise_host(dec.h, noise.ctypes.data, snr, 0, 0, 8, rec.ctypes.data, its.ctypes.data), "maxiter")
        refused(lib.ldpc_hip_frames_gfq_noise_host(dec.h, noise.ctypes.data, snr, 8, maxiter, 8, rec.ctypes.data, its.ctypes.data), "punctured_blocks")
        word = np.zeros(dec.N, dtype=np.int16)
        word[5] = 16
        refused(lib.ldpc_hip_gfq_set_codeword(dec.h, word.ctypes.data), "not an element of GF(16)")
        word[5] = -1
        refused(lib.ldpc_hip_gfq_set_codeword(dec.h, word.ctypes.data), "not an element of GF(16)")
        # the binary entry points keep refusing this context
        refused(lib.ldpc_hip_mt_set_state(dec.h, entry[0].ctypes.data, 624), "GF(q)")
        refused(lib.ldpc_hip_mt_frames(dec.h, snr, 0, 0, maxiter, 0.8, 8, rec.ctypes.data, its.ctypes.data), "GF(q)")
        after = dec.mt_get_state()
        assert np.array_equal(after[0], entry[0]) and after[1] == entry[1]
        assert dec.profile_read() == (0.0, 0)
        dec.mt_set_state(*L.mt19937_state(int(g["seed"])))
        assert same(frames(dec, g, 16), g, 0, 16)          # the word is still the all-zero one, the context works
        assert dec.profile_read()[1] == 1

    # other kinds of context
    H = relift(load_base_matrix(), 64)
    with L.LdpcHip(MS_DEC, H, 64) as binary, L.LdpcHipCodesGfq(4, g["hb"][None], g["hc"][None], 8) as cset:
        binary.mt_set_state(*L.mt19937_state(5))
        for h in (binary.h, cset.h):
            refused(lib.ldpc_hip_gfq_set_codeword(h, None), "not a GF(q) context")
            refused(lib.ldpc_hip_mt_set_state_gfq(h, entry[0].ctypes.data, 624), "not a GF(q) context")
            refused(lib.ldpc_hip_mt_get_state_gfq(h, st.ctypes.data, C.byref(pos)), "not a GF(q) context")
            refused(lib.ldpc_hip_mt_advance_gfq(h, 1), "not a GF(q) context")
            refused(lib.ldpc_hip_mt_frames_gfq(h, snr, 0, maxiter, 8, rec.ctypes.data, its.ctypes.data), "not a GF(q) context")
            refused(lib.ldpc_hip_frames_gfq_noise_host(h, noise.ctypes.data, snr, 0, maxiter, 8, rec.ctypes.data, its.ctypes.data), "not a GF(q) context")
        kept = binary.mt_get_state()
        want = L.mt19937_state(5)
        assert np.array_equal(kept[0], want[0]) and kept[1] == want[1]


# ---- code sets ----------------------------------------------------------------------------------------------------------------------
def _variant(hb, hc, q, rng):
    """Another candidate of the same pattern: other shifts off the special / dual-diagonal part are not needed, other coefficients are."""
    hc = hc.copy()
    there = np.argwhere(hb >= 0)
    for i, j in there[rng.permutation(len(there))[:3]]:
        hc[i, j] = hc[i, j] % (q - 1) + 1
    return hb.copy(), hc


def _sets():
    """name -> (q_bits, M, hb [C, rh, nh], hc, words [C, N], snr, maxiter, frames, seed): S1's shape without encodable codes (the
    shipped pattern: every word is the all-zero fallback), S2 and S3 with a word per candidate."""
    out = {}
    g = golden("s1_gf16_m8_zero")
    rng = np.random.RandomState(31)
    cand = [(g["hb"], g["hc"])] + [_variant(g["hb"], g["hc"], 16, rng) for _ in range(3)]
    out["s1"] = (4, 8, cand, 2.0, 15, 96, 21)
    rng = np.random.RandomState(32)
    out["s2"] = (2, 5, [hm.cm.make_code(rng, 2, 3, 6, 5, "w2") for _ in range(5)], 2.5, 20, 128, 22)
    rng = np.random.RandomState(33)
    out["s3"] = (6, 7, [hm.cm.make_code(rng, 6, 3, 6, 7, s) for s in ("xox", "oxo", "w2")], 1.5, 10, 64, 23)
    full = {}
    for name, (q_bits, M, cand, snr, maxiter, B, seed) in out.items():
        hb = np.array([c[0] for c in cand], dtype=np.int16)
        hc = np.array([c[1] for c in cand], dtype=np.int16)
        words = np.array([hm.transmitted_word(q_bits, b, c, M)[0] for b, c in cand], dtype=np.int16)
        assert words.any(axis=1).all() == (name != "s1") and words.any(axis=1).any() == (name != "s1")
        full[name] = (q_bits, M, hb, hc, words, snr, maxiter, B, seed)
    return full


SETS = {}
_LONE = {}


def the_set(name):
    if not SETS:
        SETS.update(_sets())
    return SETS[name]


def lone_records(L, name, with_words):
    """Once per set: every code's records on a context of its own, with its word (or none), from the set's entry state."""
    key = (name, with_words)
    if key not in _LONE:
        q_bits, M, hb, hc, words, snr, maxiter, B, seed = the_set(name)
        info, its = [], []
        for c in range(len(hb)):
            with L.LdpcHipGfq(q_bits, hb[c], hc[c], M) as dec:
                dec.set_codeword(words[c] if with_words else None)
                dec.mt_set_state(*L.mt19937_state(seed))
                a, b = dec.mt_frames(snr, maxiter, B)
                end = dec.mt_get_state()
            info.append(a)
            its.append(b)
        _LONE[key] = (np.array(info), np.array(its), end)
    return _LONE[key]


@pytest.mark.parametrize("with_words", [False, True], ids=["shared", "words"])
@pytest.mark.parametrize("name", ["s1", "s2", "s3"])
def test_every_code_of_a_set_equals_the_lone_context(L, torch, name, with_words, monkeypatch):
    q_bits, M, hb, hc, words, snr, maxiter, B, seed = the_set(name)
    want_info, want_its, want_end = lone_records(L, name, with_words)
    bad = want_info != 0
    assert bad.any() and not bad.all()
    with L.LdpcHipCodesGfq(q_bits, hb, hc, M) as cs:
        cs.set_codewords(words if with_words else None)
        for piece in (None, 5):
            if piece:
                monkeypatch.setenv("LDPC_HIP_GFQ_PIECE", str(piece))
            cs.mt_set_state(*L.mt19937_state(seed))
            cnt, info, its = cs.mt_simulate(snr, maxiter, B, records=True)
            end = cs.mt_get_state()
            assert np.array_equal(info, want_info) and np.array_equal(its, want_its), (name, piece)
            assert np.array_equal(end[0], want_end[0]) and end[1] == want_end[1]
            for c in range(len(hb)):
                e = want_info[c] != 0
                assert cnt[c].tolist() == [int((want_info[c][e] & ((1 << 30) - 1)).sum()), int(e.sum()), int((e & (want_its[c] >= 0)).sum()), B,
                                           int(np.abs(want_its[c]).sum())]
        monkeypatch.delenv("LDPC_HIP_GFQ_PIECE")
        noise = hm.gaussians(seed, B, cs.N * q_bits)
        cnt2, info2, its2 = cs.frames_from_noise(noise, snr, maxiter)
        assert np.array_equal(info2, want_info) and np.array_equal(its2, want_its) and np.array_equal(cnt2, cnt)
        if with_words and name != "s1":   # the words change the records, and taking them back gives the shared route again
            shared = lone_records(L, name, False)
            assert not np.array_equal(shared[1], want_its)
            cs.set_codewords(None)
            cs.mt_set_state(*L.mt19937_state(seed))
            _, info3, its3 = cs.mt_simulate(snr, maxiter, B, records=True)
            assert np.array_equal(info3, shared[0]) and np.array_equal(its3, shared[1])


def host_rule(L, info, iters, nfe, nexp, ref):
    st = {"nse": 0, "nde": 0, "nue": 0, "experiment": 0}
    L.replay_stopping_rule(info, iters, st, nfe, nexp, ref)
    return [st["experiment"], st["nse"], st["nde"], st["nue"], int(np.abs(iters[:st["experiment"]].astype(np.int64)).sum())]


# name of the set, (n_frame_errors, n_experiments, reference_frame_error), the ending most of its codes take
STOPS = [("s1", (12, 95, 1.0), "nde"), ("s2", (500, 99, 1.0), "experiments"), ("s2", (500, 127, 0.01), "reference"), ("s3", (6, 63, 1.0), "nde")]


@pytest.mark.parametrize("name,stop,ending", STOPS, ids=[s[0] + "_" + s[2] for s in STOPS])
def test_the_rule_on_the_device_equals_the_host_replay(L, torch, name, stop, ending, monkeypatch):
    q_bits, M, hb, hc, words, snr, maxiter, B, seed = the_set(name)
    with_words = name != "s1"
    info, its, _ = lone_records(L, name, with_words)
    nfe, nexp, ref = stop
    assert nexp + 1 <= B
    want = np.array([host_rule(L, info[c], its[c], nfe, nexp, ref) for c in range(len(hb))], dtype=np.uint64)
    endings = [hm.stop_rule(info[c], nfe, nexp, ref)[3] for c in range(len(hb))]
    assert ending in endings, endings
    st = L.mt19937_state(seed)
    with L.LdpcHipCodesGfq(q_bits, hb, hc, M) as cs, L.LdpcHipGfq(q_bits, hb[1], hc[1], M) as one:
        cs.set_codewords(words if with_words else None)
        for piece, first_batch, max_batch in ((None, 16, 64), (7, 1, 256)):
            if piece:
                monkeypatch.setenv("LDPC_HIP_GFQ_PIECE", str(piece))
            cs.mt_set_state(*st)
            got = cs.mt_simulate_until(snr, maxiter, nfe, nexp, ref, first_batch=first_batch, max_batch=max_batch)
            assert got.shape == (len(hb), 6) and np.array_equal(got[:, :5], want), (got.tolist(), want.tolist())
            assert (got[:, 5] >= got[:, 0]).all()
            back = cs.mt_get_state()
            assert np.array_equal(back[0], st[0]) and back[1] == st[1], "the run puts the generator back where it found it"
        monkeypatch.delenv("LDPC_HIP_GFQ_PIECE")
        # mt_advance(experiment of code 1) leaves the generator where upstream's loop leaves it for code 1: the next records are
        # the ones a lone context gives after as many frames
        k = int(want[1, 0])
        cs.mt_advance(k)
        one.set_codeword(words[1] if with_words else None)
        one.mt_set_state(*st)
        one.mt_advance(k)
        a, b = cs.mt_get_state(), one.mt_get_state()
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
        _, nxt_info, nxt_its = cs.mt_simulate(snr, maxiter, 9, records=True)
        w_info, w_its = one.mt_frames(snr, maxiter, 9)
        assert np.array_equal(nxt_info[1], w_info) and np.array_equal(nxt_its[1], w_its)
        if k + 9 <= B:
            assert np.array_equal(w_info, info[1][k:k + 9])
        # nothing to do: no frame is consumed (:591 fails before the first frame)
        cs.mt_set_state(*st)
        for x, y in ((0, nexp), (-3, nexp), (nfe, -1)):
            assert not cs.mt_simulate_until(snr, maxiter, x, y, ref).any()
        back = cs.mt_get_state()
        assert np.array_equal(back[0], st[0]) and back[1] == st[1]


def test_set_refusals_launch_nothing_and_leave_words_and_generator_alone(L, torch):
    q_bits, M, hb, hc, words, snr, maxiter, B, seed = the_set("s2")
    lib = L.load_library()
    cnt = np.full((len(hb), 5), 5, dtype=np.uint64)
    state = np.full((len(hb), 6), 5, dtype=np.uint64)
    st624 = np.zeros(624, dtype=np.uint32)
    pos = C.c_int()
    noise = np.zeros((4, 30 * 2))

    def refused(rc, text):
        assert rc == -1 and text in lib.ldpc_hip_last_error().decode(), (rc, lib.ldpc_hip_last_error())
        assert (cnt == 5).all() and (state == 5).all()

    def stop(h, maxiter=maxiter, first_batch=16, max_batch=64, st_ptr=state.ctypes.data, punct=0):
        return lib.ldpc_hip_mt_simulate_codes_gfq_stop(h, snr, punct, maxiter, 7, 100, 0.05, first_batch, max_batch, st_ptr)

    with L.LdpcHipCodesGfq(q_bits, hb, hc, M) as cs:
        cs.profile(True)
        cs.set_codewords(words)
        refused(lib.ldpc_hip_mt_simulate_codes_gfq(cs.h, snr, 0, maxiter, 4, cnt.ctypes.data, None, None), "no state")
        refused(stop(cs.h), "no state")
        refused(lib.ldpc_hip_mt_advance_codes_gfq(cs.h, 2), "no state")
        refused(lib.ldpc_hip_mt_get_state_codes_gfq(cs.h, st624.ctypes.data, C.byref(pos)), "no state")
        entry = L.mt19937_state(seed)
        cs.mt_set_state(*entry)
        refused(lib.ldpc_hip_mt_set_state_codes_gfq(cs.h, None, 0), "bad argument")
        refused(lib.ldpc_hip_mt_advance_codes_gfq(cs.h, -1), "bad argument")
        refused(lib.ldpc_hip_mt_simulate_codes_gfq(cs.h, snr, 0, maxiter, 4, None, None, None), "bad argument")
        refused(lib.ldpc_hip_mt_simulate_codes_gfq(cs.h, snr, 0, 0, 4, cnt.ctypes.data, None, None), "maxiter")
        refused(lib.ldpc_hip_mt_simulate_codes_gfq(cs.h, snr, 6, maxiter, 4, cnt.ctypes.data, None, None), "punctured_blocks")
        refused(stop(cs.h, st_ptr=None), "bad argument")
        refused(stop(cs.h, first_batch=0), "batches")
        refused(stop(cs.h, first_batch=65), "batches")
        refused(stop(cs.h, maxiter=0), "maxiter")
        refused(stop(cs.h, punct=-1), "punctured_blocks")
        refused(lib.ldpc_hip_frames_codes_gfq_noise_host(cs.h, None, snr, 0, maxiter, 4, cnt.ctypes.data, None, None), "bad argument")
        refused(lib.ldpc_hip_frames_codes_gfq_noise_host(cs.h, noise.ctypes.data, snr, 0, 0, 4, cnt.ctypes.data, None, None), "maxiter")
        bad = words.copy()
        bad[2, 7] = 4
        refused(lib.ldpc_hip_codes_gfq_set_codewords(cs.h, bad.ctypes.data), "not an element of GF(4)")
        # the binary set entry points and the single-code GF(q) ones keep refusing this context
        refused(lib.ldpc_hip_mt_set_state_codes(cs.h, entry[0].ctypes.data, 624), "code-set context")
        refused(lib.ldpc_hip_mt_advance_codes(cs.h, snr, 0, 1), "code-set context")
        refused(lib.ldpc_hip_mt_set_state_gfq(cs.h, entry[0].ctypes.data, 624), "not a GF(q) context")
        refused(lib.ldpc_hip_mt_set_state(cs.h, entry[0].ctypes.data, 624), "GF(q)")
        back = cs.mt_get_state()
        assert np.array_equal(back[0], entry[0]) and back[1] == entry[1]
        assert cs.profile_read() == (0.0, 0)
        _, info, its = cs.mt_simulate(snr, maxiter, 16, records=True)   # the words are still the set's
        want = lone_records(L, "s2", True)
        assert np.array_equal(info, want[0][:, :16]) and np.array_equal(its, want[1][:, :16])
        assert cs.profile_read()[1] == 1

    # other kinds of context
    g = golden("s1_gf16_m8_zero")
    H = relift(load_base_matrix(), 64)
    with L.LdpcHip(MS_DEC, H, 64) as binary, L.LdpcHipGfq(4, g["hb"], g["hc"], 8) as single, \
            L.LdpcHipCodes(MS_DEC, np.array([H, H], dtype=np.int16), 64) as bset:
        for h in (binary.h, single.h, bset.h):
            refused(lib.ldpc_hip_codes_gfq_set_codewords(h, None), "not a GF(q) code-set context")
            refused(lib.ldpc_hip_mt_set_state_codes_gfq(h, st624.ctypes.data, 624), "not a GF(q) code-set context")
            refused(lib.ldpc_hip_mt_get_state_codes_gfq(h, st624.ctypes.data, C.byref(pos)), "not a GF(q) code-set context")
            refused(lib.ldpc_hip_mt_advance_codes_gfq(h, 1), "not a GF(q) code-set context")
            refused(lib.ldpc_hip_mt_simulate_codes_gfq(h, snr, 0, maxiter, 4, cnt.ctypes.data, None, None), "not a GF(q) code-set context")
            refused(stop(h), "not a GF(q) code-set context")
            refused(lib.ldpc_hip_frames_codes_gfq_noise_host(h, noise.ctypes.data, snr, 0, maxiter, 4, cnt.ctypes.data, None, None), "not a GF(q) code-set context")


# ---- the C++ layer: ldpc::bp_simulation(q_mod > 2, ...) -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness_driver(tmp_path_factory):
    import os
    import subprocess
    from ldpc_testlib import ROOT
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = str(tmp_path_factory.mktemp("gfq_harness") / "gfq_harness_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "gfq_harness_driver.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_compat", "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    return exe


def _driver_input(path, g, show=0, dec=6, mod=0, perm=0):
    rh, nh = g["H"].shape
    nfe, nexp, ref = int(g["stop"][0]), int(g["stop"][1]), float(g["stop"][2])
    with open(path, "wb") as f:
        f.write(np.array([1 << int(g["q_bits"]), rh, nh, int(g["M"]), int(g["ncols2convert"]), int(g["maxiter"]), nfe, nexp,
                          int(g["punctured_blocks"]), int(g["seed"]), show, dec, mod, perm], dtype=np.int32).tobytes())
        f.write(np.array([float(g["snr"]), ref], dtype=np.float64).tobytes())
        f.write(g["H"].astype(np.int32).tobytes())
        f.write(g["coef"].astype(np.int32).tobytes())


# the harness chooses the word itself: the cases whose word is the one upstream's set-up arrives at (the encoded message, or the all-zero
# fallback of the shipped code, which its encoder refuses)
HARNESS_CASES = sorted(n for n, p in hm.CASES.items() if p["word"] == "enc" or p["code"] == "shipped")


@pytest.mark.parametrize("route", ["device", "host"])
@pytest.mark.parametrize("name", HARNESS_CASES)
def test_cpp_harness_equals_the_golden(L, torch, harness_driver, tmp_path, name, route):
    """(BER, FER), the SimCounters, the coefficient matrix written back and the generator afterwards, on both noise routes."""
    import os
    import subprocess
    g = golden(name)
    _driver_input(tmp_path / "in.bin", g, show=1)
    env = dict(os.environ)
    env.pop("LDPC_HIP_EXACT_NOISE", None)
    if route == "host":
        env["LDPC_HIP_EXACT_NOISE"] = "host"
    out = subprocess.check_output([harness_driver, str(tmp_path / "in.bin")], timeout=120, env=env).decode().split("\n")
    rows = {w[0]: w[1:] for w in (line.split() for line in out if line) if w[0] in ("pair", "next", "coef", "counters", "pair2")}
    assert set(rows) == {"pair", "next", "coef", "counters", "pair2"}, out
    want_pair = [float(v) for v in g["ber_fer"]]
    assert [float.fromhex(v) for v in rows["pair"]] == want_pair and [float.fromhex(v) for v in rows["pair2"]] == want_pair
    assert [int(v) for v in rows["coef"]] == g["coef_back"].astype(int).ravel().tolist()
    experiment, nse, nde = (int(v) for v in g["stop_state"])
    st = {"nse": 0, "nde": 0, "nue": 0, "experiment": 0}
    L.replay_stopping_rule(g["frame_info"], g["iters"], st, int(g["stop"][0]), int(g["stop"][1]), float(g["stop"][2]))
    assert (st["experiment"], st["nse"], st["nde"]) == (experiment, nse, nde)
    assert [int(v) for v in rows["counters"]] == [nse, nde, st["nue"], experiment, int(np.abs(g["iters"][:experiment].astype(np.int64)).sum())]
    per_frame = g["hb"].shape[1] * int(g["M"]) * int(g["q_bits"])
    stream = hm.gaussians(int(g["seed"]), experiment + 1, per_frame).ravel()
    assert [float.fromhex(v) for v in rows["next"]] == stream[experiment * per_frame:experiment * per_frame + 4].tolist()
    assert sum(line.startswith("SNR=") for line in out) == nde, "show_process prints a line per error frame"


@pytest.mark.parametrize("dec,mod,perm,words", [(3, 0, 0, "decoder_type 6"), (6, 1, 0, "MODULATION_SKIP"), (6, 0, 1, "permutation_type 0")])
def test_cpp_harness_fails_loudly_on_what_upstream_does_not_have(L, torch, harness_driver, tmp_path, dec, mod, perm, words):
    import subprocess
    g = golden("s1_gf16_m8_zero")
    _driver_input(tmp_path / "in.bin", g, dec=dec, mod=mod, perm=perm)
    res = subprocess.run([harness_driver, str(tmp_path / "in.bin")], capture_output=True, timeout=60)
    assert res.returncode == 1 and words in res.stderr.decode(), (res.returncode, res.stderr)


# ---- the C++ layer on a set: ldpc::bp_simulation_codes_gfq_exact ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def codes_driver(tmp_path_factory):
    import os
    import subprocess
    from ldpc_testlib import ROOT
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = str(tmp_path_factory.mktemp("gfq_codes_exact") / "gfq_codes_exact_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "gfq_codes_exact_driver.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_compat", "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    return exe


# set, stopping rule, leave_at, ncols2convert
CODES_CASES = [("s1", (12, 95, 1.0), -1, 0), ("s2", (500, 127, 0.01), 1, 0), ("s3", (6, 63, 1.0), 0, 2)]


@pytest.mark.parametrize("route", ["device", "host"])
@pytest.mark.parametrize("name,stop,leave_at,n2c", CODES_CASES, ids=[c[0] for c in CODES_CASES])
def test_cpp_set_harness_equals_the_loop_over_candidates(L, torch, codes_driver, tmp_path, name, stop, leave_at, n2c, route):
    """Both routes of bp_simulation_codes_gfq_exact (show_process 0 and 1) against reset_random(); bp_simulation_gfq_t per candidate in
    the same program, and against the host replay of the rule over the records of lone contexts: pairs, SimCounters, the coefficients
    written back, the generator afterwards (leave_at)."""
    import os
    import subprocess
    q_bits, M, hb, hc, words, snr, maxiter, B, seed = the_set(name)
    nfe, nexp, ref = stop
    C, rh, nh = hb.shape
    H = np.array([hm.inverse_left2right(m) for m in hb], dtype=np.int32)          # what a caller hands over: before left2right,
    coef = np.array([hm.inverse_left2right(m) for m in hc], dtype=np.int32)       # the first ncols2convert columns as powers
    lg, _ = hm.gf_tables(q_bits)
    given = coef.copy()
    for k in range(n2c):
        given[:, :, k] = np.where(coef[:, :, k] > 0, lg[np.maximum(coef[:, :, k], 1)], coef[:, :, k])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([1 << q_bits, C, rh, nh, M, n2c, maxiter, nfe, nexp, 0, seed, leave_at, 16, 64], dtype=np.int32).tobytes())
        f.write(np.array([snr, ref], dtype=np.float64).tobytes())
        f.write(H.tobytes())
        f.write(given.tobytes())
    env = dict(os.environ)
    env.pop("LDPC_HIP_EXACT_NOISE", None)
    if route == "host":
        env["LDPC_HIP_EXACT_NOISE"] = "host"
    out = subprocess.check_output([codes_driver, str(tmp_path / "in.bin")], timeout=120, env=env).decode().split("\n")
    rows = [line.split() for line in out if line]
    sets = {(int(w[1]), int(w[2])): w[3:] for w in rows if w[0] == "set"}
    ones = {int(w[1]): w[2:] for w in rows if w[0] == "one"}
    coefs = {(int(w[1]), int(w[2])): [int(v) for v in w[3:]] for w in rows if w[0] == "coef"}
    nxt = {int(w[1]): w[2:] for w in rows if w[0] == "next"}
    onenext = {int(w[1]): w[2:] for w in rows if w[0] == "onenext"}
    assert len(sets) == 2 * C and len(ones) == C and len(nxt) == 2, out
    info, its, _ = lone_records(L, name, name != "s1")
    leave = C - 1 if leave_at < 0 else leave_at
    for c in range(C):
        want = host_rule(L, info[c], its[c], nfe, nexp, ref)                      # experiment, nse, nde, nue, sum |iters|
        for show in (0, 1):
            assert sets[show, c] == ones[c], (show, c, sets[show, c], ones[c])
            assert coefs[show, c] == coef[c].ravel().tolist()                     # natural representation written back
        ber, fer = (float.fromhex(v) for v in ones[c][:2])
        assert [int(v) for v in ones[c][2:]] == [want[1], want[2], want[3], want[0], want[4]], c
        assert ber == want[1] / want[0] / ((nh - rh) * M) and fer == want[2] / want[0]
    assert nxt[0] == nxt[1] == onenext[leave]
    assert len({tuple(v) for v in onenext.values()}) > 1, "the candidates stop at different frames: leave_at matters"
    nde_total = sum(int(ones[c][3]) for c in range(C))
    assert sum(line.startswith("code=") for line in out) == nde_total, "show_process = 1 prints a line per error frame"


# ---- ldpc_sim on q-ary codes ------------------------------------------------------------------------------------------------------------
def _matrix_text(m):
    return "matrix (%d %d) { %s }" % (m.shape[0], m.shape[1], " ".join(str(int(v)) for v in m.ravel()))


def test_ldpc_sim_runs_q_ary_codes_single_and_in_sets(L, torch, tmp_path):
    """A reduced copy of tests/golden/jsonx/resultq.jsonx -- its GF(16) code record and two more with other coefficients, lower SNRs,
    small error_blocks / num_codewords: FER and BER of the result file equal the harness model's, and --code-sets gives the same
    numbers; --throughput keeps skipping q-ary codes with today's message."""
    import os
    import subprocess
    from ldpc_testlib import ROOT
    exe = os.path.join(ROOT, "ldpc-lib_amd", "ldpc_sim")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    shipped = subprocess.check_output([exe, "jsonx-get", os.path.join(ROOT, "tests", "golden", "jsonx", "resultq.jsonx"), "results/0/code"], text=True)
    hb0 = np.array([int(v) for v in shipped.split("{")[1].replace("}", "").split()]).reshape(4, 8)
    assert np.array_equal(hb0, np.array(hm.SHIPPED_HB))
    snrs, nfe, nexp, seed, maxiter = (2.0, 2.4), 12, 95, 1, 15
    rng = np.random.RandomState(77)
    coefs = [np.array(hm.SHIPPED_HC)] + [np.where(hb0 >= 0, rng.randint(0, 200, hb0.shape), -1) for _ in range(2)]   # 0 and values >= q get reduced
    records = "\n".join('{ _SNRs = array { %s } _decoder_type = 3 _iterations = %d _lifting = 8 _q_mod = 16 _marking = "skip" _punctured_blocks = 0\n'
                        "  code = %s\n  coef = %s\n  girth = 6 code_index = %d }" % (" ".join(map(str, snrs)), maxiter, _matrix_text(hb0), _matrix_text(c), i)
                        for i, c in enumerate(coefs))
    (tmp_path / "scenario.jsonx").write_text(
        "{ results = array { %s }\n  settings = { random_seed = %d num_codewords = %d error_blocks = %d error_minimization = { name = \"FER\" threshold = 1.0 }\n"
        "    modulation_type = 0 permutation_type = 0 permutation_block = 128 permutation_inter = 1 } }" % (records, seed, nexp, nfe))

    def numbers(path, field):
        text = subprocess.check_output([exe, "jsonx-get", path, field], text=True).strip()
        return [float(x) for x in text.replace("array {", "").replace("}", "").split()]

    want = []
    for c in coefs:                                                                # the model: reductions, set-up, word, frames, rule
        H = hm.shipped(8, 16)[0]
        HC = np.where((H > -1) & (c > -1), np.where(c % 16 == 0, 15, c % 16), c).astype(np.int16)
        hb, hc, back = hm.setup(4, H, HC, 0)
        word, encoded = hm.transmitted_word(4, hb, hc, 8)
        assert not encoded
        per = []
        for snr in snrs:
            noise = hm.gaussians(seed, nexp + 1, 64 * 4)
            info, iters, _, max_lh = hm.frames(4, hb, hc, 8, word, noise, hm.sigma_of(4, 8, snr, 0), maxiter)
            assert max_lh < 512 and (info != 0).any() and (info == 0).any()
            experiment, nse, nde, _ = hm.stop_rule(info, nfe, nexp, 1.0)
            per.append(hm.result_pair(experiment, nse, nde, 64, 32))
        want.append((HC, per))
    for flags in ([], ["--code-sets"]):
        out = str(tmp_path / ("result%d.jsonx" % len(flags)))
        log = subprocess.check_output([exe, "simulation", str(tmp_path / "scenario.jsonx"), out] + flags, text=True, timeout=120)
        assert "skipped" not in log and (("set of 3 codes" in log) == bool(flags)), log
        for i, (HC, per) in enumerate(want):
            assert numbers(out, "results/%d/simulation_logs/0/BER" % i) == [p[0] for p in per], (flags, i)
            assert numbers(out, "results/%d/simulation_logs/0/FER" % i) == [p[1] for p in per], (flags, i)
            get = lambda field: subprocess.check_output([exe, "jsonx-get", out, "results/%d/%s" % (i, field)], text=True).strip()   # noqa: E731
            assert int(get("_q_mod")) == 16 and int(get("_decoder_type")) == 6     # decoder 6 is forced whatever the record says
            assert [int(v) for v in get("coef").split("{")[1].replace("}", "").split()] == HC.astype(int).ravel().tolist()
    log = subprocess.check_output([exe, "simulation", str(tmp_path / "scenario.jsonx"), str(tmp_path / "t.jsonx"), "--throughput"], text=True, timeout=120)
    assert log.count("GF(16) codes (FHT decoder) are not built in ldpc-lib_amd, skipped") == 3
