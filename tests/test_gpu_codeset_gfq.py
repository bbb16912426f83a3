"""GF(q) code sets on the GPU (LdpcHipCodesGfq / ldpc_hip_*codes_gfq*): C candidate codes x B frames in one launch against the numpy
restatement of the decoder (tests/gfq_model.py) and against LdpcHipGfq on each code alone, tolerance 0 (return values and qhard with
array_equal, the a-posteriori vectors as uint64 images); workgroups that walk across code boundaries; edge cases; counting and the
fused run against the single-code chain; the stopping rule against host.replay_stop_rule; refusals and cross-use; the C++ layer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from codeset_gfq_sets import MAXITER, NCODES, cw2_mixture_set, mixed_set, shipped_set, weak_first_set
from codeset_stop_sets import frames_launched, schedule, stop_piece
from gfq_chain_model import count as model_count
from gfq_chain_model import sigma_of
from gfq_model import GFQ_GOLDEN_DIR, GfqModel, bpsk_symbol_probabilities
from ldpc_testlib import MS_DEC, ROOT, assert_bits_equal

import make_gfq_goldens  # noqa: E402  (tools/ is on the path through codeset_gfq_sets)

pytestmark = pytest.mark.gpu

EINVAL = -1

#        name                    q_bits M   set                               SNR  frames  kernel
SETS = {"gf16_shipped_M8":      (4, 8, lambda: shipped_set(8, 16), 2.4, 100, "gfq_codes_kernel<q=16,16x1>"),             # one wave
        "gf64_shipped_M8":      (6, 8, lambda: shipped_set(8, 64), 2.4, 60, "gfq_codes_kernel<q=64,16x4>"),
        "gf4_mixed_M70":        (2, 70, lambda: mixed_set(70, 4), 1.8, 60, "gfq_codes_kernel<generic,q=4,4x1>"),          # several waves
        "gf256_shipped_M2":     (8, 2, lambda: shipped_set(2, 256), 2.4, 60, "gfq_codes_kernel<generic,q=256,4x64>"),     # LPC 64
        "gf16_cw2_mixture_M33": (4, 33, lambda: cw2_mixture_set(33, 16), 1.6, 60, "gfq_codes_kernel<q=16,16x1>")}         # cw2 and E change inside the set


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


_CASE = {}


def case(name):
    """Once per set: the codes, the shared received words, per-code received words, and the model's results on both."""
    if name not in _CASE:
        q_bits, M, make, snr, frames, kernel = SETS[name]
        hb, hc = make()
        N = hb.shape[2] * M
        sigma = make_gfq_goldens.sigma_of(snr, hb[0])
        shared = bpsk_symbol_probabilities(np.random.RandomState(500 + q_bits * 7 + M), q_bits, N, sigma, frames)
        own = bpsk_symbol_probabilities(np.random.RandomState(600 + q_bits * 7 + M), q_bits, N, sigma, NCODES * 12).reshape(NCODES, 12, 1 << q_bits, N)
        models = [GfqModel(q_bits, hb[c], hc[c], M) for c in range(NCODES)]
        want_shared = [m.decode(shared, MAXITER) for m in models]
        want_own = [m.decode(own[c], MAXITER) for c, m in enumerate(models)]
        for a in (shared, own):
            a.setflags(write=False)
        _CASE[name] = dict(q_bits=q_bits, M=M, hb=hb, hc=hc, N=N, shared=shared, own=own, want_shared=want_shared, want_own=want_own, kernel=kernel)
    return _CASE[name]


def run_set(torch, cs, soft, maxiter, shared):
    d = torch.from_numpy(np.array(soft, order="C")).cuda()   # a copy: the shared references stay read-only
    qhard, iters, post = cs.decode(d, maxiter, shared=shared, want_post=True)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint64), np.ascontiguousarray(soft).view(np.uint64)), "the input buffer was modified"
    return iters.cpu().numpy(), qhard.cpu().numpy(), post.cpu().numpy()


def assert_codes_equal(got, want, what, nan_ok=False):
    """got: (iters [C, B], qhard [C, B, N], post [C, B, q, N]); want: per code (iters, qhard, post)."""
    for c, (wi, wq, wp) in enumerate(want):
        assert np.array_equal(got[0][c], wi), (what, "iters of code", c)
        assert np.array_equal(got[1][c], wq), (what, "qhard of code", c)
        assert_bits_equal(got[2][c], wp, f"{what}: post of code {c}", nan_ok=nan_ok)


@pytest.mark.parametrize("name", sorted(SETS))
def test_decode_bit_for_bit(L, torch, name):
    k = case(name)
    its = np.array([w[0] for w in k["want_shared"]])
    print(name, "converged per code", (its >= 0).sum(axis=1).tolist(), "of", its.shape[1])
    assert (its >= 0).any() and (its < 0).any(), "the set should hold converged and non-converged frames"
    assert len({w[0].tobytes() for w in k["want_shared"]}) > 1, "the codes of the set decode differently"
    with L.LdpcHipCodesGfq(k["q_bits"], k["hb"], k["hc"], k["M"]) as cs:
        assert cs.kernel_name == k["kernel"], cs.kernel_name
        assert (cs.C, cs.q, cs.N, cs.R) == (NCODES, 1 << k["q_bits"], k["N"], k["hb"].shape[1] * k["M"])
        assert cs.lib.ldpc_hip_codes(cs.h) == NCODES and cs.edges == max(int((b >= 0).sum()) for b in k["hb"])
        got = run_set(torch, cs, k["shared"], MAXITER, True)                        # [B][q][N], every code the same words
        assert_codes_equal(got, k["want_shared"], name + " shared")
        got = run_set(torch, cs, k["own"], MAXITER, False)                          # [C][B][q][N]
        assert_codes_equal(got, k["want_own"], name + " per code")
    # the single-code context on two members: the same bits from the other route
    d = torch.from_numpy(np.array(k["shared"], order="C")).cuda()
    for c in (1, NCODES - 1):
        with L.LdpcHipGfq(k["q_bits"], k["hb"][c], k["hc"][c], k["M"]) as one:
            qh, it, po = one.decode(d, MAXITER, want_post=True)
            torch.cuda.synchronize()
        assert np.array_equal(it.cpu().numpy(), k["want_shared"][c][0]) and np.array_equal(qh.cpu().numpy(), k["want_shared"][c][1])
        assert_bits_equal(po.cpu().numpy(), k["want_shared"][c][2])


@pytest.mark.parametrize("name", ["gf16_shipped_M8", "gf16_cw2_mixture_M33", "gf64_shipped_M8"])
def test_workgroups_walk_across_codes(L, torch, monkeypatch, name):
    """7 slots, 5 codes x 11 frames: 55 items, workgroup g takes g, g + 7, ... and so meets every code; item 11 c is the first of code c."""
    k = case(name)
    B = 11
    want_s = [tuple(a[:B] for a in w) for w in k["want_shared"]]
    want_o = [tuple(a[:B] for a in w) for w in k["want_own"]]
    with L.LdpcHipCodesGfq(k["q_bits"], k["hb"], k["hc"], k["M"]) as cs:
        default_s = run_set(torch, cs, k["shared"][:B], MAXITER, True)
        default_o = run_set(torch, cs, k["own"][:, :B], MAXITER, False)
        monkeypatch.setenv("LDPC_HIP_GFQ_SLOTS", "7")
        seven_s = run_set(torch, cs, k["shared"][:B], MAXITER, True)
        seven_o = run_set(torch, cs, k["own"][:, :B], MAXITER, False)
        monkeypatch.setenv("LDPC_HIP_GFQ_SLOTS", "1")                                 # one workgroup walks the whole set
        single = run_set(torch, cs, k["shared"][:B], MAXITER, True)
        monkeypatch.delenv("LDPC_HIP_GFQ_SLOTS")
    for what, got, want in (("default", default_s, want_s), ("7 slots", seven_s, want_s), ("1 slot", single, want_s),
                            ("default, per code", default_o, want_o), ("7 slots, per code", seven_o, want_o)):
        assert_codes_equal(got, want, f"{name} {what}")
    for a, b in zip(default_s, seven_s):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_maxiter_one_and_optional_outputs(L, torch):
    k = case("gf16_cw2_mixture_M33")
    soft = k["shared"][:20]
    models = [GfqModel(4, k["hb"][c], k["hc"][c], 33) for c in range(NCODES)]
    with L.LdpcHipCodesGfq(4, k["hb"], k["hc"], 33) as cs:
        for maxiter in (1, 3):
            assert_codes_equal(run_set(torch, cs, soft, maxiter, True), [m.decode(soft, maxiter) for m in models], f"maxiter {maxiter}")
        d = torch.from_numpy(np.array(soft, order="C")).cuda()
        full = run_set(torch, cs, soft, MAXITER, True)
        B, N, q = 20, k["N"], 16
        qh = torch.full((NCODES, B, N), -1, dtype=torch.int16, device="cuda")
        it = torch.full((NCODES, B), -99, dtype=torch.int32, device="cuda")
        po = torch.full((NCODES, B, q, N), -1.0, dtype=torch.float64, device="cuda")
        call = cs.lib.ldpc_hip_decode_codes_gfq_dev
        assert call(cs.h, d.data_ptr(), 1, B, MAXITER, qh.data_ptr(), None, None, None) == 0          # each output alone
        assert call(cs.h, d.data_ptr(), 1, B, MAXITER, None, it.data_ptr(), None, None) == 0
        assert call(cs.h, d.data_ptr(), 1, B, MAXITER, None, None, po.data_ptr(), None) == 0
        assert call(cs.h, d.data_ptr(), 1, B, MAXITER, None, None, None, None) == 0                   # and none
        torch.cuda.synchronize()
        assert np.array_equal(it.cpu().numpy(), full[0]) and np.array_equal(qh.cpu().numpy(), full[1])
        assert_bits_equal(po.cpu().numpy(), full[2])
        assert call(cs.h, None, 1, 0, MAXITER, None, None, None, None) == 0                           # an empty batch
        cs.profile(True)
        cs.decode(d, MAXITER)
        ms, n = cs.profile_read()
        assert n == 1 and ms > 0 and cs.lib.ldpc_hip_last_launch(cs.h).decode() == cs.kernel_name


def test_codeword_on_input_and_the_boundary_set(L, torch):
    """The inputs of the golden gf16_m8_boundary (exact zeros, Inf / NaN, ties, underflow; frames 0 and 1 are codewords on input)
    through a set that contains its code, against LdpcHipGfq on every member."""
    g = np.load(os.path.join(GFQ_GOLDEN_DIR, "gf16_m8_boundary.npz"))
    soft, maxiter = g["soft"], int(g["maxiter"])
    hb, hc = shipped_set(8, 16)
    assert np.array_equal(hb[0], g["hb"]) and np.array_equal(hc[0], g["hc"]) and int(g["ncols2convert"]) == 0
    assert not np.isfinite(g["post"]).all(), "the set is there for the Inf / NaN path"
    d = torch.from_numpy(soft).cuda()
    want = []
    for c in range(NCODES):
        with L.LdpcHipGfq(4, hb[c], hc[c], 8) as one:
            qh, it, po = one.decode(d, maxiter, want_post=True)
            torch.cuda.synchronize()
            want.append((it.cpu().numpy(), qh.cpu().numpy(), po.cpu().numpy()))
    assert np.array_equal(want[0][0], g["iters"]) and np.array_equal(want[0][1], g["qhard"])
    with L.LdpcHipCodesGfq(4, hb, hc, 8) as cs:
        got = run_set(torch, cs, soft, maxiter, True)
    assert_codes_equal(got, want, "boundary", nan_ok=True)
    assert_bits_equal(got[2][0], g["post"], "boundary post of code 0 against upstream", nan_ok=True)
    # frame 0 is the certain all-zero word, a codeword of every candidate: 0 iterations, post = the input bit for bit
    assert (got[0][:, 0] == 0).all() and (got[1][:, 0] == 0).all()
    for c in range(NCODES):
        assert_bits_equal(got[2][c, 0], soft[0], f"codeword on input, code {c}")
    assert got[0][0, 1] == 0
    assert_bits_equal(got[2][0, 1], soft[1], "soft codeword on input, code 0")


def test_count_errors(L, torch):
    k = case("gf16_cw2_mixture_M33")
    R = k["hb"].shape[1] * k["M"]
    with L.LdpcHipCodesGfq(4, k["hb"], k["hc"], 33) as cs:
        d = torch.from_numpy(np.array(k["shared"], order="C")).cuda()
        qhard, iters, _ = cs.decode(d, MAXITER)
        cnt, info = cs.count_errors(qhard, iters, want_frame_info=True)
        cnt2, none = cs.count_errors(qhard, iters, counters=cnt.clone())              # accumulated, frame_info optional
        torch.cuda.synchronize()
    assert none is None
    for c in range(NCODES):
        wi, wq, _ = k["want_shared"][c]
        want_cnt, want_info = model_count(wq, None, wi, R)
        assert cnt[c].tolist() == want_cnt, (c, cnt[c].tolist(), want_cnt)
        assert np.array_equal(info[c].cpu().numpy(), want_info)
        assert cnt2[c].tolist() == [2 * v for v in want_cnt]
    assert cnt[:, 1].min() > 0 and len(set(cnt[:, 0].tolist())) > 1


SIM = dict(snr=1.6, seed=77, first_frame=1000, frames=150)


@pytest.fixture(scope="module")
def sim_reference(L, torch):
    """LdpcHipGfq.simulate(random_messages=False) per code of the M = 33 mixture, and its records through channel -> decode -> count."""
    k = case("gf16_cw2_mixture_M33")
    cnts, infos = [], []
    for c in range(NCODES):
        with L.LdpcHipGfq(4, k["hb"][c], k["hc"][c], 33) as one:
            cnts.append(one.simulate(SIM["snr"], MAXITER, SIM["frames"], SIM["seed"], first_frame=SIM["first_frame"], random_messages=False))
            soft = one.channel(sigma=one.sigma(SIM["snr"]), seed=SIM["seed"], first_frame=SIM["first_frame"], B=SIM["frames"])
            qh, it, _ = one.decode(soft, MAXITER)
            infos.append(one.count_errors(qh, None, it)[1].cpu().numpy())
    return np.array(cnts, dtype=np.uint64), np.array(infos)


def test_simulate_equals_the_single_code_chain(L, torch, sim_reference, monkeypatch):
    k = case("gf16_cw2_mixture_M33")
    want_cnt, want_info = sim_reference
    print("per-code counters:", want_cnt.tolist())
    assert (want_cnt[:, 1] > 0).all() and (want_cnt[:, 1] < SIM["frames"]).all() and len({tuple(r) for r in want_cnt.tolist()}) == NCODES
    s, f0, n = SIM["seed"], SIM["first_frame"], SIM["frames"]
    with L.LdpcHipCodesGfq(4, k["hb"], k["hc"], 33) as cs:
        assert cs.sigma(SIM["snr"]) == sigma_of(4, 8, SIM["snr"])
        cnt, info = cs.simulate(SIM["snr"], MAXITER, s, f0, n, records=True)
        assert cnt.dtype == np.uint64 and np.array_equal(cnt, want_cnt) and np.array_equal(info, want_info)
        assert np.array_equal(cs.simulate(SIM["snr"], MAXITER, s, f0, n), want_cnt)                  # counters are overwritten, records optional
        a, ia = cs.simulate(SIM["snr"], MAXITER, s, f0, 61, records=True)                            # B split over two calls
        b, ib = cs.simulate(SIM["snr"], MAXITER, s, f0 + 61, n - 61, records=True)
        assert np.array_equal(a + b, want_cnt) and np.array_equal(np.concatenate([ia, ib], axis=1), want_info)
        monkeypatch.setenv("LDPC_HIP_GFQ_PIECE", "37")
        cnt, info = cs.simulate(SIM["snr"], MAXITER, s, f0, n, records=True)
        assert np.array_equal(cnt, want_cnt) and np.array_equal(info, want_info)
        monkeypatch.setenv("LDPC_HIP_GFQ_SLOTS", "5")
        cnt, info = cs.simulate(SIM["snr"], MAXITER, s, f0, n, records=True)
        assert np.array_equal(cnt, want_cnt) and np.array_equal(info, want_info)
        monkeypatch.delenv("LDPC_HIP_GFQ_PIECE")
        assert np.array_equal(cs.simulate(SIM["snr"], MAXITER, s, f0, n), want_cnt)
        assert not cs.simulate(SIM["snr"], MAXITER, s, f0, 0).any()


STOP = dict(snr=2.4, seed=9, nfe=12, nexp=1500, ref_fer=0.05, batch=64)
_STOP_REF = {}


def stop_reference(L, first_frame=0):
    if first_frame not in _STOP_REF:
        hb, hc = weak_first_set()
        with L.LdpcHipCodesGfq(4, hb, hc, 8) as cs:
            _, info = cs.simulate(STOP["snr"], MAXITER, STOP["seed"], first_frame, STOP["nexp"] + 1, records=True)
        _STOP_REF[first_frame] = np.array([L.host.replay_stop_rule(row, STOP["nfe"], STOP["nexp"], STOP["ref_fer"]) for row in info], dtype=np.uint64)
    return _STOP_REF[first_frame]


def test_stopping_rule(L, torch, monkeypatch):
    hb, hc = weak_first_set()
    snr, seed, nfe, nexp, ref_fer, batch = (STOP[x] for x in ("snr", "seed", "nfe", "nexp", "ref_fer", "batch"))
    want = stop_reference(L)
    pieces = schedule(nexp, batch, batch)
    batches = [pieces[stop_piece(int(e), pieces)][0] for e in want[:, 0]]
    print("reference (experiment, nse, nde):", want.tolist(), "stop batches of 64:", batches)
    assert len(set(batches)) >= 2, "a set whose codes all stop together shows nothing"
    assert batches[0] == min(batches) and batches.count(batches[0]) == 1, "code 0 stops first and alone: slot 0 is code 1 afterwards"
    with L.LdpcHipCodesGfq(4, hb, hc, 8) as cs:
        cs.profile(True)
        got = cs.simulate_until(snr, MAXITER, seed, nfe, nexp, ref_fer, first_batch=batch, max_batch=batch)
        _, launches = cs.profile_read()
        runs = {"64/64": (got, pieces),
                "default": (cs.simulate_until(snr, MAXITER, seed, nfe, nexp, ref_fer), schedule(nexp, 1024, 65536)),
                "3/200": (cs.simulate_until(snr, MAXITER, seed, nfe, nexp, ref_fer, first_batch=3, max_batch=200), schedule(nexp, 3, 200))}
        monkeypatch.setenv("LDPC_HIP_GFQ_PIECE", "48")
        runs["pieces of 48"] = (cs.simulate_until(snr, MAXITER, seed, nfe, nexp, ref_fer, first_batch=batch, max_batch=batch), schedule(nexp, batch, batch, piece=48))
        monkeypatch.delenv("LDPC_HIP_GFQ_PIECE")
        assert launches == max(batches) + 1, "one decode launch per piece in which a code was running"
        cs.profile_read()
        for a, b in ((0, nexp), (-3, nexp), (nfe, -1)):                               # :591 fails before the first frame
            assert not cs.simulate_until(snr, MAXITER, seed, a, b, ref_fer).any()
        assert cs.profile_read()[1] == 0, "nothing is launched"
        other = cs.simulate_until(snr, MAXITER, seed, nfe, nexp, ref_fer, first_frame=1000, first_batch=batch, max_batch=batch)
    assert got.dtype == np.uint64 and got.shape == (len(hb), 4)
    for what, (res, sched) in runs.items():
        assert np.array_equal(res[:, :3], want), (what, res.tolist(), want.tolist())
        assert res[:, 3].tolist() == [frames_launched(int(e), sched) for e in want[:, 0]], (what, res.tolist())
    assert got[:, 3].tolist() == [min(batch * (b + 1), nexp + 1) for b in batches]
    want_other = stop_reference(L, first_frame=1000)
    assert not np.array_equal(want_other, want), "other noise, other counters"
    assert np.array_equal(other[:, :3], want_other)


def test_refusals_and_cross_use(L, torch):
    lib = L.load_library()
    hb, hc = shipped_set(8, 16)
    B, N, q = 4, 64, 16
    soft = torch.ones((NCODES, B, q, N), dtype=torch.float64, device="cuda")
    qh = torch.full((NCODES, B, N), -1, dtype=torch.int16, device="cuda")
    iters = torch.full((NCODES, B), -99, dtype=torch.int32, device="cuda")
    hard = torch.full((NCODES, B, 2), -1, dtype=torch.int32, device="cuda")
    dcnt = torch.zeros((NCODES, 5), dtype=torch.int64, device="cuda")
    cnt = (C.c_ulonglong * (5 * NCODES))()
    st = (C.c_ulonglong * (4 * NCODES))(*([5] * (4 * NCODES)))
    c4, sit = (C.c_ulonglong * 4)(), C.c_ulonglong()
    state = np.zeros(624, dtype=np.uint32)

    def untouched():
        torch.cuda.synchronize()
        return bool((qh == -1).all()) and bool((iters == -99).all()) and bool((hard == -1).all()) and not bool(dcnt.any()) and bool((soft == 1.0).all())

    def stop(h, maxiter=10, first_batch=64, max_batch=64, s=st, first_frame=0):
        return lib.ldpc_hip_simulate_codes_gfq_stop(h, 2.4, maxiter, 1, first_frame, 12, 100, 0.05, first_batch, max_batch, s)

    with L.LdpcHipCodesGfq(4, hb, hc, 8) as cs, L.LdpcHipGfq(4, hb[0], hc[0], 8) as gf, L.LdpcHip(MS_DEC, hb[0], 8) as one, \
            L.LdpcHipCodes(MS_DEC, hb, 8) as bs:
        cs.profile(True)
        x = soft.data_ptr()
        # bad arguments on the set itself
        for maxiter in (0, -5):
            assert lib.ldpc_hip_decode_codes_gfq_dev(cs.h, x, 0, B, maxiter, qh.data_ptr(), iters.data_ptr(), None, None) == EINVAL
            assert lib.ldpc_hip_simulate_codes_gfq(cs.h, 2.0, maxiter, 1, 0, B, cnt, None) == EINVAL
            assert stop(cs.h, maxiter=maxiter) == EINVAL
        assert lib.ldpc_hip_decode_codes_gfq_dev(cs.h, x, 0, -1, 10, qh.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_decode_codes_gfq_dev(cs.h, None, 0, B, 10, qh.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_decode_codes_gfq_dev(cs.h, x, 1, 1 << 30, 10, None, None, None, None) == EINVAL   # C * B beyond one launch
        assert lib.ldpc_hip_count_errors_codes_gfq_dev(cs.h, None, iters.data_ptr(), B, None, dcnt.data_ptr(), None) == EINVAL
        assert lib.ldpc_hip_count_errors_codes_gfq_dev(cs.h, qh.data_ptr(), iters.data_ptr(), B, None, None, None) == EINVAL
        assert lib.ldpc_hip_simulate_codes_gfq(cs.h, 2.0, 10, 1, 0, B, None, None) == EINVAL
        assert lib.ldpc_hip_simulate_codes_gfq(cs.h, 2.0, 10, 1, -1, B, cnt, None) == EINVAL
        assert stop(cs.h, s=None) == EINVAL and stop(cs.h, first_frame=-1) == EINVAL
        assert stop(cs.h, first_batch=0) == EINVAL and stop(cs.h, first_batch=65, max_batch=64) == EINVAL
        assert list(st) == [5] * len(st), "a refused call leaves state alone"
        # the binary code-set, single-code GF(q), binary and multi-device entry points on the GF(q) set
        assert lib.ldpc_hip_decode_codes_dev(cs.h, x, 1, B, 10, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_count_errors_codes_dev(cs.h, hard.data_ptr(), iters.data_ptr(), B, None, dcnt.data_ptr(), None) == EINVAL
        assert lib.ldpc_hip_simulate_codes(cs.h, 2.0, 0, 10, 0.8, 1, 0, B, cnt, None) == EINVAL
        assert lib.ldpc_hip_simulate_codes_stop(cs.h, 2.0, 0, 10, 0.8, 1, 0, 12, 100, 0.05, 64, 64, st) == EINVAL
        assert lib.ldpc_hip_decode_gfq_dev(cs.h, x, B, 10, 0.0, qh.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_decode_gfq_host(cs.h, x, B, 10, 0.0, None, None, None) == EINVAL
        assert lib.ldpc_hip_gfq_channel_dev(cs.h, None, None, 0.7, 1, 0, B, x, None) == EINVAL
        assert lib.ldpc_hip_count_errors_gfq_dev(cs.h, qh.data_ptr(), None, iters.data_ptr(), B, dcnt.data_ptr(), None, None) == EINVAL
        assert lib.ldpc_hip_simulate_gfq(cs.h, 2.0, 10, 1, 0, B, 0, cnt) == EINVAL
        assert lib.ldpc_hip_encode_gfq_dev(cs.h, None, 0, None, None, None) == EINVAL
        assert lib.ldpc_hip_gfq_coefficients(cs.h, qh.data_ptr()) == EINVAL and lib.ldpc_hip_gfq_k(cs.h) == 0
        assert lib.ldpc_hip_decode_dev(cs.h, x, B, 10, 0.8, hard.data_ptr(), iters.data_ptr(), None, None) == EINVAL
        assert "GF(q) code-set context" in lib.ldpc_hip_last_error().decode()
        assert lib.ldpc_hip_count_errors_dev(cs.h, hard.data_ptr(), iters.data_ptr(), B, None, dcnt.data_ptr(), None) == EINVAL
        assert lib.ldpc_hip_simulate(cs.h, 2.0, 0, 0, 10, 0.8, 1, 0, B, c4, C.byref(sit)) == EINVAL
        assert lib.ldpc_hip_awgn_llr_dev(cs.h, 2.0, 0, 0, 1, 0, B, x, None) == EINVAL
        assert lib.ldpc_hip_mt_set_state(cs.h, state.ctypes.data, 624) == EINVAL
        assert lib.ldpc_hip_mt_frames_slice(cs.h, 2.0, 0, 0, 10, 0.8, B, 0, B, iters.data_ptr(), iters.data_ptr()) == EINVAL
        # the queries
        assert lib.ldpc_hip_codes(cs.h) == NCODES and lib.ldpc_hip_gfq_q(cs.h) == 16
        assert lib.ldpc_hip_codes(gf.h) == 0 and lib.ldpc_hip_codes(one.h) == 0 and lib.ldpc_hip_gfq_q(one.h) == 0 and lib.ldpc_hip_gfq_q(bs.h) == 0
        assert lib.ldpc_hip_codes(bs.h) == NCODES and lib.ldpc_hip_gfq_q(gf.h) == 16
        # the GF(q) code-set entry points on a single GF(q) code, a binary code and a binary set
        for h in (gf.h, one.h, bs.h):
            assert lib.ldpc_hip_decode_codes_gfq_dev(h, x, 1, B, 10, qh.data_ptr(), iters.data_ptr(), None, None) == EINVAL
            assert lib.ldpc_hip_count_errors_codes_gfq_dev(h, qh.data_ptr(), iters.data_ptr(), B, None, dcnt.data_ptr(), None) == EINVAL
            assert lib.ldpc_hip_simulate_codes_gfq(h, 2.0, 10, 1, 0, B, cnt, None) == EINVAL
            assert stop(h) == EINVAL and "GF(q) code-set context" in lib.ldpc_hip_last_error().decode()
        assert untouched() and cs.profile_read()[1] == 0, "a refused call must not launch anything"
        assert stop(cs.h) == 0 and list(st)[0] > 0                                     # and the context still works
    # what the builder refuses, through the open call (the table test has every case)
    h = C.c_void_p()
    bad = hc.copy()
    bad[3, 1, 0] = 0
    assert lib.ldpc_hip_open_codes_gfq(4, 4, 8, 8, hb.ctypes.data, bad.ctypes.data, NCODES, 0, C.byref(h)) == -2 and not h.value
    assert "code 3" in lib.ldpc_hip_last_error().decode()
    assert lib.ldpc_hip_open_codes_gfq(4, 4, 8, 8, hb.ctypes.data, hc.ctypes.data, 0, 0, C.byref(h)) == EINVAL and not h.value
    assert lib.ldpc_hip_open_codes_gfq(4, 4, 8, 8, hb.ctypes.data, hc.ctypes.data, NCODES, 99, C.byref(h)) == EINVAL and not h.value


def test_cpp_layer_takes_both_routes(L, torch, tmp_path):
    """ldpc::bp_simulation_codes_gfq with show_process = 0 (the rule on the device) and = 1 (the records replayed on the host) on the
    stopping-rule set: the same return values and counters, and those of simulate_until."""
    L.load_library()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = str(tmp_path / "codes_gfq_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "codes_gfq_driver.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_compat", "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    hb, hc = weak_first_set()
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(hb), hb.shape[1], hb.shape[2], 8, 16, MAXITER, STOP["nfe"], STOP["nexp"], STOP["batch"], STOP["seed"]], dtype=np.int32).tobytes())
        f.write(np.array([STOP["snr"], STOP["ref_fer"]], dtype=np.float64).tobytes())
        f.write(hb.tobytes())
        f.write(hc.tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "in.bin")], timeout=120).decode().split("\n")
    rows = {(w[0], int(w[1])): w[2:] for w in (line.split() for line in out if line.startswith(("device ", "host ")))}
    assert len(rows) == 2 * len(hb), out
    assert any(line.startswith("code=") for line in out), "show_process = 1 prints a line per error frame"
    want = stop_reference(L)
    K = (hb.shape[2] - hb.shape[1]) * 8
    for c in range(len(hb)):
        assert rows["device", c] == rows["host", c], (c, rows["device", c], rows["host", c])
        assert [int(v) for v in rows["device", c][2:]] == [int(want[c, 1]), int(want[c, 2]), int(want[c, 0])], c
        ser, fer = (float.fromhex(v) for v in rows["device", c][:2])
        assert ser == int(want[c, 1]) / int(want[c, 0]) / K and fer == int(want[c, 2]) / int(want[c, 0])
