"""An SNR grid on binary code sets (ldpc_hip_*_codes_grid*, LdpcHipCodes.*_grid*, ldpc::bp_simulation_codes_grid*, `ldpc_sim --snr-grid`;
DESIGN 4.27): P points x C codes decoded as P * C work items over one noise draw.  Everything is compared with tolerance 0 against the
single-SNR set calls (test_gpu_codeset_exact.py, test_gpu_codeset_stop.py check those against single contexts and the CPU oracle) on
the same context or the same seed; the rule test also against the CPU oracle itself."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import codeset_wide_sets as WIDE
from codeset_gfq_sets import weak_first_set
from codeset_grid_sets import (DECS, GLOBAL_GRID, GLOBAL_LIFTINGS, IMS_DEC, MAX_POINTS, PIECE, RECORD_FRAMES, RECORD_LIFTINGS, RECORD_POINTS, RULE_BATCHES,
                               RULE_DECS, RULE_EXPERIMENTS, RULE_FRAME_ERRORS, RULE_LIFTING, RULE_POINTS, RULE_REFERENCES, SEED, TASP_DEC, WIDE_POINTS,
                               WIDE_SET, ending)
from codeset_stop_sets import MAXITER, NH, RH, code_set, frames_launched, schedule
from ldpc_testlib import LMS_DEC, MS_DEC, ROOT, SimResult, c_int_p, oracle_lib

pytestmark = pytest.mark.gpu

EINVAL = -1
FIRST_FRAME = 5   # of the Philox runs


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def entry_state(L, M, rh=RH, nh=NH):
    """std::mt19937(SEED) after the codeword draws of bp_simulation.cpp:512: where the first frame's noise starts"""
    return L.mt19937_state(SEED, (nh - rh) * M)


def next_word(state, pos):
    bg = np.random.MT19937()
    s = bg.state
    s["state"]["key"] = np.array(state, dtype=np.uint32)
    s["state"]["pos"] = int(pos)
    bg.state = s
    return int(bg.random_raw(1)[0])


def same_state(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1]


def single_records(cs, st, points, B, punct=0, alpha=0.8):
    """The single-SNR set calls on the same context, one per point: stacked (counters, frame_info, iters), the generator after the
    exact call, and the Philox (counters, frame_info)"""
    exact, philox, after = [], [], None
    for snr in points:
        cs.mt_set_state(*st)
        exact.append(cs.mt_simulate(snr, MAXITER, B, punctured_blocks=punct, alpha=alpha, records=True))
        now = cs.mt_get_state()
        assert after is None or same_state(after, now), "B frames are B frames at any SNR"
        after = now
        philox.append(cs.simulate(snr, MAXITER, SEED, FIRST_FRAME, B, punctured_blocks=punct, alpha=alpha, records=True))
    return [np.stack(x) for x in zip(*exact)], after, [np.stack(x) for x in zip(*philox)]


def check_grid_records(cs, st, points, B, punct=0, alpha=0.8, want=None):
    """mt_simulate_grid and simulate_grid against single_records (or against `want`, taken earlier)"""
    (cnt, info, its), after, (pcnt, pinfo) = want or single_records(cs, st, points, B, punct, alpha)
    P = len(points)
    cs.mt_set_state(*st)
    g_cnt, g_info, g_its = cs.mt_simulate_grid(points, MAXITER, B, punctured_blocks=punct, alpha=alpha, records=True)
    assert g_cnt.shape == (P, cs.C, 5) and g_info.shape == g_its.shape == (P, cs.C, B) and g_cnt.dtype == np.uint64
    for p in range(P):
        assert np.array_equal(g_info[p], info[p]), (p, np.argwhere(g_info[p] != info[p])[:4].tolist())
        assert np.array_equal(g_its[p], its[p]), (p, np.argwhere(g_its[p] != its[p])[:4].tolist())
        assert np.array_equal(g_cnt[p], cnt[p]), (p, g_cnt[p].tolist(), cnt[p].tolist())
    assert same_state(cs.mt_get_state(), after), "the generator ends B frames further on, once"
    cs.mt_set_state(*st)
    assert np.array_equal(cs.mt_simulate_grid(points, MAXITER, B, punctured_blocks=punct, alpha=alpha), cnt), "without records"
    q_cnt, q_info = cs.simulate_grid(points, MAXITER, SEED, FIRST_FRAME, B, punctured_blocks=punct, alpha=alpha, records=True)
    assert q_cnt.shape == (P, cs.C, 5) and q_info.shape == (P, cs.C, B)
    assert np.array_equal(q_info, pinfo) and np.array_equal(q_cnt, pcnt), np.argwhere(q_info != pinfo)[:4].tolist()
    return g_info, g_its


# ---- 1. records ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dec", list(DECS.values()), ids=list(DECS))
def test_records_equal_the_single_snr_calls(L, torch, dec):
    for M in RECORD_LIFTINGS:
        with L.LdpcHipCodes(dec, code_set(M), M) as cs:
            info, _ = check_grid_records(cs, entry_state(L, M), RECORD_POINTS, RECORD_FRAMES)
        assert (info != 0).any() and (info == 0).any(), "a grid without error frames, or with nothing else, shows little"
        assert not np.array_equal(info[0], info[1]) and not np.array_equal(info[0], info[2]), "points that differ in nothing show nothing"


# ---- 2. routes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dec", WIDE.DECS, ids=[WIDE.DEC_IDS[d] for d in WIDE.DECS])
def test_wide_route(L, torch, dec):
    M, codes = WIDE.code_set(WIDE_SET)
    rh, nh = codes.shape[1:]
    assert rh > 16
    with L.LdpcHipCodes(dec, codes, M) as cs:
        assert cs.entry == "ldpc_hip_open_codes_wide" and cs.kernel_name.startswith(WIDE.KERNEL[dec])
        info, _ = check_grid_records(cs, entry_state(L, M, rh, nh), WIDE_POINTS[dec], RECORD_FRAMES)
    assert (info != 0).any() and (info == 0).any()


@pytest.mark.parametrize("dec", list(DECS.values()), ids=list(DECS))
def test_global_route(L, torch, monkeypatch, dec):
    monkeypatch.setenv("LDPC_HIP_CODES_GLOBAL_GRID", str(GLOBAL_GRID))   # few workgroups walk many items
    for M in GLOBAL_LIFTINGS:
        with L.LdpcHipCodes(dec, code_set(M), M, tier="global") as cs:
            assert cs.entry == "ldpc_hip_open_codes_global" and "global_codes_kernel" in cs.kernel_name
            info, _ = check_grid_records(cs, entry_state(L, M), RECORD_POINTS, RECORD_FRAMES)
        assert (info != 0).any() and (info == 0).any()


def test_global_route_takes_alpha_below_zero(L, torch):
    M = 20
    with L.LdpcHipCodes(MS_DEC, code_set(M), M, tier="global") as cs:
        check_grid_records(cs, entry_state(L, M), RECORD_POINTS, RECORD_FRAMES, alpha=-0.5)


# ---- 3. pieces ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dec", list(DECS.values()), ids=list(DECS))
def test_pieces_do_not_matter(L, torch, monkeypatch, dec):
    for M in RECORD_LIFTINGS:   # the liftings of test 1, the two waves per frame of M = 126 among them
        st = entry_state(L, M)
        with L.LdpcHipCodes(dec, code_set(M), M) as cs:
            want = single_records(cs, st, RECORD_POINTS, RECORD_FRAMES)   # in one piece
            monkeypatch.setenv("LDPC_HIP_CODES_PIECE", str(PIECE))        # pieces of 16, 16 and 5: the strided copies into [P][C][B]
            check_grid_records(cs, st, RECORD_POINTS, RECORD_FRAMES, want=want)
            monkeypatch.delenv("LDPC_HIP_CODES_PIECE")


# ---- 4. the rule --------------------------------------------------------------------------------------------------------------------
def oracle_run(H, M, dec, snr, nfe, nexp, ref):
    res = SimResult()
    Hc = np.ascontiguousarray(H, dtype=np.int32)
    assert oracle_lib().orc_bp_simulation(H.shape[0], H.shape[1], Hc.ctypes.data_as(c_int_p), M, MAXITER, nfe, nexp, snr, ref, dec, 0, 0, SEED, C.byref(res),
                                          None) == 0
    return [res.experiment, res.nse, res.nde, res.nue, res.sum_abs_iter], res.rng_next


@pytest.mark.parametrize("dec", list(RULE_DECS.values()), ids=list(RULE_DECS))
def test_rule_per_item(L, torch, dec):
    M, nfe, nexp = RULE_LIFTING, RULE_FRAME_ERRORS, RULE_EXPERIMENTS
    first_batch, max_batch = RULE_BATCHES
    codes = code_set(M)
    st = entry_state(L, M)
    P = len(RULE_POINTS)
    with L.LdpcHipCodes(dec, codes, M) as cs:
        single, single_philox = [], []
        for snr, ref in zip(RULE_POINTS, RULE_REFERENCES):
            cs.mt_set_state(*st)
            single.append(cs.mt_simulate_until(snr, MAXITER, nfe, nexp, ref, first_batch=first_batch, max_batch=max_batch))
            single_philox.append(cs.simulate_until(snr, MAXITER, SEED, nfe, nexp, ref, first_frame=FIRST_FRAME, first_batch=first_batch, max_batch=max_batch))
        single, single_philox = np.stack(single), np.stack(single_philox)
        endings = {ending(single[p, c]) for p in range(P) for c in range(len(codes))}
        print("single-SNR states:", single.tolist())
        assert endings == {"frame_errors", "fer_rule", "experiments"}, endings
        assert len({int(e) for e in single[:, :, 0].ravel()}) >= 6, "items that all stop together show nothing"

        cs.mt_set_state(*st)
        got = cs.mt_simulate_grid_until(RULE_POINTS, MAXITER, nfe, nexp, RULE_REFERENCES, first_batch=first_batch, max_batch=max_batch)
        assert got.shape == (P, len(codes), 6) and got.dtype == np.uint64
        assert np.array_equal(got[:, :, :5], single[:, :, :5]), (got.tolist(), single.tolist())
        pieces = schedule(nexp, first_batch, max_batch)
        assert got[:, :, 5].tolist() == [[frames_launched(int(e), pieces) for e in row] for row in single[:, :, 0]], got[:, :, 5].tolist()
        assert np.array_equal(got[:, :, 5], single[:, :, 5])
        assert same_state(cs.mt_get_state(), st), "the run puts the generator back where it found it"
        for p, (snr, ref) in enumerate(zip(RULE_POINTS, RULE_REFERENCES)):
            for c, H in enumerate(codes):
                cnt, rng_next = oracle_run(H, M, dec, snr, nfe, nexp, ref)
                assert got[p, c, :5].tolist() == cnt, (p, c, got[p, c].tolist(), cnt)
                cs.mt_set_state(*st)
                cs.mt_advance(snr, int(got[p, c, 0]))
                assert next_word(*cs.mt_get_state()) == rng_next, (p, c)

        philox = cs.simulate_grid_until(RULE_POINTS, MAXITER, SEED, nfe, nexp, RULE_REFERENCES, first_frame=FIRST_FRAME, first_batch=first_batch,
                                        max_batch=max_batch)
        assert philox.shape == (P, len(codes), 4) and np.array_equal(philox, single_philox), (philox.tolist(), single_philox.tolist())

        # nothing to do: no frame is consumed (:591 fails before the first frame)
        cs.mt_set_state(*st)
        for a, b in ((0, nexp), (-3, nexp), (nfe, -1)):
            assert not cs.mt_simulate_grid_until(RULE_POINTS, MAXITER, a, b, RULE_REFERENCES).any()
            assert not cs.simulate_grid_until(RULE_POINTS, MAXITER, SEED, a, b, RULE_REFERENCES).any()
        assert same_state(cs.mt_get_state(), st)


def test_rule_with_small_pieces(L, torch, monkeypatch):
    dec, M, nfe, nexp = MS_DEC, RULE_LIFTING, RULE_FRAME_ERRORS, RULE_EXPERIMENTS
    st = entry_state(L, M)
    with L.LdpcHipCodes(dec, code_set(M), M) as cs:
        cs.mt_set_state(*st)
        want = cs.mt_simulate_grid_until(RULE_POINTS, MAXITER, nfe, nexp, RULE_REFERENCES, first_batch=64, max_batch=256)
        monkeypatch.setenv("LDPC_HIP_CODES_PIECE", "7")
        for first_batch, max_batch in ((1, 256), (64, 1024)):
            cs.mt_set_state(*st)
            got = cs.mt_simulate_grid_until(RULE_POINTS, MAXITER, nfe, nexp, RULE_REFERENCES, first_batch=first_batch, max_batch=max_batch)
            assert np.array_equal(got[:, :, :5], want[:, :, :5]), (first_batch, max_batch)
            pieces = schedule(nexp, first_batch, max_batch, piece=7)
            assert got[:, :, 5].tolist() == [[frames_launched(int(e), pieces) for e in row] for row in want[:, :, 0]]
        monkeypatch.delenv("LDPC_HIP_CODES_PIECE")


# ---- 5. degenerate grids ------------------------------------------------------------------------------------------------------------
def test_one_point_and_equal_points(L, torch):
    M, B = 32, RECORD_FRAMES
    st = entry_state(L, M)
    with L.LdpcHipCodes(MS_DEC, code_set(M), M) as cs:
        check_grid_records(cs, st, (2.5,), B)
        info, its = check_grid_records(cs, st, (2.5, 2.5), B)
        assert np.array_equal(info[0], info[1]) and np.array_equal(its[0], its[1])
        cs.mt_set_state(*st)
        one = cs.mt_simulate_until(2.5, MAXITER, 7, 300, 1.0, first_batch=64, max_batch=64)
        cs.mt_set_state(*st)
        grid = cs.mt_simulate_grid_until(2.5, MAXITER, 7, 300, 1.0, first_batch=64, max_batch=64)   # a scalar is a grid of one point
        assert grid.shape == (1, cs.C, 6) and np.array_equal(grid[0], one)


def test_single_calls_after_a_grid_are_sized_by_themselves(L, torch):
    """The workspace counts rows: a grid call, then single-SNR calls with more frames than the grid's piece, then the grid again"""
    M = 32
    st = entry_state(L, M)
    with L.LdpcHipCodes(MS_DEC, code_set(M), M) as fresh:
        want = single_records(fresh, st, (2.5,), 200)
    with L.LdpcHipCodes(MS_DEC, code_set(M), M) as cs:
        check_grid_records(cs, st, RECORD_POINTS, 8)
        got = single_records(cs, st, (2.5,), 200)   # 200 rows > the 24 the grid reserved
        for a, b in zip(want[0] + want[2], got[0] + got[2]):
            assert np.array_equal(a, b)
        check_grid_records(cs, st, RECORD_POINTS, RECORD_FRAMES)   # 111 rows fit the 200


def test_sixty_four_points(L, torch):
    M, B = 20, 8
    points = tuple(0.5 + 0.0625 * ((37 * p) % MAX_POINTS) for p in range(MAX_POINTS))   # unsorted, all different
    with L.LdpcHipCodes(LMS_DEC, code_set(M), M) as cs:
        info, _ = check_grid_records(cs, entry_state(L, M), points, B)
    assert len(points) == MAX_POINTS and (info != 0).any() and (info == 0).any()


@pytest.mark.parametrize("dec", [LMS_DEC, TASP_DEC], ids=["lms_0p5", "tdmp_0p0"])
def test_two_punctured_blocks(L, torch, dec):
    M = 32
    with L.LdpcHipCodes(dec, code_set(M), M) as cs:
        st = entry_state(L, M)
        info, _ = check_grid_records(cs, st, (4.5, 3.0, 5.5), RECORD_FRAMES, punct=2)
        plain, _ = check_grid_records(cs, st, (4.5, 3.0, 5.5), RECORD_FRAMES)
    assert not np.array_equal(info, plain), "other positions erased, other records"


def test_integer_min_sum_with_other_parameters(L, torch):
    for M in (20, 126):
        st = entry_state(L, M)
        with L.LdpcHipCodes(IMS_DEC, code_set(M), M) as cs:
            default, _ = check_grid_records(cs, st, RECORD_POINTS, RECORD_FRAMES)
            cs.set_ims_params(1.1, 5, 7)
            other, _ = check_grid_records(cs, st, RECORD_POINTS, RECORD_FRAMES)
        assert not np.array_equal(default, other), "a quantiser that changes nothing shows nothing"


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(L, torch):
    lib = L.load_library()
    M = 32
    codes = code_set(M)
    st, pos = entry_state(L, M)
    snr = np.array(RULE_POINTS, dtype=np.float64)
    ref = np.array(RULE_REFERENCES, dtype=np.float64)
    P, Cn = len(snr), len(codes)
    cnt = np.full((P, Cn, 5), 7, dtype=np.uint64)
    state = np.full((P, Cn, 6), 7, dtype=np.uint64)
    info = np.full((P, Cn, 8), 7, dtype=np.int32)

    def calls(h, snr_p=snr.ctypes.data, P=P, punct=0, maxiter=MAXITER, alpha=0.8, ref_p=ref.ctypes.data, first_batch=64, max_batch=64):
        return [lib.ldpc_hip_simulate_codes_grid(h, snr_p, P, punct, maxiter, alpha, SEED, 0, 8, cnt.ctypes.data, info.ctypes.data),
                lib.ldpc_hip_simulate_codes_grid_stop(h, snr_p, P, punct, maxiter, alpha, SEED, 0, 12, 100, ref_p, first_batch, max_batch, state.ctypes.data),
                lib.ldpc_hip_mt_simulate_codes_grid(h, snr_p, P, punct, maxiter, alpha, 8, cnt.ctypes.data, info.ctypes.data, info.ctypes.data),
                lib.ldpc_hip_mt_simulate_codes_grid_stop(h, snr_p, P, punct, maxiter, alpha, 12, 100, ref_p, first_batch, max_batch, state.ctypes.data)]

    def untouched():
        return (cnt == 7).all() and (state == 7).all() and (info == 7).all()

    hb, hc = weak_first_set()
    with L.LdpcHip(MS_DEC, codes[1], M) as lone, L.LdpcHipCodesGfq(4, hb, hc, 8) as gfq_set:
        for ctx in (lone, gfq_set):
            assert calls(ctx.h) == [EINVAL] * 4, type(ctx).__name__
            assert "code-set context" in lib.ldpc_hip_last_error().decode()
    assert untouched()
    with L.LdpcHipCodes(MS_DEC, codes, M) as cs:
        assert calls(cs.h)[2:] == [EINVAL] * 2 and "no state" in lib.ldpc_hip_last_error().decode()   # no generator state yet
        cnt[:], state[:], info[:] = 7, 7, 7   # the two Philox calls ran
        cs.mt_set_state(st, pos)
        cs.profile(True)
        for P_bad in (0, -1, MAX_POINTS + 1):
            assert calls(cs.h, P=P_bad) == [EINVAL] * 4
            msg = lib.ldpc_hip_last_error().decode()
            assert "ldpc_hip_mt_simulate_codes_grid_stop" in msg and str(P_bad) in msg, msg
        assert calls(cs.h, snr_p=None) == [EINVAL] * 4 and "snr_db" in lib.ldpc_hip_last_error().decode()
        got = calls(cs.h, ref_p=None)
        assert got[1] == got[3] == EINVAL and "reference_frame_error" in lib.ldpc_hip_last_error().decode()
        cnt[:], info[:] = 7, 7   # the two fixed-length calls take no reference and ran
        cs.mt_set_state(st, pos)
        cs.profile_read()
        bad = np.array([2.0, np.nan, 3.0], dtype=np.float64)
        assert calls(cs.h, snr_p=bad.ctypes.data) == [EINVAL] * 4 and "point 1" in lib.ldpc_hip_last_error().decode()
        assert calls(cs.h, maxiter=0) == [EINVAL] * 4 and "maxiter" in lib.ldpc_hip_last_error().decode()
        assert calls(cs.h, punct=NH) == [EINVAL] * 4 and calls(cs.h, punct=-1) == [EINVAL] * 4
        assert calls(cs.h, alpha=float("nan")) == [EINVAL] * 4 and "NaN" in lib.ldpc_hip_last_error().decode()
        assert calls(cs.h, alpha=0.0) == [EINVAL] * 4 and calls(cs.h, alpha=-0.5) == [EINVAL] * 4   # MS_DEC off the global route
        assert "ldpc_hip_open_codes_global" in lib.ldpc_hip_last_error().decode()
        got = calls(cs.h, first_batch=0)
        assert got[1] == got[3] == EINVAL
        got = calls(cs.h, first_batch=65)
        assert got[1] == got[3] == EINVAL
        assert lib.ldpc_hip_mt_simulate_codes_grid(cs.h, snr.ctypes.data, P, 0, MAXITER, 0.8, 8, None, None, None) == EINVAL
        assert lib.ldpc_hip_mt_simulate_codes_grid_stop(cs.h, snr.ctypes.data, P, 0, MAXITER, 0.8, 12, 100, ref.ctypes.data, 64, 64, None) == EINVAL
        assert lib.ldpc_hip_simulate_codes_grid(cs.h, snr.ctypes.data, P, 0, MAXITER, 0.8, SEED, -1, 8, cnt.ctypes.data, None) == EINVAL


def test_refusals_leave_everything_alone(L, torch):
    """The refusals that test_refusals mixes with calls that run, here alone: outputs, launches and the generator"""
    lib = L.load_library()
    M = 32
    codes = code_set(M)
    st, pos = entry_state(L, M)
    snr = np.array(RULE_POINTS, dtype=np.float64)
    ref = np.array(RULE_REFERENCES, dtype=np.float64)
    bad = np.array([2.0, 3.0, np.inf], dtype=np.float64)
    P, Cn = len(snr), len(codes)
    cnt = np.full((P, Cn, 5), 7, dtype=np.uint64)
    state = np.full((P, Cn, 6), 7, dtype=np.uint64)
    info = np.full((P, Cn, 8), 7, dtype=np.int32)
    with L.LdpcHipCodes(MS_DEC, codes, M) as cs:
        cs.mt_set_state(st, pos)
        cs.profile(True)
        cs.profile_read()
        for kw in (dict(P=0), dict(P=MAX_POINTS + 1), dict(snr_p=None), dict(snr_p=bad.ctypes.data), dict(maxiter=0), dict(punct=NH), dict(alpha=float("nan")),
                   dict(alpha=0.0)):
            a = dict(snr_p=snr.ctypes.data, P=P, punct=0, maxiter=MAXITER, alpha=0.8)
            a.update(kw)
            rcs = [lib.ldpc_hip_simulate_codes_grid(cs.h, a["snr_p"], a["P"], a["punct"], a["maxiter"], a["alpha"], SEED, 0, 8, cnt.ctypes.data, info.ctypes.data),
                   lib.ldpc_hip_simulate_codes_grid_stop(cs.h, a["snr_p"], a["P"], a["punct"], a["maxiter"], a["alpha"], SEED, 0, 12, 100, ref.ctypes.data, 64, 64,
                                                         state.ctypes.data),
                   lib.ldpc_hip_mt_simulate_codes_grid(cs.h, a["snr_p"], a["P"], a["punct"], a["maxiter"], a["alpha"], 8, cnt.ctypes.data, info.ctypes.data,
                                                       info.ctypes.data),
                   lib.ldpc_hip_mt_simulate_codes_grid_stop(cs.h, a["snr_p"], a["P"], a["punct"], a["maxiter"], a["alpha"], 12, 100, ref.ctypes.data, 64, 64,
                                                            state.ctypes.data)]
            assert rcs == [EINVAL] * 4, (kw, rcs)
        for kw in (dict(ref_p=None), dict(first_batch=0), dict(first_batch=65)):
            a = dict(ref_p=ref.ctypes.data, first_batch=64)
            a.update(kw)
            rcs = [lib.ldpc_hip_simulate_codes_grid_stop(cs.h, snr.ctypes.data, P, 0, MAXITER, 0.8, SEED, 0, 12, 100, a["ref_p"], a["first_batch"], 64,
                                                         state.ctypes.data),
                   lib.ldpc_hip_mt_simulate_codes_grid_stop(cs.h, snr.ctypes.data, P, 0, MAXITER, 0.8, 12, 100, a["ref_p"], a["first_batch"], 64,
                                                            state.ctypes.data)]
            assert rcs == [EINVAL] * 2, (kw, rcs)
        assert (cnt == 7).all() and (state == 7).all() and (info == 7).all(), "a refused call leaves its outputs alone"
        assert cs.profile_read()[1] == 0, "... launches nothing"
        assert same_state(cs.mt_get_state(), (st, pos)), "... and leaves the generator alone"
        got = cs.mt_simulate_grid_until(RULE_POINTS, MAXITER, 12, 100, RULE_REFERENCES, first_batch=64, max_batch=64)
        assert (got[:, :, 0] > 0).all()   # and the context still works


# ---- 7. the C++ layer and ldpc_sim --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def compat(L):
    L.load_library()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    lib = C.CDLL(os.path.join(ROOT, "ldpc-lib_amd", "libldpc_compat.so"))
    lib.ldpc_bp_simulation_codes_exact.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                                   C.c_int, C.c_int, C.c_uint, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]
    lib.ldpc_bp_simulation_codes_grid.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                  C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_int,
                                                  C.c_void_p, C.c_void_p]
    lib.ldpc_bp_simulation_codes_grid_device_runs.restype = C.c_longlong
    return lib


@pytest.mark.parametrize("show", [0, 1])
@pytest.mark.parametrize("noise", ["device", "host"])
def test_cpp_layer(L, torch, compat, monkeypatch, noise, show):
    dec, M, nfe, nexp = MS_DEC, RULE_LIFTING, RULE_FRAME_ERRORS, RULE_EXPERIMENTS
    monkeypatch.setenv("LDPC_HIP_EXACT_NOISE", noise)
    codes = code_set(M)
    Cn, P = len(codes), len(RULE_POINTS)
    flat = np.ascontiguousarray(codes, dtype=np.int32)
    snr = np.array(RULE_POINTS, dtype=np.float64)
    ref = np.array(RULE_REFERENCES, dtype=np.float64)
    loop = np.zeros((P, Cn, 7), dtype=np.float64)
    loop_next = {}
    for p in range(P):   # the loop of the single-SNR function, each call from the reset generator
        for leave_at in (0, -1):
            nxt = C.c_uint()
            assert compat.ldpc_bp_simulation_codes_exact(Cn, RH, NH, flat.ctypes.data, M, MAXITER, nfe, nexp, snr[p], ref[p], dec, 0, 0, SEED, 0, 64, 256,
                                                         leave_at, loop[p].ctypes.data, C.addressof(nxt)) == 0
            loop_next[(p, leave_at)] = nxt.value
    assert len(set(loop_next.values())) >= 4, "pairs that all leave the generator at one place show nothing"
    assert len({loop_next[(P - 1, -1)], loop_next[(1, 0)], loop_next[(0, -1)]}) == 3, "the three pairs asked for below"
    for leave_at, leave_point in ((-1, -1), (0, 1), (-1, 0)):
        out = np.zeros((P, Cn, 7), dtype=np.float64)
        nxt = C.c_uint()
        runs = compat.ldpc_bp_simulation_codes_grid_device_runs()
        assert compat.ldpc_bp_simulation_codes_grid(1, Cn, RH, NH, flat.ctypes.data, M, MAXITER, nfe, nexp, P, snr.ctypes.data, ref.ctypes.data, dec, 0, show,
                                                    SEED, 0, 64, 256, leave_at, leave_point, out.ctypes.data, C.addressof(nxt)) == 0
        assert np.array_equal(out, loop), (leave_at, leave_point, out.tolist(), loop.tolist())
        # the numbers do not tell the one grid call from the per-SNR loop the function falls back to: the count of grid calls does
        assert compat.ldpc_bp_simulation_codes_grid_device_runs() - runs == (1 if noise == "device" and not show else 0), (noise, show)
        assert nxt.value == loop_next[(leave_point if leave_point >= 0 else P - 1, leave_at)], (leave_at, leave_point)
    assert {ending(loop[p, c, [5, 2, 3]]) for p in range(P) for c in range(Cn)} == {"frame_errors", "fer_rule", "experiments"}


@pytest.mark.parametrize("show", [0, 1])
def test_cpp_layer_philox(L, torch, compat, show):
    dec, M, nfe, nexp = LMS_DEC, RULE_LIFTING, RULE_FRAME_ERRORS, RULE_EXPERIMENTS
    codes = code_set(M)
    Cn, P = len(codes), len(RULE_POINTS)
    flat = np.ascontiguousarray(codes, dtype=np.int32)
    snr = np.array(RULE_POINTS, dtype=np.float64)
    ref = np.array(RULE_REFERENCES, dtype=np.float64)
    out = np.zeros((P, Cn, 7), dtype=np.float64)
    assert compat.ldpc_bp_simulation_codes_grid(0, Cn, RH, NH, flat.ctypes.data, M, MAXITER, nfe, nexp, P, snr.ctypes.data, ref.ctypes.data, dec, 0, show, SEED,
                                                0, 64, 256, -1, -1, out.ctypes.data, None) == 0
    with L.LdpcHipCodes(dec, codes, M) as cs:
        for p in range(P):
            want = cs.simulate_until(snr[p], MAXITER, SEED, nfe, nexp, ref[p], first_batch=64, max_batch=256)
            assert np.array_equal(out[p][:, [5, 2, 3]].astype(np.uint64), want[:, :3]), (p, out[p].tolist(), want.tolist())
            info_len = (NH - RH) * M
            assert out[p][:, 1].tolist() == [int(w[2]) / int(w[0]) for w in want] and out[p][:, 0].tolist() == [int(w[1]) / int(w[0]) / info_len for w in want]


def code_record(H, dec, M, snrs):
    rows = "\n".join("        " + " ".join("%4d" % v for v in row) for row in H)
    return """    {
      _SNRs = array { %s }
      _decoder_type = %d
      _iterations = %d
      _lifting = %d
      _q_mod = 2
      _marking = "skip"
      _punctured_blocks = 0
      code = matrix (%d %d) {
%s
      }
      girth = 6
    }""" % (" ".join(str(s) for s in snrs), dec, MAXITER, M, H.shape[0], H.shape[1], rows)


def test_ldpc_sim_snr_grid(L, torch, tmp_path):
    M = 32
    codes = code_set(M)
    snrs = (2.0, 3.0, 1.5)
    # a group of three codes, and one code with another decoder: a group of one, which --code-sets alone leaves to the single-code path
    records = [code_record(codes[c], MS_DEC, M, snrs) for c in (1, 2, 3)] + [code_record(codes[1], LMS_DEC, M, snrs)]
    scenario = tmp_path / "scenario.jsonx"
    scenario.write_text("""{
  settings = {
    random_seed = 3
    num_codewords = 300
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
    grid = subprocess.run([exe, "simulation", str(scenario), str(tmp_path / "grid.jsonx"), "--snr-grid"], capture_output=True, text=True, timeout=120, env=env)
    sets = subprocess.run([exe, "simulation", str(scenario), str(tmp_path / "sets.jsonx"), "--code-sets"], capture_output=True, text=True, timeout=120, env=env)
    assert plain.returncode == 0 and grid.returncode == 0 and sets.returncode == 0, (plain.stderr, grid.stderr, sets.stderr)
    assert "set of 3 codes from code #0 on, grid of 3 SNRs" in grid.stdout and "set of 1 codes from code #3 on, grid of 3 SNRs" in grid.stdout
    assert grid.stdout.count("one grid call") == 2 and "per-SNR calls" not in grid.stdout, "the grid ran, not the fallback loop inside the function"
    assert "grid of" not in sets.stdout and "set of 1 codes" not in sets.stdout and sets.stdout.count("set of 3 codes") == 3, "--code-sets alone is as it was"

    def without_time(path):
        text = path.read_text()
        assert len(re.findall(r"\btime = \S+", text)) == 4
        return re.sub(r"\btime = \S+", "time = -", text)

    a, b, c = (without_time(tmp_path / n) for n in ("plain.jsonx", "grid.jsonx", "sets.jsonx"))
    assert a == b and a == c
    for code in (0, 3):
        fer = subprocess.check_output([exe, "jsonx-get", str(tmp_path / "grid.jsonx"), "results/%d/simulation_logs/0/FER" % code], text=True)
        assert any(float(x) > 0 for x in fer.replace("array {", "").replace("}", "").split()), "error-free points compare nothing"
