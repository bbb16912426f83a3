"""Inputs of the integer min-sum code-set tests (test_codeset_ims_cpu.py checks them on the CPU, test_gpu_codeset_ims.py decodes
them): the code sets of test_gpu_codeset.py's builder, channel values at a fixed SNR per case, the quantiser parameter sets, a set
around the compiled reference's golden vector, the shapes only this set kernel reaches, and the CPU oracle's results
(orc_imin_sum), computed once.  The seeds and SNRs are constants: the CPU test asserts that they have the required properties,
nothing is searched at GPU time."""
import os

import numpy as np

from codeset_lche_sets import mixed_weight_set as _lche_mixed_weight_set
from codeset_lche_sets import relabelled
from codeset_lche_sets import rows17_set as _lche_rows17_set
from codeset_stop_sets import code_set as strength_set
from ldpc_testlib import GOLDEN_DIR, Oracle, _as_double_p, adversarial_llr, awgn_llr, oracle_lib, pack_bits
from test_gpu_codeset import make_code_set

IMS_DEC, MS_DEC = 4, 3
MAXITER = 20
NCODES, NFRAMES = 5, 7
LDS_LIMIT = 160 * 1024
DEFAULTS = (0.8, 1.4, 6, 8)     # alpha, thr, qbits, dbits
# (M, rh, nh) -> SNR in dB at which, in both LLR layouts, at least 6 of the 35 (code, frame) pairs converge after 2 .. MAXITER - 1
# iterations and at least 6 give up with -MAXITER
CASES = {(1, 4, 8): 1.0, (5, 4, 8): 1.5, (20, 4, 8): 2.5, (32, 4, 8): 3.0, (64, 4, 8): 3.5, (100, 3, 6): 3.5, (126, 4, 8): 4.0, (512, 2, 4): 5.5}
CASE_IDS = ["M%d_%dx%d" % c for c in CASES]
# (alpha, thr, qbits, dbits) on the shared LLRs of PARAM_CASES.  (1.0, 1.4, 15, 15) reaches the halfword bound (soft values of
# +-16383); (0.8, 1.4, 8, 4) has qbits > dbits, so the channel word exceeds max_data; (0.8, 1.4, 6, 10) changes soft values only
PARAM_SETS = [(0.75, 2.0, 7, 8), (0.8, 1.4, 6, 10), (1.25, 1.4, 6, 8), (0.8, 0.75, 5, 8), (1.0, 1.4, 15, 15), (0.8, 1.4, 8, 4), (0.5, 1.4, 2, 2)]
PARAM_IDS = ["a%g_t%g_q%d_d%d" % p for p in PARAM_SETS]
PARAM_CASES = [(32, 4, 8), (100, 3, 6)]


def lds_bytes(codes, M):
    """Dynamic LDS of ims_flood_codes_kernel: F * (4 * N + 8 * R) bytes (per frame an int16 a-posteriori value and an int16 channel
    value per variable and an 8-byte record per check), rounded up to 16, + 16 for the vote flag."""
    _, rh, nh = np.asarray(codes).shape
    F = 1 if M > 64 else 64 // M
    return ((F * (4 * nh * M + 8 * rh * M) + 15) & ~15) + 16


def table_np(codes):
    """The IMS table as include/ldpc_hip.h describes it (the record of MS_DEC): per code row_start[rh + 1], then the edges
    (block column << 16) | shift in row-major order."""
    off, tab = [], []
    for H in np.asarray(codes):
        off.append(len(tab))
        edges, row_start = [], []
        for row in H:
            row_start.append(len(edges))
            edges += [(k << 16) | int(v) for k, v in enumerate(row) if v >= 0]
        tab += row_start + [len(edges)] + edges
    return np.array(off, dtype=np.int32), np.array(tab, dtype=np.uint32).view(np.int32)


def oracle(H, M, llr, maxiter, params=DEFAULTS):
    """(packed hard words uint32 [B, W], return values int32 [B], soft output float64 [B, N]) of the CPU oracle: decision 0 for the
    hard words and the return value, decision 1 for the soft values."""
    alpha, thr, qbits, dbits = params
    lib = oracle_lib()
    o = Oracle(np.asarray(H, dtype=np.int16), M)
    llr = np.ascontiguousarray(llr, dtype=np.float64)
    B = len(llr)
    hard, soft = np.empty_like(llr), np.empty_like(llr)
    it, it1 = np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
    for f in range(B):
        y0, y1 = llr[f].copy(), llr[f].copy()
        it[f] = lib.orc_imin_sum(o.h, _as_double_p(y0), _as_double_p(hard[f]), int(maxiter), 0, alpha, thr, qbits, dbits)
        it1[f] = lib.orc_imin_sum(o.h, _as_double_p(y1), _as_double_p(soft[f]), int(maxiter), 1, alpha, thr, qbits, dbits)
    o.close()
    assert np.array_equal(it, it1)
    return pack_bits(hard), it, soft


def code_set(case):
    M, rh, nh = case
    return make_code_set(100 + M, rh, nh, M)


_REF, _PREF, _MEMO = {}, {}, {}


def reference(case):
    """Per case, once: the code set, the shared [B, N] and per-code [C, B, N] LLRs, and the oracle's results per layout and code."""
    if case not in _REF:
        M, rh, nh = case
        codes = code_set(case)
        H0 = codes[0].astype(np.int32)
        snr = CASES[case]
        shared = awgn_llr(H0, M, snr, 300 + M, NFRAMES, burn_codeword=False)
        percode = awgn_llr(H0, M, snr, 400 + M, NCODES * NFRAMES, burn_codeword=False).reshape(NCODES, NFRAMES, -1)
        ref = {"shared": [oracle(codes[c], M, shared, MAXITER) for c in range(NCODES)],
               "percode": [oracle(codes[c], M, percode[c], MAXITER) for c in range(NCODES)]}
        _REF[case] = dict(codes=codes, snr=snr, shared=shared, percode=percode, ref=ref)
    return _REF[case]


def param_reference(case, params):
    """The oracle's results per code on the case's shared LLRs with the parameter set (alpha, thr, qbits, dbits)."""
    if (case, params) not in _PREF:
        r = reference(case)
        _PREF[case, params] = [oracle(r["codes"][c], case[0], r["shared"], MAXITER, params) for c in range(NCODES)]
    return _PREF[case, params]


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


# ---- the golden of the compiled reference (16 x 32, M = 64) as code 0 of a three-code set
def golden_set():
    def make():
        g = np.load(os.path.join(GOLDEN_DIR, "ims_m64_2p0.npz"))
        M = int(g["M"])
        H = np.where(g["H"] >= 0, g["H"] % M, -1).astype(np.int16)
        codes = np.array([H, relabelled(H, M, 9001), relabelled(H, M, 9002)], dtype=np.int16)
        return dict(codes=codes, M=M, maxiter=int(g["maxiter"]), llr=np.ascontiguousarray(g["llr"]), iters=g["iters"], hard=g["hard"], soft=g["soft"])
    return _memo("golden", make)


# ---- shapes only this set kernel reaches
BIG = dict(M=67, snr=3.0, seed=3067, frames=4)


def big_set():
    """The 30 x 60 pattern of the IASP golden (206 circulants, row weights 4 .. 10) at M = 67: code 0 its shifts mod 67, codes 1 .. 4
    redrawn from seeds 9000 + c; four shared frames at 3.0 dB."""
    def make():
        g = np.load(os.path.join(GOLDEN_DIR, "iasp", "iasp_30x60_m67_2p0.npz"))
        M = BIG["M"]
        H = np.where(g["H"] >= 0, g["H"] % M, -1).astype(np.int16)
        codes = np.array([H] + [relabelled(H, M, 9000 + c) for c in range(1, NCODES)], dtype=np.int16)
        return M, codes, awgn_llr(H.astype(np.int32), M, BIG["snr"], BIG["seed"], BIG["frames"], burn_codeword=False)
    return _memo("big", make)


def rows17_set():
    """The five 17 x 34 codes at M = 20 of codeset_lche_sets.rows17_set (one block row more than the register-resident set kernels
    hold), shared LLRs at 2.5 dB."""
    def make():
        M, codes, _ = _lche_rows17_set()
        return M, codes, awgn_llr(codes[0].astype(np.int32), M, 2.5, 1718, NFRAMES, burn_codeword=False)
    return _memo("rows17", make)


def mixed_weight_set():
    """The five 5 x 20 codes at M = 8 of codeset_lche_sets.mixed_weight_set (a block row of weight 16 and two of weight 1 per code),
    shared LLRs at 5.0 dB."""
    def make():
        M, codes, _ = _lche_mixed_weight_set()
        return M, codes, awgn_llr(codes[0].astype(np.int32), M, 5.0, 117, NFRAMES, burn_codeword=False)
    return _memo("mixed", make)


ADVERSARIAL_CASES = [(20, 4, 8), (100, 3, 6)]


def adversarial_set(case):
    """adversarial_llr's finite frames (en = 0, en = inf, quantiser rounding boundaries, ties, clamps, ...) for the case's code set."""
    def make():
        codes = code_set(case)
        llr, labels = adversarial_llr(codes[0], case[0], 11)
        return codes, llr, labels
    return _memo(("adv", case), make)


def boundary_set(B):
    """M = 20 (three frames per wave), three codes x B frames, per-code LLRs: code 1 sees strongly positive LLRs (the all-zero codeword:
    integer min-sum returns 1, it has no return value 0), codes 0 and 2 noise at -3 dB."""
    M = 20
    codes = make_code_set(7, 4, 8, M, ncodes=3)
    llr = awgn_llr(codes[0].astype(np.int32), M, -3.0, 55, 3 * B, burn_codeword=False).reshape(3, B, -1)
    llr[1] = 30.0 + np.arange(B * 8 * M).reshape(B, -1) % 7
    return M, codes, llr


def maxiter_one_set():
    """The M = 20 set and seven shared frames at 8 dB: after one iteration (the syndrome of the quantised channel word itself) some
    frames have converged and others have not."""
    codes = code_set((20, 4, 8))
    return codes, awgn_llr(codes[0].astype(np.int32), 20, 8.0, 321, NFRAMES, burn_codeword=False)


SIM = dict(M=32, C=4, B=300, first=1000, snr=3.0, seed=77)


def simulate_set():
    return make_code_set(11, 4, 8, SIM["M"], ncodes=SIM["C"])


# the stopping rule: [weak, medium, strong] at M = 32 (codeset_stop_sets.code_set; the weak code has block columns of weight 1 only)
STOP = dict(M=32, snr=4.0, seed=9, nfe=12, nexp=1500, ref_fer=0.05, batch=64)


def stop_set():
    return strength_set(STOP["M"], ncodes=3)


def dense_set(rh, nh, M, seed=5):
    """One rh x nh code with a dual-diagonal part and one more circulant per row: every block row and column is used."""
    rng = np.random.RandomState(seed)
    H = -np.ones((rh, nh), dtype=np.int16)
    for j in range(rh):
        H[j, j] = rng.randint(0, M)
        H[(j + 1) % rh, j] = rng.randint(0, M)
        H[j, rh + j % (nh - rh)] = rng.randint(0, M)
    for k in range(rh, nh):
        if not (H[:, k] >= 0).any():
            H[rng.randint(rh), k] = rng.randint(0, M)
    return H[None]
