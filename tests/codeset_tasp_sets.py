"""Inputs of the TDMP code-set tests (test_codeset_tasp_cpu.py checks them on the CPU, test_gpu_codeset_tasp.py decodes them): the
code sets of test_gpu_codeset.py's builder, channel values at a fixed SNR per case, and the CPU oracle's results, computed once.
The seeds and SNRs are constants: the CPU test asserts that they have the required properties, nothing is searched at GPU time."""
import numpy as np

from ldpc_testlib import Oracle, _as_double_p, awgn_llr
from test_gpu_codeset import make_code_set

MAXITER = 20
NCODES, NFRAMES = 5, 7
LDS_LIMIT = 160 * 1024
# (M, rh, nh) -> SNR in dB at which orc_tdmp_sum_prod converges on some (c, f) and not on others, for both LLR layouts
CASES = {(1, 4, 8): 1.0, (5, 4, 8): 1.0, (20, 4, 8): 1.0, (32, 4, 8): 1.0, (64, 4, 8): 1.0, (100, 3, 6): 1.0, (126, 16, 32): 1.0, (512, 2, 4): 3.0}
CASE_IDS = ["M%d_%dx%d" % c for c in CASES]


def lds_bytes(codes, M):
    """Dynamic LDS of tasp_layered_codes_kernel: F * 8 * (N + ne_max * M) + 16."""
    codes = np.asarray(codes)
    F = 1 if M > 64 else 64 // M
    ne_max = max(int((H >= 0).sum()) for H in codes)
    return F * 8 * (codes.shape[2] * M + ne_max * M) + 16


def oracle_tdmp(H, M, llr, maxiter):
    """(hard decword [B, N], return values [B], a-posteriori probabilities [B, N]) of the CPU oracle."""
    o = Oracle(H, M)
    llr = np.ascontiguousarray(llr, dtype=np.float64)
    d, s = np.empty_like(llr), np.empty_like(llr)
    it = np.empty(len(llr), dtype=np.int32)
    for b in range(len(llr)):
        y = llr[b].copy()
        it[b] = o.lib.orc_tdmp_sum_prod(o.h, _as_double_p(y), _as_double_p(d[b]), maxiter, _as_double_p(s[b]))
    o.close()
    return d, it, s


def code_set(case):
    M, rh, nh = case
    return make_code_set(100 + M, rh, nh, M)


_REF = {}


def reference(case):
    """Per case, once: the code set, the shared [B, N] and per-code [C, B, N] LLRs, and the oracle's results per layout and code."""
    if case not in _REF:
        M, rh, nh = case
        codes = code_set(case)
        H0 = codes[0].astype(np.int32)
        snr = CASES[case]
        shared = awgn_llr(H0, M, snr, 300 + M, NFRAMES, burn_codeword=False)
        percode = awgn_llr(H0, M, snr, 400 + M, NCODES * NFRAMES, burn_codeword=False).reshape(NCODES, NFRAMES, -1)
        ref = {"shared": [oracle_tdmp(codes[c], M, shared, MAXITER) for c in range(NCODES)],
               "percode": [oracle_tdmp(codes[c], M, percode[c], MAXITER) for c in range(NCODES)]}
        _REF[case] = dict(codes=codes, snr=snr, shared=shared, percode=percode, ref=ref)
    return _REF[case]


def boundary_set(B):
    """M = 20 (three frames per wave), three codes x B frames: code 1 sees strongly positive LLRs (the all-zero codeword at the
    input), codes 0 and 2 noise at -3 dB."""
    M = 20
    codes = make_code_set(7, 4, 8, M, ncodes=3)
    llr = awgn_llr(codes[0].astype(np.int32), M, -3.0, 55, 3 * B, burn_codeword=False).reshape(3, B, -1)
    llr[1] = 30.0 + np.arange(B * 8 * M).reshape(B, -1) % 7
    return M, codes, llr


def maxiter_one_set():
    """The M = 20 set and seven shared frames at 4 dB: after one iteration some (c, f) have converged and others have not."""
    codes = code_set((20, 4, 8))
    return codes, awgn_llr(codes[0].astype(np.int32), 20, 4.0, 321, NFRAMES, burn_codeword=False)


SIM = dict(M=32, C=4, B=300, first=1000, snr=1.5, seed=77)


def simulate_set():
    return make_code_set(11, 4, 8, SIM["M"], ncodes=SIM["C"])


def driver_set():
    """Three 4 x 8 codes of very different strength at M = 32 for the stopping-rule harness (as test_gpu_codeset.py builds them, the
    weak one with two circulants per block row at least: every block column of weight 1)."""
    from ldpc_testlib import random_qc_code
    M, rh, nh = 32, 4, 8
    rng = np.random.RandomState(5)
    strong = random_qc_code(rng, rh, nh, M, [3])
    medium = random_qc_code(rng, rh, nh, M, [2])
    weak = -np.ones((rh, nh), dtype=np.int16)
    for k in range(nh):
        weak[k % rh, k] = k % M
    return M, np.array([medium, weak, strong], dtype=np.int16)
