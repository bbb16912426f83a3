"""Inputs of the wide code-set tests (ldpc_hip_open_codes_wide: min-sum, TDMP and layered min-sum at any number of block rows and
columns; test_codeset_wide_cpu.py checks the inputs on the CPU, test_gpu_codeset_wide.py decodes them): the sets, channel values at
a fixed SNR per (set, decoder), and the CPU oracle's results, computed once.  The seeds and SNRs are constants: the CPU test asserts
that every (set, decoder) has frames that converge, frames that do not, and a frame that converges after three or more iterations
(otherwise the records in LDS are never read back); nothing is searched at GPU time.

`cols33` is 3 x 33, not 2 x 33: a row holds at most 16 circulants and no block column may be empty, so two block rows cover at most 32
block columns.  3 x 33 is the smallest shape that is beyond min-sum's 32 block columns and inside every other limit."""
import numpy as np

import codeset_ims_sets as IMS
from codeset_lche_sets import relabelled
from codeset_lche_sets import rows17_set as _lche_rows17_set
from codeset_tasp_sets import oracle_tdmp
from ldpc_testlib import LMS_DEC, MS_DEC, TASP_DEC, adversarial_llr, awgn_llr, pack_bits
from test_gpu_codeset import make_code_set, oracle_decode

DECS = (MS_DEC, TASP_DEC, LMS_DEC)
DEC_IDS = {MS_DEC: "MS", TASP_DEC: "TDMP", LMS_DEC: "LMS"}
KERNEL = {MS_DEC: "ms_flood_wide_codes_kernel", TASP_DEC: "tasp_layered_codes_kernel", LMS_DEC: "lms_layered_wide_codes_kernel"}
NARROW_KERNEL = {MS_DEC: "ms_flood_codes_kernel", TASP_DEC: "tasp_layered_codes_kernel", LMS_DEC: "lms_layered_codes_kernel"}
MAXITER = 20
NCODES, NFRAMES = 5, 7
LDS_LIMIT = 160 * 1024


def kernel_name(dec, M):
    return KERNEL[dec] + ("<multiwave>" if M > 64 else "")


def is_wide(dec, rh, nh):
    """The shapes that the layers above the C-ABI send to ldpc_hip_open_codes_wide."""
    return dec in DECS and (rh > 16 or (dec == MS_DEC and nh > 32))


def lds_bytes(dec, codes, M, llr_in_lds=False):
    """Dynamic LDS of a wide set.  MS / LMS: F * (8 * N + 24 * R) bytes (an fp64 a-posteriori value per variable; min1, min2 and the
    meta word, 8 bytes each, per check), + 8 * N * F with the channel LLRs in LDS (a variant that is not built), rounded up to 16, + 16
    for the vote flag.  TDMP: F * 8 * (N + ne_max * M) + 16."""
    codes = np.asarray(codes)
    _, rh, nh = codes.shape
    F = 1 if M > 64 else 64 // M
    if dec == TASP_DEC:
        return F * 8 * (nh * M + max(int((H >= 0).sum()) for H in codes) * M) + 16
    return ((F * ((16 if llr_in_lds else 8) * nh * M + 24 * rh * M) + 15) & ~15) + 16


table_np = IMS.table_np
dense_set = IMS.dense_set


def oracle(dec, H, M, llr, maxiter, alpha=0.8):
    """(packed hard words uint32 [B, W], return values int32 [B], soft output float64 [B, N]) of the CPU oracle."""
    H = np.asarray(H, dtype=np.int16)
    if dec == TASP_DEC:
        d, it, s = oracle_tdmp(H, M, llr, maxiter)
    else:
        d, it, s = oracle_decode(H, M, dec, llr, maxiter, alpha)
    return pack_bits(d), it, s


# ---- the sets: name -> (M, codes [C, rh, nh])
def _rows17(M):
    _, codes, _ = _lche_rows17_set()
    if M == 20:
        return M, codes
    return M, np.array([relabelled(H, M, 1700 + M + c) for c, H in enumerate(codes)], dtype=np.int16)


def _cols33():
    """Five 3 x 33 codes at M = 5 (twelve frames per wave): rows of weight 14, 15 and 14, every block column used, weights 1 and 2."""
    rh, nh, M = 3, 33, 5
    rng = np.random.RandomState(3333)
    codes = -np.ones((NCODES, rh, nh), dtype=np.int16)
    for c, H in enumerate(codes):
        for k in range(nh):
            H[(k + c) % rh, k] = rng.randint(0, M)
        for j in range(rh):
            free = np.flatnonzero(H[j] < 0)
            extra = rng.choice(free, size=14 + (j == 1) - int((H[j] >= 0).sum()), replace=False)
            H[j, extra] = rng.randint(0, M, size=len(extra))
    return M, codes


def _mixed():
    """Five 17 x 34 codes at M = 8 (eight frames per wave): per code one block row of weight 16, two of weight 1 and fourteen of
    weight 3 or 4, in different places."""
    rh, nh, M = 17, 34, 8
    rng = np.random.RandomState(1734)
    codes = -np.ones((NCODES, rh, nh), dtype=np.int16)
    for c, H in enumerate(codes):
        rows = np.roll(np.arange(rh), 3 * c)
        H[rows[0], :16] = rng.randint(0, M, size=16)
        H[rows[1], 16] = rng.randint(0, M)
        H[rows[2], 17] = rng.randint(0, M)
        for q, k in enumerate(range(18, nh)):                  # sixteen block columns over the fourteen other rows
            H[rows[3 + q % 14], k] = rng.randint(0, M)
        for j in rows[3:]:
            free = np.flatnonzero(H[j] < 0)
            extra = rng.choice(free[free < 16], size=2, replace=False)
            H[j, extra] = rng.randint(0, M, size=2)
    return M, codes


def _big():
    M, codes, _ = IMS.big_set()
    return M, codes


def _narrow(case):
    M, rh, nh = case
    return M, make_code_set(100 + M, rh, nh, M)


NARROW = ["narrow_M20_4x8", "narrow_M100_3x6"]
SETS = {
    "rows17_M20": lambda: _rows17(20), "rows17_M64": lambda: _rows17(64), "rows17_M67": lambda: _rows17(67), "rows17_M130": lambda: _rows17(130),
    "cols33": _cols33, "big": _big, "mixed": _mixed,
    "narrow_M20_4x8": lambda: _narrow((20, 4, 8)), "narrow_M100_3x6": lambda: _narrow((100, 3, 6)),
}
FRAMES = {"big": 4}
# (set, decoder) -> SNR in dB of its channel values.  `mixed` has rows of weight 1: TDMP needs weight 2.
SNR = {
    ("rows17_M20", MS_DEC): 2.5, ("rows17_M20", TASP_DEC): 1.0, ("rows17_M20", LMS_DEC): 1.5,
    ("rows17_M64", MS_DEC): 2.0, ("rows17_M64", TASP_DEC): 1.5, ("rows17_M64", LMS_DEC): 1.5,
    ("rows17_M67", MS_DEC): 2.0, ("rows17_M67", TASP_DEC): 1.5, ("rows17_M67", LMS_DEC): 1.5,
    ("rows17_M130", MS_DEC): 2.0, ("rows17_M130", TASP_DEC): 1.5, ("rows17_M130", LMS_DEC): 1.5,
    ("cols33", MS_DEC): 0.0, ("cols33", TASP_DEC): 3.75, ("cols33", LMS_DEC): 3.0,
    ("big", MS_DEC): 2.0, ("big", TASP_DEC): 1.5, ("big", LMS_DEC): 2.0,
    ("mixed", MS_DEC): 1.5, ("mixed", LMS_DEC): 2.0,
    ("narrow_M20_4x8", MS_DEC): 2.5, ("narrow_M20_4x8", TASP_DEC): 2.5, ("narrow_M20_4x8", LMS_DEC): 2.5,
    ("narrow_M100_3x6", MS_DEC): 3.5, ("narrow_M100_3x6", TASP_DEC): 3.5, ("narrow_M100_3x6", LMS_DEC): 3.5,
}
PARITY = [k for k in SNR if k[0] not in NARROW]
PARITY_IDS = ["%s-%s" % (name, DEC_IDS[dec]) for name, dec in PARITY]

_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def code_set(name):
    return _memo(("set", name), SETS[name])


def reference(name, dec):
    """Per (set, decoder), once: M, the codes, the shared [B, N] and per-code [C, B, N] LLRs and the oracle's results per layout and
    code."""
    def make():
        M, codes = code_set(name)
        H0, B, seed = codes[0].astype(np.int32), FRAMES.get(name, NFRAMES), sum(map(ord, name)) + 10 * dec
        shared = awgn_llr(H0, M, SNR[name, dec], 3000 + seed, B, burn_codeword=False)
        percode = awgn_llr(H0, M, SNR[name, dec], 4000 + seed, len(codes) * B, burn_codeword=False).reshape(len(codes), B, -1)
        ref = {"shared": [oracle(dec, codes[c], M, shared, MAXITER) for c in range(len(codes))],
               "percode": [oracle(dec, codes[c], M, percode[c], MAXITER) for c in range(len(codes))]}
        return dict(M=M, codes=codes, shared=shared, percode=percode, ref=ref)
    return _memo(("ref", name, dec), make)


def adversarial_set():
    """adversarial_llr's finite frames (ties, clamps at 32767, -0.0, ...) for the rows17 set at M = 20."""
    def make():
        M, codes = code_set("rows17_M20")
        llr, labels = adversarial_llr(codes[0], M, 11)
        return M, codes, llr, labels
    return _memo("adv", make)


def boundary_set(B):
    """M = 20 (three frames per wave), three 17 x 34 codes x B frames, per-code LLRs: code 1 sees strongly positive LLRs (the all-zero
    codeword at the input: min-sum and layered min-sum return 1, TDMP 0), codes 0 and 2 noise at -3 dB."""
    M, codes = code_set("rows17_M20")
    codes = codes[:3]
    llr = awgn_llr(codes[0].astype(np.int32), M, -3.0, 55, 3 * B, burn_codeword=False).reshape(3, B, -1)
    llr[1] = 30.0 + np.arange(B * 34 * M).reshape(B, -1) % 7
    return M, codes, llr


MAXITER_ONE_SNR = {MS_DEC: 9.0, TASP_DEC: 4.5, LMS_DEC: 4.5}


def maxiter_one_set(dec):
    """The rows17 set at M = 20 and seven shared frames at an SNR at which, after one iteration, some frames have converged and others
    have not."""
    M, codes = code_set("rows17_M20")
    return M, codes, awgn_llr(codes[0].astype(np.int32), M, MAXITER_ONE_SNR[dec], 321, NFRAMES, burn_codeword=False)


# Monte-Carlo: three of the rows17 codes at M = 20
SIM = dict(C=3, B=300, first=1000, snr=2.5, seed=77)
STOP = dict(snr=2.0, seed=9, nfe=12, nexp=600, ref_fer=0.05, batch=64)


def simulate_set():
    M, codes = code_set("rows17_M20")
    return M, codes[:SIM["C"]]
