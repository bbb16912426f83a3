"""Inputs of the flooding sum-product code-set tests (decoders 1 and 2; test_codeset_sp_cpu.py checks them on the CPU,
test_gpu_codeset_sp.py decodes them): the code sets of test_gpu_codeset.py's builder, channel values at a fixed SNR per case, sets
around the compiled reference's golden vectors (tests/golden), the shapes only these set kernels reach, numpy models of the table and
of the LDS contract, and the CPU oracle's results (orc_sum_prod, orc_sum_prod_gf2), computed once.  The seeds and SNRs are constants:
the CPU test asserts that they have the required properties, nothing is searched at GPU time."""
import os

import numpy as np

from codeset_iasp_sets import general_from, redrawn
from codeset_iasp_sets import table_np as _iasp_table_np
from codeset_lche_sets import mixed_weight_set as _lche_mixed_weight_set
from codeset_lche_sets import rows17_set as _lche_rows17_set
from codeset_stop_sets import code_set as strength_set
from ldpc_testlib import GOLDEN_DIR, Oracle, awgn_llr, load_base_matrix, pack_bits, relift
from test_gpu_codeset import make_code_set

SP_DEC, ASP_DEC, IASP_DEC = 1, 2, 5
DECS = (SP_DEC, ASP_DEC)
DEC_IDS = ["sp", "asp"]
MAXITER = 20
NCODES, NFRAMES = 5, 7
LDS_LIMIT = 160 * 1024
# (M, rh, nh) -> SNR in dB at which, in both LLR layouts and for both decoders, the oracle converges on some (c, f) after
# 2 .. MAXITER - 1 iterations and gives up on another after MAXITER
CASES = {(1, 4, 8): 2.0, (5, 4, 8): 2.0, (20, 4, 8): 2.0, (32, 4, 8): 2.0, (64, 4, 8): 2.0, (100, 3, 6): 2.0, (126, 4, 8): 2.0, (512, 2, 4): 3.0}
CASE_IDS = ["M%d_%dx%d" % c for c in CASES]


def frame_bytes(dec, codes, M):
    """One frame's image: 8 * (ne_max * M + N + R) + 4 * ceil(N / 32) bytes for SP (per-edge messages, channel likelihood ratios,
    check products, hard bits), 8 * (ne_max * M + N) + 4 * ceil(N / 32) for ASP."""
    codes = np.asarray(codes)
    _, rh, nh = codes.shape
    ne_max = max(int((H >= 0).sum()) for H in codes)
    N, R = nh * M, rh * M
    return 8 * (ne_max * M + N + (R if dec == SP_DEC else 0)) + 4 * ((N + 31) // 32)


def lds_bytes(dec, codes, M):
    """What decides whether a set is accepted: ONE frame's image rounded up to 16, + 16 for the vote flags."""
    return (frame_bytes(dec, codes, M) + 15) // 16 * 16 + 16


def frames_per_workgroup(dec, codes, M):
    """floor(64 / M) for M <= 64, fewer when their images do not fit 160 KiB; 1 for M > 64."""
    F = 1 if M > 64 else 64 // M
    while F > 1 and (F * frame_bytes(dec, codes, M) + 15) // 16 * 16 + 16 > LDS_LIMIT:
        F -= 1
    return F


def threads(codes, M):
    """Workgroup size: min(1024 / L, nh) groups of L = 64 (M <= 64) or 64 * ceil(M / 64) lanes."""
    lanes = 64 if M <= 64 else (M + 63) // 64 * 64
    return min(1024 // lanes, np.asarray(codes).shape[2]) * lanes


table_np = _iasp_table_np    # the record is IASP's, for both decoders


def oracle(dec, H, M, llr, maxiter):
    """(packed hard words uint32 [B, W], return values int32 [B], soft output float64 [B, N]) of the CPU oracle: decision 0 for the
    hard words and the return value, decision 1 for the soft values."""
    o = Oracle(np.asarray(H, dtype=np.int16), M)
    hard, it, _ = o.decode(dec, llr, int(maxiter), 0)
    soft, it1, _ = o.decode(dec, llr, int(maxiter), 1)
    o.close()
    assert np.array_equal(it, it1)
    return pack_bits(hard), it, soft


def code_set(case):
    M, rh, nh = case
    return make_code_set(100 + M, rh, nh, M)


_REF, _MEMO = {}, {}


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def inputs(case):
    """Per case, once: the code set and the shared [B, N] and per-code [C, B, N] LLRs."""
    def make():
        M, rh, nh = case
        codes = code_set(case)
        H0 = codes[0].astype(np.int32)
        snr = CASES[case]
        shared = awgn_llr(H0, M, snr, 300 + M, NFRAMES, burn_codeword=False)
        percode = awgn_llr(H0, M, snr, 400 + M, NCODES * NFRAMES, burn_codeword=False).reshape(NCODES, NFRAMES, -1)
        return dict(codes=codes, snr=snr, shared=shared, percode=percode)
    return _memo(("in", case), make)


def reference(dec, case):
    """Per decoder and case, once: the inputs and the oracle's results per layout and code."""
    if (dec, case) not in _REF:
        r = dict(inputs(case))
        codes, M = r["codes"], case[0]
        r["ref"] = {"shared": [oracle(dec, codes[c], M, r["shared"], MAXITER) for c in range(NCODES)],
                    "percode": [oracle(dec, codes[c], M, r["percode"][c], MAXITER) for c in range(NCODES)]}
        _REF[dec, case] = r
    return _REF[dec, case]


# ---- the goldens of the compiled reference as code 0 of a five-code set
GOLDENS = ["sp_m64_2p0", "sp_m1_4p0", "asp_m64_2p0", "asp_cw2_m64_2p0", "asp_m128_1p7"]
GOLDEN_FRAMES = 7


def golden(name, frames=GOLDEN_FRAMES):
    """The first `frames` frames of a golden; its soft values cover fewer frames than its decisions."""
    g = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    sl = slice(0, frames)
    M = int(g["M"])
    H = np.where(g["H"] >= 0, g["H"] % M, -1).astype(np.int16)      # the shifts as a code set takes them: in [0, M)
    return dict(H=H, M=M, dec=int(g["dec_id"]), maxiter=int(g["maxiter"]), llr=np.ascontiguousarray(g["llr"][sl]), iters=g["iters"][sl],
                hard=g["hard"][sl], soft=g["soft"][sl])


def golden_set(name, frames=GOLDEN_FRAMES):
    """Code 0 = the golden's matrix, the other four its pattern with the shifts redrawn from fixed seeds."""
    def make():
        g = golden(name, frames)
        g["codes"] = np.array([g["H"]] + [redrawn(g["H"], g["M"], 9000 + c) for c in range(1, NCODES)], dtype=np.int16)
        return g
    return _memo(("golden", name, frames), make)


def cw2_mixed_set():
    """4 x 8 at M = 64: code 0 = the all-weight-2 golden matrix, then general, all-weight-2, general, all-weight-2: ASP's flag is per
    code.  The golden's first seven frames."""
    def make():
        g = golden("asp_cw2_m64_2p0")
        H, M = g["H"], g["M"]
        g["codes"] = np.array([H, general_from(H, M, 9101), redrawn(H, M, 9102), general_from(H, M, 9103), redrawn(H, M, 9104)], dtype=np.int16)
        return g
    return _memo("cw2mixed", make)


def is_cw2(H):
    return bool(((np.asarray(H) >= 0).sum(axis=0) == 2).all())


# ---- shapes only these set kernels reach
def rows17_set():
    """codeset_lche_sets.rows17_set: five 17 x 34 codes at M = 20 and seven shared frames at 2.5 dB."""
    return _memo("rows17", _lche_rows17_set)


def mixed_weight_set():
    """codeset_lche_sets.mixed_weight_set: five 5 x 20 codes at M = 8, each with a block row of weight 16 and two of weight 1; seven
    shared frames at 3 dB.  SP only: ASP's map_bin needs weight 2."""
    return _memo("mixed", _lche_mixed_weight_set)


BIG = dict(M=67, frames=4, maxiter=20, want=[13, -20, 13, 15])


def big_set():
    """The 30 x 60 matrix of tests/golden/lche/lche_30x60_m67_2p0.npz (206 circulants) as code 0 of a five-code set, and the first
    four frames of its LLRs (2.0 dB)."""
    def make():
        g = np.load(os.path.join(GOLDEN_DIR, "lche", "lche_30x60_m67_2p0.npz"))
        M = int(g["M"])
        H = np.where(g["H"] >= 0, g["H"] % M, -1).astype(np.int16)
        codes = np.array([H] + [redrawn(H, M, 9000 + c) for c in range(1, NCODES)], dtype=np.int16)
        return M, codes, np.ascontiguousarray(g["llr"][:BIG["frames"]])
    return _memo("big", make)


def appendix_c(M):
    """The 16 x 32 base matrix of Appendix C (112 circulants) at lifting M, as a one-code set."""
    base = load_base_matrix()
    return np.where(base >= 0, relift(base, M) % M, -1).astype(np.int16)[None]


def boundary_set(B):
    """M = 20 (three frames per workgroup), three codes x B frames, per-code LLRs: code 1 sees strongly positive LLRs (the all-zero
    codeword at the input: return value 0), codes 0 and 2 noise at -3 dB."""
    M = 20
    codes = make_code_set(7, 4, 8, M, ncodes=3)
    llr = awgn_llr(codes[0].astype(np.int32), M, -3.0, 55, 3 * B, burn_codeword=False).reshape(3, B, -1)
    llr[1] = 3.0 + np.arange(B * 8 * M).reshape(B, -1) % 7
    return M, codes, llr


def maxiter_one_set():
    """The M = 20 set and seven shared frames at 4 dB: after one iteration some (c, f) have converged and others have not."""
    codes = code_set((20, 4, 8))
    return codes, awgn_llr(codes[0].astype(np.int32), 20, 4.0, 321, NFRAMES, burn_codeword=False)


SIM = dict(M=32, C=4, B=300, first=1000, snr=2.0, seed=77)


def simulate_set():
    return make_code_set(11, 4, 8, SIM["M"], ncodes=SIM["C"])


# the stopping rule: [weak, medium, strong] at M = 32 (codeset_stop_sets.code_set; the weak code has two circulants per block row)
STOP = dict(M=32, snr=4.0, seed=9, nfe=12, nexp=1500, ref_fer=0.05, batch=64)


def stop_set():
    return strength_set(STOP["M"], ncodes=3)
