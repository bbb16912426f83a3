"""Inputs of the LCHE code-set tests (test_codeset_lche_cpu.py checks them on the CPU, test_gpu_codeset_lche.py decodes them): the
code sets of test_gpu_codeset.py's builder, channel values at a fixed SNR per case, sets around the compiled reference's golden
vectors (tests/golden/lche), the shapes only the LCHE set kernel reaches, and the results of the numpy restatement
(lche_model.LcheModel), computed once.  The seeds and SNRs are constants: the CPU test asserts that they have the required
properties, nothing is searched at GPU time."""
import os

import numpy as np

from codeset_stop_sets import code_set as strength_set
from lche_model import LCHE_GOLDEN_DIR, LcheModel
from ldpc_testlib import awgn_llr, load_base_matrix, pack_bits, relift
from test_gpu_codeset import make_code_set

LCHE_DEC, MS_DEC = 9, 3
MAXITER = 20
NCODES, NFRAMES = 5, 7
LDS_LIMIT = 160 * 1024
TABLE_WORDS = 96 + 214      # kLcheTab and kLcheStep
# (M, rh, nh) -> SNR in dB at which, in both LLR layouts, the model converges on some (c, f) after 2 .. MAXITER - 1 iterations and
# gives up on another after MAXITER
CASES = {(1, 4, 8): 2.0, (5, 4, 8): 3.0, (20, 4, 8): 2.0, (32, 4, 8): 2.0, (64, 4, 8): 2.0, (100, 3, 6): 1.5, (126, 4, 8): 1.5, (512, 2, 4): 3.0}
CASE_IDS = ["M%d_%dx%d" % c for c in CASES]


def lds_bytes(codes, M):
    """Dynamic LDS of lche_layered_codes_kernel: F * 8 * (N + ne_max * M) + 8 * (kTabWords + kStepWords) + 16."""
    codes = np.asarray(codes)
    F = 1 if M > 64 else 64 // M
    ne_max = max(int((H >= 0).sum()) for H in codes)
    return F * 8 * (codes.shape[2] * M + ne_max * M) + 8 * TABLE_WORDS + 16


def table_np(codes):
    """The LCHE table as include/ldpc_hip.h describes it (the record of MS_DEC): per code row_start[rh + 1], then the edges
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


def model(H, M, llr, maxiter):
    """(packed hard words uint32 [B, W], return values [B], soft output float64 [B, N] = the final L) of the model."""
    dec, it, soft = LcheModel(np.asarray(H, dtype=np.int64), M).decode(llr, maxiter)
    return pack_bits(dec), it, soft


def code_set(case):
    M, rh, nh = case
    return make_code_set(100 + M, rh, nh, M)


_REF = {}


def reference(case):
    """Per case, once: the code set, the shared [B, N] and per-code [C, B, N] LLRs, and the model's results per layout and code."""
    if case not in _REF:
        M, rh, nh = case
        codes = code_set(case)
        H0 = codes[0].astype(np.int32)
        snr = CASES[case]
        shared = awgn_llr(H0, M, snr, 300 + M, NFRAMES, burn_codeword=False)
        percode = awgn_llr(H0, M, snr, 400 + M, NCODES * NFRAMES, burn_codeword=False).reshape(NCODES, NFRAMES, -1)
        ref = {"shared": [model(codes[c], M, shared, MAXITER) for c in range(NCODES)],
               "percode": [model(codes[c], M, percode[c], MAXITER) for c in range(NCODES)]}
        _REF[case] = dict(codes=codes, snr=snr, shared=shared, percode=percode, ref=ref)
    return _REF[case]


# ---- the goldens of the compiled reference as code 0 of a five-code set
GOLDENS = ["lche_30x60_m67_2p0", "lche_rw1_m32_2p5", "lche_m64_boundary", "lche_m1_4p0", "lche_m126_1p7"]


def golden(name, frames=None):
    g = np.load(os.path.join(LCHE_GOLDEN_DIR, name + ".npz"))
    sl = slice(0, frames)
    M = int(g["M"])
    H = np.where(g["H"] >= 0, g["H"] % M, -1).astype(np.int16)      # the shifts as a code set takes them: in [0, M)
    return dict(H=H, M=M, maxiter=int(g["maxiter"]), llr=np.ascontiguousarray(g["llr"][sl]), iters=g["iters"][sl],
                hard=g["hard"][sl], soft=g["soft"][sl])


def relabelled(H, M, seed):
    """The pattern of H with every shift drawn again."""
    rng = np.random.RandomState(seed)
    return np.where(H >= 0, rng.randint(0, M, size=H.shape), -1).astype(np.int16)


def golden_set(name, frames=None):
    """Code 0 = the golden's matrix, the other four its pattern with the shifts redrawn from fixed seeds."""
    g = golden(name, frames)
    g["codes"] = np.array([g["H"]] + [relabelled(g["H"], g["M"], 9000 + c) for c in range(1, NCODES)], dtype=np.int16)
    return g


# ---- shapes only this set kernel reaches
def rows17_set():
    """Five 17 x 34 codes at M = 20 (three frames per wave): one block row more than the other set kernels hold.  A dual-diagonal
    parity part and two circulants per information column; shared LLRs at 2.5 dB."""
    rh, nh, M = 17, 34, 20
    rng = np.random.RandomState(1717)
    codes = -np.ones((NCODES, rh, nh), dtype=np.int16)
    for H in codes:
        for j in range(rh):
            H[j, j] = rng.randint(0, M)
            H[(j + 1) % rh, j] = rng.randint(0, M)
        for k in range(rh, nh):
            H[rng.choice(rh, size=3, replace=False), k] = rng.randint(0, M, size=3)
    return M, codes, awgn_llr(codes[0].astype(np.int32), M, 2.5, 1718, NFRAMES, burn_codeword=False)


def mixed_weight_set():
    """Five 5 x 20 codes at M = 8 (eight frames per wave): every code has a block row of weight 16 and two of weight 1, in different
    places; shared LLRs at 3 dB."""
    rh, nh, M = 5, 20, 8
    rng = np.random.RandomState(116)
    codes = -np.ones((NCODES, rh, nh), dtype=np.int16)
    for c, H in enumerate(codes):
        rows = np.roll(np.arange(rh), c)
        H[rows[0], :16] = rng.randint(0, M, size=16)          # weight 16
        H[rows[1], 16] = rng.randint(0, M)                    # weight 1
        H[rows[2], 17] = rng.randint(0, M)                    # weight 1
        H[rows[3], [1, 5, 18, 19]] = rng.randint(0, M, size=4)
        H[rows[4], [2, 9, 16, 17, 18, 19]] = rng.randint(0, M, size=6)
    return M, codes, awgn_llr(codes[0].astype(np.int32), M, 3.0, 117, NFRAMES, burn_codeword=False)


def boundary_set(B):
    """M = 20 (three frames per wave), three codes x B frames: code 1 sees strongly positive LLRs and two -0.0 (hard bit 0: the
    all-zero codeword at the input), codes 0 and 2 noise at -3 dB."""
    M = 20
    codes = make_code_set(7, 4, 8, M, ncodes=3)
    llr = awgn_llr(codes[0].astype(np.int32), M, -3.0, 55, 3 * B, burn_codeword=False).reshape(3, B, -1)
    llr[1] = 30.0 + np.arange(B * 8 * M).reshape(B, -1) % 7
    llr[1, :, 5] = -0.0
    llr[1, B - 1, 8 * M - 1] = -0.0
    return M, codes, llr


def maxiter_one_set():
    """The M = 20 set and seven shared frames at 4 dB: after one iteration some (c, f) have converged and others have not."""
    codes = code_set((20, 4, 8))
    return codes, awgn_llr(codes[0].astype(np.int32), 20, 4.0, 321, NFRAMES, burn_codeword=False)


SIM = dict(M=32, C=4, B=300, first=1000, snr=1.5, seed=77)


def simulate_set():
    return make_code_set(11, 4, 8, SIM["M"], ncodes=SIM["C"])


# the stopping rule: [weak, medium, strong] at M = 32 (codeset_stop_sets.code_set; the weak code has block columns of weight 1 only)
STOP = dict(M=32, snr=4.0, seed=9, nfe=12, nexp=1500, ref_fer=0.05, batch=64)


def stop_set():
    return strength_set(STOP["M"], ncodes=3)


def big_image_set():
    """16 x 32 with 112 circulants at M = 512: 8 * (16384 + 112 * 512) + 8 * 310 + 16 = 592 320 bytes."""
    base = load_base_matrix()
    return np.where(base >= 0, relift(base, 512) % 512, -1).astype(np.int16)[None]
