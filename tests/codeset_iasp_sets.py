"""Inputs of the IASP code-set tests (test_codeset_iasp_cpu.py checks them on the CPU, test_gpu_codeset_iasp.py decodes them): the
code sets of test_gpu_codeset.py's builder, channel values at a fixed SNR per case, sets around the compiled reference's golden
vectors (tests/golden/iasp), and the results of the numpy restatement (iasp_model.IaspModel), computed once.  The seeds and SNRs
are constants: the CPU test asserts that they have the required properties, nothing is searched at GPU time."""
import os

import numpy as np

from codeset_stop_sets import code_set as strength_set
from iasp_model import IASP_GOLDEN_DIR, IaspModel
from ldpc_testlib import awgn_llr, pack_bits
from test_gpu_codeset import make_code_set

IASP_DEC = 5
MAXITER = 20
NCODES, NFRAMES = 5, 7
LDS_LIMIT = 160 * 1024
# (M, rh, nh) -> SNR in dB at which the model converges on some (c, f) and not on others, for both LLR layouts.
# (512, 2, 4): a 2 x 4 code without an empty block has columns of weight 2 only, so this case is the all-weight-2 branch in the
# eight-wave instance; nothing converges on it at 1.0 dB, hence 3.0 dB as for the TDMP sets.
CASES = {(1, 4, 8): 1.0, (5, 4, 8): 1.0, (20, 4, 8): 1.0, (32, 4, 8): 1.0, (64, 4, 8): 1.0, (100, 3, 6): 1.0, (126, 16, 32): 1.0, (512, 2, 4): 3.0}
CASE_IDS = ["M%d_%dx%d" % c for c in CASES]


def lds_bytes(codes, M):
    """Dynamic LDS of iasp_codes_kernel: F * 2 * (ne_max * M + 2 * N) bytes of u16 state and words, rounded up to 16, + 16."""
    codes = np.asarray(codes)
    F = 1 if M > 64 else 64 // M
    ne_max = max(int((H >= 0).sum()) for H in codes)
    return (F * 2 * (ne_max * M + 2 * codes.shape[2] * M) + 15) // 16 * 16 + 16


def table_np(codes):
    """The IASP table as include/ldpc_hip.h describes it: per code row_start[rh + 1], the edges (block column << 16) | shift in
    row-major order, cw2, col_start[nh + 1], col_edges (row-major index of the edge << 16) | shift, columns then rows ascending."""
    off, tab = [], []
    for H in np.asarray(codes):
        off.append(len(tab))
        rh, nh = H.shape
        edges, row_start, cols = [], [], [[] for _ in range(nh)]
        for row in H:
            row_start.append(len(edges))
            for k, v in enumerate(row):
                if v >= 0:
                    cols[k].append((len(edges) << 16) | int(v))
                    edges.append((k << 16) | int(v))
        col_start = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).tolist()
        tab += row_start + [len(edges)] + edges + [int(all(len(c) == 2 for c in cols))] + col_start + [e for c in cols for e in c]
    return np.array(off, dtype=np.int32), np.array(tab, dtype=np.uint32).view(np.int32)


def model(H, M, llr, maxiter):
    """(packed hard words uint32 [B, W], return values [B], soft output float64 [B, N] = a-posteriori word / 65536) of the model."""
    soft, it, _, so = IaspModel(np.asarray(H, dtype=np.int64), M).decode(llr, maxiter, 1)
    return pack_bits((so >> 15).astype(np.float64)), it, soft


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


def golden(name, frames=None):
    g = np.load(os.path.join(IASP_GOLDEN_DIR, name + ".npz"))
    sl = slice(0, frames)
    M = int(g["M"])
    H = np.where(g["H"] >= 0, g["H"] % M, -1).astype(np.int16)      # the shifts as a code set takes them: in [0, M)
    return dict(H=H, M=M, maxiter=int(g["maxiter"]), llr=np.ascontiguousarray(g["llr"][sl]), iters=g["iters"][sl],
                hard=g["hard"][sl], soft=g["soft"][sl])


def redrawn(H, M, seed):
    """The pattern of H with every shift drawn again."""
    rng = np.random.RandomState(seed)
    return np.where(H >= 0, rng.randint(0, M, size=H.shape), -1).astype(np.int16)


def golden_set(name, ncodes, frames=None):
    """Code 0 = the golden's matrix, the others its pattern with the shifts redrawn from fixed seeds."""
    g = golden(name, frames)
    g["codes"] = np.array([g["H"]] + [redrawn(g["H"], g["M"], 9000 + c) for c in range(1, ncodes)], dtype=np.int16)
    return g


SHAPE_30x60 = "iasp_30x60_m67_2p0"
LIFTINGS = ["iasp_m1_4p0", "iasp_m126_1p7", "iasp_m64_sat", "iasp_m64_0p0"]
CW2 = {"iasp_cw2_m64_2p0": 24, "iasp_cw2_m128_2p0": 16}   # name -> frames of the golden that the set decodes


def general_from(H, M, seed):
    """H with one more circulant in every second block column (weights 2 and 3: the general branch), shifts redrawn."""
    G = redrawn(H, M, seed)
    rng = np.random.RandomState(seed + 1)
    for k in range(0, H.shape[1], 2):
        j = rng.choice(np.flatnonzero(G[:, k] < 0))
        G[j, k] = rng.randint(0, M)
    return G


def cw2_set(name):
    """Code 0 = the all-weight-2 golden matrix, then general, all-weight-2, general: the flag is per code."""
    g = golden(name, CW2[name])
    H, M = g["H"], g["M"]
    g["codes"] = np.array([H, general_from(H, M, 9101), redrawn(H, M, 9102), general_from(H, M, 9103)], dtype=np.int16)
    return g


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


# the stopping rule: [weak, medium, strong] at M = 32 (codeset_stop_sets.code_set; the weak code has two circulants per block row)
STOP = dict(M=32, snr=4.0, seed=9, nfe=12, nexp=1500, ref_fer=0.05, batch=64)


def stop_set():
    return strength_set(STOP["M"], ncodes=3)


def big_image_set():
    """16 x 32 with 112 circulants at M = 512: 2 * (112 * 512 + 2 * 16384) + 16 = 180 240 bytes."""
    from ldpc_testlib import load_base_matrix, relift
    base = load_base_matrix()
    return np.where(base >= 0, relift(base, 512) % 512, -1).astype(np.int16)[None]
