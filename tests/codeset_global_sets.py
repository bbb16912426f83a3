"""Inputs of the tests of the global-memory tier of a code set (ldpc_hip_open_codes_global, csrc/ldpc_codeset_global.hpp;
test_codeset_global_cpu.py checks the inputs on the CPU, test_gpu_codeset_global.py decodes them): the sets, channel values at fixed
SNRs, a numpy restatement of the route's table, and the CPU references -- the C oracle for decoders 1, 2, 3, 4, 7 and 8, the numpy
restatements iasp_model / lche_model for 5 and 9 -- computed once.  Seeds and SNRs are constants; nothing is searched at GPU time.

Every set holds codes of DIFFERENT edge counts.  `A` sets (decoders 2, 5, 7: row weights >= 2) hold one code whose block columns all
have exactly two circulants (cw2: decoders 2 and 5 take upstream's own branch for it) next to codes that are not; `B` sets (the
other decoders) hold a code with a block row of weight 1."""
import numpy as np

import codeset_iasp_sets as IASP
import codeset_ims_sets as IMS
import codeset_lche_sets as LCHE
import codeset_sp_sets as SP
from codeset_tasp_sets import oracle_tdmp
from ldpc_testlib import (ASP_DEC, IASP_DEC, IMS_DEC, LCHE_DEC, LMS_DEC, MS_DEC, SP_DEC, TASP_DEC, awgn_llr, cycle_code, load_base_matrix, pack_bits,
                          random_qc_code, relift)
from test_gpu_codeset import oracle_decode

DECS = (SP_DEC, ASP_DEC, MS_DEC, IMS_DEC, IASP_DEC, TASP_DEC, LMS_DEC, LCHE_DEC)
DEC_IDS = {SP_DEC: "SP", ASP_DEC: "ASP", MS_DEC: "MS", IMS_DEC: "IMS", IASP_DEC: "IASP", TASP_DEC: "TDMP", LMS_DEC: "LMS", LCHE_DEC: "LCHE"}
KERNEL = {SP_DEC: "sp_global_codes_kernel", ASP_DEC: "asp_global_codes_kernel", MS_DEC: "ms_global_codes_kernel", IMS_DEC: "ims_global_codes_kernel",
          IASP_DEC: "iasp_global_codes_kernel", TASP_DEC: "tasp_global_codes_kernel", LMS_DEC: "lms_global_codes_kernel",
          LCHE_DEC: "lche_global_codes_kernel"}
MIN_RW2 = (ASP_DEC, IASP_DEC, TASP_DEC)      # map_bin / imap_bin read SB[1]
NAMES = {ASP_DEC: "advanced sum-product", IASP_DEC: "integer advanced sum-product", TASP_DEC: "TDMP sum-product"}
MAXITER = 20
LIFTINGS = (5, 64, 67, 130)
IMS_DEFAULTS = IMS.DEFAULTS

_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def is_cw2(H):
    return bool(((np.asarray(H) >= 0).sum(axis=0) == 2).all())


def kind(dec):
    return "A" if dec in MIN_RW2 else "B"


def oracle(dec, H, M, llr, maxiter=MAXITER, alpha=0.8, ims=IMS_DEFAULTS):
    """(packed hard words uint32 [B, W], return values int32 [B], soft output float64 [B, N]) of the CPU reference of a decoder."""
    H = np.asarray(H, dtype=np.int16)
    if dec in (MS_DEC, LMS_DEC):
        d, it, s = oracle_decode(H, M, dec, llr, maxiter, alpha)
        return pack_bits(d), it, s
    if dec == TASP_DEC:
        d, it, s = oracle_tdmp(H, M, llr, maxiter)
        return pack_bits(d), it, s
    if dec == IMS_DEC:
        return IMS.oracle(H, M, llr, maxiter, (alpha,) + tuple(ims[1:]))
    if dec in (SP_DEC, ASP_DEC):
        return SP.oracle(dec, H, M, llr, maxiter)
    if dec == IASP_DEC:
        return IASP.model(H, M, llr, maxiter)
    assert dec == LCHE_DEC
    return LCHE.model(H, M, llr, maxiter)


def table_np(codes):
    """The record of ldpc_hip_codes_table_global_host as include/ldpc_hip.h describes it: per code row_start[rh + 1], edges (block column
    << 16) | shift in row-major order, cw2, col_start[nh + 1], col_edges (block row << 16) | shift and col_slot (the row-major index of
    the edge), both in column-major order."""
    off, tab = [], []
    for H in np.asarray(codes):
        off.append(len(tab))
        rh, nh = H.shape
        edges, row_start, index = [], [], {}
        for j, row in enumerate(H):
            row_start.append(len(edges))
            for k, v in enumerate(row):
                if v >= 0:
                    index[j, k] = len(edges)
                    edges.append((k << 16) | int(v))
        col_start, col_edges, col_slot = [], [], []
        for k in range(nh):
            col_start.append(len(col_edges))
            for j in range(rh):
                if H[j, k] >= 0:
                    col_edges.append((j << 16) | int(H[j, k]))
                    col_slot.append(index[j, k])
        tab += row_start + [len(edges)] + edges + [int(is_cw2(H))] + col_start + [len(col_edges)] + col_edges + col_slot
    return np.array(off, dtype=np.int32), np.array(tab, dtype=np.uint32).view(np.int32)


def _weight_one_row(rng, H, M):
    """H with its last block row cut down to one circulant; a block column that loses its only circulant gets one in block row 0."""
    H = H.copy()
    rh = H.shape[0]
    H[rh - 1, :] = -1
    H[rh - 1, rh - 1] = rng.randint(0, M)
    for k in np.flatnonzero((H >= 0).sum(axis=0) == 0):
        H[0, k] = rng.randint(0, M)
    return H


def small_set(M, which, rh=4, nh=8):
    """Three rh x nh codes at lifting M.  A: cw2, general, general; B: general, one with a block row of weight 1, general."""
    def make():
        rng = np.random.RandomState(7000 + M)
        g1 = random_qc_code(rng, rh, nh, M, [3])
        other = cycle_code(rng, rh, nh, M) if which == "A" else _weight_one_row(rng, random_qc_code(rng, rh, nh, M, [3, 2]), M)
        g2 = random_qc_code(rng, rh, nh, M, [2, 4, 3, 4])
        ne = lambda H: int((H >= 0).sum())
        while ne(g2) in (ne(g1), ne(other)):   # three different edge counts: one more circulant in an empty information block
            j, k = np.argwhere(g2[:, rh:] < 0)[0]
            g2[j, rh + k] = rng.randint(0, M)
        return np.array([other, g1, g2] if which == "A" else [g1, other, g2], dtype=np.int16)
    return _memo(("small", M, which, rh, nh), make)


def mixed_table_set():
    """What the table test asks for: a cw2 code next to one that is not, different edge counts, and a block row of weight 1 next to one of
    weight 16 (3 x 18 at M = 7)."""
    def make():
        rng = np.random.RandomState(318)
        rh, nh, M = 3, 18, 7
        a = -np.ones((rh, nh), dtype=np.int16)
        a[0, :16] = rng.randint(0, M, size=16)          # weight 16
        a[1, 16] = rng.randint(0, M)                    # weight 1
        a[2, :] = rng.randint(0, M, size=nh)            # weight 18
        return M, np.array([cycle_code(rng, rh, nh, M), a], dtype=np.int16)
    return _memo("mixed_table", make)


# Channel values of a parity case: frame f is drawn at SNRS[f] dB, from hopeless to clean, so that every (set, decoder) has frames that
# give up, frames that converge and -- the CPU test asserts all three -- one that needs three or more iterations
SNRS = (-3.0, 0.5, 1.5, 2.0, 2.5, 3.0, 4.0, 6.0)


def ladder_llr(H, M, seed, snrs=SNRS):
    return np.concatenate([awgn_llr(np.asarray(H, dtype=np.int32), M, s, seed + 17 * f, 1, burn_codeword=False) for f, s in enumerate(snrs)])


def reference(M, dec):
    """Per (lifting, decoder), once: the codes, the shared [B, N] and per-code [C, B, N] LLRs and the reference's results per layout and code."""
    def make():
        codes = small_set(M, kind(dec))
        shared = ladder_llr(codes[0], M, 100 * M + dec)
        percode = np.array([ladder_llr(codes[0], M, 100 * M + dec + 1000 * (c + 1)) for c in range(len(codes))])
        ref = {"shared": [oracle(dec, H, M, shared) for H in codes], "percode": [oracle(dec, H, M, percode[c]) for c, H in enumerate(codes)]}
        return dict(M=M, codes=codes, shared=shared, percode=percode, ref=ref)
    return _memo(("ref", M, dec), make)


# ---- beyond the limits of every other set entry point
def beyond_set(M):
    """Two 2 x 4 codes: all eight circulants (every block column holds two: cw2), and the same with one circulant less."""
    def make():
        rng = np.random.RandomState(M)
        a = rng.randint(0, M, size=(2, 4)).astype(np.int16)
        b = a.copy()
        b[1, 3] = -1
        return np.array([a, b], dtype=np.int16)
    return _memo(("beyond", M), make)


def beyond_reference(M, dec, frames=4, snrs=(-3.0, 2.0, 4.0, 7.0)):
    def make():
        codes = beyond_set(M)
        llr = ladder_llr(codes[0], M, 31 * M + dec, snrs[:frames])
        return codes, llr, [oracle(dec, H, M, llr) for H in codes]
    return _memo(("beyond_ref", M, dec), make)


def appendix_c_m256():
    """The Appendix C matrix relifted to M = 256 and a relabeling of it: the set whose TDMP image takes 294 928 bytes of LDS; 8 frames."""
    def make():
        H = relift(load_base_matrix(), 256).astype(np.int16)
        codes = np.array([H, LCHE.relabelled(H, 256, 2560)], dtype=np.int16)
        llr = np.concatenate([awgn_llr(H.astype(np.int32), 256, s, 2561 + f, 1, burn_codeword=False) for f, s in enumerate((0.0, 1.0, 1.2, 1.4, 1.6, 1.8, 2.0, 3.0))])
        return codes, llr, [oracle(TASP_DEC, c, 256, llr, 15) for c in codes]
    return _memo("appc256", make)


# ---- workgroups that walk many items: M = 5, the small sets, B frames at 2.5 dB
def walk_inputs(dec, B):
    def make():
        codes = small_set(5, kind(dec))
        llr = awgn_llr(codes[0].astype(np.int32), 5, 2.5, 5000 + dec, B, burn_codeword=False)
        return codes, llr
    return _memo(("walk", dec, B), make)


def walk_reference(dec, B):
    def make():
        codes, llr = walk_inputs(dec, B)
        return [oracle(dec, H, 5, llr) for H in codes]
    return _memo(("walk_ref", dec, B), make)


# ---- both routes: sets that today's entry points take (M = 20, 4 x 8); code 1 is weak (its information columns have weight 1) and
# stops first under the stopping rule
def both_routes_set(dec):
    def make():
        codes = small_set(20, kind(dec)).copy()
        rng = np.random.RandomState(2020)
        weak = codes[1].copy()
        for k in range(4, 8):
            rows = np.flatnonzero(weak[:, k] >= 0)
            keep = rows[:2] if dec in MIN_RW2 else rows[:1]
            weak[np.setdiff1d(rows, keep), k] = -1
        for j in np.flatnonzero((weak >= 0).sum(axis=1) < 2):     # decoders 2, 5, 7 need row weight 2
            if dec in MIN_RW2:
                weak[j, 4 + rng.randint(0, 4)] = rng.randint(0, 20)
        codes[1] = weak
        return codes
    return _memo(("both", dec), make)


SIM = dict(snr=2.5, seed=77, first=1000, B=300)
STOP = dict(snr=2.0, seed=9, nfe=12, nexp=600, ref_fer=0.05, batch=64)
