"""Shared test helpers: fixtures, ctypes bindings to the CPU oracle (oracle/liboracle.so) and, when it was
built in the container that has the upstream tree, to the compiled reference (oracle/_ref/libldpc_ref.so).

Everything here is test infrastructure; the product (ldpc-lib_amd) never imports it.
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")

# decoders.h:16-28 enum DEC_ID
BP_DEC, SP_DEC, ASP_DEC, MS_DEC, IMS_DEC, IASP_DEC, FHT_DEC, TASP_DEC, LMS_DEC, LCHE_DEC = range(10)

c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)
c_short_p = C.POINTER(C.c_short)


def load_base_matrix():
    """the 16x32 base matrix the reference's own `search` produced (shifts mod 126)."""
    return np.loadtxt(os.path.join(GOLDEN_DIR, "h16x32_m126.txt"), dtype=np.int32)


def relift(H, M):
    """main_simulation.cpp:400-414: entries > 0 become entry % M; in column rows-1 a result of 0 becomes 1."""
    H = np.array(H, dtype=np.int32, copy=True)
    rows = H.shape[0]
    for i in range(H.shape[0]):
        for j in range(H.shape[1]):
            if H[i, j] > 0:
                t = int(H[i, j]) % M
                if j == rows - 1 and t == 0:
                    t = 1
                H[i, j] = t
    return H


def _as_double_p(a):
    return a.ctypes.data_as(c_double_p)


class SimResult(C.Structure):
    _fields_ = [("ber", C.c_double), ("fer", C.c_double), ("nse", C.c_longlong), ("nde", C.c_longlong),
                ("nue", C.c_longlong), ("experiment", C.c_longlong), ("sum_abs_iter", C.c_longlong),
                ("rng_next", C.c_uint)]


_oracle_lib = None


def oracle_lib():
    """Load (building on demand with plain gcc/g++) the CPU restatement."""
    global _oracle_lib
    if _oracle_lib is not None:
        return _oracle_lib
    so = os.path.join(ORACLE_DIR, "liboracle.so")
    srcs = [os.path.join(ORACLE_DIR, f) for f in ("ldpc_oracle.c", "ldpc_oracle.h", "harness_oracle.cpp", "harness_oracle.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["make", "-s", "-C", ORACLE_DIR, "liboracle.so"])
    lib = C.CDLL(so)
    lib.orc_open.restype = C.c_void_p
    lib.orc_open.argtypes = [C.c_int, C.c_int, C.c_int, c_short_p]
    lib.orc_close.argtypes = [C.c_void_p]
    lib.orc_n.argtypes = [C.c_void_p]
    lib.orc_min_sum.argtypes = [C.c_void_p, c_double_p, c_double_p, C.c_int, C.c_int, C.c_double]
    lib.orc_lmin_sum.argtypes = [C.c_void_p, c_double_p, c_double_p, C.c_int, C.c_int]
    lib.orc_sum_prod.argtypes = [C.c_void_p, c_double_p, c_double_p, C.c_int, C.c_int]
    lib.orc_imin_sum.argtypes = [C.c_void_p, c_double_p, c_double_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int]
    lib.orc_sum_prod_gf2.argtypes = [C.c_void_p, c_double_p, c_double_p, C.c_int, C.c_int]
    lib.orc_bp.argtypes = [C.c_void_p, c_double_p, c_double_p, C.c_int, C.c_int]
    lib.orc_bp_stale.argtypes = [C.c_void_p]
    lib.orc_bp_stale.restype = C.POINTER(C.c_ubyte)
    lib.orc_tdmp_sum_prod.argtypes = [C.c_void_p, c_double_p, c_double_p, C.c_int, c_double_p]
    lib.orc_syndrome_nonzero.argtypes = [C.c_void_p, c_double_p]
    lib.orc_qam_modulate.argtypes = [C.c_int, c_double_p, C.c_int, c_double_p]
    lib.orc_qam_demodulate.argtypes = [C.c_int, C.c_double, C.c_double, c_double_p, C.c_int, c_double_p, C.c_int]
    lib.orc_bp_simulation.argtypes = [C.c_int, C.c_int, c_int_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                      C.c_double, C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(SimResult), c_int_p]
    lib.orc_rng_gaussians.argtypes = [C.c_uint, C.c_int, c_double_p, C.c_int]
    lib.orc_awgn_llr.argtypes = [C.c_uint, C.c_int, C.c_double, C.c_double, c_double_p, C.c_int]
    _oracle_lib = lib
    return lib


def ref_lib():
    """The compiled upstream reference (only exists where oracle/Makefile's `ref` target was run). None if absent."""
    so = os.path.join(ORACLE_DIR, "_ref", "libldpc_ref.so")
    if not os.path.exists(so):
        return None
    lib = C.CDLL(so)
    lib.ref_open.restype = C.c_void_p
    lib.ref_open.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, c_short_p]
    lib.ref_close.argtypes = [C.c_void_p]
    lib.ref_decode.argtypes = [C.c_void_p, C.c_int, c_double_p, c_double_p, C.c_int, C.c_int]
    if hasattr(lib, "ref_decode_alpha"):
        lib.ref_decode_alpha.argtypes = [C.c_void_p, C.c_int, c_double_p, c_double_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int]
    lib.ref_qam_modulate.argtypes = [C.c_int, c_double_p, C.c_int, c_double_p]
    lib.ref_qam_demodulate.argtypes = [C.c_int, C.c_double, C.c_double, c_double_p, C.c_int, c_double_p, C.c_int]
    return lib


IMS_DEFAULTS = (1.4, 6, 8)   # decoders.cpp MS_THR, MS_QBITS, MS_DBITS


class _Decoder:
    """Common batch front end: decode(llr[B,N]) -> (decword[B,N] float64, iters[B] int32, llr_after[B,N]).
    alpha: the normalisation factor of MS_DEC and IMS_DEC (upstream's MS_ALPHA by default); ims = (thr, qbits, dbits) of IMS_DEC.  The
    other decoders ignore both, as upstream's do."""

    def decode(self, dec_id, llr, maxiter, decision=0, alpha=0.8, ims=IMS_DEFAULTS):
        llr = np.ascontiguousarray(llr, dtype=np.float64)
        single = llr.ndim == 1
        if single:
            llr = llr[None, :]
        B, N = llr.shape
        assert N == self.N
        dec = np.empty((B, N), dtype=np.float64)
        its = np.empty(B, dtype=np.int32)
        after = llr.copy()
        for b in range(B):
            its[b] = self._one(dec_id, after[b], dec[b], maxiter, decision, alpha, ims)
        if single:
            return dec[0], int(its[0]), after[0]
        return dec, its, after


class Oracle(_Decoder):
    def __init__(self, H, M):
        self.lib = oracle_lib()
        H = np.ascontiguousarray(H, dtype=np.int16)
        self.rh, self.nh = H.shape
        self.M = M
        self.N = self.nh * M
        self.R = self.rh * M
        self.h = self.lib.orc_open(self.rh, self.nh, M, H.ctypes.data_as(c_short_p))
        assert self.h

    def close(self):
        if self.h:
            self.lib.orc_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _one(self, dec_id, y, dec, maxiter, decision, alpha=0.8, ims=IMS_DEFAULTS):
        yp, dp = _as_double_p(y), _as_double_p(dec)
        if dec_id == MS_DEC:
            return self.lib.orc_min_sum(self.h, yp, dp, maxiter, decision, alpha)
        if dec_id == LMS_DEC:
            return self.lib.orc_lmin_sum(self.h, yp, dp, maxiter, decision)
        if dec_id == SP_DEC:
            return self.lib.orc_sum_prod(self.h, yp, dp, maxiter, decision)
        if dec_id == IMS_DEC:
            return self.lib.orc_imin_sum(self.h, yp, dp, maxiter, decision, alpha, *ims)
        if dec_id == BP_DEC:
            return self.lib.orc_bp(self.h, yp, dp, maxiter, decision)
        if dec_id == ASP_DEC:
            return self.lib.orc_sum_prod_gf2(self.h, yp, dp, maxiter, decision)
        if dec_id == TASP_DEC:  # decision is dead upstream: decword is always hard; decision=1 here returns the posteriors
            if decision:
                tmp = np.empty_like(dec)
                return self.lib.orc_tdmp_sum_prod(self.h, yp, _as_double_p(tmp), maxiter, dp)
            return self.lib.orc_tdmp_sum_prod(self.h, yp, dp, maxiter, None)
        raise ValueError(dec_id)


class Reference(_Decoder):
    """The compiled upstream decoders (oracle/_ref). Construct only when ref_lib() is not None."""

    def __init__(self, dec_id, H, M):
        self.lib = ref_lib()
        assert self.lib is not None
        H = np.ascontiguousarray(H, dtype=np.int16)
        self.rh, self.nh = H.shape
        self.M = M
        self.N = self.nh * M
        self.dec_id = dec_id
        self.h = self.lib.ref_open(dec_id, self.rh, self.nh, M, H.ctypes.data_as(c_short_p))
        assert self.h

    def close(self):
        if self.h:
            self.lib.ref_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _one(self, dec_id, y, dec, maxiter, decision, alpha=0.8, ims=IMS_DEFAULTS):
        assert dec_id == self.dec_id
        if dec_id in (MS_DEC, IMS_DEC) and (alpha != 0.8 or np.signbit(alpha) or tuple(ims) != IMS_DEFAULTS):
            return self.lib.ref_decode_alpha(self.h, dec_id, _as_double_p(y), _as_double_p(dec), maxiter, decision, alpha, *ims)
        return self.lib.ref_decode(self.h, dec_id, _as_double_p(y), _as_double_p(dec), maxiter, decision)


def code_rate(H):
    rh, nh = H.shape
    return (nh - rh) / nh


def awgn_llr(H, M, snr_db, seed, frames, burn_codeword=True):
    """LLRs in the reference's draw order (bp_simulation.cpp:512,600-605): one mt19937 stream, the
    (nh-rh)*M next_random_int draws of random_codeword() first, then frames*N Gaussians."""
    lib = oracle_lib()
    rh, nh = H.shape
    N = nh * M
    out = np.empty(frames * N, dtype=np.float64)
    lib.orc_awgn_llr(seed, (nh - rh) * M if burn_codeword else 0, snr_db, code_rate(H), _as_double_p(out), frames * N)
    return out.reshape(frames, N)


def pack_bits(dec):
    """decword (0.0/1.0 doubles, [B,N]) -> little-endian packed uint32 words [B, ceil(N/32)] (bit i of word w = variable 32*w+i)."""
    dec = np.asarray(dec)
    B, N = dec.shape
    W = (N + 31) // 32
    bits = np.zeros((B, W * 32), dtype=np.uint8)
    bits[:, :N] = dec != 0
    return np.packbits(bits.reshape(B, W, 32), axis=2, bitorder="little").view(np.uint32).reshape(B, W)


# ---- CPU twin of the device noise generator (ldpc-lib_amd/csrc/ldpc_frontend.hpp) ---------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10 (Salmon et al. 2011).  All arguments uint32 arrays (broadcastable)."""
    c = [np.asarray(x, dtype=np.uint64) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0 = np.uint64(k0)
    k1 = np.uint64(k1)
    M0, M1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = M0 * c[0]
        p1 = M1 * c[2]
        n0 = ((p1 >> np.uint64(32)) ^ c[1] ^ k0) & mask
        n1 = p1 & mask
        n2 = ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & mask
        n3 = p0 & mask
        c = [n0, n1, n2, n3]
        k0 = (k0 + np.uint64(0x9E3779B9)) & mask
        k1 = (k1 + np.uint64(0xBB67AE85)) & mask
    return [x.astype(np.uint32) for x in c]


def philox_gauss_pairs(seed, frames, npairs, tag=0):
    """Box-Muller pairs exactly as gauss_pair() on the device (up to libm-vs-ocml rounding): returns [len(frames), 2*npairs]."""
    frames = np.asarray(frames, dtype=np.uint64)[:, None]
    pair = np.arange(npairs, dtype=np.uint64)[None, :]
    x = philox4x32_10(frames & np.uint64(0xFFFFFFFF), frames >> np.uint64(32), pair, np.uint64(tag),
                      np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    a = ((x[0].astype(np.uint64) << np.uint64(32)) | x[1].astype(np.uint64)) >> np.uint64(11)
    b = ((x[2].astype(np.uint64) << np.uint64(32)) | x[3].astype(np.uint64)) >> np.uint64(11)
    u1 = (a.astype(np.float64) + 0.5) / 9007199254740992.0
    u2 = (b.astype(np.float64) + 0.5) / 9007199254740992.0
    rad = np.sqrt(-2.0 * np.log(u1))
    g = np.empty((frames.shape[0], 2 * npairs))
    g[:, 0::2] = rad * np.cos(2.0 * np.pi * u2)
    g[:, 1::2] = rad * np.sin(2.0 * np.pi * u2)
    return g


def bpsk_sigma(H, snr_db, punctured_blocks=0):
    rh, nh = H.shape
    rate = (nh - rh) / (nh - punctured_blocks)
    return np.sqrt(10.0 ** (-snr_db / 10.0) / 2 / rate)   # bp_simulation.cpp:444-445


def syndrome_np(H, M, hard_bits):
    """hard_bits [B,N] 0/1 -> [B] bool: any parity check fails (edge rule: check (j,n) -- variable (k,(n+c)%M))."""
    hard_bits = np.asarray(hard_bits, dtype=np.uint8)
    B = hard_bits.shape[0]
    rh, nh = H.shape
    cols = hard_bits.reshape(B, nh, M)
    fail = np.zeros(B, dtype=bool)
    for j in range(rh):
        s = np.zeros((B, M), dtype=np.uint8)
        for k in range(nh):
            if H[j, k] >= 0:
                s ^= np.roll(cols[:, k, :], -int(H[j, k]) % M, axis=1)
        fail |= s.any(axis=1)
    return fail


def unpack_bits(hard_words, N):
    """packed uint32 [B,W] -> [B,N] uint8"""
    w = np.ascontiguousarray(hard_words).view(np.uint32)
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")
    return bits[:, :N]


def random_qc_code(rng, rh, nh, M, info_weight):
    """A random protograph of the usual shape: dual-diagonal parity part (block columns 0..rh-1, shifts 0, one extra entry
    closing the chain) and `info_weight[k]` random circulants in every information column."""
    H = -np.ones((rh, nh), dtype=np.int16)
    for j in range(rh):
        H[j, j] = 0
        if j + 1 < rh:
            H[j + 1, j] = 0
    H[0, rh - 1] = 1 % M
    H[rh // 2, rh - 1] = 0 if H[rh // 2, rh - 1] < 0 else H[rh // 2, rh - 1]
    for k in range(rh, nh):
        rows = rng.choice(rh, size=min(rh, info_weight[(k - rh) % len(info_weight)]), replace=False)
        for j in rows:
            H[j, k] = rng.randint(0, M)
    for j in range(rh):                      # every check sees at least two information columns
        while (H[j, rh:] >= 0).sum() < 2:
            H[j, rh + rng.randint(0, nh - rh)] = rng.randint(0, M)
    return H


def cycle_code(rng, rh, nh, M):
    """A protograph in which EVERY block column has exactly two circulants (and every block row at least two): the shape upstream's
    sum_prod_gf2_decod_qc_lm decodes in its own branch (asp_all_cw_2, decoders.cpp:1027-1044, :2431-2480)."""
    while True:
        H = -np.ones((rh, nh), dtype=np.int16)
        for k in range(nh):
            for j in rng.choice(rh, size=2, replace=False):
                H[j, k] = rng.randint(0, M)
        if ((H >= 0).sum(axis=1) >= 2).all():
            return H


def multi_block_code(rng, M, blocks=(4, 4), ninfo=6):
    """A base matrix whose parity part consists of several dual-diagonal blocks (bp_simulation.cpp:142-191 encodes them from the last
    to the first): block q has its own double diagonal and special column (shifts 0, s > 0, 0); earlier blocks' rows also touch the
    parity columns of later blocks, which they treat like information columns."""
    b = int(sum(blocks))
    H = -np.ones((b, b + ninfo), dtype=np.int16)
    off = 0
    for rb in blocks:
        hi = off + rb
        for t in range(rb - 1):
            H[off + t, off + t] = 0
            H[off + t + 1, off + t] = 0
        H[off, hi - 1] = 0
        H[off + rb // 2, hi - 1] = 1 + rng.randint(0, max(M - 1, 1)) if M > 1 else 0
        H[hi - 1, hi - 1] = 0
        for _ in range(2):                       # rows of this block on parity columns of LATER blocks
            if hi < b:
                H[off + rng.randint(0, rb), rng.randint(hi, b)] = rng.randint(0, M)
        off = hi
    for k in range(b, b + ninfo):
        for j in rng.choice(b, size=3, replace=False):
            H[j, k] = rng.randint(0, M)
    for j in range(b):
        while (H[j, b:] >= 0).sum() < 1:
            H[j, b + rng.randint(0, ninfo)] = rng.randint(0, M)
    return H


# ---- bitwise comparison and adversarial channel values ---------------------------------------------------------------------------
def assert_bits_equal(got, want, what="", nan_ok=False):
    """float64 arrays identical bit for bit.  np.array_equal treats +0.0 == -0.0 (and NaN != NaN), so it checks a "bit-identical"
    claim only up to the sign of zero; this compares the uint64 images and names the first differing index with both values in hex.
    nan_ok: NaN positions must match exactly and every other value bit for bit; the NaNs' payloads and signs are not compared (the
    default NaN of x86 arithmetic has the sign bit set, the GPU's does not)."""
    got = np.ascontiguousarray(np.asarray(got), dtype=np.float64)
    want = np.ascontiguousarray(np.asarray(want), dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    g, w = got.view(np.uint64), want.view(np.uint64)
    bad = g != w
    if nan_ok:
        gn, wn = np.isnan(got), np.isnan(want)
        bad = (bad & ~(gn & wn)) | (gn != wn)
    if bad.any():
        flat = np.flatnonzero(bad)
        i = np.unravel_index(flat[0], got.shape)
        raise AssertionError(f"{what}: {flat.size} of {got.size} values differ; first at {tuple(int(x) for x in i)}: got {got[i]!r} "
                             f"(0x{int(g[i]):016x}), want {want[i]!r} (0x{int(w[i]):016x})")


# ---- min-sum normalisation factors other than upstream's MS_ALPHA = 0.8 ---------------------------------------------------------------
# 1.0: no scaling; 0.5: an exact power of two; 0.75: a second inexact factor; 1.25, 2.0: messages grow into the 32767 clamp of STATE3 on
# their own; 1e-310: denormal products; 0.0: zero factor; -0.0, -0.8: sign bit set (upstream's product keeps it, decoders.cpp:4719-4720)
MS_ALPHAS = (1.0, 0.5, 0.75, 1.25, 2.0, 1e-310, 0.0, -0.0, -0.8)
# integer min-sum: ialpha = (int)(alpha * 16) = 8, 15, 16, 0, and 20 and -12, which an int8 message does not hold
IMS_ALPHAS = (0.5, 0.99, 1.0, 0.03, 1.25, -0.8)
ALPHA_SWEEP_SNRS = (1.4, 3.0, 4.5, 6.0, 8.0, 15.0)


def alpha_sweep_llr(H, M, seed=0, per_snr=4):
    """The batch the alpha tests decode: per_snr AWGN frames at each of ALPHA_SWEEP_SNRS (at 15 dB the frames arrive as codewords: with a
    zero, denormal or negative factor nothing else returns 1), zeros of both signs, values beyond the clamp and a denormal-ish value at
    the start of frame 0, and one frame of adversarial_llr's "alphabet {1}" family (min1 == min2 in every check, at every alpha)."""
    Hi = np.asarray(H, dtype=np.int32)
    llr = np.concatenate([awgn_llr(Hi, M, s, 700 + 10 * seed + i, per_snr) for i, s in enumerate(ALPHA_SWEEP_SNRS)])
    llr[0, :5] = [0.0, -0.0, 40000.0, -40000.0, 1e-300]
    adv, labels = adversarial_llr(H, M, seed)
    tie = adv[labels.index("alphabet {1}: min1 == min2 everywhere")]
    return np.ascontiguousarray(np.concatenate([llr, tie[None, :]]))


# default integer min-sum parameters (decoders.cpp MS_THR / MS_QBITS): the quantiser-boundary frames are tuned for them
IMS_THR, IMS_QBITS = 1.4, 6


def _ims_coef(y):
    """sqrt(N / en) with en summed in index order, as upstream's quantiser (and every IMS tier) computes it."""
    en = 0.0
    for v in (y * y).tolist():
        en += v
    return np.sqrt(len(y) / en) if en else np.inf


def _quantiser_boundary_frame(rng, N, thr=IMS_THR, qbits=IMS_QBITS):
    """+-1 everywhere but every 8th value, which is picked so that the energy-normalised quantiser's val * max_quant / thr + 0.5 sits
    within an ulp of an integer -- where floor() of it differs from floor(val * (max_quant / thr) + 0.5): the order of the
    multiply and the divide decides the quantised value.  The scale coef depends on the frame's energy, so the picks are iterated
    until coef no longer moves."""
    mq = (1 << (qbits - 1)) - 1
    y = np.where(rng.rand(N) < 0.04, -1.0, 1.0)
    slots = np.arange(3, N, 8)
    steps = np.arange(-256, 257, dtype=np.int64)
    level = rng.randint(1, mq, size=slots.size)
    target = (level - 0.5) * thr / mq                       # val * coef on the rounding boundary of quantiser level `level`
    y[slots] = np.copysign(target / np.sqrt((N - (target ** 2).sum()) / (N - slots.size)), y[slots])   # solves en = N / coef^2
    for _ in range(20):
        coef = _ims_coef(y)
        t = (level - 0.5) * thr / (mq * coef)
        v = (t.view(np.int64)[:, None] + steps[None, :]).view(np.float64)     # t and its 256 neighbours on either side
        a = np.minimum(v * coef, thr)
        hit = np.floor(a * mq / thr + 0.5) != np.floor(a * (mq / thr) + 0.5)
        j = np.where(hit.any(axis=1), hit.argmax(axis=1), 256)                 # a slot without a sensitive neighbour keeps t
        y[slots] = np.copysign(v[np.arange(slots.size), j], y[slots])
        if _ims_coef(y) == coef:
            break
    return y


def adversarial_llr(H, M, seed):
    """Deterministic batch of finite channel LLRs aimed at the arguments the kernels make at the edges of their input range (the
    sign bit and the `+ 0.0` canonicalisation, subnormals, the MAX_VAL / INPUT_LIMIT / +-40 clamps, the integer quantiser's
    en = 0 and en = inf cases, exact min1 == min2 ties, quantiser rounding boundaries, codewords and all-negative frames).  Each
    family appears as whole frames and mixed into AWGN frames.  Returns (llr [B, N] float64, labels [B])."""
    rng = np.random.RandomState(seed)
    rh, nh = np.asarray(H).shape
    N = nh * M
    base = awgn_llr(np.asarray(H, dtype=np.int32), M, 2.0, 1000 + seed, 16, burn_codeword=False)
    nxt = iter(range(len(base)))

    def awgn():
        return base[next(nxt)].copy()

    def signs(p=0.05):   # the zero codeword's sign pattern (all positive) with a fraction p of flips
        return np.where(rng.rand(N) < p, -1.0, 1.0)

    def pick(values, p=0.05):
        return rng.choice(np.asarray(values, dtype=np.float64), size=N) * signs(p)

    lim = [20.0, 40.0, np.nextafter(20.0, 0), np.nextafter(20.0, 99), np.nextafter(40.0, 0), np.nextafter(40.0, 99), 19.999999, 39.999999]
    families = [
        ("+0.0", np.zeros(N)),
        ("-0.0", -np.zeros(N)),
        ("random +-0.0", np.where(rng.rand(N) < 0.5, -0.0, 0.0)),
        ("+-1e-310 subnormals", 1e-310 * signs()),
        ("+-1e-170, squares underflow", 1e-170 * signs()),
        ("subnormals and exact zeros", pick([1e-310, 5e-324, 2.2e-308, 0.0, -0.0, 0.0])),
        ("+-1e155", 1e155 * signs(0.08)),
        ("+-1e200", 1e200 * signs(0.08)),
        ("+-20 / +-40 and neighbours", pick(lim, 0.08)),
        ("alphabet {1, 2, 3}", pick([1.0, 2.0, 3.0], 0.04)),
        ("alphabet {1}: min1 == min2 everywhere", pick([1.0], 0.03)),
        ("+-1", pick([1.0], 0.08)),
        ("integer quantiser boundaries", _quantiser_boundary_frame(rng, N)),
        ("all -1", -np.ones(N)),
    ]
    llr, labels = [], []
    for name, y in families:
        llr.append(y)
        labels.append(name)
    a = awgn()
    llr.append(a * 1e6); labels.append("awgn x 1e6")
    a = awgn()
    llr.append(np.abs(a) + 0.1); labels.append("a codeword")
    a = awgn()
    llr.append(-(np.abs(a) + 0.1)); labels.append("all negative")
    for name, stride, z in (("every 5th -0.0", 5, -0.0), ("every 7th +0.0", 7, 0.0), ("every 5th +0.0", 5, 0.0), ("every 7th -0.0", 7, -0.0)):
        a = awgn()
        a[rng.randint(stride)::stride] = z
        llr.append(a); labels.append("awgn, " + name)
    for name, y in families[3:10]:   # the value families mixed into AWGN frames
        a = awgn()
        m = rng.rand(N) < 0.2
        a[m] = np.abs(y[m]) * np.sign(a[m])
        llr.append(a); labels.append("awgn with " + name)
    llr = np.ascontiguousarray(np.array(llr, dtype=np.float64))
    assert np.isfinite(llr).all()
    return llr, labels
