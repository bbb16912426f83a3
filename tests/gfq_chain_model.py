"""Restatements of what upstream does around its GF(q) decoder, written from the description in include/ldpc_hip.h and DESIGN.md 4.11:

  left2right        decoders.cpp:174-195
  encode            encode_NBQCLDPC, decoders.cpp:1381-1705, in numpy (frames and the M positions of a block vectorised, every step in
                    upstream's order, products through MulTable / InvTable built as upstream builds them)
  syndrome          an independent check of a codeword: H c = 0 over GF(q), products through the logarithm tables
  channel           bp_simulation.cpp:581-582, :638-676, scalar, Python floats and math.exp (glibc's exp; no FMA anywhere)
  count             bp_simulation.cpp:746-755, :805-810
  messages          the K uniform symbols per frame ldpc_hip_simulate_gfq draws (Philox, stream tag 4)
  make_code         test codes upstream's encoder accepts: random information part, a special column of the chosen scheme, rh - 1
                    dual-diagonal columns with shift 0 and one coefficient per column

Test infrastructure only.
"""
import math
import os

import numpy as np

from gfq_model import gf_tables
from ldpc_testlib import philox4x32_10

CHAIN_GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gfq_chain")
TAG_MESSAGE = 4
SCHEMES = ("w2", "xox", "oxo")


class EncodeRefused(Exception):
    """What the library answers with LDPC_HIP_EUNSUPPORTED; .rule names the rule."""

    def __init__(self, rule):
        super().__init__(rule)
        self.rule = rule


def left2right(matr):
    m = np.array(matr)
    rh, nh = m.shape
    assert nh >= rh
    return np.concatenate([m[:, rh:], m[:, rh - 1:rh], m[:, :rh - 1]], axis=1)


def _rotate(x, shift, M):
    """upstream's rotate(): y[I] = x[(I + shift) % M] along the last axis."""
    return np.roll(x, -(shift % M), axis=-1)


def encode(q_bits, hb, hc, M, msg):
    """hb, hc [rh, nh] (hc as decod_init left it), msg [B, K] -> (codeword [B, N] int16, ok [B] int32)."""
    HB = np.asarray(hb, dtype=np.int64)
    HC = np.asarray(hc, dtype=np.int64)
    b, c = HB.shape
    q = 1 << q_bits
    mod = q - 1
    if b < 2:
        raise EncodeRefused("rh < 2")
    if c <= b:
        raise EncodeRefused("nh <= rh")
    for i in range(b):
        for j in range(c):
            if HB[i, j] < -1:
                raise EncodeRefused("shift below -1")
            if HB[i, j] != -1 and (HC[i, j] <= 0 or HC[i, j] >= q):
                raise EncodeRefused("coefficient")                       # :1421-1425
    cb = c - b
    rows = [i for i in range(b) if HB[i, cb] != -1]
    if len(rows) not in (2, 3):
        raise EncodeRefused("wrong weight")                               # :1493-1495
    if HB[0, cb] == -1:
        raise EncodeRefused("empty (0, nh-rh)")
    if HB[b - 1, cb] == -1:
        raise EncodeRefused("empty (rh-1, nh-rh)")
    for j in range(b - 1):
        if HB[j, cb + 1 + j] == -1:
            raise EncodeRefused("empty (j, nh-rh+1+j)")
    alpha, gamma = int(HC[0, cb]), int(HC[b - 1, cb])
    d1 = int(HB[0, cb])
    pos_beta = rows[1]
    if len(rows) == 2:
        if alpha == gamma:
            raise EncodeRefused("weight 2, equal coefficients")           # :1461-1465
        if HB[0, cb] != 0 or HB[b - 1, cb] != 0:
            raise EncodeRefused("weight 2, non-zero shifts")              # :1467-1471
        beta, scheme = alpha ^ gamma, "xox"
    else:
        if alpha != gamma:
            raise EncodeRefused("weight 3, end coefficients differ")      # :1477-1481
        beta, d2 = int(HC[pos_beta, cb]), int(HB[pos_beta, cb])
        scheme = "oxo" if d1 == 0 else "xox"                             # :1491

    lg, alog = gf_tables(q_bits)
    a, bb = np.meshgrid(np.arange(q), np.arange(q), indexing="ij")      # MulTable / InvTable, :1507-1527
    mul = np.where((a == 0) | (bb == 0), 0, alog[(lg[a] + lg[bb]) % mod])
    inv = np.zeros(q, dtype=np.int64)
    for i in range(1, q):
        inv[i] = np.nonzero(mul[i] == 1)[0][-1]

    msg = np.asarray(msg, dtype=np.int64)
    B = msg.shape[0]
    r, n = b * M, c * M
    k = n - r
    assert msg.shape == (B, k) and msg.min(initial=0) >= 0 and msg.max(initial=0) < q
    cw = np.zeros((B, n), dtype=np.int64)
    cw[:, :k] = msg
    synd = np.zeros((B, b, M), dtype=np.int64)
    for j in range(cb):                                                   # :1544-1569
        y = cw[:, j * M:(j + 1) * M]
        for i in range(b):
            if HB[i, j] != -1:
                synd[:, i] ^= mul[_rotate(y, int(HB[i, j]), M), HC[i, j]]
    sumsynd = np.zeros((B, M), dtype=np.int64)
    for i in range(b):
        sumsynd ^= synd[:, i]
    mblock = mul[sumsynd, inv[beta]]                                      # :1580-1581
    if scheme == "oxo":
        mblock = _rotate(mblock, M - d2, M)                               # :1584-1590
    cw[:, k:k + M] = mblock
    if len(rows) == 2:                                                    # :1598-1604
        synd[:, 0] ^= mul[mblock, alpha]
        synd[:, b - 1] ^= mul[mblock, gamma]
    else:
        mblock = mul[mblock, alpha]
        buf = _rotate(mblock, d1, M) if scheme == "xox" else mblock       # :1609-1623
        synd[:, 0] ^= buf
        synd[:, pos_beta] ^= sumsynd
        synd[:, b - 1] ^= buf
    for i in range(cb + 2, c + 1):                                        # :1629-1644
        j = i - c + b - 2
        cw[:, (i - 1) * M:i * M] = mul[synd[:, j], inv[HC[j, i - 1]]]
        synd[:, j + 1] ^= synd[:, j]
    synd[:] = 0                                                           # :1648-1692
    for j in range(c):
        y = cw[:, j * M:(j + 1) * M]
        for i in range(b):
            if HB[i, j] != -1:
                synd[:, i] ^= mul[_rotate(y, int(HB[i, j]), M), HC[i, j]]
    ok = (synd.reshape(B, -1) == 0).all(axis=1).astype(np.int32)
    return cw.astype(np.int16), ok


def syndrome(q_bits, hb, hc, M, cw):
    """[B, R] syndrome of the words cw [B, N]: row block i, lane I: sum_j hc[i, j] * cw[j * M + (I + hb[i, j]) % M] over GF(q)."""
    hb = np.asarray(hb, dtype=np.int64)
    hc = np.asarray(hc, dtype=np.int64)
    cw = np.asarray(cw, dtype=np.int64)
    q = 1 << q_bits
    lg, alog = gf_tables(q_bits)
    rh, nh = hb.shape
    out = np.zeros((cw.shape[0], rh * M), dtype=np.int64)
    lanes = np.arange(M)
    for i in range(rh):
        for j in range(nh):
            if hb[i, j] < 0:
                continue
            x = cw[:, j * M + (lanes + hb[i, j]) % M]
            out[:, i * M:(i + 1) * M] ^= np.where(x == 0, 0, alog[(lg[x] + lg[hc[i, j]]) % (q - 1)])
    return out


def sigma_of(rh, nh, snr_db):
    bitrate = (nh - rh) / nh
    return math.sqrt(math.pow(10, -snr_db / 10) / 2 / bitrate)           # bp_simulation.cpp:444-445


def channel(q_bits, codeword, noise, sigma):
    """codeword [B, N] (or None), noise [B, N * q_bits] -> soft [B, q, N]; every operation a Python float operation in upstream's order."""
    noise = np.asarray(noise, dtype=np.float64)
    B = noise.shape[0]
    N = noise.shape[1] // q_bits
    q = 1 << q_bits
    sigma = float(sigma)
    out = np.empty((B, q, N))
    for f in range(B):
        for i in range(N):
            sym = 0 if codeword is None else int(codeword[f][i])
            x = []
            for k in range(q_bits):
                bit = (sym >> (q_bits - 1 - k)) & 1                       # word2bin: most significant bit first
                x.append(sigma * float(noise[f, i * q_bits + k]) + 2.0 * bit - 1.0)
            qy = []
            for s in range(q):
                lh = 0.0
                for k in range(q_bits):
                    v = float((s >> (q_bits - 1 - k)) & 1) * 2 - 1
                    lh += v * x[k]
                LH = lh / (sigma * sigma)
                try:
                    qy.append(math.exp(LH))
                except OverflowError:                                      # C's exp returns +Inf where Python raises
                    qy.append(math.inf)
            tot = 0.0
            for s in range(q):
                tot += qy[s]
            for s in range(q):
                if math.isinf(qy[s]) and math.isinf(tot):
                    out[f, s, i] = math.nan                                # Inf / Inf
                elif tot == 0.0:
                    out[f, s, i] = math.nan if qy[s] == 0.0 else math.inf
                else:
                    out[f, s, i] = qy[s] / tot
    return out


def channel_lh_range(q_bits, codeword, noise, sigma):
    """All LH = lh / sigma^2 of a set, for the golden maker's check of exp()'s range."""
    soft = []
    noise = np.asarray(noise, dtype=np.float64)
    B, N = noise.shape[0], noise.shape[1] // q_bits
    for f in range(B):
        for i in range(N):
            sym = 0 if codeword is None else int(codeword[f][i])
            x = [sigma * float(noise[f, i * q_bits + k]) + 2.0 * ((sym >> (q_bits - 1 - k)) & 1) - 1.0 for k in range(q_bits)]
            for s in range(1 << q_bits):
                lh = 0.0
                for k in range(q_bits):
                    lh += (float((s >> (q_bits - 1 - k)) & 1) * 2 - 1) * x[k]
                soft.append(lh / (sigma * sigma))
    return np.array(soft)


def count(qhard, codeword, iters, R, counters=None):
    """-> (counters [nse, nde, nue, frames, sum |iters|] accumulated, frame_info [B])."""
    qhard = np.asarray(qhard)
    B, N = qhard.shape
    cnt = [0] * 5 if counters is None else [int(v) for v in counters]
    info = np.zeros(B, dtype=np.int32)
    for f in range(B):
        nse = nse_info = 0
        for i in range(N):
            want = 0 if codeword is None else int(codeword[f][i])
            if int(qhard[f, i]) != want:
                nse += 1
                if i >= R:
                    nse_info += 1
        it = int(iters[f])
        info[f] = nse_info | ((1 << 30) if nse else 0)
        cnt[3] += 1
        cnt[4] += abs(it)
        if nse > 0:
            cnt[0] += nse_info
            cnt[1] += 1
            if it >= 0:
                cnt[2] += 1
    return cnt, info


def messages(q, K, seed, first_frame, B):
    """Symbol i of global frame g: word i % 4 of Philox block (g, i / 4, tag 4), reduced mod q."""
    g = (first_frame + np.arange(B, dtype=np.uint64))[:, None]
    blk = np.arange((K + 3) // 4, dtype=np.uint64)[None, :]
    w = philox4x32_10(g & np.uint64(0xffffffff), g >> np.uint64(32), blk, np.uint64(TAG_MESSAGE), seed & 0xffffffff, seed >> 32)
    out = np.stack(w, axis=-1).reshape(B, -1)[:, :K]
    return (out & np.uint32(q - 1)).astype(np.int16)


def make_code(rng, q_bits, rh, nh, M, scheme, break_diagonal=False):
    """(hb, hc) int16 [rh, nh] that encode_NBQCLDPC accepts (and, for rh >= 2 and nh > rh, that the decoder opens: every block row
    has weight >= 2, no coefficient 0)."""
    assert scheme in SCHEMES and nh > rh >= 2 and (scheme == "w2" or rh >= 3)
    q = 1 << q_bits
    cb = nh - rh
    hb = -np.ones((rh, nh), dtype=np.int64)
    hc = -np.ones((rh, nh), dtype=np.int64)
    for j in range(cb):
        w = rng.randint(2, rh + 1)
        for i in rng.permutation(rh)[:w]:
            hb[i, j] = rng.randint(0, M)
    for i in range(rh):                      # every block row meets the information part
        if (hb[i, :cb] >= 0).sum() == 0:
            hb[i, rng.randint(0, cb)] = rng.randint(0, M)
    there = np.argwhere(hb[:, :cb] >= 0)     # the extreme shifts are always present
    hb[tuple(there[0])] = 0
    hb[tuple(there[-1])] = M - 1
    mid = rh // 2 if rh >= 3 else None
    d = rng.randint(1, M) if M > 1 else 0
    x, y = rng.choice(np.arange(1, q), 2, replace=False)
    if scheme == "w2":
        hb[0, cb] = hb[rh - 1, cb] = 0
        hc[0, cb], hc[rh - 1, cb] = x, y
    elif scheme == "xox":
        hb[0, cb] = hb[rh - 1, cb] = d
        hb[mid, cb] = 0
        hc[0, cb] = hc[rh - 1, cb] = x
        hc[mid, cb] = y
    else:
        hb[0, cb] = hb[rh - 1, cb] = 0
        hb[mid, cb] = d
        hc[0, cb] = hc[rh - 1, cb] = x
        hc[mid, cb] = y
    for j in range(rh - 1):
        hb[j, cb + 1 + j] = hb[j + 1, cb + 1 + j] = 0
        hc[j, cb + 1 + j] = hc[j + 1, cb + 1 + j] = rng.randint(1, q)
    if break_diagonal:
        hb[1, cb + 1] = 1 % M if M > 1 else 0
        hc[1, cb + 1] = hc[0, cb + 1] % (q - 1) + 1   # a different coefficient: the two rows no longer cancel
    hc = np.where((hb >= 0) & (hc < 0), rng.randint(1, q, hb.shape), hc)
    return hb.astype(np.int16), hc.astype(np.int16)
