"""A plain numpy restatement of upstream's GF(q) sum-product decoder with Walsh-Hadamard check nodes (FHT_DEC, decoder id 6:
sum_prod_gfq_decod_lm with map_graph, the SUM_PROD_GFQ_ORIG / COLUMN_BY_COLUMN build, p_thr = 0), written from the description in
include/ldpc_hip.h and DESIGN.md 4.10.  Frames and circulant lanes are vectorised; everything whose order matters is not: butterfly
stages run low to high, products run left to right, sums over the q symbols ascend one by one from 0 (np.sum is pairwise and would
round differently).  numpy's float64 +, -, *, / are the IEEE operations, so the results equal the compiled reference bit for bit
(tools/make_gfq_goldens.py and tests/test_gfq_cpu.py check that).  Test infrastructure only.
"""
import os

import numpy as np

GFQ_GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gfq")

# first primitive polynomial of each degree 1..10 in upstream's bank
PRIMITIVE = {1: 3, 2: 7, 3: 13, 4: 19, 5: 37, 6: 67, 7: 131, 8: 285, 9: 529, 10: 1033}


def gf_tables(q_bits):
    """(log, alog) as upstream leaves them in zeroed arrays: alog[i] = x^i for i < q - 1, alog[q - 1] = 0, log[0] = -1."""
    q = 1 << q_bits
    lg = np.zeros(q, dtype=np.int64)
    alog = np.zeros(q, dtype=np.int64)
    lg[0] = -1
    e = 1
    for i in range(q - 1):
        alog[i] = e
        lg[e] = i
        e <<= 1
        if e >= q:
            e ^= PRIMITIVE[q_bits]
    return lg, alog


def mul_div_tables(q_bits, coefs):
    """mul[c][s] = s * coefs[c], div[c][s] = s / coefs[c] in GF(2^q_bits); column 0 stays 0."""
    q = 1 << q_bits
    lg, alog = gf_tables(q_bits)
    mul = np.zeros((len(coefs), q), dtype=np.int64)
    div = np.zeros((len(coefs), q), dtype=np.int64)
    for c, v in enumerate(coefs):
        for s in range(1, q):
            mul[c, s] = alog[(lg[s] + lg[v]) % (q - 1)]
            div[c, s] = alog[(lg[s] - lg[v]) % (q - 1)]
    return mul, div


def fht(y):
    """Walsh-Hadamard butterflies along the last axis: stage i pairs the indices that differ in bit i, low stage first; the lower
    index gets a + b, the upper a - b."""
    q = y.shape[-1]
    f = 1
    while f < q:
        v = y.reshape(y.shape[:-1] + (q // (2 * f), 2, f))
        a, b = v[..., 0, :], v[..., 1, :]
        y = np.stack([a + b, a - b], axis=-2).reshape(y.shape)
        f *= 2
    return y


def _sum_ascending(v):
    s = np.zeros(v.shape[:-1], dtype=np.float64)
    for j in range(v.shape[-1]):
        s = s + v[..., j]
    return s


class GfqModel:
    def __init__(self, q_bits, hb, hc, M, ncols2convert=0):
        hb = np.asarray(hb, dtype=np.int64)
        hc = np.asarray(hc, dtype=np.int64)
        self.q_bits, self.q, self.M = int(q_bits), 1 << int(q_bits), int(M)
        self.rh, self.nh = hb.shape
        self.N, self.R = self.nh * self.M, self.rh * self.M
        assert 2 <= q_bits <= 10
        self.rows = []   # per block row: list of (edge index, column, shift, coefficient)
        e = 0
        for j in range(self.rh):
            row = []
            for k in range(self.nh):
                if hb[j, k] >= 0:
                    assert 1 <= hc[j, k] < self.q, "coefficient outside 1 .. q-1"
                    row.append((e, k, int(hb[j, k]) % self.M, int(hc[j, k])))
                    e += 1
            assert len(row) >= 2, "block row of weight < 2"
            self.rows.append(row)
        self.E = e
        self.cols = [[ed for row in self.rows for ed in row if ed[1] == k] for k in range(self.nh)]   # ascending rows
        self.cw2 = all(len(c) == 2 for c in self.cols)
        self.coefs = sorted({ed[3] for row in self.rows for ed in row})
        self.rl = {v: i for i, v in enumerate(self.coefs)}
        self.mul, self.div = mul_div_tables(q_bits, self.coefs)
        _, alog = gf_tables(q_bits)
        self.hc_after = hc.copy()   # the tables come from hc as given; the conversion only rewrites the matrix
        for j in range(self.rh):
            for k in range(ncols2convert):
                if self.hc_after[j, k] > -1:
                    self.hc_after[j, k] = alog[self.hc_after[j, k]]
        self.hc_after = self.hc_after.astype(np.int16)

    def decode(self, soft, maxiter):
        """soft [B, q, N] -> (iters [B] int32, qhard [B, N] int16, post [B, q, N])."""
        soft = np.ascontiguousarray(soft, dtype=np.float64)
        if soft.ndim == 2:
            soft = soft[None]
        B = soft.shape[0]
        assert soft.shape[1:] == (self.q, self.N)
        q, M = self.q, self.M
        lanes = np.arange(M)
        x = soft.transpose(0, 2, 1)                       # [B, N, q]
        post = x.copy()
        win = np.empty((B, self.E, M, q))
        wout = np.zeros((B, self.E, M, q))
        for row in self.rows:
            for e, k, sh, _ in row:
                win[:, e] = x[:, k * M + (lanes + sh) % M]
        iters = np.full(B, -maxiter, dtype=np.int32)
        qhard = np.zeros((B, self.N), dtype=np.int16)
        live = np.arange(B)
        qinv = 1.0 / float(q)
        with np.errstate(all="ignore"):
            for it in range(maxiter):
                if live.size == 0:
                    break
                p = post[live]
                mx = np.zeros(p.shape[:-1])
                pos = np.zeros(p.shape[:-1], dtype=np.int16)
                for j in range(q):
                    up = mx < p[..., j]
                    mx = np.where(up, p[..., j], mx)
                    pos = np.where(up, np.int16(j), pos)
                qhard[live] = pos
                bad = np.zeros(live.size, dtype=bool)
                for row in self.rows:
                    acc = np.zeros((live.size, M), dtype=np.int64)
                    for e, k, sh, v in row:
                        acc ^= self.mul[self.rl[v]][pos[:, k * M + (lanes + sh) % M]]
                    bad |= acc.any(axis=1)
                iters[live[~bad]] = it
                live = live[bad]
                if live.size == 0:
                    break
                wi, wo, xs = win[live], wout[live], x[live]
                for row in self.rows:                      # check nodes
                    rw = len(row)
                    S = [fht(wi[:, e][..., self.div[self.rl[v]]]) for e, _, _, v in row]
                    F, Bk = [None] * rw, [None] * rw
                    F[0] = S[0]
                    for s in range(1, rw - 1):
                        F[s] = S[s] * F[s - 1]
                    Bk[rw - 1] = S[rw - 1]
                    for s in range(rw - 2, 0, -1):
                        Bk[s] = S[s] * Bk[s + 1]
                    for s, (e, _, _, v) in enumerate(row):
                        Z = Bk[1] if s == 0 else F[rw - 2] if s == rw - 1 else F[s - 1] * Bk[s + 1]
                        out = fht(Z)[..., self.mul[self.rl[v]]] * qinv
                        wo[:, e] = np.where(out < 0.00001, 0.00001, out)
                po = np.empty_like(xs)
                for k, col in enumerate(self.cols):         # symbol nodes
                    xv = xs[:, k * M:(k + 1) * M]
                    at = [(lanes - sh) % M for _, _, sh, _ in col]
                    outs = [wo[:, e][:, at[i]] for i, (e, _, _, _) in enumerate(col)]
                    if self.cw2:
                        y0, y1 = xv * outs[0], xv * outs[1]
                        so = y1 * outs[0]
                        so = so * (1.0 / _sum_ascending(so))[..., None]
                        new = [y1 * (1.0 / _sum_ascending(y1))[..., None], y0 * (1.0 / _sum_ascending(y0))[..., None]]
                    elif len(col) == 2:
                        so = xv * outs[0] * outs[1]
                        so = so * (1.0 / _sum_ascending(so))[..., None]
                        n0, n1 = xv * outs[1], xv * outs[0]
                        new = [n0 * (1.0 / _sum_ascending(n0))[..., None], n1 * (1.0 / _sum_ascending(n1))[..., None]]
                    else:
                        so = xv
                        for o in outs:
                            so = so * o
                        so = so * (1.0 / _sum_ascending(so))[..., None]
                        new = []
                        for o in outs:
                            t = so / o
                            new.append(t * (1.0 / _sum_ascending(t))[..., None])
                    po[:, k * M:(k + 1) * M] = so
                    for i, (e, _, _, _) in enumerate(col):
                        wi[:, e][:, at[i]] = new[i]
                win[live], wout[live], post[live] = wi, wo, po
        return iters, qhard, np.ascontiguousarray(post.transpose(0, 2, 1))


def bpsk_symbol_probabilities(rng, q_bits, N, sigma, B, bits=None):
    """Probability vectors [B, q, N] of the all-zero word (or `bits` [N * q_bits]) after BPSK + AWGN, formed as upstream's q-ary
    harness forms them (bp_simulation.cpp:638-676): y = sigma * g + 2 * bit - 1 per bit, likelihood of symbol s at position i
    exp(sum_k (2 * bit_k(s) - 1) * y[i * q_bits + k] / sigma^2), most significant bit first, normalised by the ascending sum."""
    q = 1 << q_bits
    tx = np.zeros(N * q_bits) if bits is None else np.asarray(bits, dtype=np.float64)
    y = sigma * rng.standard_normal((B, N * q_bits)) + 2.0 * tx - 1.0
    y = y.reshape(B, N, q_bits)
    out = np.empty((B, q, N))
    with np.errstate(all="ignore"):   # at very high SNR exp overflows and the vector becomes Inf / Inf = NaN, as upstream's would
        for s in range(q):
            v = np.array([2.0 * ((s >> (q_bits - 1 - k)) & 1) - 1.0 for k in range(q_bits)])
            lh = np.zeros((B, N))
            for k in range(q_bits):
                lh = lh + v[k] * y[:, :, k]
            out[:, s, :] = np.exp(lh / (sigma * sigma))
        tot = np.zeros((B, N))
        for s in range(q):
            tot = tot + out[:, s, :]
        return out / tot[:, None, :]
