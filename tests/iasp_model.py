"""Integer advanced sum-product decoder (IASP_DEC, decoder id 5) restated in numpy: the live checker of the GPU tests.

Written from the contract of upstream's isum_prod_gf2_decod_qc_lm (decoders.cpp:3822-4121, IASP_FIXED_POINT branch) with its
helpers imap_bin (:2235-2271), icheck_syndrome (:3772-3803) and imake_output (:3805-3820).  Every value lives in the width
upstream stores it in: states, channel word and a-posteriori word are u16 (Q12 states, Q16 words), imap_bin's products i16,
the general branch's column products u32 with a u64 multiply.  Stores into u16 / i16 wrap (the all-columns-of-weight-2 branch
depends on that), divisions are C's (every operand is non-negative, so floor division is the same).  The one transcendental is
the channel transform's exp, taken from libm (math.exp) element by element.

Vectorised over frames: all frames iterate together, and a frame's outputs are frozen at the iteration its syndrome clears.
"""
import math
import os

import numpy as np

IASP_GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iasp")   # tools/make_iasp_goldens.py

ONE_SOFT = 1 << 12   # SOFT_FPP 12 (decoders.cpp:79-91)
MAX_SOFT = ONE_SOFT - 1
INPUT_LIMIT = 20.0


def _u16(x):
    return np.asarray(x, dtype=np.int64) & 0xFFFF


def _i16(x):
    return ((np.asarray(x, dtype=np.int64) + 0x8000) & 0xFFFF) - 0x8000


def _u32(x):
    return np.asarray(x, dtype=np.int64) & 0xFFFFFFFF


def channel_prior(llr):
    """What upstream leaves in soft[]: 1 / (1 + exp(clamp(x, -20, 20))), fp64, libm's exp."""
    llr = np.asarray(llr, dtype=np.float64)
    y = np.minimum(np.maximum(llr, -INPUT_LIMIT), INPUT_LIMIT)   # maxd(mind(x, 20), -20): NaN-free inputs only
    e = np.fromiter((math.exp(v) for v in y.ravel()), dtype=np.float64, count=y.size).reshape(y.shape)
    return 1.0 / (1.0 + e)


class IaspModel:
    def __init__(self, H, M):
        H = np.asarray(H, dtype=np.int64)
        self.rh, self.nh = H.shape
        self.M = M
        self.N = self.nh * M
        # edges in row-major order (upstream's state slot = position in the row, columns ascending)
        self.rows = []      # per row: list of (edge id, column, shift)
        self.cols = [[] for _ in range(self.nh)]   # per column: list of (edge id, shift), rows ascending
        e = 0
        for j in range(self.rh):
            r = []
            for k in range(self.nh):
                if H[j, k] != -1:
                    c = int(H[j, k]) % M
                    r.append((e, k, c))
                    e += 1
            self.rows.append(r)
        for j in range(self.rh):
            for (eid, k, c) in self.rows[j]:
                self.cols[k].append((eid, c))
        self.ne = e
        if min(len(r) for r in self.rows) < 2:
            raise ValueError("IASP: every block row needs at least two circulants (imap_bin reads SB[1] / SF[rw-2])")
        self.all_cw2 = all(len(c) == 2 for c in self.cols)   # decod_init :1062-1095
        self.n_idx = np.arange(M)

    # check n of an edge with shift c sees variable (n + c) mod M; variable t sees check (t - c) mod M
    def _gather_chk(self, word, k, c):
        return word[:, k * self.M + (self.n_idx + c) % self.M]

    def _syndrome_fail(self, so):
        hard = so >> 15
        fail = np.zeros(so.shape[0], dtype=bool)
        for r in self.rows:
            s = np.zeros((so.shape[0], self.M), dtype=np.int64)
            for (_, k, c) in r:
                s ^= self._gather_chk(hard, k, c)
            fail |= s.any(axis=1)
        return fail

    def _check_nodes(self, st):
        for r in self.rows:
            rw = len(r)
            P = [_i16(ONE_SOFT - 2 * st[e]) for (e, _, _) in r]
            SF = [None] * rw
            SB = [None] * rw
            SF[0] = P[0]
            for i in range(1, rw - 1):
                SF[i] = _i16((P[i] * SF[i - 1] + 2048) >> 12)
            SB[rw - 1] = P[rw - 1]
            for i in range(rw - 2, 0, -1):
                SB[i] = _i16((P[i] * SB[i + 1] + 2048) >> 12)
            out = [None] * rw
            out[0] = _u16((ONE_SOFT - SB[1] + 1) >> 1)
            for i in range(1, rw - 1):
                Z = (SF[i - 1] * SB[i + 1] + 2048) >> 12
                out[i] = _u16((ONE_SOFT - Z + 1) >> 1)
            out[rw - 1] = _u16((ONE_SOFT - SF[rw - 2] + 1) >> 1)
            for i, (e, _, _) in enumerate(r):
                st[e] = np.maximum(out[i], 1)

    def _var_general(self, st, y, so):
        M = self.M
        for k in range(self.nh):
            sl = slice(k * M, (k + 1) * M)
            yk = y[:, sl]
            P1 = _u32(yk << 16)
            P0 = _u32((65536 - yk) << 16)
            data = []
            for (e, c) in self.cols[k]:
                d = st[e][:, (self.n_idx - c) % M]
                data.append(d)
                d1 = _u16(d << 4)
                d0 = _u16((MAX_SOFT - d) << 4)          # MAX_SOFT, not ONE_SOFT (decoders.cpp:4008)
                P1 = _u32((P1 * d1) >> 16)
                P0 = _u32((P0 * d0) >> 16)
            x = P1 >> 1
            yy = (P0 >> 1) + x
            flg = yy > (ONE_SOFT << 4)
            yy = np.where(flg, yy >> 12, yy)
            x = np.where(flg, x, _u32(x << 12))
            yy = np.maximum(yy, 1)
            s = x // yy
            s = np.maximum(np.minimum(s, MAX_SOFT), 1)
            so[:, sl] = _u16(s << 4)
            sov = so[:, sl] << 8
            for (e, c), d in zip(self.cols[k], data):    # local update :4054-4100
                sos = np.maximum(d, 1)
                p1 = sov // sos
                t = np.maximum(ONE_SOFT - sos, 1)
                p0 = (ONE_SOFT * ONE_SOFT - sov) // t
                yv = (p1 + p0 + 32) >> 6
                y1 = np.maximum(yv, 1)
                dd = (p1 << 6) // y1
                nd = np.minimum(np.maximum(dd, 1), MAX_SOFT)
                st[e] = nd[:, (self.n_idx + c) % M]

    def _var_cw2(self, st, y, so):
        M = self.M
        for k in range(self.nh):
            sl = slice(k * M, (k + 1) * M)
            (e0, c0), (e1, c1) = self.cols[k]
            data0 = st[e0][:, (self.n_idx - c0) % M]
            data1 = st[e1][:, (self.n_idx - c1) % M]
            ip1 = _u16(y[:, sl])
            ip0 = _u16(65536 - ip1)
            d1 = _u16(data1 << 4)
            d0 = _u16(data0 << 4)
            t1 = _u16(65536 - d1)
            t0 = _u16(65536 - d0)
            q10 = _u16(_u32(ip1 * d1 + 32768) >> 16)
            q11 = _u16(_u32(ip1 * d0 + 32768) >> 16)
            q00 = _u16(_u32(ip0 * t1 + 32768) >> 16)
            q01 = _u16(_u32(ip0 * t0 + 32768) >> 16)
            p1 = _u16(_u32(q10 * d0 + 32768) >> 16)
            p0 = _u16(_u32(q00 * t0 + 32768) >> 16)
            p0 = np.maximum(_u16(p1 + p0), 1)
            so[:, sl] = np.maximum(_u16(_u32(p1 << 16) // p0), 1 << 4)
            q00 = np.maximum(_u16(q00 + q10), 1)
            q01 = np.maximum(_u16(q01 + q11), 1)
            n0 = np.maximum(_u16(_u32(q10 << 12) // q00), 1)
            n1 = np.maximum(_u16(_u32(q11 << 12) // q01), 1)
            st[e0] = n0[:, (self.n_idx + c0) % M]
            st[e1] = n1[:, (self.n_idx + c1) % M]

    def decode(self, llr, maxiter, decision=1):
        """llr [B, N] -> (decword [B, N] float64, iters [B] int32, prior [B, N] float64 = what upstream leaves in soft[],
        soft_out [B, N] int64 holding upstream's u16 a-posteriori word)."""
        llr = np.atleast_2d(np.asarray(llr, dtype=np.float64))
        B, N = llr.shape
        assert N == self.N
        M = self.M
        prior = channel_prior(llr)
        q = np.trunc(prior * ONE_SOFT + 0.5).astype(np.int64)     # (int)(p * 4096 + 0.5): fp64 multiply, then fp64 add
        q = np.maximum(np.minimum(q, MAX_SOFT), 1)
        st = [None] * self.ne
        for r in self.rows:
            for (e, k, c) in r:
                st[e] = self._gather_chk(q, k, c).copy()
        y = _u16(q << 4)
        so = _u16(q << 4)
        iters = np.zeros(B, dtype=np.int32)
        out_so = so.copy()
        active = self._syndrome_fail(so)
        steps = 0
        while active.any() and steps < maxiter:
            self._check_nodes(st)
            if self.all_cw2:
                self._var_cw2(st, y, so)
            else:
                self._var_general(st, y, so)
            fail = self._syndrome_fail(so)
            steps += 1
            done = active & ~fail
            iters[done] = steps
            out_so[done] = so[done]
            active &= fail
        iters[active] = -steps
        out_so[active] = so[active]
        dec = out_so / 65536.0 if decision else (out_so >> 15).astype(np.float64)
        return dec, iters, prior, out_so


def decode(H, M, llr, maxiter, decision=1):
    return IaspModel(H, M).decode(llr, maxiter, decision)
