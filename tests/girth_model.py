"""numpy restatement of upstream's girth / ACE trace, trace_bound_pol_mon_pm (trace_pm.cpp:58-299, NATURAL_POLYNOM build), and of the
caller's reduction (main_simulation.cpp:177-201).  Written from the upstream source as its own statement of the computation -- dense
[E, E, M] arrays, int64 so that an overflow of upstream's 32-bit sums shows as `peak` instead of wrapping -- and checked against the
compiled reference's recorded results (tests/golden/girth/, tools/make_girth_goldens.py).  Test infrastructure only."""
import glob
import json
import os

import numpy as np

GIRTH_GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "girth")
GMAX, GTARGET = 20, 4        # trace_pm.h:8-9
_BIG = 1 << 40


def graph(hd, M):
    """(E, pred_begin [E + 1], pred [n, 3]): edges are the non-empty circulants column by column, rows ascending (tanner_mon :331-345);
    the predecessors (j, a, as) of J are the rows j of column J of Apm (hp2a_mon_pm :391-465), j ascending."""
    hd = np.asarray(hd, dtype=np.int64)
    rh, nh = hd.shape
    edges = [(j, k) for k in range(nh) for j in range(rh) if hd[j, k] >= 0]
    cw = (hd >= 0).sum(axis=0)
    begin, pred = [0], []
    for (j2, k2) in edges:
        for j, (j1, k1) in enumerate(edges):
            if j1 != j2 and k1 != k2 and hd[j1, k2] >= 0:
                pred.append((j, ((M - hd[j1, k2]) % M + hd[j2, k2]) % M, 2 * cw[k2]))
        begin.append(len(pred))
    return len(edges), np.array(begin, dtype=np.int32), np.array(pred, dtype=np.int32).reshape(-1, 3)


def trace(hd, M, gmax=GMAX, gtarget=GTARGET, min_ace=None, max_spec=None):
    """(S [gmax], SA [gmax], return value, peak): what trace_bound_pol_mon_pm leaves in S and SA and returns; peak is the largest
    coefficient or spectrum sum met on the way (upstream's int holds it while peak < 2^31)."""
    E, begin, pred = graph(hd, M)
    S = np.zeros(gmax, dtype=np.int64)
    SA = np.zeros(gmax, dtype=np.int64)
    B = np.zeros((E, E, M), dtype=np.int64)
    A = np.zeros((E, E, M), dtype=np.int64)
    for J in range(E):
        for j, a, s in pred[begin[J]:begin[J + 1]]:
            B[j, J, a] = 1                                       # :117-129
            A[j, J, a] = s
    h = np.arange(M)
    cnt, ok, peak = 0, 1, 1
    for d in range(3, gmax, 2):
        Y = np.zeros_like(B)
        AY = np.zeros_like(A)
        for J in range(E):                                       # mul_mat_mat_mon :688-733
            p = pred[begin[J]:begin[J + 1]]
            if len(p) == 0:
                continue
            idx = (h[None, :] - p[:, 1:2]) % M                   # [P, M]: the operand of coefficient h is coefficient h - a
            rows = np.arange(len(p))[:, None]
            tb = B[:, p[:, 0], :][:, rows, idx]                  # [E, P, M]
            ta = np.where(tb != 0, A[:, p[:, 0], :][:, rows, idx] + p[:, 2][None, :, None], _BIG)
            Y[:, J, :] = tb.sum(axis=1)
            m = ta.min(axis=1)
            AY[:, J, :] = np.where(m == _BIG, 0, m)
        B, A = Y, AY
        peak = max(peak, int(B.max()) if E else 0)
        for I in range(E):                                       # :183-213
            if B[I, I, 0] == 0:
                continue
            S[d] += B[I, I, 0]
            SA[d] = min(SA[d], A[I, I, 0]) if SA[d] > 0 else A[I, I, 0]
            at = np.flatnonzero(B[I, I])                         # the list before removal; at[0] == 0
            before = A[I, I, at].copy()
            B[I, I, 0] = 0
            A[I, I, :] = 0
            A[I, I, at[1:]] = before[:-1]                        # the k-th remaining term takes the ace of the (k - 1)-th term before
        peak = max(peak, int(S[d]))
        ok = 1
        if S[d] > 0:                                             # :250-272
            ok = 0
            if max_spec is not None and S[d] // (d + 1) <= max_spec[cnt]:
                ok = 1
            if min_ace is not None and SA[d] // 2 >= min_ace[cnt]:
                ok = 1
            if not ok:
                break
            cnt += 1
            if cnt == gtarget:
                break
    for i in range(3, gmax, 2):                                  # :276-280
        S[i] //= i + 1
        SA[i] //= 2
    return S.astype(np.int32), SA.astype(np.int32), ok, peak


def trace_matrix(S, SA):
    """main_simulation.cpp:177-201: (girth, ACE [4], girth_spectrum [4]); girth 21 when S is all zero."""
    S, SA = list(S), list(SA)
    girth = next((i + 1 for i in range(len(S)) if S[i]), GMAX + 1)
    ace = [int(v) for v in SA[girth - 1:] if v][:GTARGET]
    spec = [int(v) for v in S[girth - 1:] if v][:GTARGET]
    return girth, ace + [0] * (GTARGET - len(ace)), spec + [0] * (GTARGET - len(spec))


def load_goldens():
    """{name: dict(codes int16 [C, rh, nh], M, gmax, gtarget, min_ace, max_spec, S [C, gmax], SA [C, gmax], ret [C])}"""
    out = {}
    for path in sorted(glob.glob(os.path.join(GIRTH_GOLDEN_DIR, "*.json"))):
        with open(path) as f:
            g = json.load(f)
        g["codes"] = np.array(g["codes"], dtype=np.int16)
        g["S"] = np.array(g["S"], dtype=np.int32)
        g["SA"] = np.array(g["SA"], dtype=np.int32)
        g["ret"] = np.array(g["ret"], dtype=np.int32)
        out[os.path.splitext(os.path.basename(path))[0]] = g
    return out
