"""Inputs of the GF(q) code-set tests (test_codeset_gfq_cpu.py, test_gpu_codeset_gfq.py): candidate sets built the way upstream's ggp
search builds them -- one pattern, other shifts and coefficients per candidate --, a set that mixes the two kinds of symbol node, the
weak code of the stopping-rule test, and the record of ldpc_hip_codes_gfq_table_host restated in numpy.  Constants and seeded draws
only: nothing is searched at test time."""
import os
import sys

import numpy as np

from ldpc_testlib import ROOT, random_qc_code

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_gfq_goldens  # noqa: E402

NCODES = 5
MAXITER = 15


def relabel(hb, hc, M, q, rng):
    """The same pattern with fresh shifts in [0, M) and fresh coefficients in [1, q): what differs between two ggp candidates."""
    there = hb >= 0
    nb = np.where(there, rng.randint(0, M, hb.shape), -1).astype(np.int16)
    nc = np.where(there, rng.randint(1, q, hb.shape), -1).astype(np.int16)
    return nb, nc


def candidates(first, M, q, seed, ncodes=NCODES):
    """[first, relabelled, relabelled, ...] as (hb [C, rh, nh], hc [C, rh, nh])."""
    rng = np.random.RandomState(seed)
    pairs = [first] + [relabel(first[0], first[1], M, q, rng) for _ in range(ncodes - 1)]
    return np.array([p[0] for p in pairs], dtype=np.int16), np.array([p[1] for p in pairs], dtype=np.int16)


def shipped_set(M, q, seed=40, ncodes=NCODES):
    return candidates(make_gfq_goldens.shipped(M, q), M, q, seed, ncodes)


def mixed_set(M, q, seed=41, ncodes=NCODES):
    return candidates(make_gfq_goldens.mixed(M, q, seed=11), M, q, seed, ncodes)


def mixed_4x8(M, q, seed=7):
    """A 4 x 8 code -- the shape of the shipped one -- with block columns of weight 2, 3 and 4: not the cw2 form of the symbol node."""
    rng = np.random.RandomState(seed)
    hb = np.asarray(random_qc_code(rng, 4, 8, M, [3, 4, 2, 3]), dtype=np.int16)
    hc = np.where(hb >= 0, rng.randint(1, q, hb.shape), -1).astype(np.int16)
    assert {int((hb[:, k] >= 0).sum()) for k in range(8)} >= {2, 3}
    return hb, hc


def cw2_mixture_set(M=33, q=16, seed=42):
    """Shipped-pattern codes (every block column of weight 2, cw2 = 1) and mixed-pattern codes (cw2 = 0) of the same 4 x 8 shape in
    turn, so that cw2 and E change at every code boundary."""
    rng = np.random.RandomState(seed)
    a, b = make_gfq_goldens.shipped(M, q), mixed_4x8(M, q)
    pairs = [a, b, relabel(a[0], a[1], M, q, rng), relabel(b[0], b[1], M, q, rng), relabel(a[0], a[1], M, q, rng)]
    return np.array([p[0] for p in pairs], dtype=np.int16), np.array([p[1] for p in pairs], dtype=np.int16)


def weak_first_set(M=8, q=16, seed=43, ncodes=4):
    """The stopping-rule set: code 0 has all shifts 0 and all coefficients 1 on the shipped pattern (M copies of one tiny graph full of
    short cycles), the others are candidates of the shipped pattern."""
    hb, hc = shipped_set(M, q, seed, ncodes)
    hb[0] = np.where(hb[0] >= 0, 0, -1)
    hc[0] = np.where(hb[0] >= 0, 1, -1)
    return hb, hc


def record(hb, hc, M):
    """The record of one code as ldpc_hip_codes_gfq_table_host lays it out."""
    rh, nh = hb.shape
    rows, cols = np.nonzero(hb >= 0)                     # row-major: rows ascending, columns ascending inside a row
    E = len(rows)
    row_start = np.concatenate([[0], np.cumsum((hb >= 0).sum(axis=1))])
    col_start = np.concatenate([[0], np.cumsum((hb >= 0).sum(axis=0))])
    ce_edge = np.concatenate([np.flatnonzero(cols == k) for k in range(nh)])
    cw2 = int(((hb >= 0).sum(axis=0) == 2).all())
    return np.concatenate([[E, cw2], row_start, col_start, cols, hb[rows, cols] % M, hc[rows, cols] - 1, ce_edge]).astype(np.int32)
