#!/usr/bin/env python3
"""Time of the girth / ACE trace of a set of candidate codes (profiles/r28_girth_time.txt).

Appendix-C shape (16 x 32, E = 112 circulants): C relabelings of the base matrix (same protograph, fresh shifts in the information
part) at M = 64 and M = 126, gmax 20, gtarget 4, the bounds of upstream's trace_matrix (every matrix passes).  Per (M, C): the wall time
of one synchronous ldpc_hip_girth_codes call -- graph building on the host, uploads, all launches, the copy back -- as the median of
the repeats after one warm-up call, and that time per code.  The first code of every set is the base matrix itself and its result is
checked against the golden record, so a timed call is a correct one.

    python tools/time_girth.py [--out profiles/r28_girth_time.txt] [--repeats 20]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# what the numbers stand beside: the Monte-Carlo run of the same set (profiles/r09_codeset_time.txt, one simulate_codes call, min-sum,
# M = 64, 4096 frames per code) and upstream's own trace_bound_pol_mon_pm (g++ -O3) on one code
SIMULATE_MS = {1: 2.159, 16: 15.799, 256: 236.999}
REFERENCE_CPU_MS = {64: 436.0, 126: 953.0}


def relabel(base, M, rng):
    H = base.copy()
    info = H[:, H.shape[0]:]
    info[info >= 0] = rng.randint(0, M, size=int((info >= 0).sum()))
    return H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_girth_time.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    import torch

    import girth_model as gm
    import ldpc_lib_amd as L
    assert torch.cuda.is_available(), "the timing needs a GPU"
    goldens = gm.load_goldens()
    lines = [f"tools/time_girth.py: 16 x 32, E = 112, gmax 20, gtarget 4, bounds that every matrix passes, {torch.cuda.get_device_name(0)}; "
             f"wall time of one synchronous ldpc_hip_girth_codes call, median of {a.repeats} after one warm-up call",
             "M     C     one call [ms]   per code [ms]   deepest d reached in the set"]
    per_code = {}
    for M in (64, 126):
        g = goldens["appc_m%d" % M]
        base = g["codes"][0].astype(np.int64)
        rng = np.random.RandomState(28)
        for C in (1, 16, 256):
            codes = np.array([base] + [relabel(base, M, rng) for _ in range(C - 1)], dtype=np.int16)
            bounds = dict(min_ace=g["min_ace"], max_spec=g["max_spec"])
            S, SA, status = L.girth_codes(codes, M, **bounds)   # warm-up
            assert np.array_equal(S[0], g["S"][0]) and np.array_equal(SA[0], g["SA"][0]) and status[0] == g["ret"][0] and not (status & 2).any()
            t = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                L.girth_codes(codes, M, **bounds)
                t.append(time.perf_counter() - t0)
            ms = 1e3 * float(np.median(t))
            per_code[M, C] = ms / C
            lines.append(f"{M:<5d} {C:<5d} {ms:<15.3f} {ms / C:<15.4f} {int(max(np.flatnonzero(s).max() for s in S))}")
    lines += ["",
              "beside them: one simulate_codes call on a set of the same shape (profiles/r09_codeset_time.txt: min-sum, M = 64, 4096 frames per code):",
              *[f"  C = {C}: {ms} ms, {ms / C:.3f} ms per code; the trace at M = 64 takes {per_code[64, C] / (ms / C):.2f} of that per code"
                for C, ms in SIMULATE_MS.items()],
              "and upstream's trace_pm.cpp + 3d_array.cpp compiled unchanged (g++ -O3 -w), ONE run each on the CPU of a different, CPU-only machine:",
              *[f"  M = {M}: {ms:.0f} ms per code; {ms / per_code[M, 1]:.0f} x the C = 1 call here, {ms / per_code[M, 256]:.0f} x the per-code time at C = 256"
                for M, ms in REFERENCE_CPU_MS.items()]]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
