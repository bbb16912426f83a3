#!/usr/bin/env python3
"""One launch over C candidate codes against C single-code simulations (profiles/r09_codeset_time.txt).

Appendix-C shape (16 x 32, M = 64): C random relabelings of the base matrix (same protograph, fresh shifts), 4096 frames per code,
2.0 dB, 50 iterations, JIT mode off so that the single-code route is on its table tier too.  Per C: wall time of one
LdpcHipCodes.simulate call, wall time of C consecutive LdpcHip.simulate calls on pre-opened contexts, their ratio, and the decode
kernel times of both routes from HIP events.

    python tools/time_codeset.py [--out profiles/r09_codeset_time.txt] [--repeats 5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

M, FRAMES, SNR, MAXITER, SEED = 64, 4096, 2.0, 50, 1


def relabel(base, rng):
    """The base matrix's protograph with fresh random shifts in the information part (the dual-diagonal part keeps its shifts)."""
    H = base.copy()
    rh = H.shape[0]
    info = H[:, rh:]
    info[info >= 0] = rng.randint(0, M, size=int((info >= 0).sum()))
    return H


def median_wall(fn, repeats):
    fn()   # warm-up: workspaces, first launch
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_codeset_time.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--decoder", type=int, default=3)
    a = ap.parse_args()
    import torch

    import ldpc_lib_amd as L
    from ldpc_testlib import load_base_matrix, relift
    L.load_library().ldpc_hip_set_jit_mode(0)
    base = relift(load_base_matrix(), M).astype(np.int16)
    rng = np.random.RandomState(9)
    lines = [f"tools/time_codeset.py: 16 x 32, M = {M}, {FRAMES} frames per code, {SNR} dB, {MAXITER} iterations, decoder {a.decoder}, JIT mode 0, "
             f"{torch.cuda.get_device_name(0)}; median of {a.repeats} after one warm-up",
             "C     one simulate_codes call [ms]   C x LdpcHip.simulate [ms]   ratio   decode kernel, set [ms]   decode kernels, single [ms]   single-code kernel"]
    for C in (1, 16, 256):
        codes = np.array([base] + [relabel(base, rng) for _ in range(C - 1)], dtype=np.int16)
        with L.LdpcHipCodes(a.decoder, codes, M) as cs:
            t_set = median_wall(lambda: cs.simulate(SNR, MAXITER, SEED, 0, FRAMES), a.repeats)
            cs.profile(True)
            cnt = cs.simulate(SNR, MAXITER, SEED, 0, FRAMES)
            k_set, _ = cs.profile_read()
        singles = [L.LdpcHip(a.decoder, H, M) for H in codes]

        def run_singles():
            return [s.simulate(SNR, MAXITER, SEED, 0, FRAMES) for s in singles]

        t_one = median_wall(run_singles, a.repeats)
        for s in singles:
            s.profile(True)
        res = run_singles()
        k_one = sum(s.profile_read()[0] for s in singles)
        names = sorted({s.last_launch() for s in singles})
        for q, r in enumerate(res):   # the two routes count the same errors
            assert [r["nse"], r["nde"], r["nue"], r["frames"], r["sum_abs_iters"]] == cnt[q].tolist(), (q, r, cnt[q])
        for s in singles:
            s.close()
        lines.append(f"{C:<5d} {t_set:<30.3f} {t_one:<27.3f} {t_one / t_set:<7.2f} {k_set:<24.3f} {k_one:<29.3f} {', '.join(names)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
