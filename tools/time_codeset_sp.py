#!/usr/bin/env python3
"""Flooding sum-product (decoders 1 and 2) over a code set: one launch against one context per code
(profiles/r17_codeset_sp_time.txt).

Three shapes, 4096 frames per code, C random relabelings (same pattern, fresh shifts), both decoders:
  16 x 32, M = 64, 50 iterations, 2.0 dB   the Appendix-C base matrix;
  16 x 32, M = 126, 15 iterations, 1.7 dB  the shape of upstream's files/input32_16.jsonx;
  30 x 60, M = 67, 50 iterations, 2.0 dB   the matrix of tests/golden/lche/lche_30x60_m67_2p0.npz (files/input12L.jsonx's shape).
  route A  one LdpcHipCodes(DEC_SP | DEC_ASP).simulate call (sp_flood_codes_kernel / asp_flood_codes_kernel);
  route B  C consecutive LdpcHip.simulate calls on pre-opened contexts, JIT mode off: the path users have today.  The kernel it runs
           is written down per line.
Routes A and B alternate in one session; median wall time of --repeats rounds after one warm-up round, then one profiled round for
the summed HIP-event times of the decode kernels.  Every result line is appended to --out as soon as it is measured.

    python tools/time_codeset_sp.py [--out profiles/r17_codeset_sp_time.txt] [--repeats 5] [--sizes 1,16,256] [--decoders 1,2] [--shapes 0,1,2] [--append]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES, SEED = 4096, 1
NAMES = {1: "SP_DEC (1)", 2: "ASP_DEC (2)"}


def shapes():
    from ldpc_testlib import load_base_matrix, relift
    base = load_base_matrix()
    a = np.where(base >= 0, relift(base, 64) % 64, -1).astype(np.int16)
    b = np.where(base >= 0, relift(base, 126) % 126, -1).astype(np.int16)
    g = np.load(os.path.join(ROOT, "tests", "golden", "lche", "lche_30x60_m67_2p0.npz"))
    assert int(g["M"]) == 67 and g["H"].shape == (30, 60)
    c = np.where(g["H"] >= 0, g["H"] % 67, -1).astype(np.int16)
    return [("16 x 32, M = 64, 50 iterations, 2.0 dB", a, 64, 50, 2.0), ("16 x 32, M = 126, 15 iterations, 1.7 dB", b, 126, 15, 1.7),
            ("30 x 60, M = 67, 50 iterations, 2.0 dB", c, 67, 50, 2.0)]


def relabel(base, M, rng):
    """The base matrix's pattern with fresh random shifts."""
    return np.where(base >= 0, rng.randint(0, M, size=base.shape), -1).astype(np.int16)


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return 1e3 * (time.perf_counter() - t0), r


def counters(r):
    return [r["nse"], r["nde"], r["nue"], r["frames"], r["sum_abs_iters"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_codeset_sp_time.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="1,16,256")
    ap.add_argument("--decoders", default="1,2")
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--append", action="store_true", help="add to --out instead of starting it again")
    a = ap.parse_args()
    import torch

    import ldpc_lib_amd as L
    lib = L.load_library()
    lib.ldpc_hip_set_jit_mode(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if not a.append:
        open(a.out, "w").close()

    def emit(line):
        """Every result line goes to the file as soon as it exists: an interrupted run keeps what it has measured."""
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    if not a.append:
        emit(f"tools/time_codeset_sp.py: {FRAMES} frames per code, {torch.cuda.get_device_name(0)}; routes A and B alternated, median wall time of "
             f"{a.repeats} rounds after one warm-up round")
        emit("A = one simulate_codes call; B = C x LdpcHip.simulate on pre-opened contexts, JIT mode 0; kernel = summed HIP-event time of the decode launches")
    all_shapes = shapes()
    for dec in [int(v) for v in a.decoders.split(",")]:
        for n_shape in [int(v) for v in a.shapes.split(",")]:
            title, base, M, maxiter, snr = all_shapes[n_shape]
            rng = np.random.RandomState(9)
            emit(f"{NAMES[dec]}: {title}")
            emit("C     A wall [ms]   B wall [ms]   B / A   A kernel [ms]   B kernel [ms]   A frames/s per code   B frames/s per code   kernels of A; of B")
            for C in [int(v) for v in a.sizes.split(",")]:
                codes = np.array([relabel(base, M, rng) for _ in range(C)], dtype=np.int16)
                cs = L.LdpcHipCodes(dec, codes, M)
                singles = [L.LdpcHip(dec, H, M) for H in codes]

                def route_a():
                    return cs.simulate(snr, maxiter, SEED, 0, FRAMES)

                def route_b():
                    return [s.simulate(snr, maxiter, SEED, 0, FRAMES) for s in singles]

                ta, tb = [], []
                for rnd in range(a.repeats + 1):   # round 0 warms up: workspaces, first launches
                    t, cnt = wall(route_a)
                    ta.append(t)
                    t, res = wall(route_b)
                    tb.append(t)
                    print(f"C = {C}, round {rnd}: A {ta[-1]:.1f} ms, B {tb[-1]:.1f} ms", flush=True)
                for q, r in enumerate(res):   # the two routes count the same errors
                    assert counters(r) == cnt[q].tolist(), (q, r, cnt[q])
                cs.profile(True)
                route_a()
                ka, _ = cs.profile_read()
                for s in singles:
                    s.profile(True)
                route_b()
                kb = sum(s.profile_read()[0] for s in singles)
                names = sorted({s.last_launch() for s in singles})
                wa, wb = float(np.median(ta[1:])), float(np.median(tb[1:]))
                emit(f"{C:<5d} {wa:<13.3f} {wb:<13.3f} {wb / wa:<7.2f} {ka:<15.3f} {kb:<15.3f} {FRAMES / wa * 1e3:<21.0f} {FRAMES / wb * 1e3:<21.0f} "
                     f"{cs.kernel_name}; {', '.join(names)}")
                emit(f"      rounds A [ms]: {' '.join('%.2f' % t for t in ta)}; rounds B [ms]: {' '.join('%.2f' % t for t in tb)}")
                emit(f"      mean iterations per frame: {cnt[:, 4].sum() / cnt[:, 3].sum():.2f}; frame errors: {int(cnt[:, 1].sum())} of {int(cnt[:, 3].sum())}")
                cs.close()
                for s in singles:
                    s.close()


if __name__ == "__main__":
    main()
