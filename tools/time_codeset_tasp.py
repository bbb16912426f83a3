#!/usr/bin/env python3
"""TDMP sum-product (decoder 7) over a code set: one launch against one context per code (profiles/r10_codeset_tasp_time.txt).

Upstream's shipped search scenario (files/input32_16.jsonx): 16 x 32, M = 126, 15 iterations, 1.7 dB; C random relabelings of the
Appendix-C base matrix (same protograph, fresh shifts), 4096 frames per code.
  route A  one LdpcHipCodes(TASP_DEC).simulate call (tasp_layered_codes_kernel);
  route B  C consecutive LdpcHip.simulate calls on pre-opened contexts, JIT mode off (tasp_global_kernel; the lone shipped matrix
           runs its ahead-of-time instance);
  route C  C = 16 only: JIT on, compile in the foreground, open + simulate + close per code -- what an unseen code costs today.
Routes A and B alternate in one session; median wall time of --repeats rounds after one warm-up round, then one profiled round for
the summed HIP-event times of the decode kernels.

    python tools/time_codeset_tasp.py [--out profiles/r10_codeset_tasp_time.txt] [--repeats 5] [--sizes 1,16,256]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

M, FRAMES, SNR, MAXITER, SEED, DEC = 126, 4096, 1.7, 15, 1, 7


def relabel(base, rng):
    """The base matrix's protograph with fresh random shifts in the information part (the dual-diagonal part keeps its shifts)."""
    H = base.copy()
    rh = H.shape[0]
    info = H[:, rh:]
    info[info >= 0] = rng.randint(0, M, size=int((info >= 0).sum()))
    return H


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return 1e3 * (time.perf_counter() - t0), r


def counters(r):
    return [r["nse"], r["nde"], r["nue"], r["frames"], r["sum_abs_iters"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_codeset_tasp_time.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="1,16,256")
    ap.add_argument("--no-jit-route", action="store_true")
    a = ap.parse_args()
    import torch

    import ldpc_lib_amd as L
    from ldpc_testlib import load_base_matrix, relift
    lib = L.load_library()
    lib.ldpc_hip_set_jit_mode(0)
    base = relift(load_base_matrix(), M).astype(np.int16)
    rng = np.random.RandomState(9)
    lines = [f"tools/time_codeset_tasp.py: 16 x 32, M = {M}, {FRAMES} frames per code, {SNR} dB, {MAXITER} iterations, decoder {DEC}, "
             f"{torch.cuda.get_device_name(0)}; routes A and B alternated, median of {a.repeats} rounds after one warm-up round",
             "A = one simulate_codes call; B = C x LdpcHip.simulate on pre-opened contexts, JIT mode 0; kernel = summed HIP-event time of the decode launches",
             "C     A wall [ms]   B wall [ms]   B / A   A kernel [ms]   B kernel [ms]   A frames/s per code   B frames/s per code   kernels of B"]
    for C in [int(v) for v in a.sizes.split(",")]:
        codes = np.array([base] + [relabel(base, rng) for _ in range(C - 1)], dtype=np.int16)
        cs = L.LdpcHipCodes(DEC, codes, M)
        singles = [L.LdpcHip(DEC, H, M) for H in codes]

        def route_a():
            return cs.simulate(SNR, MAXITER, SEED, 0, FRAMES)

        def route_b():
            return [s.simulate(SNR, MAXITER, SEED, 0, FRAMES) for s in singles]

        ta, tb = [], []
        for rnd in range(a.repeats + 1):   # round 0 warms up: workspaces, first launches
            t, cnt = wall(route_a)
            ta.append(t)
            t, res = wall(route_b)
            tb.append(t)
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
        lines.append(f"{C:<5d} {wa:<13.3f} {wb:<13.3f} {wb / wa:<7.2f} {ka:<15.3f} {kb:<15.3f} {FRAMES / wa * 1e3:<21.0f} {FRAMES / wb * 1e3:<21.0f} {', '.join(names)}")
        lines.append(f"      rounds A [ms]: {' '.join('%.2f' % t for t in ta)}; rounds B [ms]: {' '.join('%.2f' % t for t in tb)}")
        if C == 16 and not a.no_jit_route:
            # route C: the unseen codes 1 .. 15 (code 0 has an ahead-of-time instance) through hiprtc, compile in the foreground
            lib.ldpc_hip_set_jit_mode(1)

            def route_c():
                out = []
                for H in codes[1:]:
                    with L.LdpcHip(DEC, H, M) as s:
                        out.append((s.simulate(SNR, MAXITER, SEED, 0, FRAMES), s.last_launch()))
                return out

            tc, res_c = wall(route_c)
            lib.ldpc_hip_set_jit_mode(0)
            for q, (r, _) in enumerate(res_c):
                assert counters(r) == cnt[q + 1].tolist(), (q, r)
            lines.append(f"      route C, JIT on, 15 unseen codes, open + simulate + close each (one pass, no warm-up): {tc:.1f} ms = {tc / 15:.1f} ms per code "
                         f"({sorted({n for _, n in res_c})[0]}); route A per code at C = 16: {wa / 16:.3f} ms")
        cs.close()
        for s in singles:
            s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
