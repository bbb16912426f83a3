#!/usr/bin/env python3
"""Integer advanced sum-product (decoder 5) over a code set: one launch against one context per code
(profiles/r14_codeset_iasp_time.txt).

Upstream's third search input (files/input12L.jsonx): 30 x 60 base matrices at M = 67, 50 iterations, 1.0 dB; C random relabelings
of the golden 30 x 60 matrix (tests/golden/iasp/iasp_30x60_m67_2p0.npz: same pattern, fresh shifts), 4096 frames per code.
  route A  one LdpcHipCodes(IASP_DEC).simulate call (iasp_codes_kernel<multiwave>);
  route B  C consecutive LdpcHip.simulate calls on pre-opened contexts, JIT mode off (iasp_global_kernel);
  route C  after the last size: JIT on, compile in the foreground, open + simulate + close per code for --jit-codes unseen codes
           (15 by default) -- what an unseen code costs today.
Routes A and B alternate in one session; median wall time of --repeats rounds after one warm-up round, then one profiled round for
the summed HIP-event times of the decode kernels.  Every result line is appended to --out as soon as it is measured.

    python tools/time_codeset_iasp.py [--out profiles/r14_codeset_iasp_time.txt] [--repeats 5] [--sizes 1,16,256]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

M, FRAMES, SNR, MAXITER, SEED, DEC = 67, 4096, 1.0, 50, 1, 5


def relabel(base, rng):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_codeset_iasp_time.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="1,16,256")
    ap.add_argument("--no-jit-route", action="store_true")
    ap.add_argument("--jit-codes", type=int, default=15, help="unseen codes of route C")
    a = ap.parse_args()
    import torch

    import ldpc_lib_amd as L
    lib = L.load_library()
    lib.ldpc_hip_set_jit_mode(0)
    g = np.load(os.path.join(ROOT, "tests", "golden", "iasp", "iasp_30x60_m67_2p0.npz"))
    assert int(g["M"]) == M and g["H"].shape == (30, 60)
    base = np.where(g["H"] >= 0, g["H"] % M, -1).astype(np.int16)
    rng = np.random.RandomState(9)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()

    def emit(line):
        """Every result line goes to the file as soon as it exists: an interrupted run keeps what it has measured."""
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    emit(f"tools/time_codeset_iasp.py: 30 x 60, M = {M}, {FRAMES} frames per code, {SNR} dB, {MAXITER} iterations, decoder {DEC}, "
         f"{torch.cuda.get_device_name(0)}; routes A and B alternated, median of {a.repeats} rounds after one warm-up round")
    emit("A = one simulate_codes call; B = C x LdpcHip.simulate on pre-opened contexts, JIT mode 0; kernel = summed HIP-event time of the decode launches")
    emit("C     A wall [ms]   B wall [ms]   B / A   A kernel [ms]   B kernel [ms]   A frames/s per code   B frames/s per code   kernels of B")
    per_code_a = {}
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
        per_code_a[C] = wa / C
        emit(f"{C:<5d} {wa:<13.3f} {wb:<13.3f} {wb / wa:<7.2f} {ka:<15.3f} {kb:<15.3f} {FRAMES / wa * 1e3:<21.0f} {FRAMES / wb * 1e3:<21.0f} {', '.join(names)}")
        emit(f"      rounds A [ms]: {' '.join('%.2f' % t for t in ta)}; rounds B [ms]: {' '.join('%.2f' % t for t in tb)}")
        cs.close()
        for s in singles:
            s.close()
    if not a.no_jit_route and a.jit_codes > 0:
        # route C, after the last size: --jit-codes unseen codes through hiprtc, compile in the foreground, one line per code (a
        # 30 x 60 instance takes hiprtc a long time); their counters against one set of the same codes
        unseen = np.array([relabel(base, rng) for _ in range(a.jit_codes)], dtype=np.int16)
        lib.ldpc_hip_set_jit_mode(1)
        tc, res_c = [], []
        for q, H in enumerate(unseen):
            def open_simulate_close():
                with L.LdpcHip(DEC, H, M) as s:
                    return s.simulate(SNR, MAXITER, SEED, 0, FRAMES), s.last_launch()
            t, r = wall(open_simulate_close)
            tc.append(t)
            res_c.append(r)
            emit(f"      route C, JIT on, unseen code {q + 1} of {a.jit_codes}, open + simulate + close: {t:.1f} ms ({r[1]})")
        lib.ldpc_hip_set_jit_mode(0)
        with L.LdpcHipCodes(DEC, unseen, M) as cs:
            cnt = cs.simulate(SNR, MAXITER, SEED, 0, FRAMES)
        for q, (r, _) in enumerate(res_c):
            assert counters(r) == cnt[q].tolist(), (q, r)
        ref = 16 if 16 in per_code_a else (max(per_code_a) if per_code_a else None)
        emit(f"      route C: {sum(tc) / len(tc):.1f} ms per unseen code (one pass, no warm-up)" +
             (f"; route A per code at C = {ref}: {per_code_a[ref]:.3f} ms" if ref else ""))


if __name__ == "__main__":
    main()
