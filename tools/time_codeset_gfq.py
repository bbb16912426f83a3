#!/usr/bin/env python3
"""FHT_DEC (decoder 6) over a GF(q) code set: one launch against one context per code (profiles/r12_codeset_gfq_time.txt).

Upstream's shipped non-binary result (files/resultq_codes.jsonx): GF(16), 4 x 8, M = 8, 15 iterations; 2.7 dB; C relabelings of the
shipped code (same pattern, fresh shifts and coefficients), the all-zero word sent.
  route A  one LdpcHipCodesGfq.simulate call (gfq_codes_kernel: one channel draw, one decode launch and one count launch per piece);
  route B  C consecutive LdpcHipGfq.simulate(random_messages=False) calls on pre-opened contexts (gfq_kernel: channel, decode and
           count per code, and a synchronisation per call).
Routes A and B alternate in one session; median wall time of --repeats rounds after one warm-up round, then one profiled round for
the summed HIP-event times of the decode kernels.

    python tools/time_codeset_gfq.py [--out profiles/r12_codeset_gfq_time.txt] [--repeats 5] [--sizes 1,16,256] [--frames 512,4096]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

Q_BITS, M, SNR, MAXITER, SEED = 4, 8, 2.7, 15, 1


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return 1e3 * (time.perf_counter() - t0), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_codeset_gfq_time.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="1,16,256")
    ap.add_argument("--frames", default="512,4096")
    a = ap.parse_args()
    import torch

    import ldpc_lib_amd as L
    from codeset_gfq_sets import shipped_set
    lines = [f"tools/time_codeset_gfq.py: GF({1 << Q_BITS}), 4 x 8, M = {M}, {SNR} dB, {MAXITER} iterations, decoder 6, {torch.cuda.get_device_name(0)}; "
             f"routes A and B alternated, median of {a.repeats} rounds after one warm-up round",
             "A = one simulate_codes_gfq call; B = C x LdpcHipGfq.simulate(random_messages=False) on pre-opened contexts; kernel = summed HIP-event time "
             "of the decode launches; frames/s = C x frames / time",
             "C     frames  A wall [ms]   B wall [ms]   B / A   A kernel [ms]   B kernel [ms]   A frames/s (wall)   B frames/s (wall)   A frames/s (kernel)   B frames/s (kernel)"]
    verdict = None
    for C in [int(v) for v in a.sizes.split(",")]:
        hb, hc = shipped_set(M, 1 << Q_BITS, ncodes=C)
        cs = L.LdpcHipCodesGfq(Q_BITS, hb, hc, M)
        singles = [L.LdpcHipGfq(Q_BITS, hb[c], hc[c], M) for c in range(C)]
        for frames in [int(v) for v in a.frames.split(",")]:
            def route_a():
                return cs.simulate(SNR, MAXITER, SEED, 0, frames)

            def route_b():
                return [s.simulate(SNR, MAXITER, frames, SEED, first_frame=0, random_messages=False) for s in singles]

            ta, tb = [], []
            for rnd in range(a.repeats + 1):   # round 0 warms up: workspaces, first launches
                t, cnt = wall(route_a)
                ta.append(t)
                t, res = wall(route_b)
                tb.append(t)
            for q, r in enumerate(res):   # the two routes count the same errors
                assert r == cnt[q].tolist(), (q, r, cnt[q])
            cs.profile(True)
            route_a()
            ka, _ = cs.profile_read()
            cs.profile(False)
            for s in singles:
                s.profile(True)
            route_b()
            kb = sum(s.profile_read()[0] for s in singles)
            for s in singles:
                s.profile(False)
            wa, wb = float(np.median(ta[1:])), float(np.median(tb[1:]))
            total = C * frames
            lines.append(f"{C:<5d} {frames:<7d} {wa:<13.3f} {wb:<13.3f} {wb / wa:<7.2f} {ka:<15.3f} {kb:<15.3f} {total / wa * 1e3:<19.0f} {total / wb * 1e3:<19.0f} "
                         f"{total / ka * 1e3:<21.0f} {total / kb * 1e3:<21.0f}")
            lines.append(f"      rounds A [ms]: {' '.join('%.2f' % t for t in ta)}; rounds B [ms]: {' '.join('%.2f' % t for t in tb)}")
            if C == 256 and frames == 512:
                verdict = (wa, wb)
        cs.close()
        for s in singles:
            s.close()
    if verdict:
        lines.append(f"acceptance (C = 256, 512 frames per code): route A {verdict[0]:.3f} ms, route B {verdict[1]:.3f} ms: A is "
                     f"{'not slower' if verdict[0] <= verdict[1] else 'SLOWER'} than B")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if verdict and verdict[0] > verdict[1]:
        sys.exit(1)


if __name__ == "__main__":
    main()
