#!/usr/bin/env python3
"""The global-memory tier of a code set (ldpc_hip_open_codes_global) against one single-code context per candidate
(profiles/r29_codeset_global_time.txt).

Shapes: relabelings of the 16 x 32 Appendix-C matrix (the same pattern, fresh shifts), 4096 frames per code --
  tdmp256, tdmp512   TDMP sum-product, 15 iterations, M = 256 and M = 512
  ims256, ims512     integer min-sum, 50 iterations, M = 256 and M = 512
  ms1024             min-sum, 50 iterations, M = 1024
  ms256, lms256, sp256, asp256, iasp256, lche256   the other decoders of the tier at M = 256, on request (--shapes): min-sum and
                     layered min-sum 50 iterations at 2.0 dB, the sum-product family and LCHE 15 iterations at 1.7 dB
  route A  one LdpcHipCodes(dec, codes, M, tier="global").simulate call: the channel once, the set kernel over all codes, the count;
  route B  what a caller does without a set: C consecutive LdpcHip(dec).simulate calls on pre-opened contexts, JIT mode off.  The
           contexts are opened 32 at a time outside the timed region (each holds a workspace) and the times of the groups are added.
           TDMP and M = 1024 run the single-code shape-unlimited tier.  Integer min-sum at M <= 512 has a table-driven kernel
           (ims_flood_kernel), which is what such a caller gets; --force-global-b opens route B with LDPC_HIP_FORCE_GLOBAL=1 instead, so
           that ims_global_kernel runs.  Every line names the kernels of both routes.
Every line records the FER and the mean iteration count it measured.  Routes A and B alternate in one session; median wall time of
--repeats rounds after one warm-up round (the line lists every round).  Every result line is appended to --out as soon as it exists.

    python tools/time_codeset_global.py [--out profiles/r29_codeset_global_time.txt] [--repeats 5] [--sizes 1,16,256]
                                        [--shapes tdmp256,tdmp512,ims256,ims512,ms1024] [--force-global-b] [--append]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES, SEED, GROUP = 4096, 1, 32
# shape -> (decoder id, name, M, iterations, SNR in dB)
SHAPES = {"tdmp256": (7, "TDMP", 256, 15, 1.7), "tdmp512": (7, "TDMP", 512, 15, 1.7), "ims256": (4, "IMS", 256, 50, 2.0),
          "ims512": (4, "IMS", 512, 50, 2.0), "ms1024": (3, "MS", 1024, 50, 2.0),
          # the other decoders of the tier at M = 256 (profiles/global_frame_refactor_time.txt); not part of the default run
          "ms256": (3, "MS", 256, 50, 2.0), "lms256": (8, "LMS", 256, 50, 2.0), "sp256": (1, "SP", 256, 15, 1.7),
          "asp256": (2, "ASP", 256, 15, 1.7), "iasp256": (5, "IASP", 256, 15, 1.7), "lche256": (9, "LCHE", 256, 15, 1.7)}
DEFAULT_SHAPES = "tdmp256,tdmp512,ims256,ims512,ms1024"


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_codeset_global_time.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="1,16,256")
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--force-global-b", action="store_true", help="route B opens with LDPC_HIP_FORCE_GLOBAL=1: the single-code global tier on every shape")
    ap.add_argument("--append", action="store_true", help="keep what --out already holds")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if not a.append:
        open(a.out, "w").close()

    def emit(line):
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    import torch

    import ldpc_lib_amd as L
    from ldpc_testlib import load_base_matrix, relift
    lib = L.load_library()
    lib.ldpc_hip_set_jit_mode(0)
    if not a.append:
        emit(f"tools/time_codeset_global.py: {FRAMES} frames per code, alpha 0.8, {torch.cuda.get_device_name(0)}; routes A and B alternated, "
             "median wall time of the rounds after one warm-up round")
        emit("A = one simulate_codes call on the global-memory tier of a set (ldpc_hip_open_codes_global); B = C x LdpcHip.simulate on contexts "
             f"opened {GROUP} at a time outside the timed region, JIT mode 0; B / A > 1: the set is faster")
    for shape in a.shapes.split(","):
        dec, name, M, maxiter, snr = SHAPES[shape]
        base0 = load_base_matrix()
        base = np.where(base0 >= 0, relift(base0, M) % M, -1).astype(np.int16)
        rng = np.random.RandomState(9)
        emit(f"shape {shape}, {name} (decoder {dec}): {base.shape[0]} x {base.shape[1]}, M = {M}, {int((base >= 0).sum())} circulants, {maxiter} iterations, "
             f"{snr} dB, {a.repeats} rounds" + (", route B with LDPC_HIP_FORCE_GLOBAL=1" if a.force_global_b else ""))
        emit("C     A wall [ms]   B wall [ms]   B / A   A frames/s per code   B frames/s per code   mean |iterations|   FER      kernel of A; kernels of B")
        for C in [int(v) for v in a.sizes.split(",")]:
            codes = np.array([base] + [relabel(base, M, rng) for _ in range(C - 1)], dtype=np.int16)
            cs = L.LdpcHipCodes(dec, codes, M, tier="global")
            ta, tb, names, cnt, res = [], [], set(), None, None

            def open_group(g):
                """Route B's contexts for codes [g, g + GROUP), each after a 1024-frame call of its own: the workspace of the single-code
                tier is allocated by the first launch that needs it, outside the timed region."""
                if a.force_global_b:
                    os.environ["LDPC_HIP_FORCE_GLOBAL"] = "1"
                singles = [L.LdpcHip(dec, H, M) for H in codes[g:g + GROUP]]
                os.environ.pop("LDPC_HIP_FORCE_GLOBAL", None)
                for s in singles:
                    s.simulate(snr, maxiter, SEED, 0, 1024)
                return singles

            kept = open_group(0) if C <= GROUP else None   # one group: it stays open over the rounds
            for rnd in range(a.repeats + 1):   # round 0 warms up: workspaces, first launches
                t, cnt = wall(lambda: cs.simulate(snr, maxiter, SEED, 0, FRAMES))
                ta.append(t)
                t, res = 0.0, []
                for g in range(0, C, GROUP):   # opening and closing are not timed
                    singles = kept or open_group(g)
                    dt, r = wall(lambda: [s.simulate(snr, maxiter, SEED, 0, FRAMES) for s in singles])
                    t += dt
                    res += r
                    names |= {s.lib.ldpc_hip_last_launch(s.h).decode() for s in singles}
                    if not kept:
                        for s in singles:
                            s.close()
                tb.append(t)
                print(f"{shape}, C = {C}, round {rnd}: A {ta[-1]:.1f} ms, B {tb[-1]:.1f} ms", flush=True)
            for q, r in enumerate(res):            # the two routes count the same errors
                assert counters(r) == cnt[q].tolist(), (q, r, cnt[q])
            wa, wb = float(np.median(ta[1:])), float(np.median(tb[1:]))
            its = float(cnt[:, 4].sum()) / float(cnt[:, 3].sum())
            fer = float(cnt[:, 1].sum()) / float(cnt[:, 3].sum())
            emit(f"{C:<5d} {wa:<13.3f} {wb:<13.3f} {wb / wa:<7.2f} {FRAMES / wa * 1e3:<21.0f} {FRAMES / wb * 1e3:<21.0f} {its:<19.2f} {fer:<8.4f} "
                 f"{cs.kernel_name}; {', '.join(sorted(names))}")
            emit(f"      rounds A [ms]: {' '.join('%.2f' % t for t in ta)}; rounds B [ms]: {' '.join('%.2f' % t for t in tb)}")
            cs.close()
            for s in kept or []:
                s.close()


if __name__ == "__main__":
    main()
