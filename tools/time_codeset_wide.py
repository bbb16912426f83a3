#!/usr/bin/env python3
"""Min-sum, TDMP and layered min-sum (decoders 3, 7, 8) over a wide code set (ldpc_hip_open_codes_wide): one launch against what the
library offered for the shape before (profiles/r22_codeset_wide_time.txt).

Two workloads, 4096 frames per code; MS and LMS 50 iterations, TDMP 15 iterations at 1.7 dB:
  30x60  the 30 x 60 pattern of tests/golden/iasp/iasp_30x60_m67_2p0.npz at M = 67 and C - 1 relabellings (same pattern, fresh shifts).
         route A  one LdpcHipCodes(dec, wide=True).simulate call: the channel, the set kernel over all codes, the count;
         route B  C consecutive LdpcHip(dec).simulate calls on pre-opened contexts, JIT mode off: the shape-unlimited tier, which is
                  what the library offered for a set of this shape before the wide route.
  16x32  the Appendix-C base matrix at M = 64 and C - 1 relabellings: both set routes fit.
         route A  the wide set (records in LDS; TDMP: the same kernel as route B);
         route B  the register-resident set kernel of the same decoder (LdpcHipCodes(dec)).
The SNR of MS and LMS is chosen so that the frame error rate lies between 0.01 and 0.3; every line records the FER it measured.
Routes A and B alternate in one session; median wall time of --repeats rounds after one warm-up round, then one profiled round for
the summed HIP-event times of the decode launches.  Every result line is appended to --out as soon as it is measured.

    python tools/time_codeset_wide.py [--out profiles/r22_codeset_wide_time.txt] [--repeats 5] [--sizes 1,16,256]
                                      [--workloads 30x60,16x32] [--decoders 3,7,8] [--append]
    python tools/time_codeset_wide.py --probe     # FER of one code per SNR, to choose the operating points
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
NAMES = {3: "MS", 7: "TDMP", 8: "LMS"}
MAXITER = {3: 50, 7: 15, 8: 50}
# (workload, decoder) -> SNR in dB.  TDMP: upstream's scenario; MS and LMS: FER between 0.01 and 0.3 (--probe)
SNR = {("30x60", 3): 2.5, ("30x60", 7): 1.7, ("30x60", 8): 2.0, ("16x32", 3): 2.0, ("16x32", 7): 1.7, ("16x32", 8): 1.5}


def relabel(base, M, rng):
    """The base matrix's pattern with fresh random shifts."""
    return np.where(base >= 0, rng.randint(0, M, size=base.shape), -1).astype(np.int16)


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return 1e3 * (time.perf_counter() - t0), r


def counters(r):
    return [r["nse"], r["nde"], r["nue"], r["frames"], r["sum_abs_iters"]]


def workload(name):
    """(M, base matrix int16 with shifts in [0, M))."""
    if name == "16x32":
        from ldpc_testlib import load_base_matrix, relift
        base = load_base_matrix()
        return 64, np.where(base >= 0, relift(base, 64) % 64, -1).astype(np.int16)
    g = np.load(os.path.join(ROOT, "tests", "golden", "iasp", "iasp_30x60_m67_2p0.npz"))
    assert g["H"].shape == (30, 60)
    return 67, np.where(g["H"] >= 0, g["H"] % 67, -1).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_codeset_wide_time.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="1,16,256")
    ap.add_argument("--workloads", default="30x60,16x32")
    ap.add_argument("--decoders", default="3,7,8")
    ap.add_argument("--probe", action="store_true", help="FER of one code of each workload per SNR for MS and LMS, nothing is timed")
    ap.add_argument("--append", action="store_true", help="keep what --out already holds")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if not (a.append or a.probe):
        open(a.out, "w").close()

    def emit(line):
        """Every result line goes to the file as soon as it exists: an interrupted run keeps what it has measured."""
        print(line, flush=True)
        if not a.probe:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    import torch

    import ldpc_lib_amd as L
    lib = L.load_library()
    lib.ldpc_hip_set_jit_mode(0)
    decs = [int(v) for v in a.decoders.split(",")]
    if a.probe:
        for name in a.workloads.split(","):
            M, base = workload(name)
            for dec in decs:
                with L.LdpcHipCodes(dec, base[None], M, wide=True) as cs:
                    for snr in (1.0, 1.25, 1.5, 1.75, 2.0, 2.25, 2.5):
                        cnt = cs.simulate(snr, MAXITER[dec], SEED, 0, FRAMES)
                        print(f"{name} {NAMES[dec]} {snr} dB: FER {cnt[0, 1] / cnt[0, 3]:.4f}, mean |iterations| {cnt[0, 4] / cnt[0, 3]:.2f}", flush=True)
        return
    if not a.append:
        emit(f"tools/time_codeset_wide.py: {FRAMES} frames per code, alpha 0.8, {torch.cuda.get_device_name(0)}; routes A and B alternated, "
             f"median of {a.repeats} rounds after one warm-up round")
        emit("A = one simulate_codes call on the wide set (ldpc_hip_open_codes_wide); B = 30x60: C x LdpcHip.simulate on pre-opened contexts, JIT "
             "mode 0; 16x32: one simulate_codes call on the register-resident set; kernel = summed HIP-event time of the decode launches")
    for name in a.workloads.split(","):
        M, base = workload(name)
        for dec in decs:
            snr, maxiter = SNR[name, dec], MAXITER[dec]
            rng = np.random.RandomState(9)
            emit(f"workload {name}, {NAMES[dec]} (decoder {dec}): {base.shape[0]} x {base.shape[1]}, M = {M}, {int((base >= 0).sum())} circulants, "
                 f"{maxiter} iterations, {snr} dB")
            emit("C     A wall [ms]   B wall [ms]   B / A   A kernel [ms]   B kernel [ms]   A frames/s per code   B frames/s per code   mean |iterations|   FER      kernel of A; kernels of B")
            for C in [int(v) for v in a.sizes.split(",")]:
                codes = np.array([base] + [relabel(base, M, rng) for _ in range(C - 1)], dtype=np.int16)
                cs = L.LdpcHipCodes(dec, codes, M, wide=True)
                if name == "16x32":
                    other = L.LdpcHipCodes(dec, codes, M)
                    singles = [other]

                    def route_b():
                        return other.simulate(snr, maxiter, SEED, 0, FRAMES)
                else:
                    singles = [L.LdpcHip(dec, H, M) for H in codes]

                    def route_b():
                        return [s.simulate(snr, maxiter, SEED, 0, FRAMES) for s in singles]

                def route_a():
                    return cs.simulate(snr, maxiter, SEED, 0, FRAMES)

                ta, tb = [], []
                for rnd in range(a.repeats + 1):   # round 0 warms up: workspaces, first launches
                    t, cnt = wall(route_a)
                    ta.append(t)
                    t, res = wall(route_b)
                    tb.append(t)
                    print(f"{name} {NAMES[dec]}, C = {C}, round {rnd}: A {ta[-1]:.1f} ms, B {tb[-1]:.1f} ms", flush=True)
                if name == "16x32":                # the two routes count the same errors
                    assert np.array_equal(res, cnt), (res, cnt)
                else:
                    for q, r in enumerate(res):
                        assert counters(r) == cnt[q].tolist(), (q, r, cnt[q])
                cs.profile(True)
                route_a()
                ka, _ = cs.profile_read()
                for s in singles:
                    s.profile(True)
                route_b()
                kb = sum(s.profile_read()[0] for s in singles)
                names = sorted({s.lib.ldpc_hip_last_launch(s.h).decode() for s in singles})
                wa, wb = float(np.median(ta[1:])), float(np.median(tb[1:]))
                its = float(cnt[:, 4].sum()) / float(cnt[:, 3].sum())
                fer = float(cnt[:, 1].sum()) / float(cnt[:, 3].sum())
                emit(f"{C:<5d} {wa:<13.3f} {wb:<13.3f} {wb / wa:<7.2f} {ka:<15.3f} {kb:<15.3f} {FRAMES / wa * 1e3:<21.0f} {FRAMES / wb * 1e3:<21.0f} "
                     f"{its:<19.2f} {fer:<8.4f} {cs.kernel_name}; {', '.join(names)}")
                emit(f"      rounds A [ms]: {' '.join('%.2f' % t for t in ta)}; rounds B [ms]: {' '.join('%.2f' % t for t in tb)}")
                cs.close()
                for s in singles:
                    s.close()


if __name__ == "__main__":
    main()
