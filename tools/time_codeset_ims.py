#!/usr/bin/env python3
"""Integer min-sum (decoder 4) over a code set: one launch against one context per code (profiles/r16_codeset_ims_time.txt).

Two workloads, 4096 frames per code, 50 iterations:
  16x32  the Appendix-C base matrix at M = 64 and C - 1 relabellings of it (same pattern, fresh shifts), 2.0 dB;
  30x60  the 30 x 60 pattern of tests/golden/iasp/iasp_30x60_m67_2p0.npz at M = 67 and C - 1 relabellings, 3.0 dB (some frames converge early,
         others run all 50 iterations: the mean is 25).
  route A  one LdpcHipCodes(IMS_DEC).simulate call: the channel, the quantiser once per frame (ims_coef_kernel,
           ims_quantise_kernel), ims_flood_codes_kernel over all codes, the count;
  route B  C consecutive LdpcHip(IMS_DEC).simulate calls on pre-opened contexts, JIT mode off: ims_flood_kernel (16 x 32; the lone
           shipped matrix, code 0, runs its ahead-of-time int8 instance instead) or ims_global_kernel (30 x 60).
Routes A and B alternate in one session; median wall time of --repeats rounds after one warm-up round, then one profiled round for
the summed HIP-event times of the decode launches (route A's include the quantiser, route B's ims_coef_kernel where it runs).
The quantiser's share of route A comes from a kernel trace: --kernel-stats names the per-kernel statistics (a CSV with the columns
Name, Calls and TotalDurationNs) of a traced run of this tool with --sizes 16 --repeats 1 and one workload, and the tool appends
each kernel's share of the traced GPU time and the ratio ims_quantise_kernel / ims_flood_codes_kernel.
Every result line is appended to --out as soon as it is measured.

    python tools/time_codeset_ims.py [--out profiles/r16_codeset_ims_time.txt] [--repeats 5] [--sizes 1,16,256] [--workloads 16x32,30x60]
    python tools/time_codeset_ims.py --kernel-stats stats.csv [--out ...]     # appends the shares of a traced run
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES, MAXITER, SEED, DEC = 4096, 50, 1, 4


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
    """(M, SNR, base matrix int16 with shifts in [0, M))."""
    if name == "16x32":
        from ldpc_testlib import load_base_matrix, relift
        base = load_base_matrix()
        return 64, 2.0, np.where(base >= 0, relift(base, 64) % 64, -1).astype(np.int16)
    g = np.load(os.path.join(ROOT, "tests", "golden", "iasp", "iasp_30x60_m67_2p0.npz"))
    assert g["H"].shape == (30, 60)
    return 67, 3.0, np.where(g["H"] >= 0, g["H"] % 67, -1).astype(np.int16)


def kernel_shares(path, emit):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])))
    total = sum(r[2] for r in rows)
    emit(f"kernel trace {os.path.basename(path)}: {total / 1e6:.3f} ms of kernels in all; share per kernel (both routes of the traced run):")
    for name, calls, ns in sorted(rows, key=lambda r: -r[2]):
        if ns / total >= 0.0005:
            emit(f"      {100 * ns / total:6.2f} %  {ns / 1e6:10.3f} ms  {calls:6d} calls  {name[:110]}")
    a = {k: sum(ns for name, _, ns in rows if k in name) for k in ("ims_flood_codes_kernel", "ims_quantise_kernel", "ims_coef_kernel")}
    if a["ims_flood_codes_kernel"]:
        emit(f"      ims_quantise_kernel / ims_flood_codes_kernel = {a['ims_quantise_kernel'] / a['ims_flood_codes_kernel']:.4f} "
             f"(ims_coef_kernel, which route B's ahead-of-time instance launches too, in all: {a['ims_coef_kernel'] / 1e6:.3f} ms)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_codeset_ims_time.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="1,16,256")
    ap.add_argument("--workloads", default="16x32,30x60")
    ap.add_argument("--kernel-stats", default=None, help="per-kernel statistics of a traced run: append the shares and exit")
    ap.add_argument("--append", action="store_true", help="keep what --out already holds")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if not (a.append or a.kernel_stats):
        open(a.out, "w").close()

    def emit(line):
        """Every result line goes to the file as soon as it exists: an interrupted run keeps what it has measured."""
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    if a.kernel_stats:
        kernel_shares(a.kernel_stats, emit)
        return
    import torch

    import ldpc_lib_amd as L
    lib = L.load_library()
    lib.ldpc_hip_set_jit_mode(0)
    emit(f"tools/time_codeset_ims.py: {FRAMES} frames per code, {MAXITER} iterations, decoder {DEC}, default quantiser (1.4, 6, 8), alpha 0.8, "
         f"{torch.cuda.get_device_name(0)}; routes A and B alternated, median of {a.repeats} rounds after one warm-up round")
    emit("A = one simulate_codes call; B = C x LdpcHip.simulate on pre-opened contexts, JIT mode 0; kernel = summed HIP-event time of the decode "
         "launches (A: quantiser + ims_flood_codes_kernel)")
    for name in a.workloads.split(","):
        M, snr, base = workload(name)
        rng = np.random.RandomState(9)
        emit(f"workload {name}: {base.shape[0]} x {base.shape[1]}, M = {M}, {int((base >= 0).sum())} circulants, {snr} dB")
        emit("C     A wall [ms]   B wall [ms]   B / A   A kernel [ms]   B kernel [ms]   A frames/s per code   B frames/s per code   mean |iterations|   kernels of B")
        for C in [int(v) for v in a.sizes.split(",")]:
            codes = np.array([base] + [relabel(base, M, rng) for _ in range(C - 1)], dtype=np.int16)
            cs = L.LdpcHipCodes(DEC, codes, M)
            singles = [L.LdpcHip(DEC, H, M) for H in codes]

            def route_a():
                return cs.simulate(snr, MAXITER, SEED, 0, FRAMES)

            def route_b():
                return [s.simulate(snr, MAXITER, SEED, 0, FRAMES) for s in singles]

            ta, tb = [], []
            for rnd in range(a.repeats + 1):   # round 0 warms up: workspaces, first launches
                t, cnt = wall(route_a)
                ta.append(t)
                t, res = wall(route_b)
                tb.append(t)
                print(f"{name}, C = {C}, round {rnd}: A {ta[-1]:.1f} ms, B {tb[-1]:.1f} ms", flush=True)
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
            its = float(cnt[:, 4].sum()) / float(cnt[:, 3].sum())
            emit(f"{C:<5d} {wa:<13.3f} {wb:<13.3f} {wb / wa:<7.2f} {ka:<15.3f} {kb:<15.3f} {FRAMES / wa * 1e3:<21.0f} {FRAMES / wb * 1e3:<21.0f} "
                 f"{its:<19.2f} {', '.join(names)}")
            emit(f"      rounds A [ms]: {' '.join('%.2f' % t for t in ta)}; rounds B [ms]: {' '.join('%.2f' % t for t in tb)}")
            cs.close()
            for s in singles:
                s.close()


if __name__ == "__main__":
    main()
