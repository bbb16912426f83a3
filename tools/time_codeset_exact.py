#!/usr/bin/env python3
"""Exact replay of a set of candidate codes in one context against one exact run per candidate (profiles/r21_codeset_exact_time.txt).

Both routes compute what `for (candidate) { reset_random(); bp_simulation(...); }` computes -- upstream's own mt19937 / polar-method
noise from std::mt19937(1) after the codeword draws, the same for every candidate -- and must return the same five counters per code.
  route A  LdpcHipCodes.mt_simulate_until: the noise drawn once per piece, every launch over the codes still running, the rule on
           the device (batches of 1024 frames times 4 up to 65536);
  route B  C consecutive single-code exact runs, what ldpc::bp_simulation_t does per candidate: LdpcHip contexts opened beforehand
           with JIT mode 0, per code mt_set_state, then mt_frames in that harness's batch schedule (256 frames times 4 up to 65536,
           capped by n_experiments + 1 - frames so far) with the rule on the host (host.replay_stopping_rule).  The contexts are
           opened, run once untimed and closed 32 at a time outside the timed region: 256 of them with their workspaces do not fit
           the device at once.
Neither route moves the generator to the end of a code's run afterwards (mt_advance / the harness's roll-back): the same extra work on
both sides.  Routes A and B alternate in one session; wall time is the median of --repeats rounds after one warm-up round.
Workloads: 16 x 32, M = 64, min-sum, 2.0 dB, 50 iterations, n_experiments 4000 (cfg2); 16 x 32, M = 126, TDMP, 1.7 dB, 15 iterations,
50 error frames (the shipped scenario).  The codes are those of tools/time_codeset_stop.py: relabelings of the Appendix-C matrix, every
eighth one deliberately weak.  C = 1 is the Appendix-C matrix itself.
The generator's share of route A: the decode launches' summed HIP-event time (profile_read) in one more round, and the wall time of
mt_advance over as many frames as route A draws (the generator alone, nothing decoded), each against A's wall time.

    python tools/time_codeset_exact.py [--out profiles/r21_codeset_exact_time.txt] [--repeats 5] [--sizes 1,16,256]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SEED, FIRST_BATCH, MAX_BATCH = 1, 1024, 65536
# title, decoder, M, SNR, iterations, n_frame_errors, n_experiments
WORKLOADS = [("min-sum (3): 16 x 32, M = 64, 2.0 dB, 50 iterations, n_experiments 4000", 3, 64, 2.0, 50, 10**9, 4000),
             ("TDMP (7): 16 x 32, M = 126, 1.7 dB, 15 iterations, 50 error frames", 7, 126, 1.7, 15, 50, 10**8)]


GROUP = 32   # single-code contexts open at a time


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return 1e3 * (time.perf_counter() - t0), r


def route_b(L, dec, codes, M, entry, snr, maxiter, nfe, nexp):
    """(wall ms of the runs, [C, 5] = experiment, nse, nde, nue, sum |iters| per code, calls of mt_frames, kernel of the contexts)"""
    ms, out, calls, name = 0.0, [], 0, ""
    for g in range(0, len(codes), GROUP):
        singles = [L.LdpcHip(dec, H, M) for H in codes[g:g + GROUP]]
        name = singles[0].kernel_name
        run_singles(L, singles, entry, snr, maxiter, nfe, nexp)   # untimed: the contexts' workspaces and the generator's buffers exist afterwards
        t, (part, n) = wall(lambda: run_singles(L, singles, entry, snr, maxiter, nfe, nexp))
        ms, out, calls = ms + t, out + part, calls + n
        for one in singles:
            one.close()
    return ms, np.array(out, dtype=np.uint64), calls, name


def run_singles(L, singles, entry, snr, maxiter, nfe, nexp):
    out, calls = [], 0
    for one in singles:
        one.mt_set_state(*entry)
        st = {"nse": 0, "nde": 0, "nue": 0, "experiment": 0}
        sit, batch, stop = 0, 256, nfe <= 0 or nexp < 0
        while not stop:
            B = min(batch, nexp + 1 - st["experiment"])
            info, its = one.mt_frames(snr, maxiter, B)
            calls += 1
            before = st["experiment"]
            stop = L.replay_stopping_rule(info, its, st, nfe, nexp, 1.0)
            sit += int(np.abs(its[:st["experiment"] - before].astype(np.int64)).sum())
            if batch < MAX_BATCH:
                batch = min(batch * 4, MAX_BATCH)
        out.append([st["experiment"], st["nse"], st["nde"], st["nue"], sit])
    return out, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_codeset_exact_time.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="1,16,256")
    a = ap.parse_args()
    import torch

    import ldpc_lib_amd as L
    from ldpc_testlib import load_base_matrix, relift
    from time_codeset_stop import code_set
    L.load_library().ldpc_hip_set_jit_mode(0)
    lines = [f"tools/time_codeset_exact.py: exact replay from std::mt19937({SEED}), reference FER 1.0, {torch.cuda.get_device_name(0)}; routes A and B alternated, "
             f"median wall time of {a.repeats} rounds after one warm-up round",
             "A = one LdpcHipCodes.mt_simulate_until (noise drawn once per piece, rule on the device); B = C x (LdpcHip.mt_set_state, mt_frames per batch, rule on "
             "the host) on pre-opened contexts, JIT mode 0",
             "A decode = summed HIP-event time of A's decode launches in one more round; generator = wall time of mt_advance over the frames A draws"]
    for title, dec, M, snr, maxiter, nfe, nexp in WORKLOADS:
        base = relift(load_base_matrix(), M).astype(np.int16)
        entry = L.mt19937_state(SEED, (base.shape[1] - base.shape[0]) * M)
        lines.append(title)
        lines.append("C     A wall [ms]   B wall [ms]   B / A   A frames drawn   A frames decoded   B frames   B calls   A decode [ms]   generator [ms]   generator / A   "
                     "kernels of A; of B")
        for C in [int(v) for v in a.sizes.split(",")]:
            codes = base[None] if C == 1 else code_set(base, C, M, np.random.RandomState(9))
            cs = L.LdpcHipCodes(dec, codes, M)

            def route_a():
                cs.mt_set_state(*entry)
                return cs.mt_simulate_until(snr, maxiter, nfe, nexp, 1.0, first_batch=FIRST_BATCH, max_batch=MAX_BATCH)

            ta, tb = [], []
            for rnd in range(a.repeats + 1):   # round 0 warms up: workspaces, first launches
                t, st = wall(route_a)
                ta.append(t)
                t, sb, calls_b, single_name = route_b(L, dec, codes, M, entry, snr, maxiter, nfe, nexp)
                tb.append(t)
            assert np.array_equal(st[:, :5], sb), "the two routes must count the same"
            cs.profile(True)
            route_a()
            ka, _ = cs.profile_read()
            cs.profile(False)
            drawn = int(st[:, 5].max())   # the pieces come in frame order: the longest-running code has seen every frame drawn
            tg = []
            for rnd in range(a.repeats + 1):
                cs.mt_set_state(*entry)
                tg.append(wall(lambda: cs.mt_advance(snr, drawn))[0])
            names = f"{cs.kernel_name}; {single_name}"
            cs.close()
            wa, wb, wg = float(np.median(ta[1:])), float(np.median(tb[1:])), float(np.median(tg[1:]))
            lines.append(f"{C:<5d} {wa:<13.3f} {wb:<13.3f} {wb / wa:<7.2f} {drawn:<16d} {int(st[:, 5].sum()):<18d} {int(sb[:, 0].sum()):<10d} {calls_b:<9d} {ka:<15.3f} "
                         f"{wg:<16.3f} {wg / wa:<15.2f} {names}")
            lines.append(f"      rounds A [ms]: {' '.join('%.2f' % t for t in ta)}; rounds B [ms]: {' '.join('%.2f' % t for t in tb)}; "
                         f"rounds generator [ms]: {' '.join('%.2f' % t for t in tg)}")
            if C == 1:
                lines.append(f"      the Appendix-C matrix: {int(st[0, 2])} error frames in {int(st[0, 0])}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
