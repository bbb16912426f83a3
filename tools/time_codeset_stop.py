#!/usr/bin/env python3
"""A code-set Monte-Carlo run with the stopping rule on the device against the loop over whole-set batches with the rule on the host
(profiles/r11_codeset_stop_time.txt).

Workloads: the shape of profiles/r09 (16 x 32, M = 64, min-sum, 2.0 dB, 50 iterations) and of profiles/r10 (16 x 32, M = 126, TDMP,
1.7 dB, 15 iterations -- upstream's files/input32_16.jsonx); per shape C = 16 and C = 256 codes: random relabelings of the Appendix-C
base matrix (same protograph, fresh shifts) and, as every eighth code, a deliberately weak one (one or two circulants kept per
information column), so that the codes stop at different times.  The rule's settings are a search's: 25 error frames, reference
FER 0.1 (the FER threshold of input32_16.jsonx), at most --experiments frames per code, batches of 1024 frames times 4 up to 65536.
  route A  LdpcHipCodes.simulate_until: the rule on the device, every launch over the codes still running;
  route B  the loop of ldpc::bp_simulation_codes before this route existed: LdpcHipCodes.simulate(records=True) per batch for the
           whole set, the rule replayed on the host per running code (host.replay_stopping_rule, which visits error frames only).
Routes A and B alternate in one session; wall time is the median of --repeats rounds after one warm-up round.  Both routes must
return the same experiment / nse / nde per code.  Frames decoded and bytes copied to the host are counts, not measurements.

    python tools/time_codeset_stop.py [--out profiles/r11_codeset_stop_time.txt] [--repeats 5] [--sizes 16,256] [--experiments 20000]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED, NFE, REF_FER, FIRST_BATCH, MAX_BATCH = 1, 25, 0.1, 1024, 65536
WORKLOADS = [("r09: M = 64, min-sum (3), 2.0 dB, 50 iterations", 3, 64, 2.0, 50),
             ("r10: M = 126, TDMP (7), 1.7 dB, 15 iterations", 7, 126, 1.7, 15)]


def relabel(base, rng, M):
    """The base matrix's protograph with fresh random shifts in the information part (the dual-diagonal part keeps its shifts)."""
    H = base.copy()
    rh = H.shape[0]
    info = H[:, rh:]
    info[info >= 0] = rng.randint(0, M, size=int((info >= 0).sum()))
    return H


def weaken(H, keep):
    """Only the first `keep` circulants of every information column stay: a code with far less coding gain on the same shape."""
    H = H.copy()
    rh = H.shape[0]
    for k in range(rh, H.shape[1]):
        rows = np.flatnonzero(H[:, k] >= 0)
        H[rows[keep:], k] = -1
    return H


def code_set(base, C, M, rng):
    codes = []
    for q in range(C):
        H = relabel(base, rng, M)
        codes.append(weaken(H, 1 + (q // 8) % 2) if q % 8 == 7 else H)
    return np.array(codes, dtype=np.int16)


def route_b(cs, L, snr, maxiter, nexp):
    """(state [C, 3], frames decoded, bytes copied to the host)"""
    C = cs.C
    states = [dict(nse=0, nde=0, nue=0, experiment=0) for _ in range(C)]
    running = [True] * C
    first, batch, decoded, copied = 0, FIRST_BATCH, 0, 0
    while any(running):
        B = min(batch, nexp + 1 - first)
        if B <= 0:
            break
        cnt, info = cs.simulate(snr, maxiter, SEED, first, B, records=True)
        decoded += C * B
        copied += info.nbytes + cnt.nbytes
        zeros = np.zeros(B, dtype=np.int32)
        for q in range(C):
            if running[q] and L.replay_stopping_rule(info[q], zeros, states[q], NFE, nexp, REF_FER):
                running[q] = False
        first += B
        if batch < MAX_BATCH:
            batch = min(batch * 4, MAX_BATCH)
    return np.array([[s["experiment"], s["nse"], s["nde"]] for s in states], dtype=np.uint64), decoded, copied


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return 1e3 * (time.perf_counter() - t0), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_codeset_stop_time.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="16,256")
    ap.add_argument("--experiments", type=int, default=20000)
    a = ap.parse_args()
    import torch

    import ldpc_lib_amd as L
    from codeset_stop_sets import schedule, stop_piece
    from ldpc_testlib import load_base_matrix, relift
    L.load_library().ldpc_hip_set_jit_mode(0)
    nexp = a.experiments
    lines = [f"tools/time_codeset_stop.py: 16 x 32 code sets, {NFE} error frames, reference FER {REF_FER}, at most {nexp} experiments, batches {FIRST_BATCH} x 4 .. {MAX_BATCH}, "
             f"seed {SEED}, {torch.cuda.get_device_name(0)}; routes A and B alternated, median wall time of {a.repeats} rounds after one warm-up round",
             "A = simulate_until (rule on the device, launches over the running codes); B = simulate(records=True) per batch for the whole set, rule on the host",
             "frames = (code, frame) pairs decoded; to host = bytes copied device -> host; kernel = summed HIP-event time of A's decode launches in one more round"]
    for title, dec, M, snr, maxiter in WORKLOADS:
        base = relift(load_base_matrix(), M).astype(np.int16)
        lines.append(title)
        lines.append("C     A wall [ms]   B wall [ms]   B / A   A frames     B frames     B / A   A to host [B]   B to host [B]   A kernel [ms]   A launches   codes by last batch (A)")
        for C in [int(v) for v in a.sizes.split(",")]:
            codes = code_set(base, C, M, np.random.RandomState(9))
            cs = L.LdpcHipCodes(dec, codes, M)
            ta, tb = [], []
            for rnd in range(a.repeats + 1):   # round 0 warms up: workspaces, first launches
                t, st = wall(lambda: cs.simulate_until(snr, maxiter, SEED, NFE, nexp, REF_FER, first_batch=FIRST_BATCH, max_batch=MAX_BATCH))
                ta.append(t)
                t, (sb, frames_b, bytes_b) = wall(lambda: route_b(cs, L, snr, maxiter, nexp))
                tb.append(t)
            assert np.array_equal(st[:, :3], sb), "the two routes must count the same"
            cs.profile(True)
            cs.simulate_until(snr, maxiter, SEED, NFE, nexp, REF_FER, first_batch=FIRST_BATCH, max_batch=MAX_BATCH)
            ka, launches = cs.profile_read()
            cs.close()
            pieces = schedule(nexp, FIRST_BATCH, MAX_BATCH)
            last = [pieces[stop_piece(int(e), pieces)][0] for e in st[:, 0]]
            hist = " ".join(f"{b}:{last.count(b)}" for b in sorted(set(last)))
            frames_a = int(st[:, 3].sum())
            bytes_a = 4 * launches + st.nbytes
            wa, wb = float(np.median(ta[1:])), float(np.median(tb[1:]))
            lines.append(f"{C:<5d} {wa:<13.3f} {wb:<13.3f} {wb / wa:<7.2f} {frames_a:<12d} {frames_b:<12d} {frames_b / frames_a:<7.2f} {bytes_a:<15d} {bytes_b:<15d} "
                         f"{ka:<15.3f} {launches:<12d} {hist}")
            lines.append(f"      rounds A [ms]: {' '.join('%.2f' % t for t in ta)}; rounds B [ms]: {' '.join('%.2f' % t for t in tb)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
