#!/usr/bin/env python3
"""An SNR grid on a code set in one call against the loop of single-SNR set calls (profiles/r34_codeset_grid_time.txt).

Both routes compute what `for (snr) { reset_random(); for (candidate) bp_simulation(...); }` computes -- upstream's own mt19937 /
polar-method noise from std::mt19937(1) after the codeword draws, the same for every (SNR, candidate) pair -- on ONE open code-set
context and must return the same states.
  route A  one LdpcHipCodes.mt_simulate_grid_until: the P x C pairs as one set of work items, the noise drawn once per piece for all
           points, every launch over the items still running, the rule on the device;
  route B  P x (mt_set_state, LdpcHipCodes.mt_simulate_until): what `ldpc_sim --code-sets` does per group today.
Batches of 1024 frames times 4 up to 65536 on both routes, reference FER 1.0 at every point.  Routes A and B alternate in one session;
wall time is the median of --repeats rounds after one warm-up round.  Workloads: those of tools/time_codeset_exact.py (16 x 32,
M = 64, min-sum, 50 iterations, n_experiments 4000; 16 x 32, M = 126, TDMP, 15 iterations, 50 error frames; relabelings of the
Appendix-C matrix, every eighth one deliberately weak, C = 1 the matrix itself) at P = 8 points from 1.0 dB in steps of 0.25.
The states compared are the five counters per (point, code); frames_decoded is reported, not compared, because the grid's pieces are
shorter where the 1 GiB bound on a piece's buffers, which hold all P points, cuts them.  Per row: frames drawn (A draws max over the items once; B draws per point), frames decoded (the sum of frames_decoded), pieces
launched (the batch schedule restated), and the generator's share of A: the wall time of mt_advance over the frames A draws against
A's wall time -- a lower bound, since A's emit pass also writes P rows per frame where mt_advance writes none.

--existing-only times the EXISTING single-SNR call alone (mt_simulate_until, min-sum, C = 16, 2.0 dB) and prints its rounds; with
--tree DIR the library is imported from another built checkout (the parent commit's), so that both can be timed in one session.

    python tools/time_codeset_grid.py [--out profiles/r34_codeset_grid_time.txt] [--repeats 5] [--sizes 1,4,16,256]
    python tools/time_codeset_grid.py --existing-only [--tree DIR]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED, FIRST_BATCH, MAX_BATCH = 1, 1024, 65536
POINTS = tuple(1.0 + 0.25 * p for p in range(8))
# title, decoder, M, iterations, n_frame_errors, n_experiments
WORKLOADS = [("min-sum (3): 16 x 32, M = 64, 50 iterations, n_experiments 4000", 3, 64, 50, 10**9, 4000),
             ("TDMP (7): 16 x 32, M = 126, 15 iterations, 50 error frames", 7, 126, 15, 50, 10**8)]


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return 1e3 * (time.perf_counter() - t0), r


def piece_frames(cs, points):
    """Frames per piece as the library cuts them: 65536, or what 1 GiB holds of the buffers of all points (no LDPC_HIP_CODES_PIECE here)"""
    per_frame = cs.C * (4 * cs.hard_words + 8) + 8 * cs.N
    return max(1, min(1 << 16, (1 << 30) // (per_frame * points)))


def pieces_until(frames, nexp, piece):
    """Pieces of the batch schedule, each batch cut into pieces of `piece` frames, up to the one that holds frame number `frames`"""
    n, first, batch = 0, 0, FIRST_BATCH
    while first < frames:
        B = min(batch, nexp + 1 - first)
        n += min(-(-B // piece), -(-(frames - first) // piece))
        first += B
        if batch < MAX_BATCH:
            batch = min(batch * 4, MAX_BATCH)
    return n


def existing_only(L, repeats):
    """The existing single-SNR call: min-sum, M = 64, C = 16, 2.0 dB, 50 iterations, n_experiments 4000"""
    from ldpc_testlib import load_base_matrix, relift
    from time_codeset_stop import code_set
    dec, M, maxiter, nfe, nexp = 3, 64, 50, 10**9, 4000
    base = relift(load_base_matrix(), M).astype(np.int16)
    entry = L.mt19937_state(SEED, (base.shape[1] - base.shape[0]) * M)
    codes = code_set(base, 16, M, np.random.RandomState(9))
    with L.LdpcHipCodes(dec, codes, M) as cs:
        ts = []
        for rnd in range(repeats + 1):
            cs.mt_set_state(*entry)
            t, st = wall(lambda: cs.mt_simulate_until(2.0, maxiter, nfe, nexp, 1.0, first_batch=FIRST_BATCH, max_batch=MAX_BATCH))
            ts.append(t)
    print(f"existing mt_simulate_until, min-sum, C = 16, 2.0 dB ({os.path.dirname(L.__file__)}): median {np.median(ts[1:]):.3f} ms, spread "
          f"{min(ts[1:]):.3f} .. {max(ts[1:]):.3f}; rounds [ms]: {' '.join('%.3f' % t for t in ts)}; checksum {int(st[:, :5].sum())}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r34_codeset_grid_time.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="1,4,16,256")
    ap.add_argument("--existing-only", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    for d in (tree, os.path.join(tree, "tests"), os.path.join(tree, "tools")):
        sys.path.insert(0, d)
    import torch

    import ldpc_lib_amd as L
    from ldpc_testlib import load_base_matrix, relift
    from time_codeset_stop import code_set
    L.load_library().ldpc_hip_set_jit_mode(0)
    if a.existing_only:
        return existing_only(L, a.repeats)
    P = len(POINTS)
    refs = (1.0,) * P
    lines = [f"tools/time_codeset_grid.py: exact replay from std::mt19937({SEED}), P = {P} points {POINTS[0]} .. {POINTS[-1]} dB, reference FER 1.0, "
             f"{torch.cuda.get_device_name(0)}; routes A and B alternated, median wall time of {a.repeats} rounds after one warm-up round",
             "A = one LdpcHipCodes.mt_simulate_grid_until (P x C items, noise drawn once per piece for all points); B = P x (mt_set_state, "
             "LdpcHipCodes.mt_simulate_until) on the same context; both return the same states (asserted)",
             "generator = wall time of mt_advance over the frames A draws (a lower bound of the generator's share: A's emit pass writes P rows per frame)"]
    for title, dec, M, maxiter, nfe, nexp in WORKLOADS:
        base = relift(load_base_matrix(), M).astype(np.int16)
        entry = L.mt19937_state(SEED, (base.shape[1] - base.shape[0]) * M)
        lines.append(title)
        lines.append("C     A wall [ms]   B wall [ms]   B / A   A frames drawn   B frames drawn   A frames decoded   B frames decoded   A pieces   B pieces   "
                     "generator [ms]   generator / A   kernel")
        for C in [int(v) for v in a.sizes.split(",")]:
            codes = base[None] if C == 1 else code_set(base, C, M, np.random.RandomState(9))
            cs = L.LdpcHipCodes(dec, codes, M)

            def route_a():
                cs.mt_set_state(*entry)
                return cs.mt_simulate_grid_until(POINTS, maxiter, nfe, nexp, refs, first_batch=FIRST_BATCH, max_batch=MAX_BATCH)

            def route_b():
                out = []
                for snr in POINTS:
                    cs.mt_set_state(*entry)
                    out.append(cs.mt_simulate_until(snr, maxiter, nfe, nexp, 1.0, first_batch=FIRST_BATCH, max_batch=MAX_BATCH))
                return np.stack(out)

            ta, tb = [], []
            for rnd in range(a.repeats + 1):   # round 0 warms up: workspaces, first launches
                t, sa = wall(route_a)
                ta.append(t)
                t, sb = wall(route_b)
                tb.append(t)
            # the five counters of every (point, code); frames_decoded may differ: a piece holds the buffers of all P points within
            # 1 GiB, so the grid's pieces are shorter where that bound cuts and an item that stops pays for a shorter piece
            assert np.array_equal(sa[:, :, :5], sb[:, :, :5]), "the two routes must return the same states"
            drawn_a = int(sa[:, :, 5].max())                  # the pieces come in frame order: the longest-running item has seen every frame drawn
            drawn_b = int(sb[:, :, 5].max(axis=1).sum())      # ... per point
            pieces_a = pieces_until(drawn_a, nexp, piece_frames(cs, P))
            pieces_b = sum(pieces_until(int(f), nexp, piece_frames(cs, 1)) for f in sb[:, :, 5].max(axis=1))
            tg = []
            for rnd in range(a.repeats + 1):
                cs.mt_set_state(*entry)
                tg.append(wall(lambda: cs.mt_advance(POINTS[0], drawn_a))[0])
            name = cs.kernel_name
            cs.close()
            wa, wb, wg = float(np.median(ta[1:])), float(np.median(tb[1:])), float(np.median(tg[1:]))
            lines.append(f"{C:<5d} {wa:<13.3f} {wb:<13.3f} {wb / wa:<7.2f} {drawn_a:<16d} {drawn_b:<16d} {int(sa[:, :, 5].sum()):<18d} {int(sb[:, :, 5].sum()):<18d} "
                         f"{pieces_a:<10d} {pieces_b:<10d} {wg:<16.3f} {wg / wa:<15.2f} {name}")
            lines.append(f"      rounds A [ms]: {' '.join('%.2f' % t for t in ta)}; rounds B [ms]: {' '.join('%.2f' % t for t in tb)}; "
                         f"rounds generator [ms]: {' '.join('%.2f' % t for t in tg)}")
            print(lines[-2], flush=True)   # progress: a row at C = 256 takes a while
            lines.append(f"      frames consumed per point (code 0): {' '.join(str(int(e)) for e in sa[:, 0, 0])}; error frames: {' '.join(str(int(e)) for e in sa[:, 0, 2])}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
