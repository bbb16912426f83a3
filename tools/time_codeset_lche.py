#!/usr/bin/env python3
"""Low-complexity high-efficiency decoder (decoder 9) over a code set: one launch against one context per code
(profiles/r15_codeset_lche_time.txt).

Two shapes, 50 iterations, 4096 frames per code, C random relabelings (same pattern, fresh shifts):
  16 x 32, M = 64, 1.5 dB  the Appendix-C base matrix; every code is relabelled, the shipped matrix itself has an ahead-of-time instance;
  30 x 60, M = 67, 2.0 dB  the matrix of tests/golden/lche/lche_30x60_m67_2p0.npz (upstream's files/input12L.jsonx shape).
  route A  one LdpcHipCodes(DEC_LCHE).simulate call (lche_layered_codes_kernel);
  route B  C consecutive LdpcHip.simulate calls on pre-opened contexts, JIT mode off (lche_global_kernel): the path users have today;
  route C  on the first shape, after the last size: JIT on, compile in the foreground, open + simulate + close per code for
           --jit-codes unseen codes -- what an unseen code costs through hiprtc.
Routes A and B alternate in one session; median wall time of --repeats rounds after one warm-up round, then one profiled round for
the summed HIP-event times of the decode kernels.  Then, per shape and for C = 16 and 256, simulate_until (the stopping rule on the
device) against the per-batch loop of tools/time_codeset_stop.py, with that tool's code sets and rule settings.  Every result line
is appended to --out as soon as it is measured.

    python tools/time_codeset_lche.py [--out profiles/r15_codeset_lche_time.txt] [--repeats 5] [--sizes 1,16,256] [--stop-sizes 16,256]
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

FRAMES, MAXITER, SEED, DEC = 4096, 50, 1, 9


def shapes():
    from ldpc_testlib import load_base_matrix, relift
    base = load_base_matrix()
    a = np.where(base >= 0, relift(base, 64) % 64, -1).astype(np.int16)
    g = np.load(os.path.join(ROOT, "tests", "golden", "lche", "lche_30x60_m67_2p0.npz"))
    assert int(g["M"]) == 67 and g["H"].shape == (30, 60)
    b = np.where(g["H"] >= 0, g["H"] % 67, -1).astype(np.int16)
    return [("16 x 32, M = 64, 1.5 dB", a, 64, 1.5), ("30 x 60, M = 67, 2.0 dB", b, 67, 2.0)]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_codeset_lche_time.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="1,16,256")
    ap.add_argument("--stop-sizes", default="16,256")
    ap.add_argument("--experiments", type=int, default=20000)
    ap.add_argument("--jit-codes", type=int, default=3, help="unseen codes of route C (0: skip it)")
    a = ap.parse_args()
    import torch

    import ldpc_lib_amd as L
    import time_codeset_stop as T
    from codeset_stop_sets import schedule, stop_piece
    assert T.SEED == SEED   # route_b of the stopping-rule tool draws with its own seed
    lib = L.load_library()
    lib.ldpc_hip_set_jit_mode(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()

    def emit(line):
        """Every result line goes to the file as soon as it exists: an interrupted run keeps what it has measured."""
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    emit(f"tools/time_codeset_lche.py: {FRAMES} frames per code, {MAXITER} iterations, decoder {DEC}, {torch.cuda.get_device_name(0)}; "
         f"routes A and B alternated, median wall time of {a.repeats} rounds after one warm-up round")
    emit("A = one simulate_codes call; B = C x LdpcHip.simulate on pre-opened contexts, JIT mode 0; kernel = summed HIP-event time of the decode launches")
    for n_shape, (title, base, M, snr) in enumerate(shapes()):
        rng = np.random.RandomState(9)
        emit(title)
        emit("C     A wall [ms]   B wall [ms]   B / A   A kernel [ms]   B kernel [ms]   A frames/s per code   B frames/s per code   kernels of A; of B")
        per_code_a = {}
        for C in [int(v) for v in a.sizes.split(",")]:
            codes = np.array([relabel(base, M, rng) for _ in range(C)], dtype=np.int16)
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
            emit(f"{C:<5d} {wa:<13.3f} {wb:<13.3f} {wb / wa:<7.2f} {ka:<15.3f} {kb:<15.3f} {FRAMES / wa * 1e3:<21.0f} {FRAMES / wb * 1e3:<21.0f} "
                 f"{cs.kernel_name}; {', '.join(names)}")
            emit(f"      rounds A [ms]: {' '.join('%.2f' % t for t in ta)}; rounds B [ms]: {' '.join('%.2f' % t for t in tb)}")
            emit(f"      mean iterations per frame: {cnt[:, 4].sum() / cnt[:, 3].sum():.2f}; frame errors: {int(cnt[:, 1].sum())} of {int(cnt[:, 3].sum())}")
            cs.close()
            for s in singles:
                s.close()
        if n_shape == 0 and a.jit_codes > 0:
            # route C: unseen codes through hiprtc, compile in the foreground; their counters against one set of the same codes
            unseen = np.array([relabel(base, M, rng) for _ in range(a.jit_codes)], dtype=np.int16)
            lib.ldpc_hip_set_jit_mode(1)
            tc, res_c = [], []
            for q, H in enumerate(unseen):
                def open_simulate_close():
                    with L.LdpcHip(DEC, H, M) as s:
                        return s.simulate(snr, MAXITER, SEED, 0, FRAMES), s.last_launch()
                t, r = wall(open_simulate_close)
                tc.append(t)
                res_c.append(r)
                emit(f"      route C, JIT on, unseen code {q + 1} of {a.jit_codes}, open + simulate + close: {t:.1f} ms ({r[1]})")
            lib.ldpc_hip_set_jit_mode(0)
            with L.LdpcHipCodes(DEC, unseen, M) as cs:
                cnt = cs.simulate(snr, MAXITER, SEED, 0, FRAMES)
            for q, (r, _) in enumerate(res_c):
                assert counters(r) == cnt[q].tolist(), (q, r)
            ref = 16 if 16 in per_code_a else (max(per_code_a) if per_code_a else None)
            emit(f"      route C: {sum(tc) / len(tc):.1f} ms per unseen code (one pass, no warm-up)" +
                 (f"; route A per code at C = {ref}: {per_code_a[ref]:.3f} ms" if ref else ""))
        if not a.stop_sizes:
            continue
        # the stopping rule on the device against the per-batch loop, as tools/time_codeset_stop.py measures it for min-sum and TDMP
        nexp = a.experiments
        emit(f"{title}: simulate_until (A) against simulate(records=True) per batch with the rule on the host (B); {T.NFE} error frames, reference FER "
             f"{T.REF_FER}, at most {nexp} experiments, batches {T.FIRST_BATCH} x 4 .. {T.MAX_BATCH}; every eighth code is a weak one")
        emit("C     A wall [ms]   B wall [ms]   B / A   A frames     B frames     A kernel [ms]   A launches   codes by last batch (A)")
        for C in [int(v) for v in a.stop_sizes.split(",")]:
            codes = T.code_set(base, C, M, np.random.RandomState(9))
            cs = L.LdpcHipCodes(DEC, codes, M)
            ta, tb = [], []
            for rnd in range(a.repeats + 1):
                t, st = wall(lambda: cs.simulate_until(snr, MAXITER, SEED, T.NFE, nexp, T.REF_FER, first_batch=T.FIRST_BATCH, max_batch=T.MAX_BATCH))
                ta.append(t)
                t, (sb, frames_b, _) = wall(lambda: T.route_b(cs, L, snr, MAXITER, nexp))
                tb.append(t)
                print(f"stop, C = {C}, round {rnd}: A {ta[-1]:.1f} ms, B {tb[-1]:.1f} ms", flush=True)
            assert np.array_equal(st[:, :3], sb), "the two routes must count the same"
            cs.profile(True)
            cs.simulate_until(snr, MAXITER, SEED, T.NFE, nexp, T.REF_FER, first_batch=T.FIRST_BATCH, max_batch=T.MAX_BATCH)
            ka, launches = cs.profile_read()
            cs.close()
            pieces = schedule(nexp, T.FIRST_BATCH, T.MAX_BATCH)
            last = [pieces[stop_piece(int(e), pieces)][0] for e in st[:, 0]]
            hist = " ".join(f"{b}:{last.count(b)}" for b in sorted(set(last)))
            wa, wb = float(np.median(ta[1:])), float(np.median(tb[1:]))
            emit(f"{C:<5d} {wa:<13.3f} {wb:<13.3f} {wb / wa:<7.2f} {int(st[:, 3].sum()):<12d} {frames_b:<12d} {ka:<15.3f} {launches:<12d} {hist}")
            emit(f"      rounds A [ms]: {' '.join('%.2f' % t for t in ta)}; rounds B [ms]: {' '.join('%.2f' % t for t in tb)}")


if __name__ == "__main__":
    main()
