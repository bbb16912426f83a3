#!/usr/bin/env python3
"""Exact replay of upstream's q-ary frame loop, timed (profiles/rNN_gfq_exact_time.txt): the shipped GF(16) 4 x 8 code at M = 8,
2.7 dB, 15 iterations, the all-zero word (what upstream's harness sends for this code).

  (a) one code, 65 536 frames: LdpcHipGfq.mt_frames (the generator's stream) against LdpcHipGfq.simulate(random_messages=False) (Philox
      noise drawn inside the channel kernel); the difference is the generator's share plus the records copied to the host.
  (b) sets of 16 and 256 candidates at 512 and 4096 frames per code, three forms alternated:
        shared   LdpcHipCodesGfq.mt_simulate without words: one copy of the soft values per piece;
        words    the same with a word per code (all-zero words, so the counters must agree): the soft values formed per code;
        lone     one LdpcHipGfq.mt_frames run per candidate on contexts opened beforehand, 32 at a time.
      The counters of the three forms are asserted equal.
Times are HIP-event times: an event on the null stream before the call and one after it (the library's launches of these entry points
go to the null stream), so the span covers the device work of the call and the host gaps between its launches, not Python's way into
the call; HIP events of the decode launches alone (profile_read) give the decode kernel's part.  The shared and the words form run on
two contexts of their own, and every context is run once untimed first: no timed call allocates a workspace.  Median of --repeats
rounds after one warm-up round.

    python tools/time_gfq_exact.py [--out profiles/rNN_gfq_exact_time.txt] [--repeats 5]
"""
import argparse
import glob
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SNR, MAXITER, SEED, GROUP = 2.7, 15, 1, 32


def wall(fn):
    """(HIP-event milliseconds between the entry and the end of fn's device work on the null stream, fn's result)"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def next_free(name):
    used = [int(m.group(1)) for m in (re.match(r"r(\d+)_", os.path.basename(p)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*_*"))) if m]
    return os.path.join(ROOT, "profiles", "r%02d_%s" % (max(used) + 1, name))


def counters_of(info, its):
    out = []
    for a, b in zip(info, its):
        e = a != 0
        out.append([int((a[e] & ((1 << 30) - 1)).sum()), int(e.sum()), int((e & (b >= 0)).sum()), len(a), int(np.abs(b).sum())])
    return np.array(out, dtype=np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=65536)
    a = ap.parse_args()
    import torch

    import gfq_harness_model as hm
    import ldpc_lib_amd as L
    assert torch.cuda.is_available()
    hb, hc = (hm.cm.left2right(m) for m in hm.shipped(8, 16))
    entry = L.mt19937_state(SEED)
    med = lambda t: float(np.median(t[1:]))   # noqa: E731
    lines = [f"tools/time_gfq_exact.py: the shipped GF(16) 4 x 8 code, M = 8, {SNR} dB, {MAXITER} iterations, the all-zero word; "
             f"HIP-event time around each call, median of {a.repeats} rounds after one warm-up round, forms alternated, every context warmed up untimed",
             f"(a) one code, {a.frames} frames"]
    with L.LdpcHipGfq(4, hb, hc, 8) as dec:
        tm, tp = [], []
        for _ in range(a.repeats + 1):
            dec.mt_set_state(*entry)
            tm.append(wall(lambda: dec.mt_frames(SNR, MAXITER, a.frames))[0])
            tp.append(wall(lambda: dec.simulate(SNR, MAXITER, a.frames, seed=1, random_messages=False))[0])
        dec.profile(True)
        dec.mt_set_state(*entry)
        dec.mt_frames(SNR, MAXITER, a.frames)
        km, _ = dec.profile_read()
        dec.simulate(SNR, MAXITER, a.frames, seed=1, random_messages=False)
        kp, _ = dec.profile_read()
        dec.profile(False)
        tg = []
        for _ in range(a.repeats + 1):
            dec.mt_set_state(*entry)
            tg.append(wall(lambda: dec.mt_advance(a.frames))[0])
        lines.append(f"    mt_frames {med(tm):.3f} ms (decode kernel {km:.3f} ms)   simulate(random_messages=0) {med(tp):.3f} ms (decode kernel {kp:.3f} ms)   "
                     f"difference {med(tm) - med(tp):.3f} ms   generator alone (mt_advance) {med(tg):.3f} ms   {dec.kernel_name}")
        lines.append(f"    rounds mt_frames [ms]: {' '.join('%.2f' % t for t in tm)}; simulate: {' '.join('%.2f' % t for t in tp)}; generator: {' '.join('%.2f' % t for t in tg)}")
    lines.append("(b) sets: C candidates (the shipped pattern with other coefficients) x frames per code")
    lines.append("C     frames   shared [ms]   words [ms]   lone [ms]   lone / shared   lone / words   words / shared")
    rng = np.random.RandomState(9)
    for C in (16, 256):
        hbs = np.repeat(hb[None], C, axis=0)
        hcs = np.array([np.where(hb >= 0, rng.randint(1, 16, hb.shape), -1) if c else hc for c in range(C)], dtype=np.int16)
        zeros = np.zeros((C, hb.shape[1] * 8), dtype=np.int16)
        for frames in (512, 4096):
            with L.LdpcHipCodesGfq(4, hbs, hcs, 8) as cs, L.LdpcHipCodesGfq(4, hbs, hcs, 8) as cw:
                cw.set_codewords(zeros)
                ts, tw, tl = [], [], []
                for one in (cs, cw):   # untimed: the workspaces of both forms exist afterwards
                    one.mt_set_state(*entry)
                    one.mt_simulate(SNR, MAXITER, frames)
                for _ in range(a.repeats + 1):
                    cs.mt_set_state(*entry)
                    t, shared = wall(lambda: cs.mt_simulate(SNR, MAXITER, frames))
                    ts.append(t)
                    cw.mt_set_state(*entry)
                    t, words = wall(lambda: cw.mt_simulate(SNR, MAXITER, frames))
                    tw.append(t)
                    t, lone = 0.0, []
                    for g in range(0, C, GROUP):
                        singles = [L.LdpcHipGfq(4, hbs[c], hcs[c], 8) for c in range(g, min(g + GROUP, C))]

                        def run():
                            out = []
                            for one in singles:
                                one.mt_set_state(*entry)
                                out.append(one.mt_frames(SNR, MAXITER, frames))
                            return out
                        run()   # untimed: workspaces and the generator's buffers exist afterwards
                        dt, part = wall(run)
                        t, lone = t + dt, lone + part
                        for one in singles:
                            one.close()
                    tl.append(t)
                    assert np.array_equal(shared, words) and np.array_equal(shared, counters_of([p[0] for p in lone], [p[1] for p in lone]))
            lines.append(f"{C:<5d} {frames:<8d} {med(ts):<13.3f} {med(tw):<12.3f} {med(tl):<11.3f} {med(tl) / med(ts):<15.2f} {med(tl) / med(tw):<14.2f} {med(tw) / med(ts):.2f}")
            lines.append(f"      rounds shared [ms]: {' '.join('%.2f' % t for t in ts)}; words: {' '.join('%.2f' % t for t in tw)}; lone: {' '.join('%.2f' % t for t in tl)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = a.out or next_free("gfq_exact_time.txt")
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
