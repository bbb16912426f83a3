#!/usr/bin/env python3
"""Times the GF(q) chain around FHT_DEC on one GPU: HIP-event times of the encode, channel, decode and count launches and the
frames/s of ldpc_hip_simulate_gfq, three repeats each, for GF(16) codes with M = 8 at 2.7 dB and M = 128 at 2.0 dB (the shapes of
profiles/r07_gfq_time.txt; the codes are generated ones, 4 x 8 with a weight-3 special column, because upstream's shipped example is
not encodable).  The compiled upstream encode_NBQCLDPC, where oracle/_ref exists, is timed on one core in a fresh process before
the GPU is opened.

    python3 tools/time_gfq_chain.py > profiles/r08_gfq_chain_time.txt
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gfq_chain_model as cm  # noqa: E402

SHAPES = ((8, 2.7, 16384), (128, 2.0, 2048))   # M, SNR [dB], frames per call
MAXITER = 15


def code(M):
    return cm.make_code(np.random.RandomState(M), 4, 4, 8, M, "xox")


def cpu_reference():
    from gfq_chain_ref import EncoderReference, chain_ref_available
    if not chain_ref_available():
        print("compiled upstream encoder: oracle/_ref absent")
        return
    for M, _, _ in SHAPES:
        hb, hc = code(M)
        msg = np.random.RandomState(1).randint(0, 16, (2000, 4 * M))
        ref = EncoderReference(4, hb, hc, M)
        t0 = time.perf_counter()
        ref.encode(msg)
        dt = time.perf_counter() - t0
        ref.close()
        print(f"compiled upstream encode_NBQCLDPC, one core, M = {M}: {dt / 2000 * 1e6:.1f} us/frame = {2000 / dt:.0f} frames/s", file=sys.stderr)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "cpu":
        return cpu_reference()
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "cpu"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, check=True)
    print(out.stderr.decode().strip())
    import torch

    import ldpc_lib_amd
    for M, snr, B in SHAPES:
        hb, hc = code(M)
        with ldpc_lib_amd.LdpcHipGfq(4, hb, hc, M) as dec:
            msg = torch.from_numpy(cm.messages(16, dec.k, 1, 0, B)).cuda()
            sigma = dec.sigma(snr)
            print(f"GF(16) 4 x 8, M = {M}, N = {dec.N}, {snr} dB, {B} frames per launch, maxiter {MAXITER}, kernel {dec.kernel_name}")
            for rep in range(4):   # repeat 0 warms up
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
                ev[0].record()
                cw, ok = dec.encode(msg)
                ev[1].record()
                soft = dec.channel(codeword=cw, sigma=sigma, seed=rep, B=B)
                ev[2].record()
                qhard, iters, _ = dec.decode(soft, MAXITER)
                ev[3].record()
                cnt, _ = dec.count_errors(qhard, cw, iters)
                ev[4].record()
                torch.cuda.synchronize()
                ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(4)]
                t0 = time.perf_counter()
                c = dec.simulate(snr, MAXITER, B, seed=rep)
                dt = time.perf_counter() - t0
                if rep:
                    gbs = B * 16 * dec.N * 8 / (ms[1] * 1e-3) / 1e9
                    print(f"  repeat {rep}: encode {ms[0]:.3f} ms  channel {ms[1]:.3f} ms ({gbs:.0f} GB/s written)  decode {ms[2]:.3f} ms  "
                          f"count {ms[3]:.3f} ms  | outside the decoder {100 * (ms[0] + ms[1] + ms[3]) / sum(ms):.1f} %  "
                          f"decode alone {B / (ms[2] * 1e-3):.0f} frames/s  | simulate {B / dt:.0f} frames/s, FER {c[1] / c[3]:.4f}")


if __name__ == "__main__":
    main()
