#!/usr/bin/env python3
"""Frames per second and mean iterations of the low-complexity high-efficiency decoder (LCHE_DEC, decoder 9) on each tier:
the ahead-of-time instance on the example code at M = 64 (2.0 dB and 0 dB, 50 iterations), the hiprtc instance on the 30 x 60
shape of upstream's files/input12L.jsonx at M = 67, and the shape-unlimited tier forced on the M = 64 code.  Device-resident
LLRs, decode only, HIP events around `reps` launches after one warm-up launch.

    python tools/time_lche.py [--frames B] [--reps R] [--quick]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(L, torch, label, H, M, snr, maxiter, B, reps, force_global=False):
    from ldpc_testlib import LCHE_DEC
    if force_global:
        os.environ["LDPC_HIP_FORCE_GLOBAL"] = "1"
    try:
        dec = L.LdpcHip(LCHE_DEC, H, M)
    finally:
        os.environ.pop("LDPC_HIP_FORCE_GLOBAL", None)
    with dec:
        llr = dec.awgn_llr(snr, 1, 0, B)
        hard, iters, _ = dec.decode(llr, maxiter)            # warm-up (hiprtc instance already compiled at open)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            dec.decode(llr, maxiter, out=(hard, iters, None))
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        it = iters.cpu().numpy()
        res = {"case": label, "kernel": dec.kernel_name, "N": int(H.shape[1] * M), "frames": B, "maxiter": maxiter, "snr_db": snr,
               "ms_per_launch": round(ms, 4), "frames_per_s": round(B / (ms * 1e-3)), "mean_abs_iters": round(float(np.abs(it).mean()), 3),
               "failed_frames": int((it < 0).sum())}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="fewer frames and one repetition (for a kernel trace)")
    args = ap.parse_args()
    if args.quick:
        args.frames, args.reps = 8192, 1
    import torch
    import ldpc_lib_amd as L
    from ldpc_testlib import load_base_matrix, random_qc_code, relift
    assert torch.cuda.is_available()
    H64 = relift(load_base_matrix(), 64)
    H30 = random_qc_code(np.random.RandomState(67), 30, 60, 67, [2, 3, 3, 16, 2, 3])
    B = args.frames
    run(L, torch, "aot_m64_2p0", H64, 64, 2.0, 50, B, args.reps)
    run(L, torch, "aot_m64_1p5", H64, 64, 1.5, 50, B, args.reps)
    run(L, torch, "aot_m64_0p0", H64, 64, 0.0, 50, max(B // 4, 1024), args.reps)
    run(L, torch, "hiprtc_30x60_m67_2p0", H30, 67, 2.0, 50, max(B // 4, 1024), args.reps)
    run(L, torch, "global_m64_2p0", H64, 64, 2.0, 50, max(B // 8, 1024), args.reps, force_global=True)


if __name__ == "__main__":
    main()
