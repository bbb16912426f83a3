#!/usr/bin/env python3
"""Frames per second of the GF(q) sum-product decoder (FHT_DEC, decoder 6) on the GF(16) code of upstream's
files/resultq_codes.jsonx (4 x 8 base matrix, 15 iterations) at lifting 8 and 128: the worst case (an SNR at which no frame
converges) and one operating point.  Device-resident inputs, decode only, HIP events around `reps` launches after one warm-up.

Next to it the compiled upstream reference on the same box (tests/gfq_ref.py, where oracle/_ref exists): the same inputs' kind of
frames through sum_prod_gfq_decod_lm in fresh worker processes, one and `--cores` at a time, measured BEFORE this process opens
the GPU.

    python tools/time_gfq.py [--frames B] [--reps R] [--cores 16] [--quick]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

MAXITER = 15
CASES = [("gf16_m8_worst", 8, -1.0), ("gf16_m8_2p7", 8, 2.7), ("gf16_m128_worst", 128, -1.0), ("gf16_m128_2p0", 128, 2.0)]


def ref_worker(M, snr, frames, seed):
    """One core of the reference: prints frames and the seconds spent inside the decode calls."""
    import make_gfq_goldens as G
    from gfq_model import bpsk_symbol_probabilities
    from gfq_ref import GfqReference
    hb, hc = G.shipped(M, 16)
    soft = bpsk_symbol_probabilities(np.random.RandomState(seed), 4, hb.shape[1] * M, G.sigma_of(snr, hb), frames)
    ref = GfqReference(4, hb, hc, M)
    ref.decode(soft[:2], MAXITER)
    t = time.perf_counter()
    iters = ref.decode(soft, MAXITER)[0]
    dt = time.perf_counter() - t
    print(json.dumps({"frames": frames, "seconds": dt, "failed": int((iters < 0).sum())}), flush=True)


def reference(label, M, snr, frames, cores):
    """Frames per second of `cores` concurrent fresh reference processes (wall clock over the slowest)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--ref-worker", str(M), str(snr), str(frames)]
    procs = [subprocess.Popen(cmd + [str(100 + i)], stdout=subprocess.PIPE) for i in range(cores)]
    outs = [json.loads(p.communicate()[0].decode().strip().splitlines()[-1]) for p in procs]
    assert all(p.returncode == 0 for p in procs)
    slowest = max(o["seconds"] for o in outs)
    res = {"case": label, "reference_cores": cores, "frames": frames * cores, "seconds": round(slowest, 4),
           "frames_per_s": round(frames * cores / slowest, 1), "failed_frames": sum(o["failed"] for o in outs)}
    print(json.dumps(res), flush=True)
    return res


def device_inputs(torch, hb, M, snr, B, seed):
    """bpsk_symbol_probabilities of tests/gfq_model.py on the device (input generation only; not timed)."""
    import make_gfq_goldens as G
    q_bits, q, N = 4, 16, hb.shape[1] * M
    sigma = G.sigma_of(snr, hb)
    g = torch.Generator(device="cuda").manual_seed(seed)
    y = sigma * torch.randn((B, N, q_bits), dtype=torch.float64, device="cuda", generator=g) - 1.0
    v = torch.tensor([[2.0 * ((s >> (q_bits - 1 - k)) & 1) - 1.0 for k in range(q_bits)] for s in range(q)], dtype=torch.float64, device="cuda")
    p = torch.exp(torch.einsum("bnk,sk->bsn", y, v) / (sigma * sigma))
    return (p / p.sum(dim=1, keepdim=True)).contiguous()


def run(L, torch, label, M, snr, B, reps):
    import make_gfq_goldens as G
    hb, hc = G.shipped(M, 16)
    with L.LdpcHipGfq(4, hb, hc, M) as dec:
        soft = device_inputs(torch, hb, M, snr, B, 7)
        qhard, iters, _ = dec.decode(soft, MAXITER)              # warm-up: the workspace is allocated here
        torch.cuda.synchronize()
        dec.profile(True)
        for _ in range(reps):
            dec.decode(soft, MAXITER)
        total_ms, n = dec.profile_read()
        ms = total_ms / n
        it = iters.cpu().numpy()
        sum_rw = int((hb >= 0).sum())
        iters_run = float(np.where(it < 0, MAXITER, it).mean())   # check / symbol passes a frame went through
        moved = 2 * (2 * 8 * 16 * sum_rw * M) * iters_run * B    # read + written, soft_in and soft_outs, per frame-iteration
        res = {"case": label, "kernel": dec.kernel_name, "M": M, "N": dec.N, "q": dec.q, "frames": B, "maxiter": MAXITER, "snr_db": snr,
               "ms_per_launch": round(ms, 4), "frames_per_s": round(B / (ms * 1e-3)), "mean_iterations_run": round(iters_run, 3),
               "failed_frames": int((it < 0).sum()), "algorithmic_GB_per_s": round(moved / (ms * 1e-3) / 1e9, 1),
               "fraction_of_8TB_per_s_effective": round(moved / (ms * 1e-3) / 8e12, 4)}
    print(json.dumps(res), flush=True)
    return res


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--ref-worker":
        return ref_worker(int(sys.argv[2]), float(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cores", type=int, default=16)
    ap.add_argument("--quick", action="store_true", help="fewer frames and one repetition (for a kernel trace)")
    args = ap.parse_args()
    if args.quick:
        args.frames, args.reps = 8192, 1
    from gfq_ref import gfq_ref_available
    refs = {}
    if gfq_ref_available():   # before the GPU is opened, in fresh processes
        for label, M, snr in CASES:
            per_core = 400 if M == 8 else 24
            refs[label] = (reference(label, M, snr, per_core, 1), reference(label, M, snr, per_core, args.cores))
    else:
        print(json.dumps({"note": "oracle/_ref is not built here: no reference timing"}), flush=True)
    import torch
    import ldpc_lib_amd as L
    assert torch.cuda.is_available()
    for label, M, snr in CASES:
        B = args.frames if M == 8 else max(args.frames // 16, 256)   # M = 128: 131 KB of input per frame; the batch that memory allows comfortably
        r = run(L, torch, label, M, snr, B, args.reps)
        if label in refs:
            one, many = refs[label]
            print(json.dumps({"case": label, "speedup_over_reference_1_core": round(r["frames_per_s"] / one["frames_per_s"], 1),
                              "speedup_over_reference_%d_cores" % args.cores: round(r["frames_per_s"] / many["frames_per_s"], 1)}), flush=True)


if __name__ == "__main__":
    main()
