#!/usr/bin/env python3
"""Labelling the Appendix C protograph under a girth bound: ldpc_hip_label_codes against upstream's generate_code on one core
(profiles/r30_label_time.txt).  Three calls at seed 1:

  g8_m126   target girth 8, M = 126, 10^6 attempts: exhausts            (the shipped search's first try, files/input32_16.jsonx)
  g8_m399   target girth 8, M = 399: accepts at attempt 238 688          (its retry, main_good_code_search.cpp:298)
  g6_m126   target girth 6, M = 126, 256 labellings in one call          (256 consecutive calls upstream)

    python3 tools/time_label.py --upstream [--out FILE]   where the upstream tree is mounted: compiles tools/make_label_goldens.py's reference
                                                          with -O3 and times the three cases on this CPU (one run each, the CPU is named)
    python3 tools/time_label.py --gpu [--out FILE]        on the GPU: whole-call time, synchronous, after a warm-up call, median of --repeats;
                                                          then per case one child process under `rocprofv3 --kernel-trace` for the split
                                                          over tape generation (mt_jump / mt_generate), redraw pass (mark / sort), check and
                                                          select kernels; the equations a lane evaluates before it dies
    python3 tools/time_label.py --workload CASE           one call of CASE (what the profiled child runs)
Every result line is appended to --out as soon as it is measured."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = {"g8_m126": (8, 126, 1000000, 1), "g8_m399": (8, 399, 1000000, 1), "g6_m126": (6, 126, 1000000, 256)}   # g, M, attempts, labellings


def emit(out, line):
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def cpu_name():
    for line in open("/proc/cpuinfo"):
        if line.startswith("model name"):
            return line.split(":", 1)[1].strip()
    return "unknown CPU"


def upstream(out):
    import make_label_goldens as mg
    exe = mg.build_reference("-O3", os.path.join(ROOT, "oracle", "_ref", "label_ref_O3"))
    proto = mg.appendix_c()
    emit(out, f"# upstream generate_code, g++ -O3, one core of: {cpu_name()}; one run each")
    for name, (g, M, A, K) in CASES.items():
        gold, seconds = mg.reference(proto, g, M, A, 1, K, exe=exe)
        done = sum(c["attempts"] for c in gold["calls"])
        emit(out, f"upstream {name}: {1e3 * sum(seconds):.3f} ms for {K} call(s), {done} attempts, {sum(c['ok'] for c in gold['calls'])} accepted, eqs {gold['eqs']}")


def one_call(name):
    import label_model as lm
    import ldpc_lib_amd as L
    import make_label_goldens as mg
    g, M, A, K = CASES[name]
    state, pos = lm.Stream(seed=1).state()
    t0 = time.perf_counter()
    codes, index, tested, _, _ = L.label_codes(mg.appendix_c(), g, M, A, state, pos, want=K)
    return 1e3 * (time.perf_counter() - t0), len(codes), tested, L.label_last_stats()


def gpu(out, repeats):
    import torch
    import ldpc_lib_amd as L
    emit(out, f"# ldpc_hip_label_codes on {torch.cuda.get_device_name(0)}: whole call (equation table on the host included), synchronous, "
              f"median of {repeats} after one warm-up call")
    for name in CASES:
        one_call(name)
        runs = [one_call(name) for _ in range(repeats)]
        ms = float(np.median([r[0] for r in runs]))
        _, found, tested, (rounds, redraws, evaluated, checked) = runs[0]
        g, M, A, K = CASES[name]
        t0 = time.perf_counter()
        import make_label_goldens as mg
        L.label_equations(mg.appendix_c(), g)
        table_ms = 1e3 * (time.perf_counter() - t0)
        emit(out, f"device {name}: {ms:.3f} ms (of it the host's equation table {table_ms:.3f} ms), {found} accepted, {tested} attempts tested, {rounds} rounds, "
                  f"{redraws} redraws, {checked} attempts checked, {evaluated / max(checked, 1):.1f} equations per lane before it dies")
    for name in CASES:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--workload", name]
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
            if run.returncode != 0 or not traces:
                emit(out, f"kernels {name}: no trace (exit status {run.returncode}) {run.stderr[-300:]!r}")
                continue
            total = {}
            for r in csv.DictReader(open(max(traces, key=os.path.getsize))):
                key = r["Kernel_Name"].split("(")[0].split("::")[-1]
                total[key] = total.get(key, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
            tape = sum(v for k, v in total.items() if k.startswith("mt_"))
            redraw = total.get("mark_kernel", 0.0) + total.get("sort_kernel", 0.0)
            emit(out, f"kernels {name} (one call, rocprofv3 --kernel-trace): tape generation {tape:.3f} ms, redraw pass {redraw:.3f} ms, "
                      f"check {total.get('check_kernel', 0.0):.3f} ms, select {total.get('select_kernel', 0.0):.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_label_time.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--upstream", action="store_true")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--workload")
    a = ap.parse_args()
    if a.workload:
        print(one_call(a.workload))
    if a.upstream:
        upstream(a.out)
    if a.gpu:
        gpu(a.out, a.repeats)


if __name__ == "__main__":
    main()
