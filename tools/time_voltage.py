#!/usr/bin/env python3
"""The voltage check and the bank search on the Appendix C protograph: ldpc_hip_check_voltages and ldpc_hip_label_bank against upstream's
check_voltages and the loop of random_search_bank_good_codes on one core (profiles/r31_voltage_time.txt).  Cases, all at seed 1:

  check_g6    target girth 6 (343 equations), 4096 labellings with voltages below 126 on all 112 edges, max_modulo 1000
  check_g8    target girth 8 (5200 equations), 4096 labellings below 399, max_modulo 4096; the last 1024 below 32767 (no zero sum)
              -- both bounds are above every |sum| of the labellings below T, so the bounded check is upstream's unbounded one;
              each case with the shipped kernel layout (lanes over divisor candidates) and with LDPC_HIP_VOLTAGE_LAYOUT=moduli
  bank_g6     the shipped conventions (32 edges fixed to 0), T = 126, 10^6 attempts, want 150 000: all 10^6 are tested
  bank_g8     target girth 8, T = 399, 10^6 attempts, want 1

    python3 tools/time_voltage.py --upstream [--out FILE]   where the upstream tree is mounted: compiles tools/make_voltage_goldens.py's
                                                            reference with -O3 and times the cases on this CPU (one run each; the time
                                                            of the calls alone, without reading the labellings)
    python3 tools/time_voltage.py --gpu [--out FILE]        on the GPU: whole-call time, synchronous, the equation table on the host
                                                            included, after a warm-up call, median of --repeats
Every result line is appended to --out as soon as it is measured."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CHECKS = {"check_g6": (6, 126, 1000), "check_g8": (8, 399, 4096)}                       # g, voltages below, max_modulo
BANKS = {"bank_g6": (6, 126, 1000000, 150000), "bank_g8": (8, 399, 1000000, 1)}        # g, T, attempts, want
K = 4096


def emit(out, line):
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def cpu_name():
    for line in open("/proc/cpuinfo"):
        if line.startswith("model name"):
            return line.split(":", 1)[1].strip()
    return "unknown CPU"


def labellings(name):
    g, below, mm = CHECKS[name]
    rng = np.random.RandomState(1)
    V = rng.randint(0, below, size=(K, 112))
    if name == "check_g8":
        V[3072:] = rng.randint(0, 32767, size=(1024, 112))
    return V


def upstream(out):
    import make_voltage_goldens as mvg
    exe = mvg.build_reference("-O3", os.path.join(ROOT, "oracle", "_ref", "voltage_ref_O3"))
    appc = mvg.appendix_c()
    emit(out, f"# upstream, g++ -O3, one core of: {cpu_name()}; one run each")
    for name, (g, below, mm) in CHECKS.items():
        gold, seconds = mvg.reference_check((appc > 0).astype(int), g, mm, labellings(name), None, exe=exe)
        st = np.bincount([mvg.status_of(r) for r in gold["results"]], minlength=3).tolist()
        emit(out, f"upstream {name}: {1e3 * seconds:.3f} ms for {K} check_voltages(v, {mm}), {1e6 * seconds / K:.2f} us each, statuses {st}, eqs {gold['eqs']}")
    for name, (g, T, A, want) in BANKS.items():
        gold, seconds = mvg.reference_bank(appc, g, T, 0, A, want, 1, exe=exe)
        emit(out, f"upstream {name}: {1e3 * seconds:.3f} ms, {gold['attempts_tested']} attempts, {1e6 * seconds / gold['attempts_tested']:.2f} us each, "
                  f"{len(gold['accepted'])} accepted, eqs {gold['eqs']}")


def gpu(out, repeats):
    import torch
    import label_model as lm
    import ldpc_lib_amd as L
    import make_voltage_goldens as mvg
    appc = mvg.appendix_c()
    emit(out, f"# on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs): whole call (equation table on the host included), synchronous, median of {repeats} after one warm-up call")

    def median(call):
        call()
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = call()
            times.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(times)), res

    for name, (g, below, mm) in CHECKS.items():
        V = np.ascontiguousarray(labellings(name), dtype=np.int32)
        table_ms, _ = median(lambda: L.label_equations((appc > 0).astype(np.int16), g))
        for layout in ("candidates", "moduli"):
            os.environ["LDPC_HIP_VOLTAGE_LAYOUT"] = layout
            ms, res = median(lambda: L.check_voltages(appc, g, V, mm))
            emit(out, f"device {name} layout {layout}: {ms:.3f} ms for {K} labellings (of it the host's equation table {table_ms:.3f} ms), "
                      f"{1e3 * ms / K:.2f} us each, statuses {np.bincount(res['status'], minlength=3).tolist()}")
        del os.environ["LDPC_HIP_VOLTAGE_LAYOUT"]
    state, pos = lm.Stream(seed=1).state()
    for name, (g, T, A, want) in BANKS.items():
        ms, res = median(lambda: L.label_bank(appc, g, T, A, state, pos, want=want))
        emit(out, f"device {name}: {ms:.3f} ms, {res[3]} attempts, {1e3 * ms / res[3]:.3f} us each, {len(res[0])} accepted, {L.label_last_stats()[0]} rounds")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_voltage_time.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--upstream", action="store_true")
    ap.add_argument("--gpu", action="store_true")
    a = ap.parse_args()
    if a.upstream:
        upstream(a.out)
    if a.gpu:
        gpu(a.out, a.repeats)


if __name__ == "__main__":
    main()
