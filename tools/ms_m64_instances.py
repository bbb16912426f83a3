#!/usr/bin/env python3
"""Registers of every instance of ms_m64_body that the GPU tests compile with hiprtc, and of five synthetic protographs: each one
cross-compiled as a one-kernel translation unit (__launch_bounds__(64, 2), the Code struct as ldpc_jit.hpp writes it), in both
variants: ms_m64_body (with soft values) and ms_m64_hard_body (without: what a launch without soft_out runs).
usage: ms_m64_instances.py [--csrc DIR] [--args "<template arguments after the code>"] [--body NAME] [name ...]
--csrc: a directory with another ldpc_spec.hpp (a parent commit's, say), for a before / after table.  Needs hipcc, no GPU."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_ms_m64_allrows as allrows   # noqa: E402
import test_gpu_ms_m64_carry as carry       # noqa: E402
import test_gpu_ms_m64_eqslot as eqslot     # noqa: E402
import test_gpu_ms_m64_local as local       # noqa: E402
import test_gpu_ms_m64_prefix as prefix     # noqa: E402
import test_gpu_ms_m64_retain as retain     # noqa: E402
import test_gpu_ms_m64_rotation as rotation  # noqa: E402
from test_ms_m64_local_cpu import _atomics_expected, _code_struct  # noqa: E402

M = 64


def proto(rh, nh, w):
    """row j has the w block columns (j w + 3 j + s) mod NH, s = 0..w-1, shift (11 j + 5 k + 1) mod 64; no local column"""
    H = -np.ones((rh, nh), dtype=np.int16)
    for j in range(rh):
        for s in range(w):
            k = (j * w + 3 * j + s) % nh
            H[j, k] = (11 * j + 5 * k + 1) % M
    return H


def instances():
    out = {}
    for mod, name, codes in ((rotation, "rotation", rotation.CASES), (retain, "retain", retain.CASES), (carry, "carry", carry.ROW_SETS),
                             (local, "local", local.CODES), (allrows, "allrows", allrows.CODES)):
        for case, make in codes.items():
            out[f"{name}:{case}"] = make()
    out["carry:slot_matrix"] = carry._slot_matrix()
    out["eqslot:record_rows_last_14x28"] = eqslot._record_rows_last()
    out["prefix:weights_2_and_3"] = prefix._weights_two_and_three()
    for rh, nh, w in ((8, 32, 16), (12, 32, 12), (20, 40, 8), (24, 32, 8), (30, 60, 6)):
        out[f"proto:{rh}x{nh}_w{w}"] = proto(rh, nh, w)
    return out


BODIES = ("ms_m64_body", "ms_m64_hard_body")


def build_asm(csrc, H, targs="", body="ms_m64_body"):
    """the instance's assembly text"""
    with tempfile.TemporaryDirectory() as td:
        src, out = os.path.join(td, "k.hip"), os.path.join(td, "k.s")
        open(src, "w").write(f'#include "{csrc}/ldpc_spec.hpp"\n{_code_struct(H)}'
                             'extern "C" __global__ void __launch_bounds__(64, 2) k(const ldpc_spec::SpecArgs a) '
                             f'{{ ldpc_spec::{body}<Code{targs}>(a); }}\n')
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only",
                               "-S", src, "-o", out], stderr=subprocess.DEVNULL)
        return open(out).read()


def figures(asm):
    meta = {k: int(re.search(r"^\s*" + re.escape(k) + r":\s*(\d+)", asm, re.M).group(1))
            for k in (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size")}
    return meta, len(re.findall(r"^\s+ds_add_f64\s", asm, re.M))


def build(csrc, H, targs, body="ms_m64_body"):
    return figures(build_asm(csrc, H, targs, body))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "ldpc-lib_amd", "csrc"))
    ap.add_argument("--args", default="")
    ap.add_argument("--body", default=None, choices=BODIES, help="one variant only (--args applies to ms_m64_body)")
    ap.add_argument("names", nargs="*")
    a = ap.parse_args()
    todo = {n: H for n, H in instances().items() if not a.names or n in a.names}
    targs = ", " + a.args if a.args else ""
    bodies = (a.body,) if a.body else BODIES[:1] if a.args else BODIES
    jobs = [(n, b) for n in todo for b in bodies]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        res = dict(zip(jobs, ex.map(lambda nb: build(a.csrc, todo[nb[0]], targs if nb[1] == BODIES[0] else "", nb[1]), jobs)))
    for n, b in jobs:
        H = todo[n]
        meta, adds = res[n, b]
        print(f"  {n:38s}{'hard' if b == BODIES[1] else 'soft'}{H.shape[0]:3d} x {H.shape[1]:<3d}{int((H >= 0).sum()):4d} edges   VGPRs {meta['.vgpr_count']:3d}   spilled {meta['.vgpr_spill_count']:3d}   "
              f"scratch {meta['.private_segment_fixed_size']:4d} B   ds_add_f64 {adds:3d} (expected {_atomics_expected(H):3d})   "
              f"carried rows {eqslot.carried_rows(H):2d} -> {allrows.carry_rows(H):2d} of {H.shape[0]:2d}")


if __name__ == "__main__":
    main()
