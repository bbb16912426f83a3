"""CPU: ms_m64_body with local block columns, on cross-compiled one-kernel translation units (no GPU).

A local block column (every edge shift 0, first and last block row at most three apart: ms_m64_local_col of ldpc_spec.hpp) stays out
of LDS inside the iteration.  Checked here on the shipped instance and on the hand-written 3 x 6 code of
test_gpu_ms_m64_local.py, built the way tests/test_ms_m64_registers_cpu.py builds the shipped one:
  - the classification function of the header gives the expected local columns (a static_assert per block column);
  - no spilled VGPR, no scratch at two waves per SIMD;
  - the kernel holds one ds_add_f64 per edge that is neither local nor the first of its block column (65 for the shipped code:
    112 edges, 32 first ones, 15 further edges of the dual diagonal), straight-line code in which every edge appears once."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from ldpc_testlib import load_base_matrix, relift
from test_gpu_ms_m64_local import CODES, M, local_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not installed")


def _code_struct(H):
    """the `struct Code` that ldpc_jit.hpp writes for a base matrix"""
    rh, nh = H.shape
    rows = [[(k, int(H[j, k]) % M) for k in range(nh) if H[j, k] >= 0] for j in range(rh)]
    wmax = max(len(r) for r in rows)
    seen, first = set(), []
    for r in rows:
        first.append([0 if k in seen else 1 for k, _ in r])   # a block column appears once per row
        seen.update(k for k, _ in r)

    def tab(vals):
        return "{" + ", ".join("{" + ", ".join(str(v) for v in row + [0] * (wmax - len(row))) + "}" for row in vals) + "}"

    return (f"struct Code {{\n    static constexpr int RH = {rh}, NH = {nh}, M = {M}, WMAX = {wmax};\n"
            f"    static constexpr int RW[{rh}] = {{{', '.join(str(len(r)) for r in rows)}}};\n"
            f"    static constexpr int COL[{rh}][{wmax}] = {tab([[k for k, _ in r] for r in rows])};\n"
            f"    static constexpr int SH[{rh}][{wmax}] = {tab([[c for _, c in r] for r in rows])};\n"
            f"    static constexpr int FIRST[{rh}][{wmax}] = {tab(first)};\n}};\n")


def _metadata(asm, key):
    m = re.search(r"^\s*" + re.escape(key) + r":\s*(\d+)\s*$", asm, re.M)
    assert m, f"{key} not in the kernel's metadata"
    return int(m.group(1))


def _compile(tmp_path, code, code_name, H):
    csrc = os.path.join(ROOT, "ldpc-lib_amd", "csrc")
    loc = local_columns(H)
    checks = "".join(f"static_assert(ldpc_spec::ms_m64_local_col<{code_name}>({k}) == {'true' if k in loc else 'false'}, \"block column {k}\");\n"
                     for k in range(H.shape[1]))
    src = tmp_path / "k.hip"
    src.write_text(f'#include "{csrc}/ldpc_spec.hpp"\n#include "{csrc}/code_appendix_c_m64.hpp"\n{code}{checks}'
                   'extern "C" __global__ void __launch_bounds__(64, 2) k(const ldpc_spec::SpecArgs a) '
                   f'{{ ldpc_spec::ms_m64_body<{code_name}>(a); }}\n')
    out = tmp_path / "k.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                           str(src), "-o", str(out)], stderr=subprocess.DEVNULL)
    return out.read_text()


def _atomics_expected(H):
    loc = local_columns(H)
    edges = int((H >= 0).sum())
    local_edges = int((H[:, loc] >= 0).sum())
    first_of_others = sum(1 for k in range(H.shape[1]) if k not in loc and (H[:, k] >= 0).any())
    return edges - local_edges - first_of_others


@needs_hipcc
@pytest.mark.parametrize("case", ["shipped_16x32", "hand_written_3x6"])
def test_local_columns_are_classified_fit_the_registers_and_cost_no_atomic(case, tmp_path):
    H = CODES[case]()
    if case == "shipped_16x32":
        assert np.array_equal(H, relift(load_base_matrix(), M))
        asm = _compile(tmp_path, "", "ldpc_spec::CodeAppendixCM64", H)
        assert _atomics_expected(H) == 65
    else:
        asm = _compile(tmp_path, _code_struct(H), "Code", H)
        assert _atomics_expected(H) == 13 - 4 - 4
    got = {k: _metadata(asm, k) for k in (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size")}
    adds = len(re.findall(r"^\s+ds_add_f64\s", asm, re.M))
    print(got, "ds_add_f64", adds)
    assert got[".vgpr_spill_count"] == 0, got
    assert got[".private_segment_fixed_size"] == 0, got
    assert got[".vgpr_count"] <= 256, got
    assert adds == _atomics_expected(H), (adds, _atomics_expected(H))
