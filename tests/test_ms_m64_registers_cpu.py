"""CPU: the shipped flagship instance of ms_m64_body (CodeAppendixCM64, two waves per SIMD) must fit its registers.

The body keeps decoded check-to-variable values in registers from STATE1 to STATE3, as many as an edge budget allows; the budget
was chosen as the largest that compiles without a spill.  A compiler or header change that pushes the kernel over 256 VGPRs would
not fail any result check -- it would spill to scratch and run at a fraction of the speed -- so the limits are asserted here on the
cross-compiled one-kernel translation unit, the way tools/isa_histogram.py builds it.  Needs hipcc, no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _metadata(asm, key):
    m = re.search(r"^\s*" + re.escape(key) + r":\s*(\d+)\s*$", asm, re.M)
    assert m, f"{key} not in the kernel's metadata"
    return int(m.group(1))


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not installed")
def test_shipped_ms_m64_instance_has_no_spills_at_two_waves_per_simd(tmp_path):
    csrc = os.path.join(ROOT, "ldpc-lib_amd", "csrc")
    src = tmp_path / "k.hip"
    src.write_text(f'#include "{csrc}/ldpc_spec.hpp"\n#include "{csrc}/code_appendix_c_m64.hpp"\n'
                   'extern "C" __global__ void __launch_bounds__(64, 2) k(const ldpc_spec::SpecArgs a) '
                   '{ ldpc_spec::ms_m64_body<ldpc_spec::CodeAppendixCM64>(a); }\n')
    out = tmp_path / "k.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                           str(src), "-o", str(out)], stderr=subprocess.DEVNULL)
    asm = out.read_text()
    got = {k: _metadata(asm, k) for k in (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size")}
    print(got)
    assert got[".vgpr_spill_count"] == 0, got
    assert got[".private_segment_fixed_size"] == 0, got
    assert got[".vgpr_count"] <= 256, got
