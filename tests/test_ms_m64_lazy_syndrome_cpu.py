"""CPU: the shipped instances of ms_m64_body form the syndrome of their filter rows only, in registers that they have.

Both shipped instances (with and without soft values) are cross-compiled twice in one translation unit through the body's FRSET
switch: as shipped, and with every block row forming its syndrome word inside STATE3 (FRSET = RH, the body of the round before).
Asserted on the assembly, in the blocks tools/isa_histogram.py counts (every block of a loop: the iterations, the on-demand pass,
the frame prologue and the outputs):

  - no spilled VGPR, no scratch, at most 256 VGPRs -- for all four;
  - the rule for the filter rows, restated, against the header's constants;
  - v_xor_b32 + v_or_b32 of the shipped instance are fewer than those of the FRSET = RH instance by at least the syndrome
    instructions of the rows past the filter.  A block row of weight RW has RW - 1 xors (the first edge's word starts the chain) and
    one or into the word of the vote: RW per row, the number of EDGES past the filter in all, 98 of the shipped code's 112 at two
    filter rows.  (Edges plus rows, 112, do not exist to remove: the instance with every row has 96 xors and 15 ors for 112
    edges in 16 rows -- the first row's or is a copy.  Measured: 290 -> 192 in both instances.)  The
    on-demand pass is inside the counted blocks: it must not bring the instructions back, and it does not -- its xors and ors are
    scalar.

Only these two mnemonics and the resource metadata are counted.  Needs hipcc, no GPU."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from ldpc_testlib import load_base_matrix, relift

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ldpc-lib_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FILTER_ROWS = 2   # kMsM64FilterRows
EXIT_ROWS = 4     # kMsM64ExitRows


def filter_rows(rh):
    """ms_m64_filter_rows"""
    return min(FILTER_ROWS, rh)


def _asm(tmp_path, soft):
    tag = "soft" if soft else "hard"
    flag = "true" if soft else "false"
    src, out = tmp_path / f"k_{tag}.hip", tmp_path / f"k_{tag}.s"
    body = "ldpc_spec::ms_m64_body<ldpc_spec::CodeAppendixCM64, 1 << 30, ldpc_spec::kMsM64YDepth, -1, -1, " + flag + ", -1, -1, {fr}>(a);"
    src.write_text(f'#include "{CSRC}/ldpc_spec.hpp"\n#include "{CSRC}/code_appendix_c_m64.hpp"\n'
                   'extern "C" __global__ void __launch_bounds__(64, 2) k_shipped(const ldpc_spec::SpecArgs a) { ' + body.format(fr=-1) + ' }\n'
                   'extern "C" __global__ void __launch_bounds__(64, 2) k_every_row(const ldpc_spec::SpecArgs a) { '
                   + body.format(fr="ldpc_spec::CodeAppendixCM64::RH") + ' }\n')
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                           str(src), "-o", str(out)], stderr=subprocess.DEVNULL)
    return out.read_text()


def _function(asm, name):
    """the lines of one kernel's code"""
    lines = asm.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def _xor_or_in_loops(lines):
    """tools/isa_histogram.py's blocks -- every block whose label carries a "Loop" annotation -- and of those the two mnemonics"""
    n, in_loop = 0, False
    for l in lines:
        if re.match(r"^\.LBB\d+_\d+:", l):
            in_loop = "Loop" in l
            continue
        m = re.match(r"^\s+([a-z_0-9]+)\s", l)
        if in_loop and m and re.fullmatch(r"v_(xor|or)_b32(_e32|_e64)?", m.group(1)):
            n += 1
    return n


def _metadata(asm, name):
    """resource figures of one kernel from the code object's metadata"""
    entries = re.split(r"^  - (?=\.)", asm[asm.index("amdhsa.kernels:"):], flags=re.M)
    mine = [e for e in entries if re.search(r"^\s*\.name:\s*" + re.escape(name) + r"\s*$", e, re.M)]
    assert len(mine) == 1, (name, len(mine))
    return {k: int(re.search(r"^\s*" + re.escape(k) + r":\s*(\d+)\s*$", mine[0], re.M).group(1))
            for k in (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size")}


def test_the_rule_for_the_filter_rows_is_the_headers():
    text = open(os.path.join(CSRC, "ldpc_spec.hpp")).read()
    assert re.search(r"constexpr int kMsM64FilterRows = (\d+), kMsM64ExitRows = (\d+);", text).groups() == (str(FILTER_ROWS), str(EXIT_ROWS))
    assert "constexpr int ms_m64_filter_rows() { return kMsM64FilterRows < C::RH ? kMsM64FilterRows : C::RH; }" in text
    assert [filter_rows(rh) for rh in (1, 2, 3, 16, 30)] == [1, 2, 2, 2, 2]


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not installed")
def test_the_shipped_instances_lose_the_syndrome_of_the_rows_past_the_filter_and_spill_nothing(tmp_path):
    H = relift(load_base_matrix(), 64)
    rh = H.shape[0]
    fr = filter_rows(rh)
    edges_past = int((H[fr:] >= 0).sum())
    assert (rh, fr, int((H >= 0).sum()), edges_past) == (16, 2, 112, 98)
    with ThreadPoolExecutor(max_workers=2) as ex:
        asm = dict(zip((True, False), ex.map(lambda soft: _asm(tmp_path, soft), (True, False))))
    for soft in (True, False):
        for name in ("k_shipped", "k_every_row"):
            got = _metadata(asm[soft], name)
            print("soft" if soft else "hard", name, got)
            assert got[".vgpr_spill_count"] == 0 and got[".private_segment_fixed_size"] == 0 and got[".vgpr_count"] <= 256, (soft, name, got)
        shipped, every = (_xor_or_in_loops(_function(asm[soft], n)) for n in ("k_shipped", "k_every_row"))
        print("soft" if soft else "hard", "v_xor_b32 + v_or_b32 in the loops: shipped", shipped, "every row", every, "edges past the filter", edges_past)
        assert shipped <= every - edges_past, (soft, shipped, every, edges_past)
