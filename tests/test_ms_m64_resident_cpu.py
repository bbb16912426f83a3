"""CPU: the rule for ms_m64_body's resident channel values and its slot map, held against the header, and the registers of the two
shipped instances, cross-compiled (needs hipcc, no GPU).

  - test_gpu_ms_m64_resident.py restates kMsM64FrameLdsBytes, ms_m64_spare_cols, ms_m64_resident_cols, ms_m64_resident_slot,
    ms_m64_local_place and ms_m64_local_bit in Python; a translation unit of static_asserts per code holds the restatement against
    the header's functions, for every code of that file and for the frame's share at every block-column count the host admits;
  - the figures of the issue: kLdsBudget = 163 776; 32 block columns leave 6 spare columns, 36 leave 2, 38 none, 39 (7 frames per
    CU) 5; the shipped code has 17 resident columns without soft values (all of its non-local ones) and 6 with them;
  - the two shipped instances, as tools/ms_m64_instances.py compiles them: 15 carried rows, no spilled VGPR, no scratch, at most
    256 VGPRs, the same 65 ds_add_f64; the instance without soft values has no channel load inside its iteration loop but the 15 of
    the local columns and 15 LDS stores fewer than the one with them."""
import importlib.util
import os
import re
import subprocess

import pytest

import test_gpu_ms_m64_resident as res
from test_gpu_ms_m64_allrows import carry_rows
from test_gpu_ms_m64_local import local_columns
from test_ms_m64_allrows_cpu import _loop_count
from test_ms_m64_local_cpu import HIPCC, ROOT, _code_struct, needs_hipcc

CSRC = os.path.join(ROOT, "ldpc-lib_amd", "csrc")


def test_the_figures_of_the_rule():
    assert res.LDS_BUDGET == 163776
    assert [res.spare_columns(nh) for nh in (32, 36, 38, 39)] == [6, 2, 0, 5] and res.frames_per_cu(39) == 7
    H = res._shipped()
    assert (res.resident_columns(H, False), res.resident_columns(H, True)) == (17, 6) and len(res.nonlocal_columns(H)) == 17


def _syntax_only(tmp_path, text):
    src = tmp_path / "rule.hip"
    src.write_text(f'#include "{CSRC}/ldpc_spec.hpp"\n#include "{CSRC}/code_appendix_c_m64.hpp"\n{text}')
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only", str(src)])


@needs_hipcc
def test_the_frame_share_equals_the_header_at_every_block_column_count(tmp_path):
    text = f"static_assert(ldpc_spec::kMsM64LdsBudget == {res.LDS_BUDGET} && ldpc_spec::kMsM64FramesPerCu == {res.FRAMES_PER_CU}, \"constants\");\n"
    for nh in range(1, 65):
        text += (f"static_assert(ldpc_spec::kMsM64LdsBytes({nh * 64}) == {res.image_bytes(nh)} && "
                 f"ldpc_spec::kMsM64FrameLdsBytes({nh * 64}) == {res.frame_lds_bytes(nh)}, \"{nh} block columns\");\n")
    _syntax_only(tmp_path, text)


@needs_hipcc
@pytest.mark.parametrize("case", list(res.CODES))
def test_the_restated_rule_and_slot_map_equal_the_header(case, tmp_path):
    H = res.CODES[case]()
    name = "ldpc_spec::CodeAppendixCM64" if case == "shipped_16x32" else "Code"
    text = "" if case == "shipped_16x32" else _code_struct(H)
    text += f"static_assert(ldpc_spec::ms_m64_spare_cols<{name}>() == {res.spare_columns(H.shape[1])}, \"spare\");\n"
    text += f"static_assert(ldpc_spec::ms_m64_local_cols<{name}>() == {len(local_columns(H))}, \"local columns\");\n"
    for soft in (False, True):
        s = "true" if soft else "false"
        text += f"static_assert(ldpc_spec::ms_m64_resident_cols<{name}, {s}>() == {res.resident_columns(H, soft)}, \"resident, soft {s}\");\n"
    # the slot map is one for both instances: a resident column of the instance with soft values never gets past the spare slots
    for i, slot in enumerate(res.resident_slots(H, False)):
        text += f"static_assert(ldpc_spec::ms_m64_resident_slot<{name}>({i}) == {slot}, \"slot of resident column {i}\");\n"
    assert res.resident_slots(H, True) == res.resident_slots(H, False)[:res.resident_columns(H, True)]
    places, bits = res.local_places(H), res.local_bits(H)
    for k in range(H.shape[1]):
        text += f"static_assert(ldpc_spec::ms_m64_local_place<{name}>({k}) == {places.get(k, -1)}, \"place of block column {k}\");\n"
        if k in bits:
            text += f"static_assert(ldpc_spec::ms_m64_local_bit<{name}>({k}) == {bits[k][1]}, \"bit of block column {k}\");\n"
    _syntax_only(tmp_path, text)


def _instances_tool():
    spec = importlib.util.spec_from_file_location("ms_m64_instances", os.path.join(ROOT, "tools", "ms_m64_instances.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _iteration_count(asm, mnemonic):
    """occurrences in the basic blocks of the iteration loop: depth 2, inside the frame loop of the persistent launch"""
    n, inside, label = 0, False, False
    for line in asm.splitlines():
        if re.match(r"^\.LBB\d+_\d+:", line):
            inside, label = "Depth=2" in line, True
        elif label and line.lstrip().startswith(";"):
            inside = inside or "Loop Header: Depth=2" in line   # the header's annotation runs over several lines
        elif re.match(r"^\.Lfunc_end", line):
            inside = label = False
        else:
            label = False
            if inside and re.match(r"^\s+" + re.escape(mnemonic), line):
                n += 1
    return n


@needs_hipcc
def test_the_two_shipped_instances_carry_15_rows_and_spill_nothing():
    tool = _instances_tool()
    H = res._shipped()
    assert tool.BODIES == ("ms_m64_body", "ms_m64_hard_body") and carry_rows(H) == 15
    asm = {body: tool.build_asm(CSRC, H, "", body) for body in tool.BODIES}
    for body in tool.BODIES:
        meta, adds = tool.figures(asm[body])
        print(body, meta, "ds_add_f64", adds)
        assert meta[".vgpr_spill_count"] == 0 and meta[".private_segment_fixed_size"] == 0 and meta[".vgpr_count"] <= 256, (body, meta)
        assert adds == 65, (body, adds)
    soft, hard = asm["ms_m64_body"], asm["ms_m64_hard_body"]
    # 15 carried rows: one block row decodes a record, as in test_ms_m64_allrows_cpu.py
    for asm in (soft, hard):
        assert _loop_count(asm, "v_cmp_eq_u32_sdwa") <= 35 - 10 * 2 and _loop_count(asm, "v_cmp_lt_f64") <= 17 - 5 * 2
    loads = {b: _iteration_count(a, "buffer_load_dwordx2") for b, a in (("soft", soft), ("hard", hard))}
    stores = {b: _iteration_count(a, "ds_write") for b, a in (("soft", soft), ("hard", hard))}
    print("in the iteration loop: channel loads", loads, "ds_write*", stores)
    assert loads["hard"] == 15, loads                 # the local columns' alone: every non-local column is resident
    assert loads["soft"] == 15 + 17 - 6, loads        # 6 resident columns, 11 streamed
    assert stores["hard"] < stores["soft"], stores    # no store per local column
