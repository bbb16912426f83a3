"""CPU: the block rows ms_m64_body carries once STATE2 streams its channel loads, on cross-compiled one-kernel translation units.

STATE2 of the body loads the channel values of the non-local block columns as a stream, kMsM64YDepth ahead; the registers that are
no longer in flight pay for further carried rows, ms_m64_carry_rows of ldpc_spec.hpp.  Checked here, built the way
tests/test_ms_m64_local_cpu.py builds its instances (needs hipcc, no GPU):

  - carry_rows of test_gpu_ms_m64_allrows.py restates that rule; a static_assert per code holds the restatement against the header's
    functions: the shipped code, the hand-written 3 x 6, a 14 x 28 and a 30 x 60;
  - every one of these instances: no spilled VGPR, no scratch, at most 256 VGPRs, the parent's number of ds_add_f64;
  - the shipped instance carries 15 of its 16 block rows (all 16 spill 6 VGPRs: profiles/r25_flagship_isa_histogram.txt); were it
    16, its iteration loop would hold no v_cmp_eq_u32_sdwa and no v_cmp_lt_f64 (the decode of a record);
  - round 20's pair ms_m64_keep_rows(ms_m64_keep_budget()) still gives 13 for the shipped code."""
import re

import pytest

from test_gpu_ms_m64_allrows import DEPTH, STATE3_REGS, carry_rows, nonlocal_columns, state3_regs, y_in_flight_r23
from test_gpu_ms_m64_carry import _thirty_rows
from test_gpu_ms_m64_eqslot import _record_rows_last, _shipped, carried_rows
from test_gpu_ms_m64_local import _hand_written
from test_ms_m64_local_cpu import _atomics_expected, _code_struct, _compile, _metadata, needs_hipcc

SHAPES = {"shipped_16x32": _shipped, "hand_written_3x6": _hand_written, "record_rows_last_14x28": _record_rows_last,
          "no_row_carried_30x60": _thirty_rows}
SHIPPED_ROWS = 15


def test_the_restated_rule_on_the_four_codes():
    assert (DEPTH, STATE3_REGS) == (8, 244)
    assert {case: (carried_rows(make()), carry_rows(make())) for case, make in SHAPES.items()} == {
        "shipped_16x32": (13, SHIPPED_ROWS), "hand_written_3x6": (3, 3), "record_rows_last_14x28": (9, 10), "no_row_carried_30x60": (0, 0)}
    H = _shipped()
    assert carry_rows(H, depth=32) == 13          # every load at once gives nothing back
    assert carry_rows(H, depth=4) == SHIPPED_ROWS  # a shallower stream pays for more, STATE3 does not fit more


def _loop_count(asm, mnemonic):
    """occurrences in the basic blocks that carry a Loop annotation (tools/isa_histogram.py)"""
    n, in_loop = 0, False
    for line in asm.splitlines():
        if re.match(r"^\.LBB\d+_\d+:", line):
            in_loop = "Loop" in line
        elif re.match(r"^\.Lfunc_end", line):
            in_loop = False
        elif in_loop and re.match(r"^\s+" + re.escape(mnemonic), line):
            n += 1
    return n


@needs_hipcc
@pytest.mark.parametrize("case", list(SHAPES))
def test_streamed_loads_and_carried_rows_fit_the_registers_and_change_no_atomic(case, tmp_path):
    H = SHAPES[case]()
    name = "ldpc_spec::CodeAppendixCM64" if case == "shipped_16x32" else "Code"
    nl, kr = nonlocal_columns(H), carry_rows(H)
    rule = (f"static_assert(ldpc_spec::kMsM64YDepth == {DEPTH} && ldpc_spec::kMsM64State3Regs == {STATE3_REGS}, \"constants\");\n"
            f"static_assert(ldpc_spec::ms_m64_nonlocal_cols<{name}>() == {len(nl)}, \"non-local block columns\");\n"
            + "".join(f"static_assert(ldpc_spec::ms_m64_nonlocal_col<{name}>({n}) == {k}, \"non-local block column {n}\");\n"
                      for n, k in enumerate(nl + [-1]))
            + f"static_assert(ldpc_spec::ms_m64_y_in_flight_r23<{name}>() == {y_in_flight_r23(H)}, \"in flight before\");\n"
            + "".join(f"static_assert(ldpc_spec::ms_m64_state3_regs<{name}>({r}) == {state3_regs(H, r)}, \"STATE3 with {r} carried rows\");\n"
                      for r in range(H.shape[0] + 1))
            + "".join(f"static_assert(ldpc_spec::ms_m64_carry_rows<{name}, {d}>() == {carry_rows(H, depth=d)}, \"carried rows at depth {d}\");\n"
                      for d in (1, 4, DEPTH, 12, 32))
            + f"static_assert(ldpc_spec::ms_m64_keep_rows<{name}>(ldpc_spec::ms_m64_keep_budget<{name}>()) == {carried_rows(H)}, \"round 20's rows\");\n")
    asm = _compile(tmp_path, ("" if case == "shipped_16x32" else _code_struct(H)) + rule, name, H)
    got = {k: _metadata(asm, k) for k in (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size")}
    adds = len(re.findall(r"^\s+ds_add_f64\s", asm, re.M))
    print(case, got, "ds_add_f64", adds, "carried rows", kr)
    assert got[".vgpr_spill_count"] == 0, got
    assert got[".private_segment_fixed_size"] == 0, got
    assert got[".vgpr_count"] <= 256, got
    assert adds == _atomics_expected(H) == {"shipped_16x32": 65, "hand_written_3x6": 5, "record_rows_last_14x28": 73,
                                            "no_row_carried_30x60": 58}[case], adds
    if case == "shipped_16x32":
        assert carried_rows(H) == 13 and kr == SHIPPED_ROWS
        record_decodes = (_loop_count(asm, "v_cmp_eq_u32_sdwa"), _loop_count(asm, "v_cmp_lt_f64"))
        print("in the loop: v_cmp_eq_u32_sdwa, v_cmp_lt_f64", record_decodes)
        if kr == 16:
            assert record_decodes == (0, 0), record_decodes
        else:
            assert record_decodes[0] <= 35 - 10 * (kr - 13) and record_decodes[1] <= 17 - 5 * (kr - 13), record_decodes
