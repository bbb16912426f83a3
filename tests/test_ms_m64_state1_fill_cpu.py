"""CPU: the shipped instances of ms_m64_body with part of STATE3's arithmetic among STATE1's LDS operations, in registers they have.

Both shipped instances (with and without soft values) are cross-compiled twice in one translation unit through the body's S1SET
switch: with the switch off (0, the body of the round before) and as shipped (-1: kMsM64State1Fill).  Asserted on the assembly:

  - no spilled VGPR, no scratch, at most 256 VGPRs -- for all four;
  - v_mul_f64 and v_add_f64 in the blocks tools/isa_histogram.py counts (every block of a loop) do not increase: the work is
    moved, not duplicated;
  - the products stand where the rule says.  The rule, restated from H: one product x = keep * |alpha| per edge of a carried row
    that goes through LDS (level 1: 75 on the shipped code), and for every local column that STATE1 fills (level 2) one product
    pr = acc * alpha and one per edge.  Counted from the head of the iteration loop to its last ds_add_f64 -- STATE1, whose last LDS
    operations on the shipped code are the atomics of block row 15, which keeps its record -- there are at least that many
    v_mul_f64, and with the switch off there is none.  (The span "between the first and the last ds_add_f64" is printed beside
    it.  It cannot hold all of them: block row 0 of the shipped code and the first two edges of block row 1 are FIRST stores,
    ds_write_b64, in front of the first atomic, and their 9 products stand right behind them: 66 of 75 at level 1.);
  - the rule for which local columns move, restated in test_gpu_ms_m64_state1_fill.py, against the header's on the shipped code
    and on the 14 x 28 whose dual diagonal straddles the carried rows, as static_asserts.

Needs hipcc, no GPU."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

from test_gpu_ms_m64_allrows import carry_rows
from test_gpu_ms_m64_eqslot import _record_rows_last
from test_gpu_ms_m64_local import _shipped, local_columns
from test_gpu_ms_m64_state1_fill import fill_columns, filter_rows
from test_ms_m64_lazy_syndrome_cpu import _function, _metadata
from test_ms_m64_local_cpu import HIPCC, ROOT, _code_struct, needs_hipcc

CSRC = os.path.join(ROOT, "ldpc-lib_amd", "csrc")


def shipped_level():
    """kMsM64State1Fill"""
    return int(re.search(r"constexpr int kMsM64State1Fill = (\d+),", open(os.path.join(CSRC, "ldpc_spec.hpp")).read()).group(1))


def products_in_state1(H, level):
    """v_mul_f64 that the rule puts among STATE1's LDS operations"""
    kr, loc = carry_rows(H), local_columns(H)
    n = 0
    if level >= 1:
        n += sum(1 for j in range(kr) for k in range(H.shape[1]) if H[j, k] >= 0 and k not in loc)
    if level >= 2:
        n += sum(1 + int((H[:, k] >= 0).sum()) for k in fill_columns(H))
    return n


def test_the_rule_counts_what_the_issue_counted_on_the_shipped_code():
    H = _shipped()
    assert int((H >= 0).sum()) == 112 and carry_rows(H) == 15 and filter_rows(H) == 2
    assert products_in_state1(H, 0) == 0 and products_in_state1(H, 1) == 75    # 82 edges that are not local, less the 7 of block row 15
    assert fill_columns(H) == list(range(2, 14)) and products_in_state1(H, 2) == 75 + 12 * 3
    assert shipped_level() in (0, 1, 2)


def _asm(tmp_path, soft):
    tag = "soft" if soft else "hard"
    flag = "true" if soft else "false"
    src, out = tmp_path / f"k_{tag}.hip", tmp_path / f"k_{tag}.s"
    body = "ldpc_spec::ms_m64_body<ldpc_spec::CodeAppendixCM64, 1 << 30, ldpc_spec::kMsM64YDepth, -1, -1, " + flag + ", -1, -1, -1, -1, {s1}>(a);"
    src.write_text(f'#include "{CSRC}/ldpc_spec.hpp"\n#include "{CSRC}/code_appendix_c_m64.hpp"\n'
                   'extern "C" __global__ void __launch_bounds__(64, 2) k_shipped(const ldpc_spec::SpecArgs a) { ' + body.format(s1=-1) + ' }\n'
                   'extern "C" __global__ void __launch_bounds__(64, 2) k_off(const ldpc_spec::SpecArgs a) { ' + body.format(s1=0) + ' }\n')
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                           str(src), "-o", str(out)], stderr=subprocess.DEVNULL)
    return out.read_text()


def _mnemonics(lines):
    """(in a block of a loop, in the iteration loop, mnemonic) of every instruction, in layout order"""
    out, in_loop, inner, label = [], False, False, False
    for l in lines:
        if re.match(r"^\.LBB\d+_\d+:", l):
            in_loop, inner, label = "Loop" in l, "Depth=2" in l, True
            continue
        if label and l.lstrip().startswith(";"):
            inner = inner or "Loop Header: Depth=2" in l   # the header's annotation runs over several lines
            continue
        label = False
        m = re.match(r"^\s+([a-z_0-9]+)\s", l)
        if m and not l.strip().startswith((".", ";")):
            out.append((in_loop, inner, m.group(1)))
    return out


def _count(seq, prefix):
    return sum(1 for m in seq if m.startswith(prefix))


def _figures(lines):
    ins = _mnemonics(lines)
    loops = [m for in_loop, _, m in ins if in_loop]
    # the iteration loop from its header on, in layout order (blocks the compiler placed in front of the header are its cold ends)
    head = next(i for i, l in enumerate(lines) if "Loop Header: Depth=2" in l)
    while not re.match(r"^\.LBB\d+_\d+:", lines[head]):   # (the annotation runs over several lines behind the label)
        head -= 1
    body = [m for _, inner, m in _mnemonics(lines[head:]) if inner]
    adds = [i for i, m in enumerate(body) if m == "ds_add_f64"]
    return {"v_mul_f64": _count(loops, "v_mul_f64"), "v_add_f64": _count(loops, "v_add_f64"),
            "to the last atomic": _count(body[:adds[-1]], "v_mul_f64"), "between the atomics": _count(body[adds[0]:adds[-1]], "v_mul_f64")}


@needs_hipcc
def test_the_shipped_instances_hold_the_products_in_state1_and_spill_nothing(tmp_path):
    H = _shipped()
    want = products_in_state1(H, shipped_level())
    with ThreadPoolExecutor(max_workers=2) as ex:
        asm = dict(zip((True, False), ex.map(lambda soft: _asm(tmp_path, soft), (True, False))))
    for soft in (True, False):
        fig = {}
        for name in ("k_shipped", "k_off"):
            got = _metadata(asm[soft], name)
            fig[name] = _figures(_function(asm[soft], name))
            print("soft" if soft else "hard", name, got, fig[name])
            assert got[".vgpr_spill_count"] == 0 and got[".private_segment_fixed_size"] == 0 and got[".vgpr_count"] <= 256, (soft, name, got)
        for mnemonic in ("v_mul_f64", "v_add_f64"):
            assert fig["k_shipped"][mnemonic] <= fig["k_off"][mnemonic], (soft, mnemonic, fig)
        assert fig["k_off"]["to the last atomic"] == 0 and fig["k_off"]["between the atomics"] == 0, (soft, fig)
        assert fig["k_shipped"]["to the last atomic"] >= want, (soft, want, fig)


@needs_hipcc
def test_the_restated_rule_for_the_columns_that_move_equals_the_header(tmp_path):
    text = ""
    for name, H in (("ldpc_spec::CodeAppendixCM64", _shipped()), ("Code", _record_rows_last())):
        if name == "Code":
            text += _code_struct(H)
        kr, fr, fill = carry_rows(H), filter_rows(H), fill_columns(H)
        text += f"static_assert(ldpc_spec::ms_m64_carry_rows<{name}, ldpc_spec::kMsM64YDepth>() == {kr} && ldpc_spec::ms_m64_filter_rows<{name}>() == {fr}, \"rows\");\n"
        text += f"static_assert(ldpc_spec::ms_m64_fill_cols<{name}>({kr}, {fr}) == {len(fill)}, \"columns that move\");\n"
        for k in range(H.shape[1]):
            text += f"static_assert(ldpc_spec::ms_m64_fill_col<{name}>({k}, {kr}, {fr}) == {'true' if k in fill else 'false'}, \"block column {k}\");\n"
            text += f"static_assert(!ldpc_spec::ms_m64_fill_col<{name}>({k}, 0, {fr}), \"nothing moves where nothing is carried\");\n"
        # the bit word takes the columns that move first, then the others, each in the order of their first block rows
        first = {k: int((H[:, k] >= 0).argmax()) for k in local_columns(H)}
        order = sorted(first, key=lambda k: (k not in fill, first[k], k))
        for p, k in enumerate(order):
            text += f"static_assert(ldpc_spec::ms_m64_local_place<{name}>({k}, {kr}, {fr}) == {p}, \"place of block column {k}\");\n"
        for i, k in enumerate(k for k in order if k in fill):
            text += f"static_assert(ldpc_spec::ms_m64_fill_col_at<{name}>({i}, {kr}, {fr}) == {k}, \"column number {i} that moves\");\n"
    src = tmp_path / "rule.hip"
    src.write_text(f'#include "{CSRC}/ldpc_spec.hpp"\n#include "{CSRC}/code_appendix_c_m64.hpp"\n{text}')
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only", str(src)])
