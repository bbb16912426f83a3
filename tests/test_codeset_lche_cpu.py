"""LCHE code sets (decoder 9, ldpc_hip_open_codes_lche / ldpc_hip_codes_table_lche_host) without a GPU: the exported entry points,
the host-side table against a numpy builder of the record and against the min-sum table, LCHE's limits (block rows and columns are
not limited, a row of weight 1 is legal), the LDS bound with its byte count, the registers of both kernel instances on the
cross-compiled library, and the properties the GPU tests (test_gpu_codeset_lche.py) need of their inputs."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import codeset_lche_sets as S
from codeset_lche_sets import LCHE_DEC, MS_DEC
from ldpc_testlib import ROOT
from test_codeset_cpu import SETS

EINVAL, EUNSUPPORTED = -1, -2
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


def _rc(lib, codes, M):
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    n = C.c_longlong(-1)
    rc = lib.ldpc_hip_codes_table_lche_host(codes.shape[1], codes.shape[2], M, codes.ctypes.data, codes.shape[0], None, None, 0, C.byref(n))
    return rc, lib.ldpc_hip_last_error().decode(), n.value


def test_symbols_header_and_null_arguments(L):
    lib = L.load_library()
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        header = f.read()
    assert hasattr(lib, "ldpc_hip_open_codes_lche") and hasattr(lib, "ldpc_hip_codes_table_lche_host")
    assert re.search(r"\bint\s+ldpc_hip_open_codes_lche\s*\(int rh, int nh, int M, const int16_t \*hd, int C, int device, ldpc_hip_ctx \*\*out\)", header)
    assert re.search(r"\bint\s+ldpc_hip_codes_table_lche_host\s*\(int rh, int nh, int M, const int16_t \*hd, int C, int32_t \*offsets, int32_t \*table,"
                     r"\s*long long capacity,\s*long long \*length\)", header)
    assert re.search(r"#define\s+LDPC_HIP_ABI_VERSION\s+4\b", header) and lib.ldpc_hip_abi_version() == 4
    h = C.c_void_p(123)
    assert lib.ldpc_hip_open_codes_lche(2, 4, 5, None, 1, 0, C.byref(h)) == EINVAL and not h.value     # refused before any device call
    assert lib.ldpc_hip_open_codes_lche(2, 4, 5, None, 1, 0, None) == EINVAL
    ok = np.array(SETS["three 2x4"][1], dtype=np.int16)
    assert lib.ldpc_hip_open_codes_lche(2, 4, 5, ok.ctypes.data, 3, 0, None) == EINVAL


def test_decoder_9_stays_refused_by_the_generic_entry_points(L):
    lib = L.load_library()
    ok = np.array(SETS["three 2x4"][1], dtype=np.int16)
    n = C.c_longlong()
    assert lib.ldpc_hip_codes_table_host(LCHE_DEC, 2, 4, 5, ok.ctypes.data, 3, None, None, 0, C.byref(n)) == EINVAL
    assert "decoder id" in lib.ldpc_hip_last_error().decode()
    h = C.c_void_p(123)
    assert lib.ldpc_hip_open_codes(LCHE_DEC, 2, 4, 5, ok.ctypes.data, 3, 0, C.byref(h)) == EINVAL and not h.value
    assert "decoder id" in lib.ldpc_hip_last_error().decode()
    with pytest.raises(Exception):
        L.codes_table(0, ok, 5)


@pytest.mark.parametrize("name", list(SETS))
def test_table_equals_numpy_and_the_min_sum_table(L, name):
    M, codes = SETS[name]
    codes = np.array(codes, dtype=np.int16)
    off, tab = L.codes_table(LCHE_DEC, codes, M)
    want_off, want_tab = S.table_np(codes)
    assert np.array_equal(off, want_off) and np.array_equal(tab, want_tab)
    ms_off, ms_tab = L.codes_table(MS_DEC, codes, M)           # every one of these sets is within min-sum's limits too
    assert np.array_equal(off, ms_off) and np.array_equal(tab, ms_tab)
    # sizes only, and a buffer that is too small
    lib = L.load_library()
    rc, _, n = _rc(lib, codes, M)
    assert rc == 0 and n == len(want_tab)
    small, o = np.empty(n - 1, dtype=np.int32), np.empty(len(codes), dtype=np.int32)
    assert lib.ldpc_hip_codes_table_lche_host(codes.shape[1], codes.shape[2], M, codes.ctypes.data, len(codes), o.ctypes.data, small.ctypes.data,
                                              n - 1, None) == EINVAL


def test_table_on_the_gpu_sets(L):
    sets = [(c[0], S.code_set(c)) for c in S.CASES] + [S.rows17_set()[:2], S.mixed_weight_set()[:2]]
    sets += [(g["M"], g["codes"]) for g in map(S.golden_set, S.GOLDENS)]
    for M, codes in sets:
        off, tab = L.codes_table(LCHE_DEC, codes, M)
        want_off, want_tab = S.table_np(codes)
        assert np.array_equal(off, want_off) and np.array_equal(tab, want_tab), (M, codes.shape)


def _ring(rh, nh, shifts=3):
    """One rh x nh code, two circulants per block column."""
    H = -np.ones((1, rh, nh), dtype=np.int16)
    for k in range(nh):
        H[0, k % rh, k] = k % shifts
        H[0, (k + 1) % rh, k] = (k + 1) % shifts
    return H


def test_accepted_shapes(L):
    """17 x 34 and 100 x 200 (rh > 16), nh > 32, a row of weight 1, a row of weight 16: all refused by at least one other set kernel.
    300 x 600 is not refused for its block rows or columns either, but no 300 x 600 code fits the fp64 LDS image: a workgroup holds
    at least 33 checks per block row (M * floor(64 / M) >= 33) and a code without an empty block column at least 600 circulants, so
    8 * 33 * (600 + 600) = 316 800 bytes at the very least.  What the builder says about it is the byte count."""
    lib = L.load_library()
    for rh, nh, M in ((17, 34, 3), (100, 200, 33), (8, 40, 3)):   # 100 x 200 at M = 33: 8 * 33 * (200 + 400) + 2496 = 160 896 bytes
        H = _ring(rh, nh)
        rc, msg, n = _rc(lib, H, M)
        assert rc == 0 and n == rh + 1 + int((H >= 0).sum()), (rh, nh, msg)
        assert np.array_equal(L.codes_table(LCHE_DEC, H, M)[1], S.table_np(H)[1])
    H = _ring(300, 600)
    rc, msg, _ = _rc(lib, H, 33)
    assert S.lds_bytes(H, 33) == 8 * 33 * (600 + 1200) + 2496 == 477696
    assert rc == EUNSUPPORTED and "477696" in msg and "rh" not in msg and "block rows" not in msg, msg
    n = C.c_longlong()
    H = _ring(17, 34)
    assert lib.ldpc_hip_codes_table_host(MS_DEC, 17, 34, 3, H.ctypes.data, 1, None, None, 0, C.byref(n)) == EINVAL   # min-sum keeps its 16 rows
    M, codes = SETS["two 3x5 M=100"]                                    # a weight-1 row
    codes = np.array(codes, dtype=np.int16)
    assert ((codes >= 0).sum(axis=2) == 1).any() and _rc(lib, codes, M)[0] == 0
    assert _rc(lib, np.zeros((2, 2, 16), dtype=np.int16), 2)[0] == 0    # rows of weight 16
    M, codes, _ = S.mixed_weight_set()
    w = (codes >= 0).sum(axis=2)
    assert all(16 in row and 1 in row for row in w.tolist()) and _rc(lib, codes, M)[0] == 0
    assert _rc(lib, np.zeros((1, 2, 4), dtype=np.int16), 512)[0] == 0   # a 2 x 4 code at M = 512


def test_refusals(L):
    lib = L.load_library()
    ok = np.array(SETS["three 2x4"][1], dtype=np.int16)
    assert _rc(lib, ok, 5)[0] == 0
    rc, msg, _ = _rc(lib, np.zeros((1, 2, 4), dtype=np.int16), 513)                  # M = 513
    assert rc == EINVAL and "513" in msg, msg
    wide = np.zeros((2, 2, 17), dtype=np.int16)                                     # row weight 17, in code 1 only
    wide[0, :, 16] = -1; wide[0, 0, 16] = 0; wide[0, 0, 0] = -1
    rc, msg, _ = _rc(lib, wide, 2)
    assert rc == EINVAL and "code 1" in msg and "row 0" in msg and "weight 17" in msg, msg
    bad = ok.copy(); bad[1, 0, :] = -1                                               # an empty block row
    rc, msg, _ = _rc(lib, bad, 5)
    assert rc == EINVAL and "code 1" in msg and "row 0" in msg, msg
    bad = ok.copy(); bad[2, :, 2] = -1                                               # an empty block column
    rc, msg, _ = _rc(lib, bad, 5)
    assert rc == EINVAL and "code 2" in msg and "column 2" in msg, msg
    for v in (5, -2):                                                                # a shift of M and a shift of -2
        bad = ok.copy(); bad[2, 1, 0] = v
        rc, msg, _ = _rc(lib, bad, 5)
        assert rc == EINVAL and "code 2" in msg and "(1, 0)" in msg and str(v) in msg, msg
    for Cn in (0, -3):
        n = C.c_longlong()
        assert lib.ldpc_hip_codes_table_lche_host(2, 4, 5, ok.ctypes.data, Cn, None, None, 0, C.byref(n)) == EINVAL
        assert "C = %d" % Cn in lib.ldpc_hip_last_error().decode()


def test_lds_bound(L):
    lib = L.load_library()
    big = S.big_image_set()
    assert big.shape == (1, 16, 32) and int((big >= 0).sum()) == 112
    want = 8 * (16384 + 112 * 512) + 8 * 310 + 16
    assert S.lds_bytes(big, 512) == want == 592320
    rc, msg, _ = _rc(lib, big, 512)
    assert rc == EUNSUPPORTED and str(want) in msg, msg
    # the formula at the two shapes of the timing tool
    from ldpc_testlib import load_base_matrix, relift
    base = load_base_matrix()
    H = np.where(base >= 0, relift(base, 64) % 64, -1).astype(np.int16)[None]
    assert S.lds_bytes(H, 64) == 76224 and _rc(lib, H, 64)[0] == 0
    g = S.golden_set("lche_30x60_m67_2p0")
    assert g["codes"].shape == (5, 30, 60) and g["M"] == 67 and int((g["codes"][0] >= 0).sum()) == 206
    assert S.lds_bytes(g["codes"], 67) == 145072 and _rc(lib, g["codes"], 67)[0] == 0
    # the largest code of a set decides, wherever it stands: 16 x 32 at M = 512 with two circulants per column is 395 712 bytes, too
    # large as well, so the pair is built at M = 128: 112 circulants need 8 * (4096 + 14336) + 2496 = 149 952 bytes, 160 of them
    # 8 * (4096 + 20480) + 2496 = 199 104
    fits = np.where(base >= 0, relift(base, 128) % 128, -1).astype(np.int16)
    more = fits.copy()
    for j in range(16):                       # three more circulants in every block row
        more[j, np.flatnonzero(more[j] < 0)[:3]] = 1
    assert int((more >= 0).sum()) == 160 and (more >= 0).sum(axis=1).max() <= 16
    assert S.lds_bytes(fits[None], 128) == 149952 and _rc(lib, fits[None], 128)[0] == 0
    for pair in ([fits, more], [more, fits]):
        rc, msg, _ = _rc(lib, np.stack(pair), 128)
        assert rc == EUNSUPPORTED and "199104" in msg, msg


@pytest.mark.parametrize("case", list(S.CASES), ids=S.CASE_IDS)
def test_gpu_inputs_have_the_required_properties(case):
    """What test_gpu_codeset_lche.py relies on, asserted here so that nothing is searched at GPU time: in both layouts the model
    alone takes both exits of the iteration loop."""
    M, rh, nh = case
    r = S.reference(case)
    codes = r["codes"]
    assert codes.shape == (S.NCODES, rh, nh)
    w = (codes >= 0).sum(axis=2)
    assert w.min() >= 1 and w.max() <= 16 and ((codes >= 0).sum(axis=1) >= 1).all()
    assert len({(H >= 0).tobytes() for H in codes}) == S.NCODES
    assert S.lds_bytes(codes, M) <= S.LDS_LIMIT
    for layout in ("shared", "percode"):
        its = np.array([x[1] for x in r["ref"][layout]])
        assert ((its > 1) & (its < S.MAXITER)).any(), (case, layout, r["snr"], its)
        assert (its == -S.MAXITER).any(), (case, layout, r["snr"], its)
        assert ((its == -S.MAXITER) | ((its >= 0) & (its <= S.MAXITER))).all()


def test_the_model_reproduces_the_goldens():
    for name in S.GOLDENS:
        g = S.golden(name)
        hard, it, soft = S.model(g["H"], g["M"], g["llr"], g["maxiter"])
        assert np.array_equal(it, g["iters"]) and np.array_equal(hard, g["hard"]), name
        assert np.array_equal(soft.view(np.uint64), g["soft"].view(np.uint64)), name
        gs = S.golden_set(name)
        assert gs["codes"].shape[0] == S.NCODES and S.lds_bytes(gs["codes"], gs["M"]) <= S.LDS_LIMIT
        assert len({H.tobytes() for H in gs["codes"]}) == (S.NCODES if g["M"] > 1 else 1), name
    assert ((S.golden("lche_rw1_m32_2p5")["H"] >= 0).sum(axis=1) == 1).any(), "a row of weight 1"


def test_other_gpu_inputs():
    for B in (1, 4):
        M, codes, llr = S.boundary_set(B)
        assert S.lds_bytes(codes, M) <= S.LDS_LIMIT
        out = [S.model(codes[c], M, llr[c], S.MAXITER) for c in range(3)]
        assert (out[1][1] == 0).all() and (out[0][1] == -S.MAXITER).all() and (out[2][1] == -S.MAXITER).all(), [o[1] for o in out]
        zeros = (llr[1] == 0) & np.signbit(llr[1])
        assert zeros.sum() == B + 1, "-0.0 among the codeword frames' LLRs"
        assert np.array_equal(out[1][2].view(np.uint64), llr[1].view(np.uint64)) and (out[1][0] == 0).all()
    codes, llr = S.maxiter_one_set()
    assert set(np.unique([S.model(codes[c], 20, llr, 1)[1] for c in range(S.NCODES)])) == {-1, 1}
    codes = S.simulate_set()
    assert len({(H >= 0).tobytes() for H in codes}) == S.SIM["C"]
    weak = S.stop_set()[0]
    assert len(S.stop_set()) == 3 and ((weak >= 0).sum(axis=0) == 1).all(), "code 0 of the stopping-rule set: block columns of weight 1"
    M, codes, _ = S.rows17_set()
    assert codes.shape == (S.NCODES, 17, 34) and ((codes >= 0).sum(axis=2) >= 1).all() and ((codes >= 0).sum(axis=1) >= 1).all()
    assert (codes >= 0).sum(axis=2).max() <= 16 and S.lds_bytes(codes, M) <= S.LDS_LIMIT
    M, codes, _ = S.mixed_weight_set()
    assert ((codes >= 0).sum(axis=1) >= 1).all() and S.lds_bytes(codes, M) <= S.LDS_LIMIT


def _kernel_metadata(asm):
    """name -> {key: value} of every kernel in the assembly's amdhsa metadata."""
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", asm)[1:]:
        name = re.search(r"\.name:\s*(\S+)", blk)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s*(\d+)\s*$", blk, re.M)}
    return out


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not installed")
def test_both_instances_have_no_scratch_and_no_spill(tmp_path):
    """The kernel keeps u[16] and p[16] of a layer in VGPRs; a compiler or header change that sent them to scratch memory would fail
    no result check.  Asserted on the cross-compiled one-kernel translation unit, the way test_ms_m64_registers_cpu.py does."""
    csrc = os.path.join(ROOT, "ldpc-lib_amd", "csrc")
    src = tmp_path / "k.hip"
    src.write_text(f'#include "{csrc}/ldpc_codeset.hpp"\n'
                   "template __global__ void ldpc::lche_layered_codes_kernel<16, false>(const ldpc::CodesetArgs);\n"
                   "template __global__ void ldpc::lche_layered_codes_kernel<16, true>(const ldpc::CodesetArgs);\n")
    out = tmp_path / "k.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           "--cuda-device-only", "-S", str(src), "-o", str(out)], stderr=subprocess.DEVNULL)
    meta = {k: v for k, v in _kernel_metadata(out.read_text()).items() if "lche_layered_codes_kernel" in k}
    print(meta)
    assert len(meta) == 2, list(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 256, (name, m)
