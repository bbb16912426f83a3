"""Integer min-sum code sets (decoder 4, ldpc_hip_open_codes_ims / ldpc_hip_codes_table_ims_host) without a GPU: the exported entry
points and the binding, the host-side table against a numpy builder of the record and against the min-sum table, the limits (block
rows and columns are not limited, rows of weight 1 .. 16), the LDS bound with its byte count, the scratch memory of the kernels on
the cross-compiled code, and the properties the GPU tests (test_gpu_codeset_ims.py) need of their inputs, against the CPU oracle."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import codeset_ims_sets as S
from codeset_ims_sets import IMS_DEC, MS_DEC
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
    rc = lib.ldpc_hip_codes_table_ims_host(codes.shape[1], codes.shape[2], M, codes.ctypes.data, codes.shape[0], None, None, 0, C.byref(n))
    return rc, lib.ldpc_hip_last_error().decode(), n.value


def test_symbols_header_binding_and_null_arguments(L):
    lib = L.load_library()
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        header = f.read()
    assert hasattr(lib, "ldpc_hip_open_codes_ims") and hasattr(lib, "ldpc_hip_codes_table_ims_host")
    assert re.search(r"\bint\s+ldpc_hip_open_codes_ims\s*\(int rh, int nh, int M, const int16_t \*hd, int C, int device, ldpc_hip_ctx \*\*out\)", header)
    assert re.search(r"\bint\s+ldpc_hip_codes_table_ims_host\s*\(int rh, int nh, int M, const int16_t \*hd, int C, int32_t \*offsets, int32_t \*table,"
                     r"\s*long long capacity,\s*long long \*length\)", header)
    assert re.search(r"#define\s+LDPC_HIP_ABI_VERSION\s+4\b", header) and lib.ldpc_hip_abi_version() == 4
    assert "one stream at a time" in re.sub(r"[\s*]+", " ", header).lower()
    assert callable(L.LdpcHipCodes.set_ims_params) and L.DEC_IMS == IMS_DEC
    h = C.c_void_p(123)
    assert lib.ldpc_hip_open_codes_ims(2, 4, 5, None, 1, 0, C.byref(h)) == EINVAL and not h.value     # refused before any device call
    assert lib.ldpc_hip_open_codes_ims(2, 4, 5, None, 1, 0, None) == EINVAL
    ok = np.array(SETS["three 2x4"][1], dtype=np.int16)
    assert lib.ldpc_hip_open_codes_ims(2, 4, 5, ok.ctypes.data, 3, 0, None) == EINVAL
    n = C.c_longlong()
    assert lib.ldpc_hip_codes_table_ims_host(2, 4, 5, None, 3, None, None, 0, C.byref(n)) == EINVAL
    with open(os.path.join(ROOT, "include", "ldpc", "bp_simulation.h")) as f:
        assert "ldpc_hip_open_codes_ims" in f.read()


@pytest.mark.parametrize("dec", [0, 1, 2, 4, 6, 9])
def test_the_generic_entry_points_still_refuse(L, dec):
    lib = L.load_library()
    ok = np.array(SETS["three 2x4"][1], dtype=np.int16)
    n = C.c_longlong()
    assert lib.ldpc_hip_codes_table_host(dec, 2, 4, 5, ok.ctypes.data, 3, None, None, 0, C.byref(n)) == EINVAL
    assert "decoder id" in lib.ldpc_hip_last_error().decode()
    h = C.c_void_p(123)
    assert lib.ldpc_hip_open_codes(dec, 2, 4, 5, ok.ctypes.data, 3, 0, C.byref(h)) == EINVAL and not h.value
    assert "decoder id" in lib.ldpc_hip_last_error().decode()


@pytest.mark.parametrize("name", list(SETS))
def test_table_equals_numpy_and_the_min_sum_table(L, name):
    M, codes = SETS[name]
    codes = np.array(codes, dtype=np.int16)
    off, tab = L.codes_table(IMS_DEC, codes, M)
    want_off, want_tab = S.table_np(codes)
    assert np.array_equal(off, want_off) and np.array_equal(tab, want_tab)
    ms_off, ms_tab = L.codes_table(MS_DEC, codes, M)           # every one of these sets is within min-sum's limits too
    assert np.array_equal(off, ms_off) and np.array_equal(tab, ms_tab)
    # sizes only, and a buffer that is too small
    lib = L.load_library()
    rc, _, n = _rc(lib, codes, M)
    assert rc == 0 and n == len(want_tab)
    small, o = np.empty(n - 1, dtype=np.int32), np.empty(len(codes), dtype=np.int32)
    assert lib.ldpc_hip_codes_table_ims_host(codes.shape[1], codes.shape[2], M, codes.ctypes.data, len(codes), o.ctypes.data, small.ctypes.data,
                                             n - 1, None) == EINVAL
    assert "room for" in lib.ldpc_hip_last_error().decode()
    assert np.array_equal(o, want_off)                         # offsets alone
    assert lib.ldpc_hip_codes_table_ims_host(codes.shape[1], codes.shape[2], M, codes.ctypes.data, len(codes), None, None, 0, None) == 0


def test_table_on_the_gpu_sets(L):
    sets = [(c[0], S.code_set(c)) for c in S.CASES] + [S.rows17_set()[:2], S.mixed_weight_set()[:2], S.big_set()[:2]]
    sets += [(S.golden_set()["M"], S.golden_set()["codes"]), (S.STOP["M"], S.stop_set()), (S.SIM["M"], S.simulate_set())]
    for M, codes in sets:
        off, tab = L.codes_table(IMS_DEC, codes, M)
        want_off, want_tab = S.table_np(codes)
        assert np.array_equal(off, want_off) and np.array_equal(tab, want_tab), (M, codes.shape)
        if codes.shape[1] <= 16 and codes.shape[2] <= 32:      # where min-sum accepts the shape: the same record
            ms_off, ms_tab = L.codes_table(MS_DEC, codes, M)
            assert np.array_equal(off, ms_off) and np.array_equal(tab, ms_tab), (M, codes.shape)
    n = C.c_longlong()
    M, codes = S.big_set()[:2]
    assert L.load_library().ldpc_hip_codes_table_host(MS_DEC, 30, 60, M, codes.ctypes.data, len(codes), None, None, 0, C.byref(n)) == EINVAL


def test_accepted_shapes(L):
    """No bound on rh or nh; rows of weight 1 and of weight 16; 16 x 32 at M = 512 fits with 131 088 bytes."""
    lib = L.load_library()
    for rh, nh, M in ((17, 34, 3), (100, 200, 33), (8, 40, 3), (300, 600, 33)):   # 300 x 600 at M = 33: 4 * 19800 + 8 * 9900 + 16 = 158 416 bytes
        H = S.dense_set(rh, nh, M)
        rc, msg, n = _rc(lib, H, M)
        assert rc == 0 and n == rh + 1 + int((H >= 0).sum()), (rh, nh, msg)
        assert np.array_equal(L.codes_table(IMS_DEC, H, M)[1], S.table_np(H)[1])
    M, codes = SETS["two 3x5 M=100"]                                    # a weight-1 row
    codes = np.array(codes, dtype=np.int16)
    assert ((codes >= 0).sum(axis=2) == 1).any() and _rc(lib, codes, M)[0] == 0
    assert _rc(lib, np.zeros((2, 2, 16), dtype=np.int16), 2)[0] == 0    # rows of weight 16
    M, codes, _ = S.mixed_weight_set()
    w = (codes >= 0).sum(axis=2)
    assert all(16 in row and 1 in row for row in w.tolist()) and _rc(lib, codes, M)[0] == 0
    H = S.dense_set(16, 32, 512)
    assert S.lds_bytes(H, 512) == 4 * 16384 + 8 * 8192 + 16 == 131088 and _rc(lib, H, 512)[0] == 0


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
        assert lib.ldpc_hip_codes_table_ims_host(2, 4, 5, ok.ctypes.data, Cn, None, None, 0, C.byref(n)) == EINVAL
        assert "C = %d" % Cn in lib.ldpc_hip_last_error().decode()
    H = S.dense_set(20, 40, 512)                                                     # the 20 x 40, M = 512 image
    want = 4 * 20480 + 8 * 10240 + 16
    assert S.lds_bytes(H, 512) == want == 163856 > S.LDS_LIMIT
    rc, msg, _ = _rc(lib, H, 512)
    assert rc == EUNSUPPORTED and "163856" in msg, msg
    with pytest.raises(Exception, match="163856"):
        L.codes_table(IMS_DEC, H, 512)


def test_lds_mirror():
    """lds_bytes against numbers worked out by hand.  30 x 60 at M = 67: one frame per workgroup, 4 * 4020 + 8 * 2010 = 32 160 bytes,
    a multiple of 16, + 16.  4 x 8 at M = 20: three frames per wave, 3 * (4 * 160 + 8 * 80) = 3840, + 16.  4 x 8 at M = 5: twelve
    frames, 12 * (4 * 40 + 8 * 20) = 3840.  3 x 6 at M = 100: 4 * 600 + 8 * 300 = 4800.  1 x 3 at M = 3 (21 frames): 21 * (36 + 24) =
    1260, rounded up to 1264, + 16."""
    M, codes, _ = S.big_set()
    assert codes.shape == (S.NCODES, 30, 60) and M == 67 and S.lds_bytes(codes, M) == 32176
    assert S.lds_bytes(S.code_set((20, 4, 8)), 20) == 3856
    assert S.lds_bytes(S.code_set((5, 4, 8)), 5) == 3856
    assert S.lds_bytes(S.code_set((100, 3, 6)), 100) == 4816
    assert S.lds_bytes(np.zeros((1, 1, 3), dtype=np.int16), 3) == 1280


@pytest.mark.parametrize("case", list(S.CASES), ids=S.CASE_IDS)
def test_parity_inputs_have_the_required_properties(case):
    """In both layouts at least 6 of the 35 (code, frame) pairs converge after 2 .. MAXITER - 1 iterations and at least 6 give up: a
    kernel that mishandles either outcome cannot hide."""
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
        assert its.shape == (S.NCODES, S.NFRAMES)
        assert ((its >= 2) & (its < S.MAXITER)).sum() >= 6, (case, layout, r["snr"], its)
        assert (its == -S.MAXITER).sum() >= 6, (case, layout, r["snr"], its)
        assert ((its == -S.MAXITER) | ((its >= 1) & (its <= S.MAXITER))).all()      # integer min-sum has no return value 0


@pytest.mark.parametrize("case", S.PARAM_CASES, ids=["M32", "M100"])
def test_parameter_sets_change_the_result(case):
    base = S.reference(case)["ref"]["shared"]
    for p in S.PARAM_SETS:
        ref = S.param_reference(case, p)
        changed = sum(int((a[2] != b[2]).sum()) for a, b in zip(ref, base))
        assert changed >= 1, (case, p)
        top = max(float(np.abs(a[2]).max()) for a in ref)
        assert top <= (1 << (p[3] - 1)) - 1
        if p == (1.0, 1.4, 15, 15):
            assert top == 16383.0, "the halfword bound is reached"
        if p == (0.8, 1.4, 6, 10) and case == (32, 4, 8):       # soft values only: the soft comparison is what catches an ignored dbits
            assert changed == 7 and all(np.array_equal(a[1], b[1]) for a, b in zip(ref, base))


def test_the_oracle_reproduces_the_golden():
    g = S.golden_set()
    assert g["codes"].shape == (3, 16, 32) and g["M"] == 64 and len(g["llr"]) == 16 and len(g["soft"]) == 4
    hard, it, soft = S.oracle(g["codes"][0], 64, g["llr"], g["maxiter"])
    assert np.array_equal(it, g["iters"]) and np.array_equal(hard, g["hard"])
    assert np.array_equal(soft[:4].view(np.uint64), g["soft"].view(np.uint64))
    assert len({H.tobytes() for H in g["codes"]}) == 3 and S.lds_bytes(g["codes"], 64) <= S.LDS_LIMIT


def test_other_gpu_inputs():
    M, codes, llr = S.big_set()
    assert int((codes[0] >= 0).sum()) == 206 and sorted(set((codes[0] >= 0).sum(axis=1).tolist())) == list(range(4, 11))
    its = np.array([S.oracle(codes[c], M, llr, S.MAXITER)[1] for c in range(S.NCODES)])
    conv = its[its > 0]
    assert len(conv) == 15 and conv.min() == 6 and conv.max() == 17 and (its == -S.MAXITER).sum() == 5, its
    for make, shape in ((S.rows17_set, (S.NCODES, 17, 34)), (S.mixed_weight_set, (S.NCODES, 5, 20))):
        M, codes, llr = make()
        assert codes.shape == shape and ((codes >= 0).sum(axis=2) >= 1).all() and ((codes >= 0).sum(axis=1) >= 1).all()
        assert (codes >= 0).sum(axis=2).max() <= 16 and S.lds_bytes(codes, M) <= S.LDS_LIMIT
        its = np.array([S.oracle(codes[c], M, llr, S.MAXITER)[1] for c in range(S.NCODES)])
        assert ((its >= 2) & (its < S.MAXITER)).sum() >= 6 and (its == -S.MAXITER).sum() >= 6, (shape, its)
    for B in (1, 4):
        M, codes, llr = S.boundary_set(B)
        out = [S.oracle(codes[c], M, llr[c], S.MAXITER) for c in range(3)]
        assert (out[1][1] == 1).all() and (out[0][1] == -S.MAXITER).all() and (out[2][1] == -S.MAXITER).all(), [o[1] for o in out]
        assert (out[1][0] == 0).all()
    codes, llr = S.maxiter_one_set()
    assert set(np.unique([S.oracle(codes[c], 20, llr, 1)[1] for c in range(S.NCODES)])) == {-1, 1}
    codes = S.simulate_set()
    assert len({(H >= 0).tobytes() for H in codes}) == S.SIM["C"]
    weak = S.stop_set()[0]
    assert len(S.stop_set()) == 3 and ((weak >= 0).sum(axis=0) == 1).all(), "code 0 of the stopping-rule set: block columns of weight 1"
    for case in S.ADVERSARIAL_CASES:
        codes, llr, labels = S.adversarial_set(case)
        assert np.isfinite(llr).all() and len(llr) == len(labels) and (llr == 0).all(axis=1).any() and (np.abs(llr) >= 1e155).all(axis=1).any()


def _kernel_metadata(asm):
    """name -> {key: value} of every kernel in the assembly's amdhsa metadata."""
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", asm)[1:]:
        name = re.search(r"\.name:\s*(\S+)", blk)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s*(\d+)\s*$", blk, re.M)}
    return out


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not installed")
def test_the_kernels_use_no_scratch(tmp_path):
    """Both instances of the decode kernel and the quantiser keep everything in registers and LDS: no scratch memory, no spilled
    vector register.  Asserted on the cross-compiled translation unit, the way test_codeset_lche_cpu.py does."""
    csrc = os.path.join(ROOT, "ldpc-lib_amd", "csrc")
    src = tmp_path / "k.hip"
    src.write_text(f'#include "{csrc}/ldpc_codeset.hpp"\n'
                   "template __global__ void ldpc::ims_flood_codes_kernel<false>(const ldpc::CodesetArgs, const ldpc::ImsCodesArgs);\n"
                   "template __global__ void ldpc::ims_flood_codes_kernel<true>(const ldpc::CodesetArgs, const ldpc::ImsCodesArgs);\n")
    out = tmp_path / "k.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           "--cuda-device-only", "-S", str(src), "-o", str(out)], stderr=subprocess.DEVNULL)
    meta = {k: v for k, v in _kernel_metadata(out.read_text()).items() if "ims_flood_codes_kernel" in k or "ims_quantise_kernel" in k}
    print(meta)
    assert len(meta) == 3, list(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)
