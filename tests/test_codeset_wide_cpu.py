"""Wide code sets (ldpc_hip_open_codes_wide / ldpc_hip_codes_table_wide_host: min-sum, TDMP and layered min-sum at any number of block
rows and columns) without a GPU: the exported entry points and the binding's route choice, the host-side table against a numpy
builder and against ldpc_hip_codes_table_host where both accept the shape, the accepted shapes, every refusal with its return code
and complete message, the LDS byte counts, the scratch memory of the new kernels on the cross-compiled code, and the properties the
GPU tests (test_gpu_codeset_wide.py) need of their inputs, against the CPU oracle."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import codeset_wide_sets as S
from codeset_wide_sets import DECS, LMS_DEC, MS_DEC, TASP_DEC
from ldpc_testlib import ROOT

EINVAL, EUNSUPPORTED = -1, -2
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
WHO = "ldpc_hip_codes_table_wide_host"
DEC_PARAM = pytest.mark.parametrize("dec", DECS, ids=[S.DEC_IDS[d] for d in DECS])


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


def _rc(lib, dec, codes, M, Cn=None):
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    n = C.c_longlong(-1)
    rc = lib.ldpc_hip_codes_table_wide_host(dec, codes.shape[1], codes.shape[2], M, codes.ctypes.data, codes.shape[0] if Cn is None else Cn,
                                            None, None, 0, C.byref(n))
    return rc, lib.ldpc_hip_last_error().decode(), n.value


def _old_rc(lib, dec, codes, M):
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    n = C.c_longlong(-1)
    rc = lib.ldpc_hip_codes_table_host(dec, codes.shape[1], codes.shape[2], M, codes.ctypes.data, codes.shape[0], None, None, 0, C.byref(n))
    return rc, lib.ldpc_hip_last_error().decode()


def test_symbols_header_and_null_arguments(L):
    lib = L.load_library()
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        header = f.read()
    assert hasattr(lib, "ldpc_hip_open_codes_wide") and hasattr(lib, "ldpc_hip_codes_table_wide_host")
    assert re.search(r"\bint\s+ldpc_hip_open_codes_wide\s*\(int decoder_id, int rh, int nh, int M, const int16_t \*hd, int C, int device, "
                     r"ldpc_hip_ctx \*\*out\)", header)
    assert re.search(r"\bint\s+ldpc_hip_codes_table_wide_host\s*\(int decoder_id, int rh, int nh, int M, const int16_t \*hd, int C,"
                     r"\s*int32_t \*offsets, int32_t \*table,\s*long long capacity,\s*long long \*length\)", header)
    assert re.search(r"#define\s+LDPC_HIP_ABI_VERSION\s+4\b", header) and lib.ldpc_hip_abi_version() == 4
    ok = np.zeros((1, 1, 2), dtype=np.int16)
    for dec in DECS:
        h = C.c_void_p(123)
        assert lib.ldpc_hip_open_codes_wide(dec, 1, 2, 5, None, 1, 0, C.byref(h)) == EINVAL and not h.value   # refused before any device call
        assert lib.ldpc_hip_open_codes_wide(dec, 1, 2, 5, ok.ctypes.data, 1, 0, None) == EINVAL
        n = C.c_longlong()
        assert lib.ldpc_hip_codes_table_wide_host(dec, 1, 2, 5, None, 1, None, None, 0, C.byref(n)) == EINVAL
    with open(os.path.join(ROOT, "include", "ldpc", "bp_simulation.h")) as f:
        assert "ldpc_hip_open_codes_wide" in f.read()


@pytest.mark.parametrize("dec", [0, 1, 2, 4, 5, 6, 9, 10])
def test_other_decoder_ids_are_refused(L, dec):
    lib = L.load_library()
    ok = np.zeros((1, 1, 2), dtype=np.int16)
    rc, msg, _ = _rc(lib, dec, ok, 1)
    assert rc == EINVAL and msg == f"{WHO}: decoder id {dec}; MS_DEC (3), TASP_DEC (7) or LMS_DEC (8)", msg
    h = C.c_void_p(123)
    assert lib.ldpc_hip_open_codes_wide(dec, 1, 2, 1, ok.ctypes.data, 1, 0, C.byref(h)) == EINVAL and not h.value
    assert lib.ldpc_hip_last_error().decode() == f"ldpc_hip_open_codes_wide: decoder id {dec}; MS_DEC (3), TASP_DEC (7) or LMS_DEC (8)"


@DEC_PARAM
def test_table(L, dec):
    """The wide table is the min-sum record; on shapes inside the old limits it is ldpc_hip_codes_table_host's table."""
    lib = L.load_library()
    for name in S.SETS:
        if (name, dec) not in S.SNR:
            continue
        M, codes = S.code_set(name)
        off, tab = L.codes_table(dec, codes, M, wide=True)
        want_off, want_tab = S.table_np(codes)
        assert np.array_equal(off, want_off) and np.array_equal(tab, want_tab), name
        if not S.is_wide(dec, *codes.shape[1:]):
            old_off, old_tab = L.codes_table(dec, codes, M)
            assert np.array_equal(off, old_off) and np.array_equal(tab, old_tab), name
        else:                                                   # and the binding takes the wide route by itself
            off2, tab2 = L.codes_table(dec, codes, M)
            assert np.array_equal(off, off2) and np.array_equal(tab, tab2), name
        rc, _, n = _rc(lib, dec, codes, M)                      # sizes only, and a buffer that is too small
        assert rc == 0 and n == len(want_tab)
        small, o = np.empty(n - 1, dtype=np.int32), np.empty(len(codes), dtype=np.int32)
        assert lib.ldpc_hip_codes_table_wide_host(dec, codes.shape[1], codes.shape[2], M, codes.ctypes.data, len(codes), o.ctypes.data,
                                                  small.ctypes.data, n - 1, None) == EINVAL
        assert lib.ldpc_hip_last_error().decode() == f"{WHO}: the table has {n} entries, room for {n - 1}"
        assert np.array_equal(o, want_off)


@DEC_PARAM
def test_accepted_shapes(L, dec):
    """17 x 34, 30 x 60, 100 x 200 and 3 x 33 (two block rows of weight 16 cannot fill 33 block columns) are accepted, and
    ldpc_hip_codes_table_host still refuses them where its kernel's limits say so."""
    lib = L.load_library()
    shapes = [S.code_set("rows17_M20")[::-1], S.code_set("rows17_M130")[::-1], S.code_set("big")[::-1], (S.dense_set(100, 200, 33), 33),
              S.code_set("cols33")[::-1]]
    for codes, M in shapes:
        rh, nh = codes.shape[1:]
        rc, msg, n = _rc(lib, dec, codes, M)
        assert rc == 0 and n == len(codes) * (rh + 1) + int((codes >= 0).sum()), (rh, nh, msg)
        assert S.lds_bytes(dec, codes, M) <= S.LDS_LIMIT
        rc, msg = _old_rc(lib, dec, codes, M)
        if rh > 16:
            assert rc == EINVAL and msg == f"ldpc_hip_codes_table_host: rh = {rh}, the resident table kernels take 16 block rows", msg
        elif dec == MS_DEC:
            assert rc == EINVAL and msg == ("ldpc_hip_codes_table_host: nh = 33, the flooding table kernel keeps the channel LLRs of 32 block "
                                            "columns in registers"), msg
        else:
            assert rc == 0, msg
    assert _rc(lib, dec, np.zeros((2, 2, 16), dtype=np.int16), 2)[0] == 0      # rows of weight 16
    if dec != TASP_DEC:
        M, codes = S.code_set("mixed")
        w = (codes >= 0).sum(axis=2)
        assert codes.shape[1:] == (17, 34) and all(16 in row and (row == 1).sum() == 2 for row in w) and _rc(lib, dec, codes, M)[0] == 0


def test_lds_byte_counts():
    """The figures of the 30 x 60, M = 67 shape with 206 circulants, worked out by hand: MS / LMS 8 * 4020 + 24 * 2010 = 80 400, + 16;
    with the channel LLRs in LDS 8 * 4020 more; TDMP 8 * (4020 + 206 * 67) = 142 576, + 16.  17 x 34 at M = 130 fits for all three.
    M = 20 packs three frames: 3 * (8 * 680 + 24 * 340) = 40 800, + 16."""
    M, codes = S.code_set("big")
    assert M == 67 and codes.shape[1:] == (30, 60) and all(int((H >= 0).sum()) == 206 for H in codes)
    for dec in (MS_DEC, LMS_DEC):
        assert S.lds_bytes(dec, codes, M) == 80416 and S.lds_bytes(dec, codes, M, llr_in_lds=True) == 112576
    assert S.lds_bytes(TASP_DEC, codes, M) == 142592
    M, codes = S.code_set("rows17_M130")
    assert M == 130 and codes.shape[1:] == (17, 34)
    assert S.lds_bytes(MS_DEC, codes, M) == 8 * 4420 + 24 * 2210 + 16 == 88416 and S.lds_bytes(MS_DEC, codes, M, True) == 123776
    assert S.lds_bytes(TASP_DEC, codes, M) <= S.LDS_LIMIT and S.lds_bytes(LMS_DEC, codes, M) == 88416
    M, codes = S.code_set("rows17_M20")
    assert S.lds_bytes(MS_DEC, codes, M) == 40816
    assert S.lds_bytes(MS_DEC, np.zeros((1, 1, 3), dtype=np.int16), 3) == 21 * (72 + 72) + 16    # 3024, a multiple of 16


@DEC_PARAM
def test_refusals(L, dec):
    """Every refusal of the wide builder, with return code and complete message, on the smallest input that trips it."""
    lib = L.load_library()
    one = np.zeros((1, 1, 2), dtype=np.int16)                                       # 1 x 2, one row of weight 2
    assert _rc(lib, dec, one, 1)[0] == 0
    for Cn in (0, -3):
        rc, msg, _ = _rc(lib, dec, one, 1, Cn=Cn)
        assert rc == EINVAL and msg == f"{WHO}: C = {Cn}, a code set holds at least one code", msg
    rc, msg, _ = _rc(lib, dec, one, 513)
    assert rc == EINVAL and msg == f"{WHO}: M = 513, the resident table kernels take M <= 512", msg
    bad = one.copy(); bad[0, 0, 1] = 1                                               # a shift of M
    rc, msg, _ = _rc(lib, dec, bad, 1)
    assert rc == EINVAL and msg == f"{WHO}: code 0, shift 1 at (0, 1) is outside [-1, 1)", msg
    bad = np.zeros((1, 2, 2), dtype=np.int16); bad[0, 1, :] = -1                     # an empty block row
    rc, msg, _ = _rc(lib, dec, bad, 1)
    assert rc == EINVAL and msg == f"{WHO}: code 0, block row 1 is empty", msg
    bad = np.zeros((1, 1, 3), dtype=np.int16); bad[0, 0, 2] = -1                     # an empty block column
    rc, msg, _ = _rc(lib, dec, bad, 1)
    assert rc == EINVAL and msg == f"{WHO}: code 0, block column 2 is empty", msg
    rc, msg, _ = _rc(lib, dec, np.zeros((1, 1, 17), dtype=np.int16), 1)              # weight 17
    assert rc == EINVAL and msg == f"{WHO}: code 0, block row 0 has weight 17; at most 16", msg
    rc, msg, _ = _rc(lib, dec, np.zeros((1, 1, 1), dtype=np.int16), 1)               # weight 1
    if dec == TASP_DEC:
        assert rc == EINVAL and msg == f"{WHO}: code 0, block row 0 has weight 1; TDMP sum-product needs at least 2", msg
    else:
        assert rc == 0, msg
    # an image beyond 160 KiB.  MS / LMS at M = 512: 8 * 512 * nh + 24 * 512 * rh > 163 824 first holds at 3 x 31 (two block rows of
    # weight 16 cover 32 block columns, and 2 x 32 takes 155 664 bytes); TDMP: 8 * 512 * (nh + ne) > 163 824 at 2 x 14 with 26 circulants
    if dec == TASP_DEC:
        H = np.zeros((1, 2, 14), dtype=np.int16); H[0, 0, 0] = H[0, 1, 1] = -1
        assert S.lds_bytes(dec, H, 512) == 163856
        want = f"{WHO}: 1 frame(s) per wave x (7168 a-posteriori values + 26 circulants x 512 checks) need an LDS image of 163856 bytes; the limit is 160 KiB"
        H2 = np.zeros((1, 2, 14), dtype=np.int16); H2[0, 0, 0] = H2[0, 1, 1] = H2[0, 0, 2] = -1
        assert S.lds_bytes(dec, H2, 512) == 159760 and _rc(lib, dec, H2, 512)[0] == 0
    else:
        H = S.dense_set(3, 31, 512)
        fits = -np.ones((1, 2, 32), dtype=np.int16); fits[0, 0, :16] = 0; fits[0, 1, 16:] = 0
        assert S.lds_bytes(dec, H, 512) == 163856 and S.lds_bytes(dec, fits, 512) == 155664
        want = (f"{WHO}: 1 frame(s) per wave x (8 x 15872 variables + 24 x 1536 checks) bytes, rounded up to 16, + 16 need an LDS image of "
                "163856 bytes; the limit is 160 KiB")
        assert _rc(lib, dec, fits, 512)[0] == 0
    rc, msg, _ = _rc(lib, dec, H, 512)
    assert rc == EUNSUPPORTED and msg == want, msg
    with pytest.raises(L.LdpcHipError, match="163856"):
        L.codes_table(dec, H, 512, wide=True)
    # packed frames count: 17 x 34 at M = 32 holds two frames per wave, 2 * (8 * 1088 + 24 * 544) + 16 = 43 536 bytes: accepted
    assert _rc(lib, dec, S.dense_set(17, 34, 32), 32)[0] == 0


@DEC_PARAM
def test_route_choice_of_the_binding(L, dec):
    """codes_table and LdpcHipCodes take the decoder's own entry point inside its limits and the wide one exactly beyond them.  Seen
    through the name in front of a refusal (an empty block row), which is raised before any device call."""
    own_open = "ldpc_hip_open_codes_tdmp" if dec == TASP_DEC else "ldpc_hip_open_codes"
    for rh, nh in ((16, 32), (17, 32), (16, 33), (17, 34), (3, 33)):
        bad = S.dense_set(rh, nh, 4).copy()
        bad[0, rh - 1, :] = -1
        wide = S.is_wide(dec, rh, nh)
        assert wide == (rh > 16 or (dec == MS_DEC and nh > 32))
        with pytest.raises(L.LdpcHipError) as e:
            L.codes_table(dec, bad, 4)
        assert str(e.value).startswith(("ldpc_hip_codes_table_wide_host: " if wide else "ldpc_hip_codes_table_host: ") * 2), str(e.value)
        with pytest.raises(L.LdpcHipError) as e:
            L.LdpcHipCodes(dec, bad, 4)
        assert str(e.value).startswith(("ldpc_hip_open_codes_wide: " if wide else own_open + ": ") * 2), str(e.value)
        with pytest.raises(L.LdpcHipError) as e:
            L.LdpcHipCodes(dec, bad, 4, wide=True)
        assert str(e.value).startswith("ldpc_hip_open_codes_wide: " * 2), str(e.value)
    assert L.DEC_MS == MS_DEC and L.DEC_TASP == TASP_DEC and L.DEC_LMS == LMS_DEC


@pytest.mark.parametrize("name,dec", list(S.SNR), ids=["%s-%s" % (n, S.DEC_IDS[d]) for n, d in S.SNR])
def test_parity_inputs_have_the_required_properties(name, dec):
    """Over the two layouts of a (set, decoder): frames that converge, frames that give up, and at least one frame that converges only
    after three or more iterations -- otherwise the records in LDS are never read back and the GPU tests pass on trivial frames."""
    r = S.reference(name, dec)
    codes, M = r["codes"], r["M"]
    w = (codes >= 0).sum(axis=2)
    assert w.min() >= (2 if dec == TASP_DEC else 1) and w.max() <= 16 and ((codes >= 0).sum(axis=1) >= 1).all()
    assert S.lds_bytes(dec, codes, M) <= S.LDS_LIMIT
    its = np.array([[x[1] for x in r["ref"][layout]] for layout in ("shared", "percode")])
    assert its.shape == (2, len(codes), S.FRAMES.get(name, S.NFRAMES))
    first = 0 if dec == TASP_DEC else 1
    assert ((its == -S.MAXITER) | ((its >= first) & (its <= S.MAXITER))).all(), its
    assert (its >= first).sum() >= 1 and (its == -S.MAXITER).sum() >= 1 and (its >= 3).sum() >= 1, (name, dec, its)


def test_other_gpu_inputs():
    for B in (1, 4):
        M, codes, llr = S.boundary_set(B)
        assert codes.shape == (3, 17, 34) and M == 20
        for dec, middle in ((MS_DEC, 1), (LMS_DEC, 1), (TASP_DEC, 0)):
            out = [S.oracle(dec, codes[c], M, llr[c], S.MAXITER) for c in range(3)]
            assert (out[1][1] == middle).all() and (out[0][1] == -S.MAXITER).all() and (out[2][1] == -S.MAXITER).all(), (dec, [o[1] for o in out])
            assert (out[1][0] == 0).all()
    for dec in DECS:
        M, codes, llr = S.maxiter_one_set(dec)
        assert set(np.unique([S.oracle(dec, codes[c], M, llr, 1)[1] for c in range(len(codes))])) == {-1, 1}, dec
    M, codes, llr, labels = S.adversarial_set()
    assert np.isfinite(llr).all() and len(llr) == len(labels) and (np.abs(llr) >= 1e155).all(axis=1).any()
    assert any((y == 0).all() and np.signbit(y).all() for y in llr), "a frame of -0.0"
    M, codes = S.simulate_set()
    assert len(codes) == S.SIM["C"] == 3 and M == 20 and codes.shape[1:] == (17, 34)


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
    """Both instances of the two new kernels keep everything in registers and LDS: no scratch memory, no spilled vector register.
    Asserted on the cross-compiled translation unit, the way test_codeset_ims_cpu.py does."""
    csrc = os.path.join(ROOT, "ldpc-lib_amd", "csrc")
    src = tmp_path / "k.hip"
    src.write_text(f'#include "{csrc}/ldpc_codeset_wide.hpp"\n'
                   "template __global__ void ldpc::ms_flood_wide_codes_kernel<false>(const ldpc::CodesetArgs);\n"
                   "template __global__ void ldpc::ms_flood_wide_codes_kernel<true>(const ldpc::CodesetArgs);\n"
                   "template __global__ void ldpc::lms_layered_wide_codes_kernel<false>(const ldpc::CodesetArgs);\n"
                   "template __global__ void ldpc::lms_layered_wide_codes_kernel<true>(const ldpc::CodesetArgs);\n")
    out = tmp_path / "k.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           "--cuda-device-only", "-S", str(src), "-o", str(out)], stderr=subprocess.DEVNULL)
    meta = {k: v for k, v in _kernel_metadata(out.read_text()).items() if "wide_codes_kernel" in k}
    print(meta)
    assert len(meta) == 4, list(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)
