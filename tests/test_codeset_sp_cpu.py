"""Flooding sum-product code sets (decoders 1 and 2, ldpc_hip_open_codes_sp / ldpc_hip_codes_table_sp_host) without a GPU: the
exported entry points, the host-side table against a numpy builder of the record and against the IASP table, the limits (block rows
and columns are not limited; SP takes any row weight, ASP 2 .. 16), the LDS contract with its byte counts, the registers of the four
kernel instances on the cross-compiled library, and the properties the GPU tests (test_gpu_codeset_sp.py) need of their inputs."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import codeset_sp_sets as S
from codeset_sp_sets import ASP_DEC, DECS, IASP_DEC, SP_DEC
from ldpc_testlib import GOLDEN_DIR, ROOT
from test_codeset_cpu import SETS

EINVAL, EUNSUPPORTED = -1, -2
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


def _rc(lib, dec, codes, M):
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    n = C.c_longlong(-1)
    rc = lib.ldpc_hip_codes_table_sp_host(dec, codes.shape[1], codes.shape[2], M, codes.ctypes.data, codes.shape[0], None, None, 0, C.byref(n))
    return rc, lib.ldpc_hip_last_error().decode(), n.value


def test_symbols_header_and_null_arguments(L):
    lib = L.load_library()
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        header = f.read()
    assert hasattr(lib, "ldpc_hip_open_codes_sp") and hasattr(lib, "ldpc_hip_codes_table_sp_host")
    assert re.search(r"\bint\s+ldpc_hip_open_codes_sp\s*\(int decoder_id, int rh, int nh, int M, const int16_t \*hd, int C, int device, ldpc_hip_ctx \*\*out\)",
                     header)
    assert re.search(r"\bint\s+ldpc_hip_codes_table_sp_host\s*\(int decoder_id, int rh, int nh, int M, const int16_t \*hd, int C, int32_t \*offsets,"
                     r"\s*int32_t \*table,\s*long long capacity,\s*long long \*length\)", header)
    assert re.search(r"#define\s+LDPC_HIP_ABI_VERSION\s+4\b", header) and lib.ldpc_hip_abi_version() == 4
    ok = np.array(SETS["three 2x4"][1], dtype=np.int16)
    for dec in DECS:
        h = C.c_void_p(123)
        assert lib.ldpc_hip_open_codes_sp(dec, 2, 4, 5, None, 1, 0, C.byref(h)) == EINVAL and not h.value     # refused before any device call
        assert lib.ldpc_hip_open_codes_sp(dec, 2, 4, 5, None, 1, 0, None) == EINVAL
        assert lib.ldpc_hip_open_codes_sp(dec, 2, 4, 5, ok.ctypes.data, 3, 0, None) == EINVAL
        n = C.c_longlong()
        assert lib.ldpc_hip_codes_table_sp_host(dec, 2, 4, 5, None, 3, None, None, 0, C.byref(n)) == EINVAL


def test_which_entry_point_takes_which_decoder(L):
    lib = L.load_library()
    ok = np.array(SETS["three 2x4"][1], dtype=np.int16)
    n = C.c_longlong()
    for dec in DECS:                                     # 1 and 2 stay refused by the generic entry points
        assert lib.ldpc_hip_codes_table_host(dec, 2, 4, 5, ok.ctypes.data, 3, None, None, 0, C.byref(n)) == EINVAL
        assert "decoder id" in lib.ldpc_hip_last_error().decode()
        h = C.c_void_p(123)
        assert lib.ldpc_hip_open_codes(dec, 2, 4, 5, ok.ctypes.data, 3, 0, C.byref(h)) == EINVAL and not h.value
        assert "decoder id" in lib.ldpc_hip_last_error().decode()
    for dec in (0, 3, 4, 5, 7, 8, 9, -1):                # and everything else by the new ones, Gallager BP (0) included
        assert lib.ldpc_hip_codes_table_sp_host(dec, 2, 4, 5, ok.ctypes.data, 3, None, None, 0, C.byref(n)) == EINVAL
        assert "decoder id" in lib.ldpc_hip_last_error().decode()
        h = C.c_void_p(123)
        assert lib.ldpc_hip_open_codes_sp(dec, 2, 4, 5, ok.ctypes.data, 3, 0, C.byref(h)) == EINVAL and not h.value
        assert "decoder id" in lib.ldpc_hip_last_error().decode()
    with pytest.raises(Exception):
        L.codes_table(0, ok, 5)


@pytest.mark.parametrize("dec", DECS, ids=S.DEC_IDS)
@pytest.mark.parametrize("name", list(SETS))
def test_table_equals_numpy_and_the_iasp_table(L, name, dec):
    M, codes = SETS[name]
    codes = np.array(codes, dtype=np.int16)
    lib = L.load_library()
    rc, msg, n = _rc(lib, dec, codes, M)
    if dec == ASP_DEC and ((codes >= 0).sum(axis=2) < 2).any():
        assert rc == EINVAL and "weight 1" in msg, msg
        return
    off, tab = L.codes_table(dec, codes, M)
    want_off, want_tab = S.table_np(codes)
    assert np.array_equal(off, want_off) and np.array_equal(tab, want_tab)
    if ((codes >= 0).sum(axis=2) >= 2).all():                  # wherever IASP accepts the set (these sets are within its LDS bound)
        i_off, i_tab = L.codes_table(IASP_DEC, codes, M)
        assert np.array_equal(off, i_off) and np.array_equal(tab, i_tab)
    # sizes only, and a buffer that is too small
    assert rc == 0 and n == len(want_tab)
    small, o = np.empty(n - 1, dtype=np.int32), np.empty(len(codes), dtype=np.int32)
    assert lib.ldpc_hip_codes_table_sp_host(dec, codes.shape[1], codes.shape[2], M, codes.ctypes.data, len(codes), o.ctypes.data, small.ctypes.data,
                                            n - 1, None) == EINVAL


def _gpu_sets():
    sets = [(c[0], S.code_set(c), DECS) for c in S.CASES]
    sets += [(g["M"], g["codes"], (g["dec"],)) for g in map(S.golden_set, S.GOLDENS)]      # a golden set runs on its own decoder
    g = S.cw2_mixed_set()
    sets += [(g["M"], g["codes"], DECS), S.rows17_set()[:2] + (DECS,), S.mixed_weight_set()[:2] + ((SP_DEC,),), S.big_set()[:2] + (DECS,)]
    sets += [(20, S.boundary_set(1)[1], DECS), (S.SIM["M"], S.simulate_set(), DECS), (S.STOP["M"], S.stop_set(), DECS)]
    return sets


def test_table_and_image_on_the_gpu_sets(L):
    for M, codes, decs in _gpu_sets():
        want_off, want_tab = S.table_np(codes)
        for dec in decs:
            off, tab = L.codes_table(dec, codes, M)
            assert np.array_equal(off, want_off) and np.array_equal(tab, want_tab), (dec, M, codes.shape)
            assert S.lds_bytes(dec, codes, M) <= S.LDS_LIMIT and S.threads(codes, M) <= 1024


def _ring(rh, nh, shifts=3):
    """One rh x nh code, two circulants per block column."""
    H = -np.ones((1, rh, nh), dtype=np.int16)
    for k in range(nh):
        H[0, k % rh, k] = k % shifts
        H[0, (k + 1) % rh, k] = (k + 1) % shifts
    return H


def test_accepted_shapes_and_row_weights(L):
    lib = L.load_library()
    for rh, nh, M in ((17, 34, 3), (100, 200, 20), (8, 40, 3)):      # rh > 16, nh > 32
        H = _ring(rh, nh)
        for dec in DECS:
            rc, msg, n = _rc(lib, dec, H, M)
            assert rc == 0 and n == len(S.table_np(H)[1]), (dec, rh, nh, msg)
            assert np.array_equal(L.codes_table(dec, H, M)[1], S.table_np(H)[1])
    M, codes = SETS["two 3x5 M=100"]                                  # a weight-1 row
    codes = np.array(codes, dtype=np.int16)
    assert ((codes >= 0).sum(axis=2) == 1).any()
    assert _rc(lib, SP_DEC, codes, M)[0] == 0
    rc, msg, _ = _rc(lib, ASP_DEC, codes, M)
    assert rc == EINVAL and "weight 1" in msg, msg
    assert _rc(lib, SP_DEC, np.zeros((2, 2, 16), dtype=np.int16), 2)[0] == 0 and _rc(lib, ASP_DEC, np.zeros((2, 2, 16), dtype=np.int16), 2)[0] == 0
    wide = np.zeros((2, 2, 17), dtype=np.int16)                       # row weight 17, in code 1 only
    wide[0, :, 16] = -1; wide[0, 0, 16] = 0; wide[0, 0, 0] = -1
    assert _rc(lib, SP_DEC, wide, 2)[0] == 0
    assert np.array_equal(L.codes_table(SP_DEC, wide, 2)[1], S.table_np(wide)[1])
    rc, msg, _ = _rc(lib, ASP_DEC, wide, 2)
    assert rc == EINVAL and "code 1" in msg and "row 0" in msg and "weight 17" in msg, msg
    M, codes, _ = S.mixed_weight_set()
    w = (codes >= 0).sum(axis=2)
    assert all(16 in row and 1 in row for row in w.tolist()) and _rc(lib, SP_DEC, codes, M)[0] == 0 and _rc(lib, ASP_DEC, codes, M)[0] == EINVAL
    for dec in DECS:
        assert _rc(lib, dec, np.zeros((1, 2, 4), dtype=np.int16), 512)[0] == 0   # a 2 x 4 code at M = 512


@pytest.mark.parametrize("dec", DECS, ids=S.DEC_IDS)
def test_refusals(L, dec):
    lib = L.load_library()
    ok = np.array(SETS["three 2x4"][1], dtype=np.int16)
    assert _rc(lib, dec, ok, 5)[0] == 0
    for M in (0, 513):
        rc, msg, _ = _rc(lib, dec, np.zeros((1, 2, 4), dtype=np.int16), M)
        assert rc == EINVAL, msg
    assert "513" in msg
    bad = ok.copy(); bad[1, 0, :] = -1                                               # an empty block row
    rc, msg, _ = _rc(lib, dec, bad, 5)
    assert rc == EINVAL and "code 1" in msg and "row 0" in msg, msg
    bad = ok.copy(); bad[2, :, 2] = -1                                               # an empty block column
    rc, msg, _ = _rc(lib, dec, bad, 5)
    assert rc == EINVAL and "code 2" in msg and "column 2" in msg, msg
    for v in (5, -2):                                                                # a shift of M and a shift of -2
        bad = ok.copy(); bad[2, 1, 0] = v
        rc, msg, _ = _rc(lib, dec, bad, 5)
        assert rc == EINVAL and "code 2" in msg and "(1, 0)" in msg and str(v) in msg, msg
    for Cn in (0, -3):
        n = C.c_longlong()
        assert lib.ldpc_hip_codes_table_sp_host(dec, 2, 4, 5, ok.ctypes.data, Cn, None, None, 0, C.byref(n)) == EINVAL
        assert "C = %d" % Cn in lib.ldpc_hip_last_error().decode()
    many = np.zeros((1, 4100, 16), dtype=np.int16)                                   # 4100 rows of weight 16: 65600 circulants in one code
    rc, msg, _ = _rc(lib, dec, many, 1)
    assert rc == EINVAL and "circulants" in msg, msg


def test_lds_contract(L):
    lib = L.load_library()
    H126, H128, H512 = S.appendix_c(126), S.appendix_c(128), S.appendix_c(512)
    assert H126.shape == (1, 16, 32) and int((H126 >= 0).sum()) == 112
    assert S.lds_bytes(SP_DEC, H126, 126) == 161808 and S.lds_bytes(ASP_DEC, H126, 126) == 145680
    assert _rc(lib, SP_DEC, H126, 126)[0] == 0 and _rc(lib, ASP_DEC, H126, 126)[0] == 0
    assert S.lds_bytes(SP_DEC, H128, 128) == 164368 and S.lds_bytes(ASP_DEC, H128, 128) == 147984
    rc, msg, _ = _rc(lib, SP_DEC, H128, 128)
    assert rc == EUNSUPPORTED and "164368" in msg, msg
    assert _rc(lib, ASP_DEC, H128, 128)[0] == 0
    for dec in DECS:
        rc, msg, _ = _rc(lib, dec, H512, 512)
        assert rc == EUNSUPPORTED and str(S.lds_bytes(dec, H512, 512)) in msg, msg
    M, codes, _ = S.big_set()
    assert codes.shape == (5, 30, 60) and M == 67 and int((codes[0] >= 0).sum()) == 206
    g = np.load(os.path.join(GOLDEN_DIR, "lche", "lche_30x60_m67_2p0.npz"))
    assert np.array_equal(codes[0], np.where(g["H"] >= 0, g["H"] % 67, -1))
    assert S.lds_bytes(SP_DEC, codes, M) == 159184 and _rc(lib, SP_DEC, codes, M)[0] == 0 and _rc(lib, ASP_DEC, codes, M)[0] == 0
    # the largest code of a set decides, wherever it stands
    more = H126[0].copy()
    more[0, np.flatnonzero(more[0] < 0)[:3]] = 1                     # 115 circulants: 114 would still fit
    assert S.lds_bytes(SP_DEC, more[None], 126) > S.LDS_LIMIT
    for pair in ([H126[0], more], [more, H126[0]]):
        rc, msg, _ = _rc(lib, SP_DEC, np.stack(pair), 126)
        assert rc == EUNSUPPORTED and str(S.lds_bytes(SP_DEC, more[None], 126)) in msg, msg
    # several frames share a workgroup only as far as their images fit: a set is never refused for that
    H64 = S.appendix_c(64)
    assert S.frames_per_workgroup(SP_DEC, H64, 64) == 1 and S.frames_per_workgroup(SP_DEC, S.appendix_c(20), 20) == 3
    H32 = S.appendix_c(32)
    assert 64 // 32 * S.frame_bytes(SP_DEC, H32, 32) + 16 <= S.LDS_LIMIT and S.frames_per_workgroup(SP_DEC, H32, 32) == 2
    M, codes, _ = S.rows17_set()
    assert S.frames_per_workgroup(SP_DEC, codes, M) == 3
    tall = _ring(100, 200)
    assert 2 * S.frame_bytes(SP_DEC, tall, 20) > S.LDS_LIMIT                 # 100 x 200 at M = 20: one frame of 112 500 bytes, not three
    assert _rc(lib, SP_DEC, tall, 20)[0] == 0 and S.frames_per_workgroup(SP_DEC, tall, 20) == 1
    tall = _ring(60, 120)
    assert S.frames_per_workgroup(SP_DEC, tall, 20) == 2 < 64 // 20 and _rc(lib, SP_DEC, tall, 20)[0] == 0   # three frames do not fit, two do


@pytest.mark.parametrize("dec", DECS, ids=S.DEC_IDS)
@pytest.mark.parametrize("case", list(S.CASES), ids=S.CASE_IDS)
def test_gpu_inputs_have_the_required_properties(case, dec):
    """What test_gpu_codeset_sp.py relies on, asserted here so that nothing is searched at GPU time: in both layouts the oracle alone
    takes both exits of the iteration loop."""
    M, rh, nh = case
    r = S.reference(dec, case)
    codes = r["codes"]
    assert codes.shape == (S.NCODES, rh, nh)
    w = (codes >= 0).sum(axis=2)
    assert w.min() >= 2 and w.max() <= 8 and ((codes >= 0).sum(axis=1) >= 1).all()
    assert len({int((H >= 0).sum()) for H in codes}) >= 3
    for layout in ("shared", "percode"):
        its = np.array([x[1] for x in r["ref"][layout]])
        assert ((its > 1) & (its < S.MAXITER)).any(), (case, layout, its)
        assert (its == -S.MAXITER).any(), (case, layout, its)
        assert ((its == -S.MAXITER) | ((its >= 0) & (its <= S.MAXITER))).all()


def test_the_oracle_reproduces_the_goldens():
    for name in S.GOLDENS:
        g = S.golden(name)
        hard, it, soft = S.oracle(g["dec"], g["H"], g["M"], g["llr"], g["maxiter"])
        assert np.array_equal(it, g["iters"]) and np.array_equal(hard, g["hard"]), name
        ns = len(g["soft"])
        assert 0 < ns and np.array_equal(soft[:ns].view(np.uint64), g["soft"].view(np.uint64)), name
        gs = S.golden_set(name)
        assert gs["codes"].shape[0] == S.NCODES and len(gs["llr"]) == S.GOLDEN_FRAMES
        assert len({H.tobytes() for H in gs["codes"]}) == (S.NCODES if g["M"] > 1 else 1), name
    assert S.is_cw2(S.golden("asp_cw2_m64_2p0")["H"]) and not S.is_cw2(S.golden("asp_m64_2p0")["H"])
    g = S.cw2_mixed_set()
    assert [S.is_cw2(H) for H in g["codes"]] == [True, False, True, False, True] and g["codes"].shape[1:] == (4, 8) and g["M"] == 64


@pytest.mark.parametrize("dec", DECS, ids=S.DEC_IDS)
def test_other_gpu_inputs(dec):
    for B in (1, 4):
        M, codes, llr = S.boundary_set(B)
        assert S.frames_per_workgroup(dec, codes, M) == 3
        out = [S.oracle(dec, codes[c], M, llr[c], S.MAXITER) for c in range(3)]
        assert (out[1][1] == 0).all() and (out[0][1] == -S.MAXITER).all() and (out[2][1] == -S.MAXITER).all(), [o[1] for o in out]
        # a codeword at the input: the soft values are the input transform, and no two of them alike in a row
        y = llr[1]
        want = np.exp(y) if dec == SP_DEC else np.exp(-y / 2) / (np.exp(y / 2) + np.exp(-y / 2))
        assert np.allclose(out[1][2], want, rtol=1e-12, atol=0) and (out[1][0] == 0).all()
    codes, llr = S.maxiter_one_set()
    assert set(np.unique([S.oracle(dec, codes[c], 20, llr, 1)[1] for c in range(S.NCODES)])) == {-1, 1}
    codes = S.simulate_set()
    assert len({(H >= 0).tobytes() for H in codes}) == S.SIM["C"] and ((codes >= 0).sum(axis=2) >= 2).all()
    assert len(S.stop_set()) == 3 and ((S.stop_set() >= 0).sum(axis=2) >= 2).all(), "the stopping-rule set: rows of weight >= 2"
    M, codes, llr = S.rows17_set()
    assert codes.shape == (S.NCODES, 17, 34) and (codes >= 0).sum(axis=2).min() >= 2 and (codes >= 0).sum(axis=2).max() <= 16
    its = np.array([S.oracle(dec, codes[c], M, llr, S.MAXITER)[1] for c in range(S.NCODES)])
    assert ((its > 1) & (its < S.MAXITER)).any() and (its == -S.MAXITER).any()
    M, codes, llr = S.big_set()
    assert S.oracle(dec, codes[0], M, llr, S.BIG["maxiter"])[1].tolist() == S.BIG["want"]
    if dec == SP_DEC:
        M, codes, llr = S.mixed_weight_set()
        its = np.array([S.oracle(dec, codes[c], M, llr, S.MAXITER)[1] for c in range(S.NCODES)])
        assert ((its > 1) & (its < S.MAXITER)).any() and (its == -S.MAXITER).any() and (its == 0).any()


def _kernel_metadata(asm):
    """name -> {key: value} of every kernel in the assembly's amdhsa metadata."""
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", asm)[1:]:
        blk = ".agpr_count:" + blk
        name = re.search(r"\.name:\s*(\S+)", blk)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s*(\d+)\s*$", blk, re.M)}
    return out


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not installed")
def test_the_four_instances_use_no_scratch(tmp_path):
    """map_bin's forward products are VGPRs; a compiler or header change that sent them to scratch memory would fail no result check.
    Asserted on the cross-compiled translation unit, the way test_codeset_lche_cpu.py does.  A workgroup has up to 1024 threads: four
    waves per SIMD, 128 of its 512 registers each."""
    csrc = os.path.join(ROOT, "ldpc-lib_amd", "csrc")
    src = tmp_path / "k.hip"
    src.write_text(f'#include "{csrc}/ldpc_codeset_sp.hpp"\n'
                   "template __global__ void ldpc::sp_flood_codes_kernel<false>(const ldpc::CodesetArgs);\n"
                   "template __global__ void ldpc::sp_flood_codes_kernel<true>(const ldpc::CodesetArgs);\n"
                   "template __global__ void ldpc::asp_flood_codes_kernel<16, false>(const ldpc::CodesetArgs);\n"
                   "template __global__ void ldpc::asp_flood_codes_kernel<16, true>(const ldpc::CodesetArgs);\n")
    out = tmp_path / "k.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           "--cuda-device-only", "-S", str(src), "-o", str(out)], stderr=subprocess.DEVNULL)
    meta = {k: v for k, v in _kernel_metadata(out.read_text()).items() if "_flood_codes_kernel" in k and "ims_" not in k}
    print(meta)
    assert len(meta) == 4, list(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["max_flat_workgroup_size"] == 1024 and m["vgpr_count"] + m["agpr_count"] <= 128, (name, m)
