"""IASP code sets (decoder 5, ldpc_hip_open_codes_iasp) without a GPU: the exported entry point, the host-side table of
ldpc_hip_codes_table_host(5, ...) against a numpy builder of the record, IASP's limits (block rows and columns are not limited), and
the properties the GPU tests (test_gpu_codeset_iasp.py) need of their inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import codeset_iasp_sets as S
from codeset_iasp_sets import IASP_DEC
from ldpc_testlib import ROOT
from test_codeset_cpu import SETS

EINVAL, EUNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


def _rc(lib, codes, M, dec=IASP_DEC):
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    n = C.c_longlong(-1)
    rc = lib.ldpc_hip_codes_table_host(dec, codes.shape[1], codes.shape[2], M, codes.ctypes.data, codes.shape[0], None, None, 0, C.byref(n))
    return rc, lib.ldpc_hip_last_error().decode(), n.value


def test_symbol_header_and_binding(L):
    lib = L.load_library()
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        header = f.read()
    assert hasattr(lib, "ldpc_hip_open_codes_iasp")
    assert re.search(r"\bint\s+ldpc_hip_open_codes_iasp\s*\(int rh, int nh, int M, const int16_t \*hd, int C, int device, ldpc_hip_ctx \*\*out\)", header)
    assert re.search(r"#define\s+LDPC_HIP_ABI_VERSION\s+4\b", header) and lib.ldpc_hip_abi_version() == 4
    h = C.c_void_p(123)
    assert lib.ldpc_hip_open_codes_iasp(2, 4, 5, None, 1, 0, C.byref(h)) == EINVAL and not h.value     # refused before any device call
    assert lib.ldpc_hip_open_codes_iasp(2, 4, 5, None, 1, 0, None) == EINVAL
    ok = np.array(SETS["three 2x4"][1], dtype=np.int16)
    assert lib.ldpc_hip_open_codes_iasp(2, 4, 5, ok.ctypes.data, 3, 0, None) == EINVAL


def test_the_other_decoder_ids_are_still_refused(L):
    lib = L.load_library()
    ok = np.array(SETS["three 2x4"][1], dtype=np.int16)
    for dec in (0, 1, 4, 6, 9):
        rc, msg, _ = _rc(lib, ok, 5, dec)
        assert rc == EINVAL and "decoder id" in msg, (dec, msg)


def mixed_cw2_set():
    """Three 3 x 6 codes at M = 7: all columns of weight 2, one column of weight 3, all of weight 2 again."""
    E = -1
    a = [[0, 1, E, 2, E, 3], [4, E, 5, E, 6, 0], [E, 1, 2, 3, 4, E]]
    b = [[0, 1, E, 2, E, 3], [4, E, 5, 6, 6, 0], [E, 1, 2, 3, 4, E]]
    c = [[6, E, 5, E, 4, 3], [E, 2, 1, 0, E, 1], [2, 3, E, 4, 5, E]]
    return 7, np.array([a, b, c], dtype=np.int16)


def test_table_builder(L):
    M, codes = mixed_cw2_set()
    assert [bool(((H >= 0).sum(axis=0) == 2).all()) for H in codes] == [True, False, True]
    off, tab = L.codes_table(IASP_DEC, codes, M)
    want_off, want_tab = S.table_np(codes)
    assert np.array_equal(off, want_off) and np.array_equal(tab, want_tab)
    rh, nh = codes.shape[1:]
    flags = [int(tab[o + rh + 1 + tab[o + rh]]) for o in off]
    assert flags == [1, 0, 1]
    # the record begins like the other decoders' (codeset_view reads row_start and edges there)
    from test_codeset_cpu import table_np as plain
    p_off, p_tab = plain(codes)
    for c in range(3):
        n = rh + 1 + int((codes[c] >= 0).sum())
        assert np.array_equal(tab[off[c]:off[c] + n], p_tab[p_off[c]:p_off[c] + n])
    # sizes only, and a buffer that is too small
    lib = L.load_library()
    rc, _, n = _rc(lib, codes, M)
    assert rc == 0 and n == len(want_tab)
    small = np.empty(n - 1, dtype=np.int32)
    o3 = np.empty(3, dtype=np.int32)
    assert lib.ldpc_hip_codes_table_host(IASP_DEC, rh, nh, M, codes.ctypes.data, 3, o3.ctypes.data, small.ctypes.data, n - 1, None) == EINVAL


def test_table_builder_on_the_gpu_sets(L):
    for case in S.CASES:
        codes = S.code_set(case)
        off, tab = L.codes_table(IASP_DEC, codes, case[0])
        want_off, want_tab = S.table_np(codes)
        assert np.array_equal(off, want_off) and np.array_equal(tab, want_tab), case


def test_table_of_the_30x60_set(L):
    g = S.golden_set(S.SHAPE_30x60, 5)
    codes, M = g["codes"], g["M"]
    assert codes.shape == (5, 30, 60) and M == 67 and int((codes[0] >= 0).sum()) == 206
    assert S.lds_bytes(codes, M) == 43712      # 2 * (206 * 67 + 2 * 4020) = 43 684 -> 43 696, + 16
    off, tab = L.codes_table(IASP_DEC, codes, M)
    want_off, want_tab = S.table_np(codes)
    assert np.array_equal(off, want_off) and np.array_equal(tab, want_tab)
    lib = L.load_library()
    for dec in (3, 7, 8):                        # the other set kernels keep their 16 block rows
        assert _rc(lib, codes, M, dec)[0] == EINVAL


def test_builder_refusals(L):
    lib = L.load_library()
    ok = np.array(SETS["three 2x4"][1], dtype=np.int16)
    assert _rc(lib, ok, 5)[0] == 0
    assert _rc(lib, np.zeros((1, 2, 4), dtype=np.int16), 513)[0] == EINVAL         # M = 513
    assert _rc(lib, np.zeros((1, 2, 4), dtype=np.int16), 512)[0] == 0              # a 2 x 4 code at M = 512
    bad = ok.copy(); bad[1, 0, 2:] = -1; bad[1, 1, 2:] = [3, 4]; bad[1, 0, 1] = -1   # weight 1 in row 0 of code 1 (every column still used)
    rc, msg, _ = _rc(lib, bad, 5)
    assert rc == EINVAL and "code 1" in msg and "row 0" in msg and "weight 1" in msg, msg
    wide = np.zeros((2, 2, 17), dtype=np.int16)                                     # row weight 17, in code 1 only
    wide[0, :, 16] = -1; wide[0, 0, 16] = 0; wide[0, 0, 0] = -1
    rc, msg, _ = _rc(lib, wide, 2)
    assert rc == EINVAL and "code 1" in msg and "row 0" in msg and "weight 17" in msg, msg
    assert _rc(lib, np.zeros((2, 2, 16), dtype=np.int16), 2)[0] == 0
    bad = ok.copy(); bad[2, :, 2] = -1                                               # an empty block column
    rc, msg, _ = _rc(lib, bad, 5)
    assert rc == EINVAL and "code 2" in msg and "column 2" in msg, msg
    bad = ok.copy(); bad[1, 0, :] = -1                                               # an empty block row
    rc, msg, _ = _rc(lib, bad, 5)
    assert rc == EINVAL and "code 1" in msg and "row 0" in msg, msg
    for v in (5, -2, 300):                                                           # a shift outside [-1, M)
        bad = ok.copy(); bad[2, 1, 0] = v
        rc, msg, _ = _rc(lib, bad, 5)
        assert rc == EINVAL and "code 2" in msg, msg
    for Cn in (0, -3):
        n = C.c_longlong()
        assert lib.ldpc_hip_codes_table_host(IASP_DEC, 2, 4, 5, ok.ctypes.data, Cn, None, None, 0, C.byref(n)) == EINVAL


def test_block_rows_and_columns_are_not_limited(L):
    lib = L.load_library()
    # 17, 65 and 300 block rows; 40 and 600 block columns
    for rh, nh, M in ((17, 18, 3), (65, 66, 3), (300, 600, 33), (8, 40, 3)):   # 300 x 600: one frame per wave, 158 416 bytes
        H = -np.ones((1, rh, nh), dtype=np.int16)
        for k in range(nh):
            H[0, k % rh, k] = k % 3
            H[0, (k + 1) % rh, k] = (k + 1) % 3
        assert (H[0] >= 0).sum(axis=1).min() >= 2 and (H[0] >= 0).sum(axis=1).max() <= 16
        rc, msg, n = _rc(lib, H, M)
        ne = int((H >= 0).sum())
        assert rc == 0 and n == rh + nh + 3 + 2 * ne, (rh, nh, msg)
        off, tab = L.codes_table(IASP_DEC, H, M)
        want_off, want_tab = S.table_np(H)
        assert np.array_equal(tab, want_tab)


def test_more_than_65535_circulants(L):
    lib = L.load_library()
    rh, nh = 4100, 8200                      # 16 circulants per block row: 65 600
    H = -np.ones((1, rh, nh), dtype=np.int16)
    for j in range(rh):
        H[0, j, [(2 * j + q) % nh for q in range(16)]] = 0
    assert int((H >= 0).sum()) == 65600 and ((H[0] >= 0).sum(axis=0) >= 1).all()
    rc, msg, _ = _rc(lib, H, 1)
    assert rc == EINVAL and "code 0" in msg and "65600" in msg, msg
    H[0, 0:5, :] = -1                        # 65 520 would fit the 16 bits, but five block rows are empty now
    assert _rc(lib, H, 1)[0] == EINVAL


def test_lds_bound(L):
    lib = L.load_library()
    big = S.big_image_set()
    assert int((big >= 0).sum()) == 112 and S.lds_bytes(big, 512) == 180240
    rc, msg, _ = _rc(lib, big, 512)
    assert rc == EUNSUPPORTED and "180240" in msg, msg
    # the largest code of a set decides, wherever it stands
    small = -np.ones_like(big)                # two circulants per block column: 2 * (64 * 512 + 2 * 16384) + 16 = 131 088 bytes
    for k in range(32):
        small[0, k % 16, k] = k
        small[0, (k + 1) % 16, k] = 2 * k
    assert ((small[0] >= 0).sum(axis=1) >= 2).all() and ((small[0] >= 0).sum(axis=0) >= 1).all()
    assert S.lds_bytes(small, 512) <= S.LDS_LIMIT and _rc(lib, small, 512)[0] == 0
    for pair in ([small[0], big[0]], [big[0], small[0]]):
        rc, msg, _ = _rc(lib, np.stack(pair), 512)
        assert rc == EUNSUPPORTED and "180240" in msg, msg
    # the same matrix at M = 256 fits: 90 128 bytes
    from ldpc_testlib import load_base_matrix, relift
    base = load_base_matrix()
    H = np.where(base >= 0, relift(base, 256) % 256, -1).astype(np.int16)[None]
    assert S.lds_bytes(H, 256) == 90128 and _rc(lib, H, 256)[0] == 0


@pytest.mark.parametrize("case", list(S.CASES), ids=S.CASE_IDS)
def test_gpu_inputs_have_the_required_properties(case):
    """What test_gpu_codeset_iasp.py relies on, asserted here so that nothing is searched at GPU time."""
    M, rh, nh = case
    r = S.reference(case)
    codes = r["codes"]
    assert codes.shape == (S.NCODES, rh, nh)
    w = (codes >= 0).sum(axis=2)
    assert w.min() >= 2 and w.max() <= 16 and ((codes >= 0).sum(axis=1) >= 1).all()
    if rh > 2:   # (a 2 x 4 code without an empty block has columns of weight 2 only)
        assert not any(((H >= 0).sum(axis=0) == 2).all() for H in codes), "the general branch"
    assert len({(H >= 0).tobytes() for H in codes}) == S.NCODES
    assert S.lds_bytes(codes, M) <= S.LDS_LIMIT
    for layout in ("shared", "percode"):
        its = np.array([x[1] for x in r["ref"][layout]])
        assert (its > 0).any() and (its < 0).any(), (case, layout, r["snr"], its)
        assert ((its == -S.MAXITER) | ((its >= 0) & (its <= S.MAXITER))).all()


def test_the_model_reproduces_the_30x60_golden():
    g = S.golden(S.SHAPE_30x60)
    hard, it, soft = S.model(g["H"], g["M"], g["llr"], g["maxiter"])
    assert np.array_equal(it, g["iters"]) and np.array_equal(hard, g["hard"]) and np.array_equal(soft.view(np.uint64), g["soft"].view(np.uint64))


def test_other_gpu_inputs():
    for B in (1, 4):
        M, codes, llr = S.boundary_set(B)
        assert ((codes >= 0).sum(axis=2) >= 2).all() and S.lds_bytes(codes, M) <= S.LDS_LIMIT
        its = [S.model(codes[c], M, llr[c], S.MAXITER)[1] for c in range(3)]
        assert (its[1] == 0).all() and (its[0] < 0).all() and (its[2] < 0).all(), its      # a codeword at the input returns 0
    codes, llr = S.maxiter_one_set()
    assert set(np.unique([S.model(codes[c], 20, llr, 1)[1] for c in range(S.NCODES)])) == {-1, 1}
    codes = S.simulate_set()
    assert ((codes >= 0).sum(axis=2) >= 2).all() and len({(H >= 0).tobytes() for H in codes}) == S.SIM["C"]
    assert ((S.stop_set() >= 0).sum(axis=2) >= 2).all() and len(S.stop_set()) == 3
    for name in S.CW2:
        g = S.cw2_set(name)
        flags = [bool(((H >= 0).sum(axis=0) == 2).all()) for H in g["codes"]]
        assert flags == [True, False, True, False], name
        assert ((g["codes"] >= 0).sum(axis=2) >= 2).all() and ((g["codes"] >= 0).sum(axis=2) <= 16).all()
        assert (g["iters"] > 0).any() and (g["iters"] < 0).any(), name
    assert {S.golden(n)["M"] for n in S.CW2} == {64, 128}, "a packed and a multi-wave case"
    for name in S.LIFTINGS:
        g = S.golden_set(name, 3)
        assert len({H.tobytes() for H in g["codes"]}) == (3 if g["M"] > 1 else 1) and S.lds_bytes(g["codes"], g["M"]) <= S.LDS_LIMIT
