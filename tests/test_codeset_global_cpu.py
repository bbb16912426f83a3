"""The global-memory tier of a code set on the host (no GPU): the exports, the table of ldpc_hip_codes_table_global_host against a
numpy restatement, every refusal of the two entry points with its complete message (all raised before any device call: the table
builder is the open entry point's own check), the old entry points' answers to M = 513 and to the big images, the route choice of the
binding, and the properties of the inputs that test_gpu_codeset_global.py decodes."""
import ctypes as C

import numpy as np
import pytest

import codeset_global_sets as S

EINVAL, EUNSUPPORTED = -1, -2
WHO = "ldpc_hip_codes_table_global_host"
IDS = "SP_DEC (1), ASP_DEC (2), MS_DEC (3), IMS_DEC (4), IASP_DEC (5), TASP_DEC (7), LMS_DEC (8) or LCHE_DEC (9)"


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


def _rc(lib, dec, codes, M, Cn=None, fn="ldpc_hip_codes_table_global_host", takes_id=True):
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    n = C.c_longlong(-1)
    head = (int(dec),) if takes_id else ()
    rc = getattr(lib, fn)(*head, codes.shape[1], codes.shape[2], int(M), codes.ctypes.data, len(codes) if Cn is None else Cn, None, None, 0, C.byref(n))
    return rc, lib.ldpc_hip_last_error().decode() if rc else "", n.value


def test_exports(L):
    lib = L.load_library()
    for name in ("ldpc_hip_open_codes_global", "ldpc_hip_codes_table_global_host"):
        assert hasattr(lib, name)
    assert lib.ldpc_hip_abi_version() == 4


@pytest.mark.parametrize("dec", S.DECS, ids=[S.DEC_IDS[d] for d in S.DECS])
def test_table_matches_numpy(L, dec):
    M, codes = S.mixed_table_set()
    w = (codes >= 0).sum(axis=2)
    assert S.is_cw2(codes[0]) and not S.is_cw2(codes[1]) and (codes[0] >= 0).sum() != (codes[1] >= 0).sum() and 1 in w[1] and 16 in w[1]
    sets = [S.small_set(m, k) for m in S.LIFTINGS for k in "AB"]
    if dec not in S.MIN_RW2:
        sets.append(codes)
    for cs in sets:
        if dec in S.MIN_RW2 and (cs >= 0).sum(axis=2).min() < 2:
            continue
        m = M if cs is codes else int(cs.max()) + 1
        off, tab = L.codes_table(dec, cs, m, tier="global")
        want_off, want_tab = S.table_np(cs)
        assert np.array_equal(off, want_off) and np.array_equal(tab, want_tab)
        ne = int((cs >= 0).sum())
        assert len(tab) == len(cs) * (cs.shape[1] + cs.shape[2] + 3) + 3 * ne


@pytest.mark.parametrize("dec", S.DECS, ids=[S.DEC_IDS[d] for d in S.DECS])
def test_refusals(L, dec):
    lib = L.load_library()
    ok = np.zeros((1, 2, 4), dtype=np.int16)
    assert _rc(lib, dec, ok, 513)[0] == 0 and _rc(lib, dec, ok, 1)[0] == 0 and _rc(lib, dec, ok, 32767)[0] == 0
    for M in (0, -1):
        assert _rc(lib, dec, ok, M)[:2] == (EINVAL, f"{WHO}: bad argument")
    n = C.c_longlong()
    assert lib.ldpc_hip_codes_table_global_host(dec, 2, 4, 5, None, 1, None, None, 0, C.byref(n)) == EINVAL
    assert lib.ldpc_hip_last_error().decode() == f"{WHO}: bad argument"
    for Cn in (0, -3):
        assert _rc(lib, dec, ok, 5, Cn=Cn)[:2] == (EINVAL, f"{WHO}: C = {Cn}, a code set holds at least one code")
    two = np.zeros((2, 2, 4), dtype=np.int16)
    for v in (-2, 5):
        bad = two.copy(); bad[1, 1, 2] = v
        assert _rc(lib, dec, bad, 5)[:2] == (EINVAL, f"{WHO}: code 1, shift {v} at (1, 2) is outside [-1, 5)")
    bad = two.copy(); bad[1, 0, :] = -1
    assert _rc(lib, dec, bad, 5)[:2] == (EINVAL, f"{WHO}: code 1, block row 0 is empty")
    bad = two.copy(); bad[1, :, 3] = -1
    assert _rc(lib, dec, bad, 5)[:2] == (EINVAL, f"{WHO}: code 1, block column 3 is empty")
    bad = two.copy(); bad[1, 1, 1:] = -1
    rc, msg, _ = _rc(lib, dec, bad, 5)
    if dec in S.MIN_RW2:
        assert (rc, msg) == (EINVAL, f"{WHO}: code 1, block row 1 has weight 1; {S.NAMES[dec]} needs at least 2")
    else:
        assert rc == 0
    # a row of weight 1025: LCHE alone refuses it (upstream's map_bin_llr holds 1024 edges)
    wide = np.zeros((1, 2, 1025), dtype=np.int16)
    rc, msg, _ = _rc(lib, dec, wide, 2)
    if dec == S.LCHE_DEC:
        assert (rc, msg) == (EUNSUPPORTED, f"{WHO}: code 0, block row 0 has weight 1025; at most 1024")
    else:
        assert rc == 0
    # the workspace: 8 x 64 dense at M = 32767, TDMP's four per-edge arrays
    big = np.zeros((1, 8, 64), dtype=np.int16)
    rc, msg, _ = _rc(lib, dec, big, 32767)
    if dec == S.TASP_DEC:
        N, R, ne = 64 * 32767, 8 * 32767, 512
        al = lambda x: (x + 15) & ~15
        slice_bytes = 2 * al(8 * N) + 2 * al(8 * R) + al(4 * R) + al(R) + al(ne * 32767) + 4 * al(8 * ne * 32767)
        assert slice_bytes > 512 << 20
        assert (rc, msg) == (EUNSUPPORTED, f"{WHO}: a workgroup's workspace slice for {N} variables, {R} checks and 512 circulants x 32767 is "
                             f"{slice_bytes} bytes; the limit is {512 << 20} (16 slices within 8 GiB)")
    rc, msg, _ = _rc(lib, dec, np.zeros((1, 1, 65536), dtype=np.int16), 2)
    assert (rc, msg) == (EUNSUPPORTED, f"{WHO}: M = 2, rh = 1, nh = 65536; an edge word holds a shift and a block row or column in 16 bits each: "
                         "all below 65536")
    rc, msg, _ = _rc(lib, dec, np.zeros((1, 1, 16384), dtype=np.int16), 16384)
    assert (rc, msg) == (EUNSUPPORTED, f"{WHO}: code length nh * M = {1 << 28}: at most 2^28 - 1 is supported (32-bit indices)")


def test_other_ids_and_open_refuses_before_the_device(L):
    lib = L.load_library()
    ok = np.zeros((1, 2, 4), dtype=np.int16)
    for dec in (0, 6, 10, -1):
        assert _rc(lib, dec, ok, 5)[:2] == (EINVAL, f"{WHO}: decoder id {dec}; {IDS}")
        h = C.c_void_p(1)
        assert lib.ldpc_hip_open_codes_global(dec, 2, 4, 5, ok.ctypes.data, 1, 0, C.byref(h)) == EINVAL and not h.value
        assert lib.ldpc_hip_last_error().decode() == f"ldpc_hip_open_codes_global: decoder id {dec}; {IDS}"
    bad = ok.copy(); bad[0, 0, :] = -1     # no GPU on this machine: a structural refusal comes first, under the entry point's name
    h = C.c_void_p(1)
    assert lib.ldpc_hip_open_codes_global(3, 2, 4, 5, bad.ctypes.data, 1, 0, C.byref(h)) == EINVAL and not h.value
    assert lib.ldpc_hip_last_error().decode() == "ldpc_hip_open_codes_global: code 0, block row 0 is empty"
    assert lib.ldpc_hip_open_codes_global(3, 2, 4, 5, ok.ctypes.data, 1, 0, None) == EINVAL


def test_old_entry_points_keep_their_answers(L):
    """M = 513 and the images beyond 160 KiB, as test_codeset_refusals_cpu.py records them."""
    lib = L.load_library()
    ok = np.zeros((1, 2, 4), dtype=np.int16)
    for fn, dec, takes in (("ldpc_hip_codes_table_host", 3, True), ("ldpc_hip_codes_table_host", 5, True), ("ldpc_hip_codes_table_host", 7, True),
                           ("ldpc_hip_codes_table_host", 8, True), ("ldpc_hip_codes_table_sp_host", 1, True), ("ldpc_hip_codes_table_sp_host", 2, True),
                           ("ldpc_hip_codes_table_lche_host", 9, False), ("ldpc_hip_codes_table_ims_host", 4, False),
                           ("ldpc_hip_codes_table_wide_host", 3, True)):
        assert _rc(lib, dec, ok, 513, fn=fn, takes_id=takes)[:2] == (EINVAL, f"{fn}: M = 513, the resident table kernels take M <= 512")
    from codeset_iasp_sets import big_image_set
    from ldpc_testlib import load_base_matrix, relift
    appc = relift(load_base_matrix(), 256).astype(np.int16)[None]
    assert _rc(lib, 7, appc, 256, fn="ldpc_hip_codes_table_host")[:2] == (
        EUNSUPPORTED, "ldpc_hip_codes_table_host: 1 frame(s) per wave x (8192 a-posteriori values + 112 circulants x 256 checks) need an LDS image of "
        "294928 bytes; the limit is 160 KiB")
    rc, msg, _ = _rc(lib, 5, big_image_set(), 512, fn="ldpc_hip_codes_table_host")
    assert rc == EUNSUPPORTED and msg.endswith("halfwords need an LDS image of 180240 bytes; the limit is 160 KiB"), msg
    for dec in (7, 5):   # and the new entry point takes both
        assert _rc(lib, dec, appc if dec == 7 else big_image_set(), 256 if dec == 7 else 512)[0] == 0


@pytest.mark.parametrize("dec", S.DECS, ids=[S.DEC_IDS[d] for d in S.DECS])
def test_route_choice_of_the_binding(L, dec):
    """Seen through the name in front of a refusal (an empty block row), raised before any device call."""
    own = {1: "_sp", 2: "_sp", 4: "_ims", 5: "_iasp", 7: "_tdmp", 9: "_lche"}.get(dec, "")
    own_table = {1: "_sp", 2: "_sp", 4: "_ims", 9: "_lche"}.get(dec, "")
    for M, tier, glob in ((4, "auto", False), (512, "auto", False), (513, "auto", True), (4, "global", True), (4100, "auto", True)):
        bad = np.zeros((2, 2, 4), dtype=np.int16)
        bad[1, 1, :] = -1
        with pytest.raises(L.LdpcHipError) as e:
            L.codes_table(dec, bad, M, tier=tier)
        name = "ldpc_hip_codes_table_global_host" if glob else f"ldpc_hip_codes_table{own_table}_host"
        assert str(e.value).startswith(f"{name}: {name}: code 1, block row 1 is empty"), str(e.value)
        with pytest.raises(L.LdpcHipError) as e:
            L.LdpcHipCodes(dec, bad, M, tier=tier)
        name = "ldpc_hip_open_codes_global" if glob else f"ldpc_hip_open_codes{own}"
        assert str(e.value).startswith(f"{name}: {name}: code 1, block row 1 is empty"), str(e.value)
    with pytest.raises(ValueError):
        L.codes_table(dec, np.zeros((1, 2, 4), dtype=np.int16), 4, tier="lds")


@pytest.mark.parametrize("M", S.LIFTINGS)
@pytest.mark.parametrize("dec", S.DECS, ids=[S.DEC_IDS[d] for d in S.DECS])
def test_parity_inputs_have_the_required_properties(M, dec):
    r = S.reference(M, dec)
    codes = r["codes"]
    ne = [(H >= 0).sum() for H in codes]
    w = (codes >= 0).sum(axis=2)
    assert len(set(ne)) == 3 and codes.shape == (3, 4, 8)
    if dec in S.MIN_RW2:
        assert w.min() >= 2 and [S.is_cw2(H) for H in codes] == [True, False, False]
    else:
        assert w.min() == 1
    its = np.array([[x[1] for x in r["ref"][layout]] for layout in ("shared", "percode")])
    assert ((its == -S.MAXITER) | ((its >= 0) & (its <= S.MAXITER))).all()
    assert (its >= 0).sum() >= 1 and (its == -S.MAXITER).sum() >= 1 and (its >= 3).sum() >= 1, its


def test_other_gpu_inputs():
    for M in (513, 4100):
        a, b = S.beyond_set(M)
        assert S.is_cw2(a) and not S.is_cw2(b) and (a >= 0).sum() == 8 and (b >= 0).sum() == 7 and (b >= 0).sum(axis=1).min() >= 2
    codes, llr, ref = S.appendix_c_m256()
    assert codes.shape == (2, 16, 32) and llr.shape == (8, 8192) and max(int((H >= 0).sum()) for H in codes) == 112
    its = np.array([r[1] for r in ref])
    assert (its > 0).any() and (its == -15).any() and (its >= 3).any(), its
    for dec in S.DECS:
        codes = S.both_routes_set(dec)
        assert len({int((H >= 0).sum()) for H in codes}) == 3 and ((codes >= 0).sum(axis=1) >= 1).all()
        assert (codes >= 0).sum(axis=2).min() >= (2 if dec in S.MIN_RW2 else 1)
