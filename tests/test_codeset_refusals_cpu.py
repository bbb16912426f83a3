"""The refusals of the code-set table builder without a GPU, word for word: every refusal through the entry point of each route
(ldpc_hip_codes_table_host, _sp_host, _lche_host, _ims_host; the open entry points share the builder), on the smallest input that
trips it.  The other test_codeset_*_cpu.py look for substrings; this one pins the complete message and the return code."""
import ctypes as C

import numpy as np
import pytest

from codeset_ims_sets import dense_set
from ldpc_testlib import load_base_matrix, relift

EINVAL, EUNSUPPORTED = -1, -2
E = -1
# route -> (entry point, whether it takes the decoder id).  The two open entry points are here for the ids they refuse, which they do
# before any device call.
ROUTES = {"generic": ("ldpc_hip_codes_table_host", True), "sp": ("ldpc_hip_codes_table_sp_host", True),
          "lche": ("ldpc_hip_codes_table_lche_host", False), "ims": ("ldpc_hip_codes_table_ims_host", False),
          "open": ("ldpc_hip_open_codes", True), "open sp": ("ldpc_hip_open_codes_sp", True)}
OK = [[[0, 1, E, 4], [E, 0, 2, 3]]]     # 2 x 4 at M = 5: every row weight >= 2, no empty column, shifts within [0, M)


def _ok(cells={}):
    """OK twice, with the changes {(row, column): value} in code 1."""
    H = np.array(OK * 2, dtype=np.int16)
    for (j, k), v in cells.items():
        H[1, j, k] = v
    return H


def _appendix_c(M):
    """The 16 x 32 base matrix of Appendix C (112 circulants) at lifting M: the shape of the test_lds_* tests."""
    base = load_base_matrix()
    return np.where(base >= 0, relift(base, M) % M, -1).astype(np.int16)[None]


# ldpc_hip_codes_table_host on an id that it does not serve
NOT_SERVED = ("ldpc_hip_codes_table_host: decoder id %d; a code set decodes with MS_DEC (3), IASP_DEC (5), TASP_DEC (7) or LMS_DEC (8), with LCHE_DEC (9) "
              "through ldpc_hip_open_codes_lche / ldpc_hip_codes_table_lche_host and with IMS_DEC (4) through ldpc_hip_open_codes_ims / "
              "ldpc_hip_codes_table_ims_host, and with SP_DEC (1) or ASP_DEC (2) through ldpc_hip_open_codes_sp / ldpc_hip_codes_table_sp_host")

# defect -> (codes [C, rh, nh], M, C as passed)
DEFECTS = {
    "ok": lambda: (_ok(), 5, 2),
    "C = 0": lambda: (_ok(), 5, 0),
    "M = 513": lambda: (_ok(), 513, 2),
    "rh = 17": lambda: (np.zeros((1, 17, 2), dtype=np.int16), 1, 1),
    "nh = 33": lambda: (np.zeros((1, 2, 33), dtype=np.int16), 1, 1),
    "shift M": lambda: (_ok({(1, 2): 5}), 5, 2),
    "empty row": lambda: (_ok({(0, 0): E, (0, 1): E, (0, 3): E}), 5, 2),
    "empty column": lambda: (_ok({(0, 0): E}), 5, 2),
    "weight 17": lambda: (np.zeros((1, 2, 17), dtype=np.int16), 1, 1),
    "weight 1": lambda: (_ok({(0, 1): E, (0, 3): E}), 5, 2),
    "lds 2 x 41, M = 512": lambda: (np.zeros((1, 2, 41), dtype=np.int16), 512, 1),
    "lds 20 x 40, M = 512": lambda: (dense_set(20, 40, 512), 512, 1),
    "lds 16 x 32, M = 256": lambda: (_appendix_c(256), 256, 1),
    "lds 16 x 32, M = 512": lambda: (_appendix_c(512), 512, 1),
}

# (route, decoder id, defect, return code, message)
CASES = [
    ("generic", 0, "ok", EINVAL, NOT_SERVED % 0),
    ("generic", 1, "ok", EINVAL, NOT_SERVED % 1),
    ("generic", 2, "ok", EINVAL, NOT_SERVED % 2),
    ("generic", 4, "ok", EINVAL, NOT_SERVED % 4),
    ("generic", 6, "ok", EINVAL, NOT_SERVED % 6),
    ("generic", 9, "ok", EINVAL, NOT_SERVED % 9),
    ("generic", 10, "ok", EINVAL, NOT_SERVED % 10),
    ("sp", 0, "ok", EINVAL, "ldpc_hip_codes_table_sp_host: decoder id 0; SP_DEC (1) or ASP_DEC (2)"),
    ("sp", 3, "ok", EINVAL, "ldpc_hip_codes_table_sp_host: decoder id 3; SP_DEC (1) or ASP_DEC (2)"),
    ("sp", 9, "ok", EINVAL, "ldpc_hip_codes_table_sp_host: decoder id 9; SP_DEC (1) or ASP_DEC (2)"),
    ("open", 1, "ok", EINVAL, "ldpc_hip_open_codes: decoder id 1; a code set decodes with MS_DEC (3) or LMS_DEC (8)"),
    ("open", 5, "ok", EINVAL, "ldpc_hip_open_codes: decoder id 5; a code set decodes with MS_DEC (3) or LMS_DEC (8)"),
    ("open", 9, "ok", EINVAL, "ldpc_hip_open_codes: decoder id 9; a code set decodes with MS_DEC (3) or LMS_DEC (8)"),
    ("open sp", 0, "ok", EINVAL, "ldpc_hip_open_codes_sp: decoder id 0; SP_DEC (1) or ASP_DEC (2)"),
    ("open sp", 3, "ok", EINVAL, "ldpc_hip_open_codes_sp: decoder id 3; SP_DEC (1) or ASP_DEC (2)"),
    ("open sp", 9, "ok", EINVAL, "ldpc_hip_open_codes_sp: decoder id 9; SP_DEC (1) or ASP_DEC (2)"),
    ("generic", 3, "ok", 0, ""),
    ("generic", 5, "ok", 0, ""),
    ("generic", 7, "ok", 0, ""),
    ("generic", 8, "ok", 0, ""),
    ("sp", 1, "ok", 0, ""),
    ("sp", 2, "ok", 0, ""),
    ("lche", 9, "ok", 0, ""),
    ("ims", 4, "ok", 0, ""),
    ("generic", 3, "C = 0", EINVAL, "ldpc_hip_codes_table_host: C = 0, a code set holds at least one code"),
    ("generic", 5, "C = 0", EINVAL, "ldpc_hip_codes_table_host: C = 0, a code set holds at least one code"),
    ("generic", 7, "C = 0", EINVAL, "ldpc_hip_codes_table_host: C = 0, a code set holds at least one code"),
    ("generic", 8, "C = 0", EINVAL, "ldpc_hip_codes_table_host: C = 0, a code set holds at least one code"),
    ("sp", 1, "C = 0", EINVAL, "ldpc_hip_codes_table_sp_host: C = 0, a code set holds at least one code"),
    ("sp", 2, "C = 0", EINVAL, "ldpc_hip_codes_table_sp_host: C = 0, a code set holds at least one code"),
    ("lche", 9, "C = 0", EINVAL, "ldpc_hip_codes_table_lche_host: C = 0, a code set holds at least one code"),
    ("ims", 4, "C = 0", EINVAL, "ldpc_hip_codes_table_ims_host: C = 0, a code set holds at least one code"),
    ("generic", 3, "M = 513", EINVAL, "ldpc_hip_codes_table_host: M = 513, the resident table kernels take M <= 512"),
    ("generic", 5, "M = 513", EINVAL, "ldpc_hip_codes_table_host: M = 513, the resident table kernels take M <= 512"),
    ("generic", 7, "M = 513", EINVAL, "ldpc_hip_codes_table_host: M = 513, the resident table kernels take M <= 512"),
    ("generic", 8, "M = 513", EINVAL, "ldpc_hip_codes_table_host: M = 513, the resident table kernels take M <= 512"),
    ("sp", 1, "M = 513", EINVAL, "ldpc_hip_codes_table_sp_host: M = 513, the resident table kernels take M <= 512"),
    ("sp", 2, "M = 513", EINVAL, "ldpc_hip_codes_table_sp_host: M = 513, the resident table kernels take M <= 512"),
    ("lche", 9, "M = 513", EINVAL, "ldpc_hip_codes_table_lche_host: M = 513, the resident table kernels take M <= 512"),
    ("ims", 4, "M = 513", EINVAL, "ldpc_hip_codes_table_ims_host: M = 513, the resident table kernels take M <= 512"),
    ("generic", 3, "shift M", EINVAL, "ldpc_hip_codes_table_host: code 1, shift 5 at (1, 2) is outside [-1, 5)"),
    ("generic", 5, "shift M", EINVAL, "ldpc_hip_codes_table_host: code 1, shift 5 at (1, 2) is outside [-1, 5)"),
    ("generic", 7, "shift M", EINVAL, "ldpc_hip_codes_table_host: code 1, shift 5 at (1, 2) is outside [-1, 5)"),
    ("generic", 8, "shift M", EINVAL, "ldpc_hip_codes_table_host: code 1, shift 5 at (1, 2) is outside [-1, 5)"),
    ("sp", 1, "shift M", EINVAL, "ldpc_hip_codes_table_sp_host: code 1, shift 5 at (1, 2) is outside [-1, 5)"),
    ("sp", 2, "shift M", EINVAL, "ldpc_hip_codes_table_sp_host: code 1, shift 5 at (1, 2) is outside [-1, 5)"),
    ("lche", 9, "shift M", EINVAL, "ldpc_hip_codes_table_lche_host: code 1, shift 5 at (1, 2) is outside [-1, 5)"),
    ("ims", 4, "shift M", EINVAL, "ldpc_hip_codes_table_ims_host: code 1, shift 5 at (1, 2) is outside [-1, 5)"),
    ("generic", 3, "empty row", EINVAL, "ldpc_hip_codes_table_host: code 1, block row 0 is empty"),
    ("generic", 5, "empty row", EINVAL, "ldpc_hip_codes_table_host: code 1, block row 0 is empty"),
    ("generic", 7, "empty row", EINVAL, "ldpc_hip_codes_table_host: code 1, block row 0 is empty"),
    ("generic", 8, "empty row", EINVAL, "ldpc_hip_codes_table_host: code 1, block row 0 is empty"),
    ("sp", 1, "empty row", EINVAL, "ldpc_hip_codes_table_sp_host: code 1, block row 0 is empty"),
    ("sp", 2, "empty row", EINVAL, "ldpc_hip_codes_table_sp_host: code 1, block row 0 is empty"),
    ("lche", 9, "empty row", EINVAL, "ldpc_hip_codes_table_lche_host: code 1, block row 0 is empty"),
    ("ims", 4, "empty row", EINVAL, "ldpc_hip_codes_table_ims_host: code 1, block row 0 is empty"),
    ("generic", 3, "empty column", EINVAL, "ldpc_hip_codes_table_host: code 1, block column 0 is empty"),
    ("generic", 5, "empty column", EINVAL, "ldpc_hip_codes_table_host: code 1, block column 0 is empty"),
    ("generic", 7, "empty column", EINVAL, "ldpc_hip_codes_table_host: code 1, block column 0 is empty"),
    ("generic", 8, "empty column", EINVAL, "ldpc_hip_codes_table_host: code 1, block column 0 is empty"),
    ("sp", 1, "empty column", EINVAL, "ldpc_hip_codes_table_sp_host: code 1, block column 0 is empty"),
    ("sp", 2, "empty column", EINVAL, "ldpc_hip_codes_table_sp_host: code 1, block column 0 is empty"),
    ("lche", 9, "empty column", EINVAL, "ldpc_hip_codes_table_lche_host: code 1, block column 0 is empty"),
    ("ims", 4, "empty column", EINVAL, "ldpc_hip_codes_table_ims_host: code 1, block column 0 is empty"),
    ("generic", 3, "weight 17", EINVAL, "ldpc_hip_codes_table_host: code 0, block row 0 has weight 17; at most 16"),
    ("generic", 5, "weight 17", EINVAL, "ldpc_hip_codes_table_host: code 0, block row 0 has weight 17; at most 16"),
    ("generic", 7, "weight 17", EINVAL, "ldpc_hip_codes_table_host: code 0, block row 0 has weight 17; at most 16"),
    ("generic", 8, "weight 17", EINVAL, "ldpc_hip_codes_table_host: code 0, block row 0 has weight 17; at most 16"),
    ("sp", 1, "weight 17", 0, ""),
    ("sp", 2, "weight 17", EINVAL, "ldpc_hip_codes_table_sp_host: code 0, block row 0 has weight 17; at most 16"),
    ("lche", 9, "weight 17", EINVAL, "ldpc_hip_codes_table_lche_host: code 0, block row 0 has weight 17; at most 16"),
    ("ims", 4, "weight 17", EINVAL, "ldpc_hip_codes_table_ims_host: code 0, block row 0 has weight 17; at most 16"),
    ("generic", 3, "weight 1", 0, ""),
    ("generic", 5, "weight 1", EINVAL, "ldpc_hip_codes_table_host: code 1, block row 0 has weight 1; integer advanced sum-product needs at least 2"),
    ("generic", 7, "weight 1", EINVAL, "ldpc_hip_codes_table_host: code 1, block row 0 has weight 1; TDMP sum-product needs at least 2"),
    ("generic", 8, "weight 1", 0, ""),
    ("sp", 1, "weight 1", 0, ""),
    ("sp", 2, "weight 1", EINVAL, "ldpc_hip_codes_table_sp_host: code 1, block row 0 has weight 1; advanced sum-product needs at least 2"),
    ("lche", 9, "weight 1", 0, ""),
    ("ims", 4, "weight 1", 0, ""),
    ("generic", 3, "rh = 17", EINVAL, "ldpc_hip_codes_table_host: rh = 17, the resident table kernels take 16 block rows"),
    ("generic", 7, "rh = 17", EINVAL, "ldpc_hip_codes_table_host: rh = 17, the resident table kernels take 16 block rows"),
    ("generic", 8, "rh = 17", EINVAL, "ldpc_hip_codes_table_host: rh = 17, the resident table kernels take 16 block rows"),
    ("generic", 3, "nh = 33", EINVAL, "ldpc_hip_codes_table_host: nh = 33, the flooding table kernel keeps the channel LLRs of 32 block columns in "
     "registers"),
    ("generic", 8, "lds 2 x 41, M = 512", EUNSUPPORTED, "ldpc_hip_codes_table_host: code length 20992 x 1 frames per wave does not fit the 160 KiB "
     "LDS image"),
    ("generic", 7, "lds 2 x 41, M = 512", EUNSUPPORTED, "ldpc_hip_codes_table_host: code length 20992 x 1 frames per wave does not fit the 160 KiB "
     "LDS image"),
    ("ims", 4, "lds 20 x 40, M = 512", EUNSUPPORTED, "ldpc_hip_codes_table_ims_host: 1 frame(s) per wave x (4 x 20480 variables + 8 x 10240 checks) "
     "bytes, rounded up to 16, + 16 need an LDS image of 163856 bytes; the limit is 160 KiB"),
    ("generic", 7, "lds 16 x 32, M = 256", EUNSUPPORTED, "ldpc_hip_codes_table_host: 1 frame(s) per wave x (8192 a-posteriori values + 112 circulants "
     "x 256 checks) need an LDS image of 294928 bytes; the limit is 160 KiB"),
    ("generic", 5, "lds 16 x 32, M = 512", EUNSUPPORTED, "ldpc_hip_codes_table_host: 1 frame(s) per wave x (112 circulants x 512 checks + 2 x 16384 "
     "variables) halfwords need an LDS image of 180240 bytes; the limit is 160 KiB"),
    ("lche", 9, "lds 16 x 32, M = 512", EUNSUPPORTED, "ldpc_hip_codes_table_lche_host: 1 frame(s) per wave x (16384 a-posteriori LLRs + 112 "
     "circulants x 512 checks) and the tables of logexp need an LDS image of 592320 bytes; the limit is 160 KiB"),
    ("sp", 1, "lds 16 x 32, M = 512", EUNSUPPORTED, "ldpc_hip_codes_table_sp_host: one frame's image, 8 x (112 circulants x 512 + 16384 variables + "
     "the checks) + 4 x 512 bytes, rounded up to 16, + 16 is 657424 bytes; the limit is 160 KiB"),
    ("sp", 2, "lds 16 x 32, M = 512", EUNSUPPORTED, "ldpc_hip_codes_table_sp_host: one frame's image, 8 x (112 circulants x 512 + 16384 variables) + "
     "4 x 512 bytes, rounded up to 16, + 16 is 591888 bytes; the limit is 160 KiB"),
]


def _call(lib, route, dec, defect):
    codes, M, Cn = DEFECTS[defect]()
    codes = np.ascontiguousarray(codes, dtype=np.int16).reshape((-1,) + codes.shape[-2:])
    name, takes_id = ROUTES[route]
    out = (0, C.byref(C.c_void_p())) if route.startswith("open") else (None, None, 0, C.byref(C.c_longlong()))
    rc = getattr(lib, name)(*((dec,) if takes_id else ()), codes.shape[1], codes.shape[2], M, codes.ctypes.data, Cn, *out)
    return rc, lib.ldpc_hip_last_error().decode() if rc else ""


@pytest.fixture(scope="module")
def lib():
    import ldpc_lib_amd
    return ldpc_lib_amd.load_library()


@pytest.mark.parametrize("route,dec,defect,want_rc,want", CASES, ids=["%s-%s-%s" % c[:3] for c in CASES])
def test_refusal(lib, route, dec, defect, want_rc, want):
    got = _call(lib, route, dec, defect)
    print(got)
    assert got == (want_rc, want)
