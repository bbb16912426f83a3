"""Integer advanced sum-product decoder (IASP_DEC, decoder id 5) without a GPU: the numpy restatement (tests/iasp_model.py) against
the compiled reference's golden vectors and, where oracle/_ref exists, against the reference itself on random shapes; the C
header and the kernel objects of the built library."""
import glob
import os
import re
import struct

import numpy as np
import pytest

from iasp_model import IASP_GOLDEN_DIR, IaspModel, channel_prior
from iasp_ref import IaspReference, iasp_ref_available
from ldpc_testlib import IASP_DEC, ROOT, awgn_llr, cycle_code, pack_bits, random_qc_code

GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(IASP_GOLDEN_DIR, "iasp_*.npz")))
needs_ref = pytest.mark.skipif(not iasp_ref_available(), reason="compiled reference (oracle/_ref) not built here")


def test_the_golden_sets_are_all_there():
    assert {"iasp_m64_2p0", "iasp_m64_1p2", "iasp_m64_0p0", "iasp_m126_1p7", "iasp_m1_4p0", "iasp_30x60_m67_2p0", "iasp_cw2_m64_2p0",
            "iasp_cw2_m128_2p0", "iasp_m64_sat"} <= set(GOLDENS)


@pytest.mark.parametrize("name", GOLDENS)
def test_model_equals_the_references_golden_vectors(name):
    g = np.load(os.path.join(IASP_GOLDEN_DIR, name + ".npz"))
    assert int(g["dec_id"]) == IASP_DEC
    soft, iters, prior, so = IaspModel(g["H"], int(g["M"])).decode(g["llr"], int(g["maxiter"]), 1)
    assert np.array_equal(iters, g["iters"])
    assert np.array_equal(pack_bits(so >> 15), g["hard"])
    assert np.array_equal(soft, g["soft"])


def test_the_weight_two_wrap_set_exercises_the_u16_wrap():
    """The 4 x 8 cycle code at M = 128 and 2 dB: a p0 that rounds to 0 gives the u16 quotient 65536 -> 0, clamped to 16, so a
    certainly-one bit reads P(1) = 1/4096.  Without the wrap the model would not match the reference (previous test)."""
    g = np.load(os.path.join(IASP_GOLDEN_DIR, "iasp_cw2_m128_2p0.npz"))
    m = IaspModel(g["H"], 128)
    assert m.all_cw2
    assert (g["iters"] < 0).sum() > 0 and (g["iters"] > 0).sum() > 0


def test_channel_prior_is_the_clamped_logistic():
    x = np.array([-25.0, -20.0, -1.5, -0.0, 0.0, 0.75, 20.0, 33.0])
    p = channel_prior(x)
    assert p[0] == p[1] and p[-1] == p[-2]
    assert p[3] == 0.5 and p[4] == 0.5
    assert np.all(np.diff(p) <= 0)


def test_rows_of_weight_one_are_refused_by_the_model():
    H = -np.ones((2, 4), dtype=np.int16)
    H[0, 0] = 0; H[1, 1] = 0; H[1, 2] = 3; H[1, 3] = 1
    with pytest.raises(ValueError):
        IaspModel(H, 8)


def _rows_of_weight(rng, rh, nh, M, w):
    """Every block row holds exactly w circulants (w <= nh), columns of weight >= 1 where possible."""
    H = -np.ones((rh, nh), dtype=np.int16)
    start = 0
    for j in range(rh):
        for q in range(w):
            H[j, (start + q) % nh] = rng.randint(0, M)
        start += max(1, w - 1)
    return H


LIVE = [  # (what, factory(rng) -> (H, M), snr, frames, maxiter)
    ("row weight 2", lambda r: (_rows_of_weight(r, 4, 6, 33, 2), 33), 3.0, 16, 30),
    ("row weight 3, M 5", lambda r: (_rows_of_weight(r, 3, 7, 5, 3), 5), 3.0, 32, 30),
    ("row weight 6, M 67", lambda r: (_rows_of_weight(r, 4, 12, 67, 6), 67), 2.5, 12, 30),
    ("row weight 9, M 128", lambda r: (_rows_of_weight(r, 4, 18, 128, 9), 128), 3.0, 8, 30),
    ("row weight 12, M 1", lambda r: (_rows_of_weight(r, 5, 20, 1, 12), 1), 4.0, 64, 20),
    ("row weight 16, M 33", lambda r: (_rows_of_weight(r, 4, 24, 33, 16), 33), 3.0, 12, 30),
    ("dual diagonal, M 67", lambda r: (random_qc_code(r, 6, 14, 67, [2, 3, 4]), 67), 2.0, 12, 40),
    ("dual diagonal, M 5", lambda r: (random_qc_code(r, 5, 12, 5, [3, 2]), 5), 3.0, 48, 40),
    ("weight-2 columns, M 33", lambda r: (cycle_code(r, 4, 8, 33), 33), 2.0, 24, 40),
    ("weight-2 columns, M 1", lambda r: (cycle_code(r, 3, 7, 1), 1), 3.0, 64, 20),
    ("weight-2 columns, M 128", lambda r: (cycle_code(r, 5, 10, 128), 128), 2.5, 16, 40),
]


@needs_ref
@pytest.mark.parametrize("i", range(len(LIVE)), ids=[w for w, *_ in LIVE])
def test_model_equals_the_live_reference_on_random_shapes(i):
    what, factory, snr, frames, maxiter = LIVE[i]
    rng = np.random.RandomState(500 + i)
    H, M = factory(rng)
    H = np.asarray(H, dtype=np.int32)
    llr = awgn_llr(H, M, snr, 11 + i, frames, burn_codeword=False)
    ref = IaspReference(H, M)
    r_soft, r_it, r_after = ref.decode(llr, maxiter, 1)
    r_hard, r_it0, _ = ref.decode(llr, maxiter, 0)
    ref.close()
    m_soft, m_it, m_prior, m_so = IaspModel(H, M).decode(llr, maxiter, 1)
    assert np.array_equal(m_it, r_it) and np.array_equal(r_it0, r_it)
    assert np.array_equal(m_soft, r_soft)
    assert np.array_equal((m_so >> 15).astype(np.float64), r_hard)
    assert np.array_equal(m_prior, r_after)           # what upstream leaves in soft[]


def test_header_defines_the_decoder_id():
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        src = f.read()
    assert re.search(r"^#define\s+LDPC_HIP_IASP_DEC\s+5\b", src, re.M)
    assert re.search(r"^#define\s+LDPC_HIP_ABI_VERSION\s+4\b", src, re.M)


def _elf_section(path, want):
    b = open(path, "rb").read()
    assert b[:4] == b"\x7fELF" and b[4] == 2
    shoff, = struct.unpack_from("<Q", b, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)
    hdr = lambda i: struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * shentsize)
    names = hdr(shstrndx)
    for i in range(shnum):
        s = hdr(i)
        start = names[4] + s[0]
        if b[start:b.index(b"\0", start)].decode() == want:
            return b[s[4]:s[4] + s[5]]
    return None


def test_library_carries_the_ahead_of_time_iasp_kernel():
    """The gfx950 code object in libldpc_hip.so's offload bundle holds the AOT instance for the example code at M = 64."""
    import ldpc_lib_amd
    so = ldpc_lib_amd.library_path()
    assert os.path.exists(so), "build() first"
    fat = _elf_section(so, ".hip_fatbin")
    assert fat is not None and fat.startswith(b"__CLANG_OFFLOAD_BUNDLE__")
    assert b"gfx950" in fat
    assert b"iasp_spec_appendix_c_m64_kernel" in fat
    assert b"_ZN4ldpc18iasp_global_kernelENS_8GlobArgsE" in fat


def test_python_and_compat_surfaces_name_the_decoder():
    import ldpc_lib_amd
    assert ldpc_lib_amd.DEC_IASP == IASP_DEC == 5
    with open(os.path.join(ROOT, "include", "ldpc", "bp_simulation.h")) as f:
        assert "LDPC_HIP_IASP_DEC" in f.read()
    with open(os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat", "decoders_compat.cpp")) as f:
        assert "decode_common(st, IASP_DEC" in f.read()
