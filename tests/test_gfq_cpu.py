"""FHT_DEC (decoder id 6, QC-LDPC codes over GF(q)) without a GPU: the numpy restatement tests/gfq_model.py against the compiled
reference's golden vectors (tests/golden/gfq/, tools/make_gfq_goldens.py) and, where oracle/_ref exists, against the live reference
on fresh frames; the field tables against brute-force polynomial multiplication; the additive C-ABI.  Soft values are compared as
uint64 images."""
import glob
import os
import re
import sys

import numpy as np
import pytest

from gfq_model import GFQ_GOLDEN_DIR, PRIMITIVE, GfqModel, bpsk_symbol_probabilities, fht, gf_tables, mul_div_tables
from gfq_ref import GfqReference, gfq_ref_available
from ldpc_testlib import ROOT, assert_bits_equal

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_gfq_goldens  # noqa: E402

GOLDENS = sorted(glob.glob(os.path.join(GFQ_GOLDEN_DIR, "*.npz")))
NEW_SYMBOLS = ("ldpc_hip_open_gfq", "ldpc_hip_gfq_q", "ldpc_hip_decode_gfq_dev", "ldpc_hip_decode_gfq_host", "ldpc_hip_gfq_coefficients")


def test_golden_sets_exist_and_are_small_data():
    names = {os.path.basename(p)[:-4] for p in GOLDENS}
    assert names == {s[0] for s in make_gfq_goldens.SETS}
    for p in GOLDENS:
        assert os.path.getsize(p) < (1 << 20), p
        assert set(np.load(p).files) == {"hb", "hc", "q_bits", "M", "ncols2convert", "maxiter", "snr", "seed", "soft", "iters", "qhard",
                                         "post", "hc_after", "state_offsets"}


def test_golden_sets_cover_what_they_are_for():
    seen_q, seen_forms = set(), set()
    for p in GOLDENS:
        g = np.load(p)
        m = GfqModel(int(g["q_bits"]), g["hb"], g["hc"], int(g["M"]), int(g["ncols2convert"]))
        seen_q.add(m.q)
        seen_forms.add("cw2" if m.cw2 else "mixed")
        if not m.cw2:
            assert {len(c) for c in m.cols} >= {2, 3}           # both other symbol-node forms
        it = g["iters"]
        if float(g["snr"]) >= 0:
            assert (it > 0).any() and (it < 0).any(), p         # converged and non-converged frames in every SNR set
        else:
            assert (it[:2] == 0).all() and not np.isfinite(g["post"]).all()   # codewords on input; Inf / NaN frames
    assert seen_q >= {4, 16, 32, 64} and seen_forms == {"cw2", "mixed"}
    big = np.load(os.path.join(GFQ_GOLDEN_DIR, "gf16_m100_2p0.npz"))
    assert int(big["M"]) > 64 and int(big["M"]) % 16 != 0
    assert int(np.load(os.path.join(GFQ_GOLDEN_DIR, "gf16_m8_n2c3_2p5.npz"))["ncols2convert"]) == 3


@pytest.mark.parametrize("path", GOLDENS, ids=lambda p: os.path.basename(p)[:-4])
def test_model_equals_golden(path):
    g = np.load(path)
    m = GfqModel(int(g["q_bits"]), g["hb"], g["hc"], int(g["M"]), int(g["ncols2convert"]))
    iters, qhard, post = m.decode(g["soft"], int(g["maxiter"]))
    assert np.array_equal(iters, g["iters"])
    assert np.array_equal(qhard, g["qhard"])
    assert_bits_equal(post, g["post"])
    assert np.array_equal(m.hc_after, g["hc_after"])
    ret0 = g["iters"] == 0
    assert_bits_equal(post[ret0], g["soft"][ret0])              # a return of 0 leaves the input in fht_soft_out


@pytest.mark.skipif(not gfq_ref_available(), reason="oracle/_ref (the compiled upstream reference) is not built here")
@pytest.mark.parametrize("q_bits,code,M,snr,n2c", [(4, "shipped", 8, 2.4, 0), (4, "shipped", 36, 1.8, 2), (4, "mixed", 12, 2.8, 0),
                                                   (6, "mixed", 5, 2.8, 4), (3, "mixed", 9, 3.2, 0), (7, "shipped", 4, 2.5, 0)])
def test_model_equals_live_reference(q_bits, code, M, snr, n2c):
    q = 1 << q_bits
    hb, hc = make_gfq_goldens.shipped(M, q) if code == "shipped" else make_gfq_goldens.mixed(M, q, seed=11)
    soft = bpsk_symbol_probabilities(np.random.RandomState(400 + q_bits + M), q_bits, hb.shape[1] * M, make_gfq_goldens.sigma_of(snr, hb), 12)
    ref = GfqReference(q_bits, hb, hc, M, n2c)
    ri, rq, rp, after = ref.decode(soft, 15)
    m = GfqModel(q_bits, hb, hc, M, n2c)
    mi, mq, mp = m.decode(soft, 15)
    assert np.array_equal(mi, ri) and np.array_equal(mq, rq)
    assert_bits_equal(mp, rp)
    assert_bits_equal(after, soft)                               # upstream does not modify its input either
    assert np.array_equal(m.hc_after, ref.coefficients())
    ref.close()


def _poly_mul(a, b, q_bits):
    """Product of two GF(2^q_bits) elements by shift-and-add with reduction by the field polynomial."""
    r = 0
    for i in range(q_bits):
        if (b >> i) & 1:
            r ^= a << i
    for i in range(2 * q_bits - 2, q_bits - 1, -1):
        if (r >> i) & 1:
            r ^= PRIMITIVE[q_bits] << (i - q_bits)
    return r


@pytest.mark.parametrize("q_bits", range(2, 11))
def test_field_tables_against_polynomial_multiplication(q_bits):
    q = 1 << q_bits
    lg, alog = gf_tables(q_bits)
    assert sorted(alog[:q - 1].tolist()) == list(range(1, q)), "the polynomial is not primitive"
    assert alog[q - 1] == 0 and lg[0] == -1
    coefs = list(range(1, q)) if q_bits <= 6 else sorted(np.random.RandomState(q_bits).choice(np.arange(1, q), 24, replace=False).tolist())
    mul, div = mul_div_tables(q_bits, coefs)
    for c, v in enumerate(coefs):
        assert mul[c, 0] == 0 and div[c, 0] == 0
        for s in range(1, q):
            assert mul[c, s] == _poly_mul(s, v, q_bits)
            assert _poly_mul(int(div[c, s]), v, q_bits) == s
        assert np.array_equal(mul[c][div[c]], np.arange(q))      # inverse permutations: what the kernels' scatter relies on


def test_transform_is_the_walsh_hadamard_matrix():
    for q in (4, 16, 32, 64):
        x = np.random.RandomState(q).rand(3, q)
        Hm = np.array([[(-1) ** bin(i & j).count("1") for j in range(q)] for i in range(q)], dtype=np.float64)
        assert np.allclose(fht(x), x @ Hm, rtol=1e-13, atol=1e-13)
        assert np.allclose(fht(fht(x)) / q, x, rtol=1e-13, atol=1e-13)


def test_header_declares_and_library_exports_the_gfq_entries():
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        header = f.read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint " + sym + r"\(", header), sym + " is not declared in include/ldpc_hip.h"
    assert re.search(r"#define LDPC_HIP_FHT_DEC 6\b", header)
    import ldpc_lib_amd
    lib = ldpc_lib_amd.load_library()
    for sym in NEW_SYMBOLS:
        assert hasattr(lib, sym), sym + " is not exported by libldpc_hip.so"
    assert hasattr(ldpc_lib_amd, "LdpcHipGfq") and ldpc_lib_amd.DEC_FHT == 6


def test_abi_version_is_still_4():
    import ldpc_lib_amd
    assert ldpc_lib_amd.load_library().ldpc_hip_abi_version() == 4
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        assert re.search(r"#define LDPC_HIP_ABI_VERSION 4\b", f.read())
