"""LCHE_DEC (decoder id 9) without a GPU: the generated phi tables, the numpy restatement tests/lche_model.py against the compiled
reference's golden vectors (tests/golden/lche/, tools/make_lche_goldens.py) and, where oracle/_ref exists, against the live
reference on AWGN, adversarial and boundary frames.  Soft values are compared as uint64 images (the sign of zero included)."""
import glob
import math
import os
import sys
from decimal import Decimal

import numpy as np
import pytest

from lche_model import LCHE_GOLDEN_DIR, LcheModel, logexp_int
from lche_ref import LcheReference, lche_ref_available
from ldpc_testlib import ROOT, adversarial_llr, assert_bits_equal, awgn_llr, load_base_matrix, pack_bits, relift

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_lche_table  # noqa: E402
import make_lche_goldens  # noqa: E402

GOLDENS = sorted(glob.glob(os.path.join(LCHE_GOLDEN_DIR, "lche_*.npz")))


def test_committed_table_header_is_the_generated_one():
    with open(gen_lche_table.HEADER) as f:
        assert f.read() == gen_lche_table.header(), "ldpc-lib_amd/csrc/lche_table.hpp is stale: run tools/gen_lche_table.py"


def test_tables_follow_the_phi_rounding_rule():
    a, b, c = gen_lche_table.tables()
    assert len(a) == len(b) == len(c) == 32
    for k in range(32):
        assert a[k] == float("%.2e" % float(gen_lche_table.phi(Decimal(k + 1) / 2)))
        assert b[k] == round(float(gen_lche_table.phi(Decimal(k + 1) / 16)), 2)
        assert c[k] == round(float(gen_lche_table.phi(Decimal(k + 1) / 512)), 2)
    assert (a[0], b[0], c[0], c[31]) == (1.41, 3.47, 6.93, 3.47)


def test_step_sums_are_sequential_subtraction():
    s = gen_lche_table.steps()
    assert len(s) == 214 and s[0] == 0.0
    acc = 0.0
    for k in range(1, 214):
        acc -= 3.46
        assert s[k] == acc
    assert s[213] != -3.46 * 213   # rounded step by step, not a product


def test_logexp_small_argument_loop():
    """The smallest subnormal takes 213 passes; signed zero is clamped like +0."""
    x = np.array([5e-324, 0.0, -0.0, 1.0 / 512, 16.0, 1e300])
    got = logexp_int(x)
    s = gen_lche_table.steps()
    _, _, c = gen_lche_table.tables()
    assert got[0] == s[213] - c[int(512 * math.ldexp(5e-324, 5 * 213) + 0.5) - 1]
    assert got[1] == got[2] == s[1] - c[3]
    assert got[3] == -c[0] and got[4] == got[5] == -gen_lche_table.tables()[0][31]


def test_golden_sets_exist():
    names = {os.path.basename(p)[:-4] for p in GOLDENS}
    assert names == {s[0] for s in make_lche_goldens.SETS}
    for p in GOLDENS:
        assert os.path.getsize(p) < 1 << 20


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[:-4] for p in GOLDENS])
def test_model_equals_the_golden_vectors(path):
    g = np.load(path)
    H, M = g["H"], int(g["M"])
    dec, its, soft = LcheModel(H, M).decode(g["llr"], int(g["maxiter"]))
    assert np.array_equal(its, g["iters"])
    assert np.array_equal(pack_bits(dec), g["hard"])
    assert_bits_equal(soft, g["soft"])
    zero = its == 0                      # a codeword at entry: the input itself comes back
    assert_bits_equal(soft[zero], g["llr"][zero])


needs_ref = pytest.mark.skipif(not lche_ref_available(), reason="oracle/_ref (the compiled reference) is absent")


def _vs_reference(H, M, llr, maxiter):
    ref = LcheReference(H, M)
    dec, its, soft, after = ref.decode(llr, maxiter)
    ref.close()
    assert_bits_equal(after, llr)        # upstream leaves its input alone
    m_dec, m_its, m_soft = LcheModel(H, M).decode(llr, maxiter)
    assert np.array_equal(m_its, its)
    assert np.array_equal(m_dec, dec)
    assert_bits_equal(m_soft, soft)


@needs_ref
@pytest.mark.parametrize("snr", [0.5, 1.5, 2.5])
def test_model_equals_the_live_reference_on_awgn(snr):
    H = relift(load_base_matrix(), 64)
    _vs_reference(H, 64, awgn_llr(H, 64, snr, 400 + int(10 * snr), 12), 50)


@needs_ref
@pytest.mark.parametrize("M", [64, 5, 33])
def test_model_equals_the_live_reference_on_adversarial_frames(M):
    H = relift(load_base_matrix(), M)
    llr, _ = adversarial_llr(H, M, 11)
    _vs_reference(H, M, llr, 30)


@needs_ref
@pytest.mark.parametrize("M", [64, 5])
def test_model_equals_the_live_reference_on_boundary_frames(M):
    H = relift(load_base_matrix(), M)
    llr = make_lche_goldens.boundary(H, M, awgn_llr(H, M, 2.0, 23, 8))
    _vs_reference(H, M, llr, 30)
