"""CPU, where oracle/_ref was built: the two references the GPU suite checks against -- the C restatement (Oracle, liboracle.so) and,
for decoder 5, the numpy model (tests/iasp_model.py) -- against the compiled upstream decoders on the adversarial channel values of
ldpc_testlib.adversarial_llr: iteration counts, decisions 0 and 1 and the clobbered input, bit for bit (the sign of zero included)."""
import numpy as np
import pytest

from iasp_model import IaspModel
from iasp_ref import IaspReference, iasp_ref_available
from ldpc_testlib import (ASP_DEC, BP_DEC, IMS_DEC, LMS_DEC, MS_DEC, SP_DEC, TASP_DEC, Oracle, Reference, adversarial_llr, assert_bits_equal,
                          load_base_matrix, ref_lib, relift)

pytestmark = pytest.mark.skipif(ref_lib() is None, reason="oracle/_ref not built (needs the upstream tree)")

DECODERS = {"ms": MS_DEC, "lms": LMS_DEC, "ims": IMS_DEC, "sp": SP_DEC, "asp": ASP_DEC, "tasp": TASP_DEC, "bp": BP_DEC}
LIFTINGS = [64, 5, 33]        # the example code, a small lifting and an odd one
MAXITER = 20


def test_the_adversarial_batch_is_finite_deterministic_and_covers_the_families():
    H = relift(load_base_matrix(), 64)
    a, la = adversarial_llr(H, 64, 3)
    b, lb = adversarial_llr(H, 64, 3)
    assert la == lb and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.isfinite(a).all()
    bits = a.view(np.uint64)
    assert ((bits == 0x8000000000000000).sum(axis=1) == a.shape[1]).any()                  # a whole frame of -0.0
    assert (np.abs(a) == 20.0).any() and (np.abs(a) == 40.0).any()
    assert (np.abs(a) == np.nextafter(20.0, 99)).any() and (np.abs(a) == np.nextafter(40.0, 0)).any()
    sub = (a != 0) & (np.abs(a) < 2.2250738585072014e-308)
    assert sub.any() and (np.abs(a) > 1e199).any()
    for fam in ("+0.0", "-0.0", "+-1e-310 subnormals", "+-1e-170, squares underflow", "+-1e200", "a codeword", "all negative",
                "integer quantiser boundaries", "awgn with +-20 / +-40 and neighbours", "awgn, every 5th -0.0"):
        assert fam in la, fam


@pytest.mark.parametrize("M", LIFTINGS)
@pytest.mark.parametrize("name", list(DECODERS))
def test_restatement_equals_compiled_reference_on_adversarial_frames(name, M):
    dec_id = DECODERS[name]
    H = relift(load_base_matrix(), M)
    llr, labels = adversarial_llr(H, M, 7)
    for decision in (0, 1) if dec_id != TASP_DEC else (0,):    # TASP: `decision` is dead upstream; the oracle's 1 returns posteriors
        # fresh states for both: Gallager BP carries its syndrome from call to call
        d1, i1, a1 = Oracle(H, M).decode(dec_id, llr, MAXITER, decision)
        d2, i2, a2 = Reference(dec_id, H, M).decode(dec_id, llr, MAXITER, decision)
        bad = np.flatnonzero(i1 != i2)
        assert not bad.size, f"iterations differ on {[labels[f] for f in bad]}: {i1[bad]} vs {i2[bad]}"
        for f in range(len(llr)):
            assert_bits_equal(d1[f], d2[f], f"{name} decision {decision} decword, frame {f} ({labels[f]})")
            assert_bits_equal(a1[f], a2[f], f"{name} decision {decision} clobbered input, frame {f} ({labels[f]})")


@pytest.mark.skipif(not iasp_ref_available(), reason="compiled reference (oracle/_ref) without the IASP decoder")
@pytest.mark.parametrize("M", LIFTINGS)
def test_iasp_model_equals_compiled_reference_on_adversarial_frames(M):
    H = relift(load_base_matrix(), M)
    llr, labels = adversarial_llr(H, M, 7)
    model = IaspModel(H, M)
    for decision in (0, 1):
        d1, i1, a1, _ = model.decode(llr, MAXITER, decision)
        d2, i2, a2 = IaspReference(H, M).decode(llr, MAXITER, decision)
        assert np.array_equal(i1, i2), [labels[f] for f in np.flatnonzero(i1 != i2)]
        assert_bits_equal(d1, d2, f"iasp decision {decision} decword")
        assert_bits_equal(a1, a2, f"iasp decision {decision} clobbered input")
