"""The inputs of tests/test_gpu_generic_tier.py, checked without a GPU: every one of its nine cells decodes a batch on which the oracle
converges on some frames and not on others, and the SNRs written into MIXED_SNR are the ones reference()'s ladder gives."""
import pytest

from test_gpu_codeset import SNR_LADDER
from test_gpu_generic_tier import DECODERS, MIXED_SNR, SHAPES, batches, cell_oracle, draw, mixed, reference


@pytest.mark.parametrize("dec", list(DECODERS), ids=["ms", "lms", "ims"])
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "M%d_%dx%d" % c)
def test_every_cell_has_frames_of_both_outcomes(case, dec):
    M = case[0]
    todo = batches(case, dec)
    assert mixed(todo[-1][1][1]), todo[-1][1][1]
    at_reference = mixed(todo[0][1][1])
    assert at_reference == ((dec, M) not in MIXED_SNR) and len(todo) == (1 if at_reference else 2)
    if not at_reference:
        H = reference(case)["codes"][1]
        first = next(snr for snr in SNR_LADDER if mixed(cell_oracle(H, M, dec, draw(case, snr))[1]))
        assert first == MIXED_SNR[dec, M]
