"""The table-driven single-code kernels of the LDS tier -- ms_flood_kernel, lms_layered_kernel, ims_flood_kernel -- asserted by name
below M = 64 and at a ragged multi-wave lifting, bit for bit against the CPU oracle: packed waves with idle lanes (M = 5, F = 12),
F = 3 (M = 20), and two waves with the second partly empty (M = 100).  The code is code 1 of test_gpu_codeset's set of the shape (it
has a weight-2 row); the frames are the 7 shared frames of its reference(case), so the last wave is ragged.  A cell's frames must
hold frames the oracle converges on and frames it does not, in one launch, or the stop bookkeeping of a packed wave is not exercised:
where the 7 frames of reference(case) do not (its own mix is over the whole set of codes, not over code 1), the cell decodes a second
batch as well: the same draw at the first SNR of reference()'s ladder at which they do, written down in MIXED_SNR.
tests/test_generic_tier_cpu.py asserts the condition, and that the constants are what the ladder gives, without a GPU."""
import numpy as np
import pytest

from ldpc_testlib import IMS_DEC, LMS_DEC, MS_DEC, Oracle, assert_bits_equal, awgn_llr, pack_bits
from test_gpu_codeset import MAXITER, NFRAMES, oracle_decode, reference

pytestmark = pytest.mark.gpu

SHAPES = [(5, 4, 8), (20, 4, 8), (100, 3, 6)]
DECODERS = {MS_DEC: "ms_flood_kernel", LMS_DEC: "lms_layered_kernel", IMS_DEC: "ims_flood_kernel"}
# (decoder, M): the first SNR of test_gpu_codeset.SNR_LADDER at which the oracle's results on code 1 are of both signs, for the cells
# in which those on the frames of reference(case) (2.0 dB in all three shapes) are not
MIXED_SNR = {(MS_DEC, 5): 1.0, (LMS_DEC, 5): 1.0, (IMS_DEC, 5): 1.0, (IMS_DEC, 20): 3.0,
             (MS_DEC, 100): 4.0, (LMS_DEC, 100): 4.0, (IMS_DEC, 100): 5.0}
_BATCHES = {}


def cell_oracle(H, M, dec, llr):
    """(decword, iters, soft) of the oracle on code H"""
    if dec != IMS_DEC:
        return oracle_decode(H, M, dec, llr, MAXITER)
    d0, it0, _ = Oracle(H, M).decode(IMS_DEC, llr, MAXITER, 0)
    d1, it1, _ = Oracle(H, M).decode(IMS_DEC, llr, MAXITER, 1)
    assert np.array_equal(it0, it1)
    return d0, it0, d1


def draw(case, snr):
    """reference(case)'s shared frames, drawn at another SNR"""
    M = case[0]
    return awgn_llr(reference(case)["codes"][0].astype(np.int32), M, snr, 300 + M, NFRAMES, burn_codeword=False)


def mixed(iters):
    return bool((iters > 0).any() and (iters < 0).any())


def batches(case, dec):
    """[(llr [7, N], the oracle's (decword, iters, soft))]: the shared frames of reference(case), then the batch at MIXED_SNR if any.
    Computed once per cell and left unchanged."""
    if (case, dec) not in _BATCHES:
        M = case[0]
        r = reference(case)
        H = r["codes"][1]
        first = r["ref"][dec, "shared"][1] if dec != IMS_DEC else cell_oracle(H, M, dec, r["shared"])
        out = [(r["shared"], first)]
        if (dec, M) in MIXED_SNR:
            llr = draw(case, MIXED_SNR[dec, M])
            out.append((llr, cell_oracle(H, M, dec, llr)))
        _BATCHES[case, dec] = out
    return _BATCHES[case, dec]


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module", autouse=True)
def no_jit(L):
    lib = L.load_library()
    before = lib.ldpc_hip_set_jit_mode(0)
    yield
    lib.ldpc_hip_set_jit_mode(before)


@pytest.mark.parametrize("dec", list(DECODERS), ids=["ms", "lms", "ims"])
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "M%d_%dx%d" % c)
def test_generic_kernels_below_m64_and_ragged(L, torch, monkeypatch, case, dec):
    M = case[0]
    monkeypatch.setenv("LDPC_HIP_MS_VARIANT", "-1")
    H = reference(case)["codes"][1]
    assert 2 in (H >= 0).sum(axis=1)
    todo = batches(case, dec)
    assert mixed(todo[-1][1][1]), ("the oracle must converge on some frames and not on others", todo[-1][1][1])
    name = DECODERS[dec] + ("<multiwave>" if M > 64 else "")
    with L.LdpcHip(dec, H, M) as one:
        assert one.kernel_name == name, one.kernel_name
        for llr, (d_ref, it_ref, s_ref) in todo:
            x = torch.from_numpy(np.ascontiguousarray(llr)).cuda()
            hard, iters, soft = one.decode(x, MAXITER, want_soft=True)
            torch.cuda.synchronize()
            assert one.last_launch() == name, one.last_launch()
            assert np.array_equal(iters.cpu().numpy(), it_ref), (iters.cpu().numpy(), it_ref)
            assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref))
            assert_bits_equal(soft.cpu().numpy(), s_ref, "soft values")
            assert_bits_equal(x.cpu().numpy(), llr, "the input is not modified")
