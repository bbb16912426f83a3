"""GPU: what the kernels of the shape-unlimited tier (ldpc_global.hpp) share -- the edge addressing in both directions, the
syndrome, the record reset and the outputs with their per-decoder bit and soft-value functors -- on the shapes where that code is
at its edges: lifting 1 (every rotation degenerate, one partial output word), a lifting that is no power of two with shifts 0 and
M - 1 (the wrap at both ends, a 25-bit tail word), the branch for weight-2 columns with u16 outputs, and more frames than the
capped grid has workgroups (a workspace slice reused for a second frame).  All nine kernels, forced on with
LDPC_HIP_FORCE_GLOBAL=1, bit for bit against what each decoder's own test compares with: the C oracle, tests/iasp_model.py for
decoder 5, tests/lche_model.py for decoder 9."""
import numpy as np
import pytest

from iasp_model import IaspModel
from lche_model import LcheModel
from ldpc_testlib import (ASP_DEC, BP_DEC, IASP_DEC, IMS_DEC, LCHE_DEC, LMS_DEC, MS_DEC, SP_DEC, TASP_DEC, Oracle, assert_bits_equal, awgn_llr, cycle_code,
                          unpack_bits)

pytestmark = pytest.mark.gpu

KERNEL = {MS_DEC: "ms_global_kernel", LMS_DEC: "lms_global_kernel", TASP_DEC: "tasp_global_kernel", LCHE_DEC: "lche_global_kernel", SP_DEC: "sp_global_kernel",
          IMS_DEC: "ims_global_kernel", ASP_DEC: "asp_global_kernel", IASP_DEC: "iasp_global_kernel", BP_DEC: "bp_global_kernel"}
# a codeword at the input: min-sum and integer min-sum run one iteration before they look and layered min-sum returns iter + 1 with
# iter = 0 (decoders.cpp:5424); the other layered decoders and the probability-domain ones return 0
CLEAN_INPUT = {MS_DEC: 1, IMS_DEC: 1, LMS_DEC: 1, TASP_DEC: 0, LCHE_DEC: 0, SP_DEC: 0, ASP_DEC: 0, IASP_DEC: 0, BP_DEC: 0}

_ = -1
SHAPES = {
    # 3 x 7 at lifting 1: N = 7, every row of weight 5, block columns of weight 2 and 3 (the general branch of decoders 2 and 5)
    "3x7-m1": (np.array([[0, 0, _, 0, 0, _, 0],
                         [_, 0, 0, 0, _, 0, 0],
                         [0, _, 0, 0, 0, 0, _]], dtype=np.int16), 1, 1.0),
    # 2 x 5 at lifting 37: N = 185 = 5 * 32 + 25, shifts 0 and 36 = M - 1 in both block rows, block columns of weight 1 and 2
    "2x5-m37": (np.array([[0, 36, 5, _, 17],
                          [36, 0, _, 9, 20]], dtype=np.int16), 37, 4.0),
    # decoders 2 and 5 only: "weight-2 columns, lifting 1" of tests/test_gpu_iasp.py -- upstream's own branch for such codes
    "cycle-3x7-m1": (cycle_code(np.random.RandomState(912), 3, 7, 1), 1, 1.0),
}
CASES = [(d, s) for s in ("3x7-m1", "2x5-m37") for d in KERNEL] + [(IASP_DEC, "cycle-3x7-m1"), (ASP_DEC, "cycle-3x7-m1")]
REUSE_FRAMES, GRID_CAP = 1032, 1024     # launch_global caps the grid at 1024 workgroups: eight of them take a second frame


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _llr(shape, frames):
    """AWGN frames of the all-zero codeword; frame 0 made a codeword at the input (every LLR positive)."""
    H, M, snr = SHAPES[shape]
    llr = awgn_llr(np.asarray(H, dtype=np.int32), M, snr, 4100 + M, frames, burn_codeword=False)
    llr[0] = np.abs(llr[0])
    return llr


def _reference(dec_id, H, M, llr, maxiter):
    """(hard bits uint8 [B, N], return values, soft values) of a fresh reference state (Gallager BP carries its syndrome on)."""
    if dec_id == IASP_DEC:
        soft, it, _after, so = IaspModel(H, M).decode(llr, maxiter, 1)
        return (so >> 15).astype(np.uint8), it, soft
    if dec_id == LCHE_DEC:
        d, it, soft = LcheModel(H, M).decode(llr, maxiter)
        return d.astype(np.uint8), it, soft
    d, it, _after = Oracle(H, M).decode(dec_id, llr, maxiter, 0)
    soft = Oracle(H, M).decode(dec_id, llr, maxiter, 1)[0]       # decoder 7: the posteriors (the host call's decword stays hard upstream)
    return (d != 0).astype(np.uint8), it, soft


_refs = {}


def _shared_reference(dec_id, shape, maxiter):
    key = (dec_id, shape, maxiter)
    if key not in _refs:
        H, M, _snr = SHAPES[shape]
        _refs[key] = _reference(dec_id, H, M, _llr(shape, 16), maxiter)
    return _refs[key]


def test_every_kernel_of_the_tier_meets_both_shapes():
    assert len(KERNEL) == 9 and {d for d, s in CASES if s == "3x7-m1"} == {d for d, s in CASES if s == "2x5-m37"} == set(KERNEL)
    for H, M, _snr in SHAPES.values():
        assert ((H >= 0).sum(axis=1) >= 2).all() and ((H >= 0).sum(axis=0) >= 1).all()
    H, M, _snr = SHAPES["2x5-m37"]
    assert (H == M - 1).any() and (H == 0).any() and (H.shape[1] * M) % 32 == 25
    assert ((SHAPES["cycle-3x7-m1"][0] >= 0).sum(axis=0) == 2).all() and not ((SHAPES["3x7-m1"][0] >= 0).sum(axis=0) == 2).all()


@pytest.mark.parametrize("maxiter", [1, 30])
@pytest.mark.parametrize("dec_id,shape", CASES, ids=[f"{KERNEL[d][:-14]}-{s}" for d, s in CASES])
def test_bit_exact_on_degenerate_rotations_and_tail_words(L, torch, monkeypatch, dec_id, shape, maxiter):
    monkeypatch.setenv("LDPC_HIP_FORCE_GLOBAL", "1")
    H, M, _snr = SHAPES[shape]
    llr = _llr(shape, 16)
    bits_ref, it_ref, soft_ref = _shared_reference(dec_id, shape, maxiter)
    assert it_ref[0] == CLEAN_INPUT[dec_id], it_ref
    # both exits of the iteration loop in every decode (at one iteration min-sum and integer min-sum converge on frame 0 only: the
    # SNR at which they mend a noisy frame of the 2 x 5 code at once is one at which no decoder fails after 30)
    assert (it_ref > 0).any() and (it_ref < 0).any(), it_ref
    with L.LdpcHip(dec_id, H, M) as dec:
        assert dec.kernel_name == KERNEL[dec_id], dec.kernel_name
        hard, iters, soft = dec.decode(torch.from_numpy(llr).cuda(), maxiter, want_soft=True)
        torch.cuda.synchronize()
        assert np.array_equal(iters.cpu().numpy(), it_ref), (iters.cpu().numpy(), it_ref)
        words = hard.cpu().numpy().view(np.uint32)
        N = H.shape[1] * M
        assert np.array_equal(unpack_bits(words, N), bits_ref)
        if N % 32:
            assert not (words[:, -1] >> (N % 32)).any()                     # nothing beyond variable N - 1 in the tail word
        assert_bits_equal(soft.cpu().numpy(), soft_ref, "soft values")


@pytest.mark.parametrize("dec_id", list(KERNEL), ids=[k[:-14] for k in KERNEL.values()])
def test_a_workgroup_that_takes_a_second_frame_finds_its_slice_reset(L, torch, monkeypatch, dec_id):
    """1032 frames on a grid capped at 1024: frames 1024 .. 1031 are decoded by workgroups 0 .. 7 in the slice that frames 0 .. 7
    left behind.  They must equal a decode of the same eight frames alone.  (Gallager BP with the frame chain off, so that a
    frame does not depend on its predecessor.)"""
    monkeypatch.setenv("LDPC_HIP_FORCE_GLOBAL", "1")
    H, M, _snr = SHAPES["2x5-m37"]
    llr = _llr("2x5-m37", REUSE_FRAMES)
    with L.LdpcHip(dec_id, H, M) as dec:
        assert dec.kernel_name == KERNEL[dec_id], dec.kernel_name
        if dec_id == BP_DEC:
            dec.set_bp_chain(False)
        x = torch.from_numpy(llr).cuda()
        hard, iters, soft = dec.decode(x, 5, want_soft=True)
        hard8, iters8, soft8 = dec.decode(x[GRID_CAP:].contiguous(), 5, want_soft=True)
        torch.cuda.synchronize()
        it = iters.cpu().numpy()
        assert (it[:8] > 0).any() and (it[:8] < 0).any(), it[:8]             # slices left behind by both exits of the iteration loop
        assert np.array_equal(it[GRID_CAP:], iters8.cpu().numpy())
        assert np.array_equal(hard.cpu().numpy()[GRID_CAP:], hard8.cpu().numpy())
        assert_bits_equal(soft.cpu().numpy()[GRID_CAP:], soft8.cpu().numpy(), "soft values of frames 1024 .. 1031")
