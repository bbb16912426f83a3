"""GPU: the rotated LDS accesses of ms_m64_body (flooding min-sum, M = 64, one frame per wavefront) on hiprtc instances.

The shipped example code uses 40 of the 64 possible shifts and never a first edge below block row 0 on a rotated circulant, so the
flagship tests alone do not pin down the address arithmetic of every shift.  The synthetic base matrices here do: the corner shifts
0, 1, 32 and 63, a block row made only of shift 63, a block row of weight 16, block columns whose first edge (the one that stores
instead of adding) sits below block row 0 and is rotated, and one matrix that uses every shift 0..63 exactly once.  Min-sum, fp64,
at 0 dB (nothing converges: all iterations run) and 2 dB; hard decisions, signed iteration counts and soft values must equal the
CPU oracle's bit for bit."""
import numpy as np
import pytest

from ldpc_testlib import MS_DEC, Oracle, assert_bits_equal, awgn_llr, pack_bits, random_qc_code

pytestmark = pytest.mark.gpu

M = 64


def _matrix(rh, nh, entries):
    H = -np.ones((rh, nh), dtype=np.int16)
    for j, k, c in entries:
        assert H[j, k] < 0 and 0 <= c < M
        H[j, k] = c
    assert ((H >= 0).sum(axis=0) >= 1).all() and ((H >= 0).sum(axis=1) >= 1).all()
    return H


def _corner_shifts():
    """4 x 8.  Row 1 is made only of shift 63; columns 5 and 6 start in row 1 and column 7 in row 2, all three on a rotated edge."""
    return _matrix(4, 8, [(0, 0, 0), (0, 1, 1), (0, 2, 32), (0, 3, 63), (0, 4, 0),
                          (1, 1, 63), (1, 3, 63), (1, 5, 63), (1, 6, 63),
                          (2, 0, 32), (2, 2, 1), (2, 5, 0), (2, 7, 63),
                          (3, 0, 63), (3, 4, 1), (3, 6, 32), (3, 7, 0)])


def _row_of_weight_sixteen():
    """3 x 16.  Row 0 has all 16 block columns (the widest row the body takes), the corner shifts among them."""
    row0 = [0, 1, 32, 63, 2, 31, 33, 62, 5, 17, 40, 50, 7, 8, 9, 63]
    e = [(0, k, c) for k, c in enumerate(row0)]
    e += [(1, k, (11 * k + 1) % M) for k in range(0, 16, 2)]
    e += [(2, k, 63 if k % 3 == 0 else (5 * k) % M) for k in range(7, 16)] + [(2, 0, 1)]
    return _matrix(3, 16, e)


def _every_shift_once():
    """8 x 16, row weight 8.  Edge number e = 8 j + s has shift (37 e + 11) mod 64: a bijection, so every shift 0..63 occurs exactly
    once.  Even rows use the even block columns and odd rows the odd ones: the odd columns start in block row 1."""
    return _matrix(8, 16, [(j, (j + 2 * s) % 16, (37 * (8 * j + s) + 11) % M) for j in range(8) for s in range(8)])


def _usual_shape():
    """6 x 14 of the usual protograph shape (dual-diagonal parity part, random information part)."""
    return random_qc_code(np.random.RandomState(64), 6, 14, M, [3, 4, 2])


CASES = {"corner_shifts": _corner_shifts, "row_of_weight_sixteen": _row_of_weight_sixteen, "every_shift_once": _every_shift_once,
         "usual_shape": _usual_shape}


def test_the_matrices_hold_what_they_are_meant_to_exercise():
    H = _corner_shifts()
    assert {0, 1, 32, 63} <= {int(c) for c in H[H >= 0]}
    assert {int(c) for c in H[1][H[1] >= 0]} == {63}                 # a row made only of shift 63
    assert H[0, 7] < 0 and H[1, 7] < 0 and H[2, 7] == 63             # a column whose first edge is below block row 0, and rotated
    assert ((_row_of_weight_sixteen() >= 0).sum(axis=1) == 16).any()
    H = _every_shift_once()
    assert sorted(int(c) for c in H[H >= 0]) == list(range(M))
    assert (H[0, 1::2] < 0).all() and (H[1, 1::2] >= 0).all()


@pytest.mark.parametrize("snr", [0.0, 2.0])
@pytest.mark.parametrize("case", list(CASES))
def test_ms_m64_hiprtc_instance_equals_the_oracle(case, snr):
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H = CASES[case]()
    maxiter, frames = 50, 24
    llr = awgn_llr(np.asarray(H, dtype=np.int32), M, snr, 640 + int(10 * snr), frames, burn_codeword=False)
    d_ref, it_ref, _ = Oracle(H, M).decode(MS_DEC, llr, maxiter, 0)
    s_ref, _, _ = Oracle(H, M).decode(MS_DEC, llr, maxiter, 1)
    with ldpc_lib_amd.LdpcHip(MS_DEC, H, M) as dec:
        assert "ms_m64_body" in dec.kernel_name and "hiprtc" in dec.kernel_name, dec.kernel_name
        hard, iters, soft = dec.decode(torch.from_numpy(llr).cuda(), maxiter, want_soft=True)
        torch.cuda.synchronize()
    assert np.array_equal(iters.cpu().numpy(), it_ref), (iters.cpu().numpy(), it_ref)
    assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref))
    assert_bits_equal(soft.cpu().numpy(), s_ref, "soft values")
