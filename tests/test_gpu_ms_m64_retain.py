"""GPU: ms_m64_body keeps the decoded check-to-variable values of its first block rows in registers from STATE1 to STATE3.

Which rows are kept is a compile-time function of the code and of an edge budget this test does not know.  The matrices land on
every side of any plausible budget: a code whose edges all fit, a row of weight 16 in front of ordinary rows, a row of weight 16
behind rows of weight 4-8 (at or past the boundary), a code with more edges than registers can hold (the first rows are kept, the
last are not), and the shipped shape, which runs the ahead-of-time instance.  Inputs: AWGN at 0 dB (nothing converges) and at
2 dB (frames leave early), and the adversarial batch (+-0.0, values beyond the 32 767 clamp, ties min1 == min2, denormals);
maxiter 1 (STATE1 on the all-zero start record: cv = +-0.0), 2 and 50.  Hard decisions, signed iteration counts and soft values
must equal the CPU oracle's bit for bit.  One more run pushes several frames through every wave of the persistent launch: a kept
value of a finished frame must not leak into the next frame of the same wave."""
import numpy as np
import pytest

from ldpc_testlib import (MS_DEC, Oracle, adversarial_llr, assert_bits_equal, awgn_llr, load_base_matrix, pack_bits, random_qc_code,
                          relift)

pytestmark = pytest.mark.gpu

M = 64
FRAMES = 24
AOT_NAME = "ms_spec_appendix_c_m64_kernel (ahead of time)"


def _matrix(rh, nh, entries):
    H = -np.ones((rh, nh), dtype=np.int16)
    for j, k, c in entries:
        assert H[j, k] < 0 and 0 <= c < M
        H[j, k] = c
    assert ((H >= 0).sum(axis=0) >= 1).all() and ((H >= 0).sum(axis=1) >= 1).all()
    return H


def _all_rows_fit():
    """4 x 8, row weight 4, 16 edges, shifts mixed with 0 and 63."""
    return _matrix(4, 8, [(0, 0, 0), (0, 1, 63), (0, 4, 5), (0, 6, 0),
                          (1, 1, 0), (1, 2, 63), (1, 5, 17), (1, 7, 63),
                          (2, 2, 0), (2, 3, 1), (2, 4, 63), (2, 6, 40),
                          (3, 0, 63), (3, 3, 0), (3, 5, 0), (3, 7, 32)])


def _heavy_row_first():
    """3 x 16, 34 edges: row 0 has all 16 block columns, two ordinary rows follow."""
    e = [(0, k, (23 * k + 7) % M if k % 5 else (0 if k % 2 else 63)) for k in range(16)]
    e += [(1, k, (13 * k + 2) % M) for k in range(1, 16, 2)]
    e += [(2, k, 0 if k % 4 == 0 else (9 * k + 63) % M) for k in range(0, 16, 2)] + [(2, 5, 63), (2, 11, 31)]
    return _matrix(3, 16, e)


def _heavy_row_last():
    """10 x 20, 75 edges: nine rows of weight 4-8 (59 edges), then a row of weight 16."""
    w = [8, 7, 6, 8, 7, 6, 8, 5, 4]
    e = []
    for j, wj in enumerate(w):
        cols = sorted({(3 * j + 7 * s) % 20 for s in range(wj)})
        assert len(cols) == wj
        e += [(j, k, 0 if (j + k) % 7 == 0 else (63 if (j + k) % 7 == 1 else (11 * j + 5 * k) % M)) for k in cols]
    e += [(9, k, (37 * k + 3) % M) for k in range(2, 18)]
    return _matrix(10, 20, e)


def _more_edges_than_fit():
    """14 x 28 of the usual protograph shape, 75 edges: more than the kept rows of the shipped shape hold, in rows of weight 4-7."""
    return random_qc_code(np.random.RandomState(1364), 14, 28, M, [3, 4, 2])


def _shipped_shape():
    return relift(load_base_matrix(), M)


CASES = {"all_rows_fit": _all_rows_fit, "heavy_row_first": _heavy_row_first, "heavy_row_last": _heavy_row_last,
         "more_edges_than_fit": _more_edges_than_fit, "shipped_shape": _shipped_shape}


def test_the_matrices_hold_what_they_are_meant_to_exercise():
    def weights(H):
        return [int(x) for x in (H >= 0).sum(axis=1)]
    H = _all_rows_fit()
    assert max(weights(H)) <= 4 and sum(weights(H)) <= 16 and {0, 63} < {int(c) for c in H[H >= 0]}
    w = weights(_heavy_row_first())
    assert w[0] == 16 and max(w[1:]) < 16 and sum(w) >= 32
    w = weights(_heavy_row_last())
    assert w[-1] == 16 and all(4 <= x <= 8 for x in w[:-1])
    assert sum(weights(_more_edges_than_fit())) >= 72
    assert _shipped_shape().shape == (16, 32)


def _inputs(H, case_no):
    Hi = np.asarray(H, dtype=np.int32)
    return {"awgn 0 dB": awgn_llr(Hi, M, 0.0, 1300 + case_no, FRAMES, burn_codeword=False),
            "awgn 2 dB": awgn_llr(Hi, M, 2.0, 1320 + case_no, FRAMES, burn_codeword=False),
            "adversarial": adversarial_llr(H, M, 13 + case_no)[0]}


def _expect_equal(dec, oracle, llr, maxiter, what, torch):
    d_ref, it_ref, _ = oracle.decode(MS_DEC, llr, maxiter, 0)
    s_ref, _, _ = oracle.decode(MS_DEC, llr, maxiter, 1)
    hard, iters, soft = dec.decode(torch.from_numpy(llr).cuda(), maxiter, want_soft=True)
    torch.cuda.synchronize()
    assert np.array_equal(iters.cpu().numpy(), it_ref), (what, iters.cpu().numpy(), it_ref)
    assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref)), what
    assert_bits_equal(soft.cpu().numpy(), s_ref, "soft values, " + what)
    return it_ref


@pytest.mark.parametrize("case", list(CASES))
def test_ms_m64_with_kept_c2v_values_equals_the_oracle(case):
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H = CASES[case]()
    oracle = Oracle(H, M)
    with ldpc_lib_amd.LdpcHip(MS_DEC, H, M) as dec:
        if case == "shipped_shape":
            assert dec.kernel_name == AOT_NAME, dec.kernel_name
        else:
            assert "ms_m64_body" in dec.kernel_name and "hiprtc" in dec.kernel_name, dec.kernel_name
        for name, llr in _inputs(H, list(CASES).index(case)).items():
            for maxiter in (1, 2, 50):
                it = _expect_equal(dec, oracle, llr, maxiter, f"{case}, {name}, maxiter {maxiter}", torch)
                if maxiter == 50 and name == "awgn 0 dB":
                    assert (it < 0).all(), "0 dB: nothing is meant to converge"
                if maxiter == 50 and name == "awgn 2 dB" and case in ("more_edges_than_fit", "shipped_shape"):
                    assert (it > 0).any() and len(set(it.tolist())) > 2, "2 dB: frames are meant to leave early, at different iterations"


def test_kept_values_do_not_leak_into_the_next_frame_of_a_persistent_wave():
    """The shipped shape, 6144 frames = three times the 2048 resident waves of an MI355X (256 CUs x 4 SIMDs x 2): every wave pulls
    further frames from the queue.  Frames that converge after a few iterations alternate with frames that run all 50 and with
    adversarial ones, so a wave starts a frame with the registers another frame left at some other iteration."""
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H = _shipped_shape()
    Hi = np.asarray(H, dtype=np.int32)
    distinct = np.concatenate([awgn_llr(Hi, M, 2.0, 1351, FRAMES, burn_codeword=False), awgn_llr(Hi, M, 0.0, 1352, 8, burn_codeword=False),
                               awgn_llr(Hi, M, 3.0, 1353, 8, burn_codeword=False), adversarial_llr(H, M, 19)[0]])
    rng = np.random.RandomState(1354)
    idx = np.concatenate([np.arange(len(distinct)), rng.randint(0, len(distinct), size=6144 - len(distinct))])
    oracle = Oracle(H, M)
    d_ref, it_ref, _ = oracle.decode(MS_DEC, distinct, 50, 0)
    s_ref, _, _ = oracle.decode(MS_DEC, distinct, 50, 1)
    assert (it_ref > 0).any() and (it_ref < 0).any()
    with ldpc_lib_amd.LdpcHip(MS_DEC, H, M) as dec:
        assert dec.kernel_name == AOT_NAME, dec.kernel_name
        hard, iters, soft = dec.decode(torch.from_numpy(distinct[idx]).cuda(), 50, want_soft=True)
        torch.cuda.synchronize()
        assert dec.last_launch() == AOT_NAME, dec.last_launch()
    bad = np.flatnonzero(iters.cpu().numpy() != it_ref[idx])
    assert not bad.size, [(int(f), int(idx[f])) for f in bad[:8]]
    assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref)[idx])
    assert_bits_equal(soft.cpu().numpy(), s_ref[idx], "soft values")
