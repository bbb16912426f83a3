#!/usr/bin/env python3
"""Golden vectors of the integer advanced sum-product decoder (IASP_DEC, decoder id 5) from the COMPILED UPSTREAM REFERENCE.

Run where oracle/_ref exists (`make -C oracle ref` with the upstream tree mounted):

    python3 tools/make_iasp_goldens.py [set names...]

Same npz keys as oracle/make_goldens.py (H, M, dec_id, snr, maxiter, llr, iters, hard, soft), LLRs from ldpc_testlib.awgn_llr
(upstream's draw order), written to tests/golden/iasp/ (a directory of their own: the oracle's golden test
reads every npz directly under tests/golden/, and the CPU oracle has no decoder 5).  oracle/ref_driver.cpp does not dispatch decoder 5, so the exported isum_prod_gf2_decod_qc_lm is called
directly on a state ref_open(5, ...) opened (tests/iasp_ref.py).  `soft` holds the decision == 1 output (soft_out / 65536) of
every frame, `hard` the decision == 0 output packed.  Before writing, every set is checked against the numpy restatement
tests/iasp_model.py.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from iasp_model import IaspModel  # noqa: E402
from iasp_ref import IaspReference, iasp_ref_available  # noqa: E402
from iasp_model import IASP_GOLDEN_DIR  # noqa: E402
from ldpc_testlib import IASP_DEC, awgn_llr, cycle_code, load_base_matrix, pack_bits, random_qc_code, relift  # noqa: E402


def appendix_c(M):
    return relift(load_base_matrix(), M)


def thirty_by_sixty(M):
    """The shape of upstream's files/input12L.jsonx (decoder_type 5): 30 x 60 at lifting 67 (tests/test_gpu_shapes.py's code)."""
    return random_qc_code(np.random.RandomState(67), 30, 60, M, [2, 3, 3, 16, 2, 3])


def cycle_m64(M):
    return cycle_code(np.random.RandomState(1), 4, 8, M)


def cycle_wrap(M):
    """4 x 8, every block column of weight 2: at M = 128 and 2 dB the u16 quotient of the weight-2 branch wraps often."""
    return cycle_code(np.random.RandomState(2), 4, 8, M)


def saturated(H, M, llr):
    """Channel values beyond the +-20 clamp, exactly +-20 and signed zeros."""
    llr = llr * 4.0
    rng = np.random.RandomState(5)
    for f in range(llr.shape[0]):
        idx = rng.choice(llr.shape[1], size=64, replace=False)
        llr[f, idx[:16]] = 20.0
        llr[f, idx[16:32]] = -20.0
        llr[f, idx[32:48]] = 0.0
        llr[f, idx[48:64]] = -0.0
    return llr


SETS = [
    # name,                code factory,    M,   snr, frames, maxiter, seed, transform
    ("iasp_m64_2p0",       appendix_c,      64,  2.0, 24, 50, 1, None),
    ("iasp_m64_1p2",       appendix_c,      64,  1.2, 16, 50, 1, None),
    ("iasp_m64_0p0",       appendix_c,      64,  0.0, 4,  50, 1, None),   # worst case: every frame runs all 50 iterations
    ("iasp_m126_1p7",      appendix_c,      126, 1.7, 8,  50, 1, None),
    ("iasp_m1_4p0",        appendix_c,      1,   4.0, 64, 20, 1, None),
    ("iasp_30x60_m67_2p0", thirty_by_sixty, 67,  2.0, 12, 50, 5, None),
    ("iasp_cw2_m64_2p0",   cycle_m64,       64,  2.0, 24, 40, 1, None),
    ("iasp_cw2_m128_2p0",  cycle_wrap,      128, 2.0, 100, 50, 1, None),
    ("iasp_m64_sat",       appendix_c,      64,  6.0, 8,  50, 3, saturated),
]
ONLY = set(sys.argv[1:])


def main():
    if not iasp_ref_available():
        sys.exit("oracle/_ref/libldpc_ref.so missing: run `make -C oracle ref` where the upstream tree is mounted")
    os.makedirs(IASP_GOLDEN_DIR, exist_ok=True)
    for name, factory, M, snr, frames, maxiter, seed, transform in SETS:
        if ONLY and name not in ONLY:
            continue
        H = np.asarray(factory(M), dtype=np.int32)
        llr = awgn_llr(H, M, snr, seed, frames)
        if transform is not None:
            llr = transform(H, M, llr)
        ref = IaspReference(H, M)
        dec0, it0, _ = ref.decode(llr, maxiter, 0)
        dec1, it1, _ = ref.decode(llr, maxiter, 1)
        ref.close()
        assert np.array_equal(it0, it1)
        m_soft, m_it, _, _ = IaspModel(H, M).decode(llr, maxiter, 1)
        assert np.array_equal(m_it, it0) and np.array_equal(m_soft, dec1), f"{name}: tests/iasp_model.py disagrees with the reference"
        np.savez_compressed(
            os.path.join(IASP_GOLDEN_DIR, name + ".npz"),
            H=H.astype(np.int16), M=np.int32(M), dec_id=np.int32(IASP_DEC), snr=np.float64(snr), maxiter=np.int32(maxiter),
            llr=llr, iters=it0.astype(np.int32), hard=pack_bits(dec0), soft=dec1,
        )
        print(f"{name}: frames={frames} iters={it0.tolist()[:12]}... fail={(it0 < 0).sum()} errbits={int((dec0 != 0).sum())}")


if __name__ == "__main__":
    main()
