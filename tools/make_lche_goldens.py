#!/usr/bin/env python3
"""Golden vectors of the low-complexity high-efficiency decoder (LCHE_DEC, decoder id 9) from the COMPILED UPSTREAM REFERENCE.

Run where oracle/_ref exists (`make -C oracle ref` with the upstream tree mounted):

    python3 tools/make_lche_goldens.py [set names...]

npz keys: H, M, dec_id, snr, maxiter, llr, iters, hard (decword packed), soft (upstream's lche_soft_out, the final
a-posteriori LLRs) and soft_out_offset (where tests/lche_ref.py found that buffer in DEC_STATE).  Written to tests/golden/lche/
(a directory of their own: the oracle's golden test reads every npz directly under tests/golden/, and the CPU oracle has no
decoder 9).  oracle/ref_driver.cpp does not dispatch decoder 9, so the exported lche_decod is called directly on a state
ref_open(9, ...) opened.  Before writing, every set is checked against the numpy restatement tests/lche_model.py, and the input
array is checked to be unmodified.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lche_model import LCHE_GOLDEN_DIR, LcheModel  # noqa: E402
from lche_ref import LcheReference, lche_ref_available, soft_out_offset  # noqa: E402
from ldpc_testlib import LCHE_DEC, awgn_llr, load_base_matrix, pack_bits, random_qc_code, relift  # noqa: E402


def appendix_c(M):
    return relift(load_base_matrix(), M)


def thirty_by_sixty(M):
    """The 30 x 60 shape of upstream's files/input12L.jsonx at lifting 67 (tests/test_gpu_shapes.py's code)."""
    return random_qc_code(np.random.RandomState(67), 30, 60, M, [2, 3, 3, 16, 2, 3])


def row_weight_one(M):
    """6 x 14 with block row 0 holding a single circulant (map_bin_llr with n = 1: A = p - p = 0)."""
    H = np.asarray(random_qc_code(np.random.RandomState(91), 6, 14, M, [2, 3]), dtype=np.int32)
    H[0, :] = -1
    H[0, 3] = 11 % M
    return H


def boundary_values():
    """Finite values at logexp_int's branch points and rounding boundaries (positive; signs are applied per frame)."""
    nx = lambda x, d: float(np.nextafter(x, d))
    v = [0.0, 5e-324, 1e-320, 2.2250738585072009e-308, 2.2250738585072014e-308, 1e-300, 1e-200, 1e-20, 1.0 / 4096]
    for x in (1.0 / 512, 1.0 / 16, 2.0, 16.0):
        v += [x, nx(x, 0.0), nx(x, np.inf)]
    v += [(k - 0.5) / 2 for k in range(5, 33)]             # 2x + 0.5 an integer
    v += [(k - 0.5) / 16 for k in range(2, 33)]            # 16x + 0.5 an integer
    v += [(k - 0.5) / 512 for k in range(2, 33)]           # 512x + 0.5 an integer
    v += [(k - 0.5) / 512 / 32 ** 3 for k in range(17, 33)]   # the same after three passes of the small-argument loop
    v += [1e10, 1e300, 1.7976931348623157e308]
    return np.array(v, dtype=np.float64)


def boundary(H, M, llr):
    """Whole frames of boundary values, AWGN frames with a quarter of the positions replaced, and codeword frames (the zero
    codeword with large magnitudes and signed zeros: returned at once, the input bit for bit)."""
    rng = np.random.RandomState(17)
    v = boundary_values()
    B, N = llr.shape
    out = llr.copy()
    for f in range(B):
        kind = f % 4
        if kind == 0:
            out[f] = rng.choice(v, size=N) * np.where(rng.rand(N) < 0.5, -1.0, 1.0)
        elif kind == 1:
            out[f] = rng.choice(v, size=N) * np.where(rng.rand(N) < 0.03, -1.0, 1.0)
        elif kind == 2:
            idx = rng.rand(N) < 0.25
            out[f, idx] = rng.choice(v, size=int(idx.sum())) * np.where(out[f, idx] < 0, -1.0, 1.0)
        else:
            out[f] = rng.choice(np.array([0.0, -0.0, 16.0, 1e300, 2.0, 5e-324]), size=N)
    return out


SETS = [
    # name,                 code factory,    M,   snr, frames, maxiter, seed, transform
    ("lche_m64_2p0",        appendix_c,      64,  2.0, 16, 50, 1, None),
    ("lche_m64_1p5",        appendix_c,      64,  1.5, 16, 50, 2, None),
    ("lche_m64_1p2",        appendix_c,      64,  1.2, 16, 50, 1, None),
    ("lche_m64_0p0",        appendix_c,      64,  0.0, 4,  50, 1, None),   # no frame converges: all 50 iterations
    ("lche_m126_1p7",       appendix_c,      126, 1.7, 8,  50, 1, None),
    ("lche_m1_4p0",         appendix_c,      1,   4.0, 64, 20, 1, None),
    ("lche_30x60_m67_2p0",  thirty_by_sixty, 67,  2.0, 8,  50, 5, None),
    ("lche_rw1_m32_2p5",    row_weight_one,  32,  2.5, 32, 30, 3, None),
    ("lche_m64_boundary",   appendix_c,      64,  2.0, 16, 50, 7, boundary),
]
ONLY = set(sys.argv[1:])


def main():
    if not lche_ref_available():
        sys.exit("oracle/_ref/libldpc_ref.so missing: run `make -C oracle ref` where the upstream tree is mounted")
    os.makedirs(LCHE_GOLDEN_DIR, exist_ok=True)
    for name, factory, M, snr, frames, maxiter, seed, transform in SETS:
        if ONLY and name not in ONLY:
            continue
        H = np.asarray(factory(M), dtype=np.int32)
        llr = awgn_llr(H, M, snr, seed, frames)
        if transform is not None:
            llr = transform(H, M, llr)
        ref = LcheReference(H, M)
        dec, its, soft, after = ref.decode(llr, maxiter, 0)
        _, its1, soft1, _ = ref.decode(llr, maxiter, 1)
        ref.close()
        assert np.array_equal(its, its1) and np.array_equal(soft.view(np.uint64), soft1.view(np.uint64)), f"{name}: decision matters"
        assert np.array_equal(after.view(np.uint64), llr.view(np.uint64)), f"{name}: the reference modified its input"
        m_dec, m_it, m_soft = LcheModel(H, M).decode(llr, maxiter)
        assert np.array_equal(m_it, its) and np.array_equal(m_dec, dec) and np.array_equal(m_soft.view(np.uint64), soft.view(np.uint64)), \
            f"{name}: tests/lche_model.py disagrees with the reference"
        path = os.path.join(LCHE_GOLDEN_DIR, name + ".npz")
        np.savez_compressed(
            path, H=H.astype(np.int16), M=np.int32(M), dec_id=np.int32(LCHE_DEC), snr=np.float64(snr), maxiter=np.int32(maxiter),
            llr=llr, iters=its.astype(np.int32), hard=pack_bits(dec), soft=soft, soft_out_offset=np.int64(soft_out_offset()),
        )
        assert os.path.getsize(path) < 1 << 20, f"{name}: golden file over 1 MiB"
        print(f"{name}: frames={frames} iters={its.tolist()[:12]}... fail={(its < 0).sum()} errbits={int((dec != 0).sum())} "
              f"bytes={os.path.getsize(path)}")


if __name__ == "__main__":
    main()
