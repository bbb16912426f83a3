#!/usr/bin/env python3
"""Golden vectors of the GF(q) sum-product decoder (FHT_DEC, decoder id 6) from the COMPILED UPSTREAM REFERENCE.

Run where oracle/_ref exists (`make -C oracle ref` with the upstream tree mounted):

    python3 tools/make_gfq_goldens.py [set names...]

npz keys: hb, hc, q_bits, M, ncols2convert, maxiter, snr, seed, soft (the input [B][q][N]), and upstream's iters (return values),
qhard, post (fht_soft_out after the call), hc_after (hc as decod_init leaves it), plus state_offsets (where tests/gfq_ref.py found
hb, hc, fht_ncols2convert and fht_soft_out in DEC_STATE).  Written to tests/golden/gfq/ (a directory of its own: the oracle's golden
test reads every npz directly under tests/golden/).  Inputs are BPSK + AWGN on the all-zero word -- a codeword of every such code --
formed in numpy as upstream's q-ary harness forms them (tests/gfq_model.py:bpsk_symbol_probabilities); they are stored, so they need
not match upstream's generator.  For each SNR set the seed is searched, with the reference alone, until the set holds converged and
non-converged frames.  Before writing, every set is checked against the numpy restatement tests/gfq_model.py bit for bit, and the
input array is checked to be unmodified.

No set has a coefficient 0 in hc: upstream files it under index q of its symbol list and then reads gf_log[q], one entry past the end
of a calloc'ed array of q shorts (find_list_of_symbols / p2table), so its tables for such a code are whatever the heap holds.  The
library refuses such a matrix.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gfq_model import GFQ_GOLDEN_DIR, GfqModel, bpsk_symbol_probabilities  # noqa: E402
from gfq_ref import GfqReference, gfq_ref_available, member_offsets  # noqa: E402
from ldpc_testlib import random_qc_code  # noqa: E402

# the GF(16) code of upstream's files/resultq_codes.jsonx (4 x 8, lifting 8, 15 iterations): shifts and coefficients as numbers
SHIPPED_HB = [[0, -1, -1, 73, 2, -1, -1, 1], [0, 0, -1, -1, -1, 11, -1, -1], [-1, 0, 0, -1, 1, -1, 13, 17], [-1, -1, 0, 12, -1, 13, 1, -1]]
SHIPPED_HC = [[1, -1, -1, 73, 2, -1, -1, 1], [1, 2, -1, -1, -1, 11, -1, -1], [-1, 2, 3, -1, 1, -1, 13, 17], [-1, -1, 3, 30, -1, 13, 1, -1]]
MAXITER = 15


def shipped(M, q):
    """Shifts reduced % M (0 -> 1 in the last column of the dual-diagonal part), coefficients % q with 0 -> q - 1: the rule of
    upstream's main_simulation.cpp:400-429.  Every block column has weight 2: the decoder's cw2 branch."""
    hb = np.array(SHIPPED_HB, dtype=np.int64)
    hc = np.array(SHIPPED_HC, dtype=np.int64)
    for j in range(hb.shape[0]):
        for k in range(hb.shape[1]):
            if hb[j, k] > 0:
                t = hb[j, k] % M
                hb[j, k] = 1 if (k == hb.shape[0] - 1 and t == 0) else t
            if hb[j, k] > -1 and hc[j, k] > -1:
                hc[j, k] = hc[j, k] % q or q - 1
    return hb.astype(np.int16), hc.astype(np.int16)


def mixed(M, q, seed=5):
    """4 x 10 with block columns of weight 2, 3 and 4: the only way into the other two symbol-node forms."""
    rng = np.random.RandomState(seed)
    hb = np.asarray(random_qc_code(rng, 4, 10, M, [2, 3, 4]), dtype=np.int16)
    hc = np.where(hb >= 0, rng.randint(1, q, hb.shape), -1).astype(np.int16)
    assert {int((hb[:, k] >= 0).sum()) for k in range(10)} >= {2, 3}
    return hb, hc


def sigma_of(snr, hb):
    rate = (hb.shape[1] - hb.shape[0]) / hb.shape[1]
    return float(np.sqrt(10 ** (-snr / 10) / 2 / rate))


def boundary_inputs(q_bits, hb, M):
    q, N = 1 << q_bits, hb.shape[1] * M
    rng = np.random.RandomState(77)
    noisy = bpsk_symbol_probabilities(rng, q_bits, N, sigma_of(2.5, hb), 6)
    frames = []
    one_hot = np.zeros((q, N))
    one_hot[0] = 1.0
    frames.append(one_hot)                                   # the zero word, certain: a codeword on input, return 0
    f = noisy[0].copy()                                      # a codeword on input with soft values: return 0
    f[0] = f.max(axis=0) + 0.25
    frames.append(f / f.sum(axis=0))
    f = one_hot.copy()                                       # one-hot with three wrong symbols: exact zeros meet exact zeros
    for i, s in ((3, 5), (17, 9), (40, 1)):
        f[:, i] = 0.0
        f[s, i] = 1.0
    frames.append(f)
    f = noisy[1].copy()                                      # exact zeros sprinkled into noisy vectors
    f[rng.randint(0, q, 40), rng.randint(0, N, 40)] = 0.0
    frames.append(f)
    f = noisy[2].copy()                                      # whole vectors of zeros (sum 0 -> Inf / NaN through the frame)
    f[:, 7] = 0.0
    frames.append(f)
    frames.append(bpsk_symbol_probabilities(rng, q_bits, N, sigma_of(30.0, hb), 1)[0])   # exp under- and overflow at high SNR (NaN vectors)
    f = noisy[3].copy()                                      # ties: equal maxima, first index wins
    f[:, ::3] = 1.0 / q
    frames.append(f)
    frames.append(noisy[4])
    frames.append(noisy[5] * 1e-300)                         # unnormalised tiny vectors: products underflow
    return np.stack(frames)


#        name             q_bits code                       M    snr   frames ncols2convert
SETS = [("gf16_m8_2p0",      4, lambda: shipped(8, 16),     8,   2.0,  24, 0),
        ("gf16_m8_3p0",      4, lambda: shipped(8, 16),     8,   3.0,  24, 0),
        ("gf16_m100_1p6",    4, lambda: shipped(100, 16),   100, 1.6,  4, 0),
        ("gf16_m100_2p0",    4, lambda: shipped(100, 16),   100, 2.0,  4, 0),
        ("gf16_mixed_3p0",   4, lambda: mixed(20, 16),      20,  3.0,  8, 0),
        ("gf64_m8_2p5",      6, lambda: shipped(8, 64),     8,   2.5,  8, 0),
        ("gf64_mixed_3p0",   6, lambda: mixed(6, 64),       6,   3.0,  8, 0),
        ("gf4_mixed_3p5",    2, lambda: mixed(20, 4),       20,  3.5,  24, 0),
        ("gf32_mixed_3p0",   5, lambda: mixed(10, 32),      10,  3.0,  8, 0),
        ("gf16_m8_n2c3_2p5", 4, lambda: shipped(8, 16),     8,   2.5,  8, 3),
        ("gf16_m8_boundary", 4, lambda: shipped(8, 16),     8,   None, 0, 0)]


def main(argv):
    assert gfq_ref_available(), "oracle/_ref/libldpc_ref.so is missing: run `make -C oracle ref` with the upstream tree mounted"
    os.makedirs(GFQ_GOLDEN_DIR, exist_ok=True)
    for name, q_bits, code, M, snr, frames, n2c in SETS:
        if argv and name not in argv:
            continue
        hb, hc = code()
        N = hb.shape[1] * M
        ref = GfqReference(q_bits, hb, hc, M, n2c)
        seed = -1
        if snr is None:
            soft = boundary_inputs(q_bits, hb, M)
            iters, qhard, post, after = ref.decode(soft, MAXITER)
            assert (iters[:2] == 0).all(), "the codeword frames of the boundary set must return 0"
        else:
            for seed in range(1000, 1400):
                soft = bpsk_symbol_probabilities(np.random.RandomState(seed), q_bits, N, sigma_of(snr, hb), frames)
                iters, qhard, post, after = ref.decode(soft, MAXITER)
                if (iters > 0).any() and (iters < 0).any():
                    break
            else:
                raise SystemExit(f"{name}: no seed gives converged and non-converged frames at {snr} dB")
        assert np.array_equal(after.view(np.uint64), soft.view(np.uint64)), "upstream modified its input"
        model = GfqModel(q_bits, hb, hc, M, n2c)
        mi, mq, mp = model.decode(soft, MAXITER)
        assert np.array_equal(mi, iters) and np.array_equal(mq, qhard), f"{name}: model != reference (iters / qhard)"
        assert np.array_equal(mp.view(np.uint64), post.view(np.uint64)), f"{name}: model != reference (fht_soft_out)"
        assert np.array_equal(model.hc_after, ref.coefficients()), f"{name}: model != reference (hc after decod_init)"
        path = os.path.join(GFQ_GOLDEN_DIR, name + ".npz")
        np.savez(path, hb=hb, hc=hc, q_bits=q_bits, M=M, ncols2convert=n2c, maxiter=MAXITER, snr=-1.0 if snr is None else snr, seed=seed,
                 soft=soft, iters=iters, qhard=qhard, post=post, hc_after=ref.coefficients(), state_offsets=np.array(member_offsets()))
        size = os.path.getsize(path)
        assert size < (1 << 20), f"{name}: {size} bytes"
        print(f"{name}: {len(iters)} frames, returns {sorted(set(iters.tolist()))}, cw2 = {model.cw2}, non-finite post values "
              f"{int((~np.isfinite(post)).sum())}, seed {seed}, {size} bytes")
        ref.close()


if __name__ == "__main__":
    main(sys.argv[1:])
