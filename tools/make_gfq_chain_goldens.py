#!/usr/bin/env python3
"""Golden vectors of the GF(q) transmit chain: tests/golden/gfq_chain/chain_*.npz, inputs and expected outputs only.  (A folder of
its own: tests/test_gfq_cpu.py and tests/test_gpu_gfq.py take every npz directly under tests/golden/gfq/ for a decoder set.)

Run where oracle/_ref exists (`make -C oracle ref` with the upstream tree mounted):

    python3 tools/make_gfq_chain_goldens.py

  chain_enc_*.npz      q_bits, M, hb, hc (as given), ncols2convert, msg -> codeword, ok of the COMPILED upstream encode_NBQCLDPC; before
                       writing, the numpy model (tests/gfq_chain_model.py) is asserted equal on every set
  chain_channel_*.npz  q_bits, codeword, noise, sigma -> soft of the scalar channel model (bp_simulation.cpp does not compile here);
                       every LH is asserted outside 512 <= |LH| <= 1100, where glibc's exp takes a path the device does not restate
  chain_sim_gf16_m8.npz  a generated GF(16), M = 8 code, 32 messages, their codewords, noise at SNR_SIM dB, and the iteration sum of
                       GfqModel on the model channel's output -- after asserting that all 32 frames decode to the transmitted word

The shipped GF(16) example (tools/make_gfq_goldens.py:shipped) is NOT encodable by upstream: after left2right its special column
(weight 2) carries a non-zero shift, so encode_NBQCLDPC returns 0 at decoders.cpp:1467-1471.  That is asserted here as the refusal
case, against the compiled reference and the model.
"""
import contextlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gfq_chain_model as cm  # noqa: E402
from gfq_chain_ref import EncoderReference, chain_ref_available  # noqa: E402
from gfq_model import GFQ_GOLDEN_DIR, GfqModel  # noqa: E402
from make_gfq_goldens import shipped  # noqa: E402

SNR_SIM = 6.0
# name: (q_bits, M, rh, nh, scheme, ncols2convert, break_diagonal)
ENC_SETS = {
    "gf4_m1_w2": (2, 1, 2, 4, "w2", 0, False),
    "gf16_m8_xox": (4, 8, 3, 6, "xox", 0, False),
    "gf16_m8_oxo_n2c2": (4, 8, 4, 8, "oxo", 2, False),
    "gf64_m67_oxo": (6, 67, 3, 6, "oxo", 0, False),
    "gf256_m128_xox": (8, 128, 4, 8, "xox", 0, False),
    "gf16_m67_w2": (4, 67, 4, 8, "w2", 0, False),
    "gf16_m8_broken": (4, 8, 4, 8, "xox", 0, True),
}
B_ENC = 37


@contextlib.contextmanager
def quiet():
    """upstream's encoder prints to the C stdout"""
    sys.stdout.flush()
    keep = os.dup(1)
    null = os.open(os.devnull, os.O_WRONLY)
    os.dup2(null, 1)
    try:
        yield
    finally:
        os.dup2(keep, 1)
        os.close(null)
        os.close(keep)


def enc_code(name):
    """The code of an encoder set, hc in the representation the caller hands over: the first ncols2convert columns as powers."""
    q_bits, M, rh, nh, scheme, n2c, brk = ENC_SETS[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    hb, hc = cm.make_code(rng, q_bits, rh, nh, M, scheme, brk)
    lg, _ = cm.gf_tables(q_bits)
    given = hc.copy()
    for k in range(n2c):
        given[:, k] = np.where(hc[:, k] > 0, lg[np.maximum(hc[:, k], 1)], hc[:, k])
    msg = rng.randint(0, 1 << q_bits, (B_ENC, (nh - rh) * M)).astype(np.int16)
    msg[0] = 0
    return q_bits, M, hb, given, n2c, msg


def main():
    assert chain_ref_available(), "needs oracle/_ref and upstream's decoders.h"
    biggest = max(os.path.getsize(os.path.join(GFQ_GOLDEN_DIR, f)) for f in os.listdir(GFQ_GOLDEN_DIR))   # no set larger than a decoder set
    os.makedirs(cm.CHAIN_GOLDEN_DIR, exist_ok=True)

    def save(name, **arrays):
        path = os.path.join(cm.CHAIN_GOLDEN_DIR, name + ".npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) <= biggest, (name, os.path.getsize(path))
        print(name, os.path.getsize(path))

    for name in ENC_SETS:
        q_bits, M, hb, hc, n2c, msg = enc_code(name)
        with quiet():
            ref = EncoderReference(q_bits, hb, hc, M, n2c)
            hc_after = ref.coefficients()
            cw, ok = ref.encode(msg)
            ref.close()
        cw_m, ok_m = cm.encode(q_bits, hb, hc_after, M, msg)
        assert np.array_equal(cw, cw_m) and np.array_equal(ok, ok_m), name
        assert ok.all() != ENC_SETS[name][6] and ok[0] == 1
        save("chain_enc_" + name, q_bits=q_bits, M=M, hb=hb, hc=hc, ncols2convert=n2c, msg=msg, codeword=cw, ok=ok)

    # the refusal case: upstream's own example, as bp_simulation.cpp prepares it
    hb, hc = shipped(8, 16)
    hb, hc = cm.left2right(hb), cm.left2right(hc)
    with quiet():
        ref = EncoderReference(4, hb, hc, 8)
        _, ok = ref.encode(np.zeros((1, 32), dtype=np.int32))
        ref.close()
    assert ok[0] == 0
    try:
        cm.encode(4, hb, hc, 8, np.zeros((1, 32), dtype=np.int64))
        raise AssertionError("the model encodes the shipped example")
    except cm.EncodeRefused as e:
        assert e.rule == "weight 2, non-zero shifts", e.rule

    for q_bits, sigma, tag in ((2, None, "gf4"), (4, None, "gf16"), (6, None, "gf64"), (4, 1e-6, "overflow")):
        N, B = 64, 4
        sigma = cm.sigma_of(4, 8, 2.7) if sigma is None else sigma
        for seed in range(100 + q_bits, 100000, 16):   # the seed is searched until no LH falls into the range that is not restated
            rng = np.random.RandomState(seed)
            cw = rng.randint(0, 1 << q_bits, (B, N)).astype(np.int16)
            noise = rng.standard_normal((B, N * q_bits))
            lh = np.abs(cm.channel_lh_range(q_bits, cw, noise, sigma))
            if not ((lh >= 512) & (lh <= 1100)).any():
                break
        soft = cm.channel(q_bits, cw, noise, sigma)
        assert np.isnan(soft).any() == (tag == "overflow")
        save("chain_channel_" + tag, q_bits=q_bits, codeword=cw, noise=noise, sigma=sigma, soft=soft)

    rng = np.random.RandomState(2024)
    q_bits, M, rh, nh = 4, 8, 4, 8
    hb, hc = cm.make_code(rng, q_bits, rh, nh, M, "xox")
    msg = rng.randint(0, 16, (32, (nh - rh) * M)).astype(np.int16)
    cw, ok = cm.encode(q_bits, hb, hc, M, msg)
    assert ok.all()
    noise = rng.standard_normal((32, nh * M * q_bits))
    sigma = cm.sigma_of(rh, nh, SNR_SIM)
    soft = cm.channel(q_bits, cw, noise, sigma)
    iters, qhard, _ = GfqModel(q_bits, hb, hc, M).decode(soft, 15)
    assert np.array_equal(qhard, cw) and (iters >= 0).all(), "not every frame decodes to the transmitted word: raise SNR_SIM"
    save("chain_sim_gf16_m8", q_bits=q_bits, M=M, hb=hb, hc=hc, msg=msg, codeword=cw, noise=noise, snr=SNR_SIM, maxiter=15,
         iters_sum=int(np.abs(iters).sum()))


if __name__ == "__main__":
    main()
