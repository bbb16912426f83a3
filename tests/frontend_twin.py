"""Plain CPU references of the kernels around the decoders (ldpc-lib_amd/csrc/ldpc_frontend.hpp, ldpc_encode.hpp); no GPU.

  chain_twin        codeword -> direct interleaver -> mapper -> AWGN -> demapper -> inverse interleaver -> puncturing, for any
                    (H, M), with the interleaver maps as arguments (so upstream's recorded maps can be passed)
  count_twin        the five error counters and the per-frame record of count_errors_kernel
  random_info_twin  the information bits of random_info_kernel
and the four code shapes tests/test_gpu_frontend_shapes.py runs them at (tests/test_frontend_twin_cpu.py pins the twins).
"""
import os

import numpy as np

from ldpc_testlib import GOLDEN_DIR, _as_double_p, oracle_lib, philox4x32_10, philox_gauss_pairs, random_qc_code

T_CUT = 26.0        # the demapper's exp cut-off in every test


def chain_sigma(H, snr, mod, punct):
    """bp_simulation.cpp:444-449"""
    rh, nh = np.asarray(H).shape
    rate = (nh - rh) / (nh - punct)
    if mod == 0:
        return np.sqrt(10.0 ** (-snr / 10.0) / 2 / rate)
    halfmlog = 1 if mod <= 1 else mod
    Q = 1 << (2 * mod)
    return np.sqrt(10.0 ** (-snr / 10.0) / (2 * rate * halfmlog * 2) * (2.0 * (Q - 1.0) / 3.0))


def chain_twin(H, M, cws, first, B, seed, snr, mod, punct, direct, inverse, punct_val, T=T_CUT):
    """CPU twin of ldpc_hip_channel_llr_dev: bp_simulation.cpp:566-577,596-710 with the device's Philox noise.
    direct / inverse: the interleaver's gather maps (out[i] = in[map[i]]), or None for no interleaver; cws: sent words [ncw, N]
    (frame f carries row f % ncw), or None for the all-zero word; punct_val: what the last punct * M LLRs are set to."""
    rh, nh = np.asarray(H).shape
    N = nh * M
    m = 2 if mod <= 1 else 2 * mod
    if direct is None:
        direct = inverse = np.arange(N)
    units = (N + m - 1) // m
    out = np.zeros((B, N))
    Q = 1 << (2 * mod) if mod >= 1 else 1
    sigma = chain_sigma(H, snr, mod, punct)
    g = philox_gauss_pairs(seed, first + np.arange(B), units, tag=0 if mod <= 1 else 1)
    for b in range(B):
        cw = cws[(first + b) % len(cws)] if cws is not None else np.zeros(N, dtype=np.uint8)
        tx = np.zeros(units * m)
        tx[:N] = cw[direct]                                            # Permutation(.., 0, ..) :570, zero padding :575
        if mod <= 1:
            buf = -2.0 * (sigma * g[b, :N] + 2.0 * tx[:N] - 1.0) / (sigma * sigma)
        else:
            x = np.zeros(2 * units)
            oracle_lib().orc_qam_modulate(Q, _as_double_p(np.ascontiguousarray(tx)), len(tx), _as_double_p(x))
            x = np.ascontiguousarray(x + sigma * g[b])
            dem = np.zeros(units * m)
            oracle_lib().orc_qam_demodulate(Q, float(T), float(sigma), _as_double_p(x), units, _as_double_p(dem), 0)
            buf = -dem[:N]
        y = buf[inverse]                                               # :684
        if punct:
            y[N - M * punct:] = punct_val                              # :697-710
        out[b] = y
    return out


def chain_twin_of_mode(H, M, cws, first, B, seed, snr, mod, punct, perm, punct_val):
    """chain_twin with the maps the library's host-side builder makes for perm = (mode, block, step), or None."""
    direct = inverse = None
    if perm is not None:
        from ldpc_lib_amd.binding import build_interleaver
        direct, inverse = build_interleaver(H, M, perm[0], 1 if mod <= 1 else mod, perm[1], perm[2])
    return chain_twin(H, M, cws, first, B, seed, snr, mod, punct, direct, inverse, punct_val)


def count_twin(bits, iters, R, sent=None):
    """bp_simulation.cpp:731-759,805-810 on decisions bits [B, N] (0/1), iteration counts iters [B] and the sent words sent [B, N]
    (None: the all-zero word).  Returns ([nse, nde, nue, frames, sum |iters|], frame_info int32 [B]): info = wrong bits at indices
    >= R, bit 30 of frame_info = any bit wrong; nse adds info of errored frames, nue counts errored frames with iters >= 0."""
    bits = np.asarray(bits, dtype=np.uint8)
    iters = np.asarray(iters, dtype=np.int64)
    wrong = bits if sent is None else bits ^ np.asarray(sent, dtype=np.uint8)
    info = wrong[:, R:].sum(axis=1, dtype=np.int64)                    # :738 information bits are the indices >= R
    bad = wrong.sum(axis=1, dtype=np.int64) > 0
    frame_info = (info | np.where(bad, 1 << 30, 0)).astype(np.int32)
    nse, nde, nue = int(info[bad].sum()), int(bad.sum()), int((bad & (iters >= 0)).sum())   # :805-810
    return [nse, nde, nue, len(bits), int(np.abs(iters).sum())], frame_info


def random_info_twin(seed, first, count, K):
    """random_info_kernel: word idx = first + w takes groups of 128 bits from philox4x32_10((uint32)idx, idx >> 32, group, 2, seed lo,
    seed hi); bit b of a group is (x[b >> 5] >> (b & 31)) & 1.  Returns uint8 [count, K]."""
    groups = (K + 127) // 128
    idx = (int(first) + np.arange(count, dtype=np.uint64))[:, None]
    grp = np.arange(groups, dtype=np.uint64)[None, :]
    x = philox4x32_10(idx & np.uint64(0xFFFFFFFF), idx >> np.uint64(32), grp, np.uint64(2), seed & 0xFFFFFFFF, seed >> 32)
    out = np.zeros((count, groups * 128), dtype=np.uint8)
    for b in range(128):
        out[:, b::128] = (x[b >> 5] >> np.uint32(b & 31)) & np.uint32(1)
    return out[:, :K]


# ---- the shapes of tests/test_gpu_frontend_shapes.py ---------------------------------------------------------------------------------
def _npz():
    return np.load(os.path.join(GOLDEN_DIR, "interleavers.npz"))


def recorded_interleavers(shape, M):
    """{(halfmlog, mode): (block, step, direct, inverse)} of upstream's recorded maps for base matrices of `shape` at lifting M: the
    first config of every (halfmlog, mode), modes 1..4; and the base matrix."""
    g = _npz()
    out, H = {}, None
    for k in sorted(k[:-4] for k in g.files if k.endswith("_cfg")):
        m, h, mode, bs, st = (int(x) for x in g[k + "_cfg"])
        if g[k + "_H"].shape != tuple(shape) or m != M:
            continue
        H = g[k + "_H"]
        if mode >= 1 and (h, mode) not in out:
            out[(h, mode)] = (bs, st, g[k + "_direct"].astype(np.int64), g[k + "_inverse"].astype(np.int64))
    return out, np.asarray(H, dtype=np.int16)


def code_a():
    """16 x 33 at M = 9: N = 297 (odd), R = 144 = 4 * 32 + 16, 10 packed words"""
    return recorded_interleavers((16, 33), 9)[1], 9


def code_b():
    """16 x 30 at M = 7: N = 210 (even, no multiple of 4 or 8), R = 112 = 3 * 32 + 16, 7 packed words"""
    return recorded_interleavers((16, 30), 7)[1], 7


def code_c():
    """code A's base matrix (shifts below 9) at M = 67: N = 2211, R = 1072 = 33 * 32 + 16, 70 packed words"""
    return code_a()[0], 67


def code_d():
    """3 x 7 at M = 5: N = 35, R = 15 (the information mask lies inside word 0), 2 packed words"""
    return random_qc_code(np.random.RandomState(5), 3, 7, 5, [2, 3]), 5


SATURATION_CASES = ((2, 14.0), (3, 18.0), (4, 22.0))     # (modulation, Eb/N0 in dB) on code A: 0.2 .. 0.8 of the LLRs are +-T


def saturation_reference(mod, snr, punct_val=0.5):
    """The twin's LLRs of the saturating-demapper case: code A, three random rows as sent words, no interleaver, 5 frames."""
    H, M = code_a()
    rng = np.random.RandomState(40 + mod)
    cws = rng.randint(0, 2, size=(3, H.shape[1] * M)).astype(np.uint8)
    first, B, seed = 4_000_000_123, 5, (7 << 32) | 41
    return cws, first, B, seed, chain_twin(H, M, cws, first, B, seed, snr, mod, 0, None, None, punct_val)
