"""A restatement of what upstream's harness does for q_mod > 2 (bp_simulation.cpp), from pieces the tests already have:

  setup             :348-399: decod_init with fht_ncols2convert = ncols2convert rewrites the first columns of hc from powers to field
                    elements, the rewritten hc goes back to the caller, left2right moves both matrices, decod_init runs again with 0
  message / word    :537-557: the eight symbols of :544 as include/ldpc_hip.h defines the message, through encode_NBQCLDPC; a refusal
                    or ok = 0 sends the all-zero word
  gaussians         std::mt19937(seed) + a fresh std::normal_distribution per sample (oracle/harness_oracle.cpp): frame f takes
                    samples [f * N * q_bits, (f + 1) * N * q_bits) in index order, nothing is drawn before the frame loop (:638-642)
  frames            gfq_chain_model.channel (:644-676) -> the decoder with p_thr = 0 -> gfq_chain_model.count (:746-755, :805-810); the
                    decoder is the compiled upstream (gfq_ref.GfqReference) where oracle/_ref exists, gfq_model.GfqModel otherwise
  result            the stopping rule (:591, :805-823) over the records and the pair of :840

The cases the golden sets under tests/golden/gfq_exact/ record (tools/make_gfq_exact_goldens.py) are listed here, so that the golden
maker, the CPU test that regenerates them and the GPU tests name the same things.  Test infrastructure only.
"""
import ctypes as C
import math
import os

import numpy as np

import gfq_chain_model as cm
from gfq_model import GfqModel, gf_tables
from gfq_ref import GfqReference, gfq_ref_available
from ldpc_testlib import oracle_lib

EXACT_GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gfq_exact")
UPSTREAM_MESSAGE = (6, 11, 0, 4, 2, 1, 2, 5)   # bp_simulation.cpp:544

# the shipped GF(16) 4 x 8 pattern (tests/golden/jsonx/resultq.jsonx, as tools/make_gfq_goldens.py holds it)
SHIPPED_HB = [[0, -1, -1, 73, 2, -1, -1, 1], [0, 0, -1, -1, -1, 11, -1, -1], [-1, 0, 0, -1, 1, -1, 13, 17], [-1, -1, 0, 12, -1, 13, 1, -1]]
SHIPPED_HC = [[1, -1, -1, 73, 2, -1, -1, 1], [1, 2, -1, -1, -1, 11, -1, -1], [-1, 2, 3, -1, 1, -1, 13, 17], [-1, -1, 3, 30, -1, 13, 1, -1]]

# name: q_bits, M, code, word ("enc" = the encoded message, "zero"), ncols2convert, snr, punctured_blocks, maxiter, frames, seed, and
# the stopping rule (n_frame_errors, n_experiments, reference_frame_error) the result pair is taken under
CASES = {
    "s1_gf16_m8_zero": dict(q_bits=4, M=8, code="shipped", word="zero", n2c=0, snr=2.0, punct=0, maxiter=15, frames=256, seed=11, stop=(20, 255, 1.0)),
    "s1_gf16_m8_enc": dict(q_bits=4, M=8, code="shipped", word="enc", n2c=0, snr=2.0, punct=1, maxiter=15, frames=256, seed=12, stop=(500, 199, 1.0)),
    "s2_gf4_m5_enc": dict(q_bits=2, M=5, code="w2", word="enc", n2c=0, snr=2.5, punct=0, maxiter=20, frames=512, seed=13, stop=(500, 500, 0.01)),
    "s2_gf4_m5_zero": dict(q_bits=2, M=5, code="w2", word="zero", n2c=0, snr=2.5, punct=0, maxiter=20, frames=512, seed=14, stop=(15, 500, 1.0)),
    "s3_gf64_m7_enc": dict(q_bits=6, M=7, code="xox", word="enc", n2c=2, snr=1.5, punct=0, maxiter=10, frames=64, seed=15, stop=(8, 63, 1.0)),
    "s3_gf64_m7_zero": dict(q_bits=6, M=7, code="oxo", word="zero", n2c=0, snr=1.5, punct=0, maxiter=10, frames=64, seed=16, stop=(100, 40, 1.0)),
}


def inverse_left2right(matr):
    """What left2right (decoders.cpp:174-195) turns into matr."""
    m = np.array(matr)
    rh, nh = m.shape
    out = np.empty_like(m)
    out[:, rh:] = m[:, :nh - rh]
    out[:, rh - 1] = m[:, nh - rh]
    out[:, :rh - 1] = m[:, nh - rh + 1:]
    return out


def shipped(M, q):
    """main_simulation.cpp:400-429: shifts % M (0 -> 1 in column rows - 1), coefficients % q with 0 -> q - 1."""
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


def harness_inputs(name):
    """(H, coef) int16 [rh, nh] as a caller hands them to bp_simulation(q_mod, H, coef, ...): before left2right, the first ncols2convert
    columns of coef as powers of the primitive element."""
    p = CASES[name]
    q_bits, M = p["q_bits"], p["M"]
    if p["code"] == "shipped":
        H, coef = shipped(M, 1 << q_bits)
    else:
        hb, hc = cm.make_code(np.random.RandomState(sum(map(ord, name[:2])) + q_bits), q_bits, 3, 6, M, p["code"])
        H, coef = inverse_left2right(hb), inverse_left2right(hc)
    coef = np.array(coef, dtype=np.int16)
    lg, _ = gf_tables(q_bits)
    for k in range(p["n2c"]):
        coef[:, k] = np.where(coef[:, k] > 0, lg[np.maximum(coef[:, k], 1)], coef[:, k])
    return np.array(H, dtype=np.int16), coef


def upstream_message(q_bits, K):
    msg = np.zeros(K, dtype=np.int16)
    for i in range(min(K, 8)):
        msg[i] = UPSTREAM_MESSAGE[i] & ((1 << q_bits) - 1)
    return msg


def setup(q_bits, H, coef, ncols2convert):
    """-> (hb, hc, coef_back): the matrices the frame loop runs on, and what bp_simulation leaves in the caller's coef_matrix (:384-389)."""
    _, alog = gf_tables(q_bits)
    back = np.array(coef, dtype=np.int16)
    for k in range(ncols2convert):                                        # decoders.cpp:1151-1159
        back[:, k] = np.where(back[:, k] > -1, alog[np.maximum(back[:, k], 0)], back[:, k])
    return cm.left2right(np.asarray(H, dtype=np.int16)), cm.left2right(back), back


def transmitted_word(q_bits, hb, hc, M):
    """(word [N] int16, encoded): the message through encode_NBQCLDPC; flag == 0 falls back to the all-zero word (:552-556)."""
    rh, nh = hb.shape
    msg = upstream_message(q_bits, (nh - rh) * M)
    try:
        cw, ok = cm.encode(q_bits, hb, hc, M, msg[None])
    except cm.EncodeRefused:
        return np.zeros(nh * M, dtype=np.int16), False
    if not ok[0]:
        return np.zeros(nh * M, dtype=np.int16), False
    return cw[0], True


def sigma_of(rh, nh, snr_db, punctured_blocks):
    bitrate = (nh - rh) / (nh - punctured_blocks)                         # :444
    return math.sqrt(math.pow(10, -snr_db / 10) / 2 / bitrate)           # :445


def gaussians(seed, frames, per_frame, skip_frames=0):
    """Frames [skip_frames, skip_frames + frames) of the stream of std::mt19937(seed): [frames, per_frame]."""
    out = np.empty((skip_frames + frames) * per_frame, dtype=np.float64)
    oracle_lib().orc_rng_gaussians(int(seed), 0, out.ctypes.data_as(C.POINTER(C.c_double)), out.size)
    return out[skip_frames * per_frame:].reshape(frames, per_frame)


def decoder(q_bits, hb, hc, M):
    return GfqReference(q_bits, hb, hc, M) if gfq_ref_available() else GfqModel(q_bits, hb, hc, M)


def frames(q_bits, hb, hc, M, word, noise, sigma, maxiter):
    """-> (frame_info [B], iters [B], counters [5], max |LH|) of the frame loop over the given Gaussians [B, N * q_bits]."""
    rh = hb.shape[0]
    B = noise.shape[0]
    cw = np.broadcast_to(word, (B, word.shape[0]))
    soft = cm.channel(q_bits, cw, noise, sigma)
    iters, qhard = decoder(q_bits, hb, hc, M).decode(soft, maxiter)[:2]
    cnt, info = cm.count(qhard, cw, iters, rh * M)
    return info, np.asarray(iters, dtype=np.int32), cnt, float(np.abs(cm.channel_lh_range(q_bits, cw, noise, sigma)).max())


def stop_rule(info, n_frame_errors, n_experiments, reference_frame_error):
    """(experiment, nse, nde, ending) of :591 and :805-823 over the records; ending: "nde", "experiments", "reference" or "records" (ran out)."""
    experiment = nse = nde = 0
    for rec in info:
        if not nde < n_frame_errors:
            return experiment, nse, nde, "nde"
        if not experiment <= n_experiments:
            return experiment, nse, nde, "experiments"
        experiment += 1
        rec = int(rec)
        if rec != 0:
            nse += rec & ((1 << 30) - 1)
            nde += 1
            if nde >= 10 and float(nde) / float(experiment) > 2.5 * reference_frame_error:
                return experiment, nse, nde, "reference"
    if not nde < n_frame_errors:
        return experiment, nse, nde, "nde"
    if not experiment <= n_experiments:
        return experiment, nse, nde, "experiments"
    return experiment, nse, nde, "records"


def result_pair(experiment, nse, nde, n, r):
    return float(nse) / experiment / (n - r), float(nde) / experiment   # :840


def run_case(name):
    """Everything a golden set holds, as a dict of arrays."""
    p = CASES[name]
    q_bits, M = p["q_bits"], p["M"]
    H, coef = harness_inputs(name)
    hb, hc, back = setup(q_bits, H, coef, p["n2c"])
    rh, nh = hb.shape
    N, R = nh * M, rh * M
    if p["word"] == "enc":
        word, encoded = transmitted_word(q_bits, hb, hc, M)
    else:
        word, encoded = np.zeros(N, dtype=np.int16), False
    sigma = sigma_of(rh, nh, p["snr"], p["punct"])
    noise = gaussians(p["seed"], p["frames"], N * q_bits)
    info, iters, cnt, max_lh = frames(q_bits, hb, hc, M, word, noise, sigma, p["maxiter"])
    experiment, nse, nde, ending = stop_rule(info, *p["stop"])
    ber, fer = result_pair(experiment, nse, nde, N, R)
    return dict(q_bits=q_bits, M=M, H=H, coef=coef, ncols2convert=p["n2c"], hb=hb, hc=hc, coef_back=back, word=word, encoded=int(encoded),
                snr=p["snr"], punctured_blocks=p["punct"], maxiter=p["maxiter"], seed=p["seed"], frame_info=info, iters=iters,
                counters=np.array(cnt, dtype=np.int64), max_lh=max_lh, stop=np.array(p["stop"], dtype=np.float64),
                stop_state=np.array([experiment, nse, nde], dtype=np.int64), ending=ending, ber_fer=np.array([ber, fer]))


def load(name):
    return np.load(os.path.join(EXACT_GOLDEN_DIR, name + ".npz"))
