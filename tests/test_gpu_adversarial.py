"""GPU: every decoder on every kernel tier against its reference on the adversarial channel values of ldpc_testlib.adversarial_llr
(signed zeros, subnormals, huge magnitudes, values on and next to the clamp limits, exact ties, integer quantiser boundaries,
codewords, all-negative frames), bit for bit: hard decisions, iteration counts, soft values (sign of zero included), the device input
left untouched and the host input clobbered like upstream's.  The references are the C restatement (Oracle) and, for decoder 5, the
numpy model; tests/test_adversarial_cpu.py pins both to the compiled upstream decoders on the same families."""
import os
import subprocess
import sys

import numpy as np
import pytest

from iasp_model import IaspModel
from ldpc_testlib import (ASP_DEC, BP_DEC, IASP_DEC, IMS_DEC, LMS_DEC, MS_DEC, ROOT, SP_DEC, TASP_DEC, Oracle, _as_double_p, adversarial_llr,
                          assert_bits_equal, awgn_llr, cycle_code, load_base_matrix, oracle_lib, pack_bits, relift)

pytestmark = pytest.mark.gpu

MAXITER = 20


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _base(M):
    return relift(load_base_matrix(), M)


def _other_m64_code():
    """The example protograph with other circulant shifts: not the ahead-of-time instance (tests/test_gpu_parity.py compiles it too)."""
    H = _base(64)
    H2 = H.copy()
    H2[H > 0] = (H[H > 0] * 7 + 3) % 64
    return H2


def _cw2_code():
    return cycle_code(np.random.RandomState(1), 4, 8, 64)      # the shape tests/test_gpu_shapes.py runs on asp_global_kernel


AOT = " (ahead of time)"
JIT = " instance (hiprtc)"
# id: decoder, code, lifting, environment, kernel name (exact), IMS parameters (thr, qbits, dbits) or None, frames (None: the batch as built)
CELLS = {
    "ms-m64_body-persistent-queue": (MS_DEC, _base, 64, {}, "ms_spec_appendix_c_m64_kernel" + AOT, None, 2600),
    "ms-flood_m64-atomic": (MS_DEC, _base, 64, {"LDPC_HIP_MS_VARIANT": "0"}, "ms_flood_m64_kernel<atomic>", None, None),
    "ms-flood_m64-rmw": (MS_DEC, _base, 64, {"LDPC_HIP_MS_VARIANT": "1"}, "ms_flood_m64_kernel<rmw>", None, None),
    "ms-flood-generic": (MS_DEC, _base, 64, {"LDPC_HIP_MS_VARIANT": "-1"}, "ms_flood_kernel", None, None),
    "ms-small_body-m1": (MS_DEC, _base, 1, {}, "ms_small_body" + JIT, None, None),
    "ms-small_body-m7": (MS_DEC, _base, 7, {}, "ms_small_body" + JIT, None, None),
    "ms-small_body-m16": (MS_DEC, _base, 16, {}, "ms_small_body" + JIT, None, None),
    "ms-chunk_body-m126": (MS_DEC, _base, 126, {}, "ms_chunk_appendix_c_m126_kernel" + AOT, None, None),
    "ms-ms_body-m126": (MS_DEC, _base, 126, {"LDPC_HIP_MS_CHUNK": "0"}, "ms_spec_appendix_c_m126_kernel" + AOT, None, None),
    "ms-ms_body-m200": (MS_DEC, _base, 200, {}, "ms_body" + JIT, None, None),
    "ms-flood-multiwave-m200": (MS_DEC, _base, 200, {"LDPC_HIP_MS_VARIANT": "-1"}, "ms_flood_kernel<multiwave>", None, None),
    "ms-global": (MS_DEC, _base, 64, {"LDPC_HIP_FORCE_GLOBAL": "1"}, "ms_global_kernel", None, None),
    "lms-lms_body-m64-persistent-queue": (LMS_DEC, _base, 64, {}, "lms_spec_appendix_c_m64_kernel" + AOT, None, 2600),
    "lms-lms_body-m200": (LMS_DEC, _base, 200, {}, "lms_body" + JIT, None, None),
    "lms-small_body-m24": (LMS_DEC, _base, 24, {}, "lms_small_body" + JIT, None, None),
    "lms-layered-generic": (LMS_DEC, _base, 64, {"LDPC_HIP_MS_VARIANT": "-1"}, "lms_layered_kernel", None, None),
    "lms-global": (LMS_DEC, _base, 64, {"LDPC_HIP_FORCE_GLOBAL": "1"}, "lms_global_kernel", None, None),
    "ims-ims_body-int8": (IMS_DEC, _base, 64, {}, "ims_spec_appendix_c_m64_kernel" + AOT, None, None),
    "ims-ims_body-int8-thr2-q6": (IMS_DEC, _base, 64, {}, "ims_spec_appendix_c_m64_kernel" + AOT, (2.0, 6, 8), None),
    "ims-ims_body-int8-thr0.75-q5": (IMS_DEC, _base, 64, {}, "ims_spec_appendix_c_m64_kernel" + AOT, (0.75, 5, 8), None),
    "ims-small_body-m20": (IMS_DEC, _base, 20, {}, "ims_small_body" + JIT, None, None),
    "ims-flood-dbits10": (IMS_DEC, _base, 64, {}, "ims_flood_kernel", (1.4, 6, 10), None),
    "ims-flood-table-m512": (IMS_DEC, _base, 512, {"LDPC_HIP_MS_VARIANT": "-1"}, "ims_flood_kernel<multiwave>", None, None),
    "ims-global": (IMS_DEC, _base, 64, {"LDPC_HIP_FORCE_GLOBAL": "1"}, "ims_global_kernel", None, None),
    "sp-sp_body-aot": (SP_DEC, _base, 64, {}, "sp_spec_appendix_c_m64_kernel" + AOT, None, None),
    "sp-sp_body-hiprtc": (SP_DEC, lambda M: _other_m64_code(), 64, {}, "sp_body" + JIT, None, None),
    "sp-flood": (SP_DEC, _base, 64, {"LDPC_HIP_MS_VARIANT": "-1"}, "sp_flood_kernel", None, None),
    "sp-global": (SP_DEC, _base, 64, {"LDPC_HIP_FORCE_GLOBAL": "1"}, "sp_global_kernel", None, None),
    "asp-asp_body-aot": (ASP_DEC, _base, 64, {}, "asp_spec_appendix_c_m64_kernel" + AOT, None, None),
    "asp-asp_body-hiprtc-m20": (ASP_DEC, _base, 20, {}, "asp_body" + JIT, None, None),
    "asp-global": (ASP_DEC, _base, 64, {"LDPC_HIP_FORCE_GLOBAL": "1"}, "asp_global_kernel", None, None),
    "asp-global-weight2-columns": (ASP_DEC, lambda M: _cw2_code(), 64, {}, "asp_global_kernel", None, None),
    "tasp-tasp_body-aot-m64": (TASP_DEC, _base, 64, {}, "tasp_spec_appendix_c_m64_kernel" + AOT, None, None),
    "tasp-tasp_body-aot-m126": (TASP_DEC, _base, 126, {}, "tasp_spec_appendix_c_m126_kernel" + AOT, None, None),
    "tasp-tasp_body-hiprtc-m40": (TASP_DEC, _base, 40, {}, "tasp_body" + JIT, None, None),
    "tasp-global": (TASP_DEC, _base, 64, {"LDPC_HIP_FORCE_GLOBAL": "1"}, "tasp_global_kernel", None, None),
    "bp-bp_body-aot": (BP_DEC, _base, 64, {}, "bp_spec_appendix_c_m64_kernel" + AOT, None, None),
    "bp-bp_body-hiprtc-m9": (BP_DEC, _base, 9, {}, "bp_body" + JIT, None, None),
    "bp-global": (BP_DEC, _base, 64, {"LDPC_HIP_FORCE_GLOBAL": "1"}, "bp_global_kernel", None, None),
    "iasp-iasp_body-aot": (IASP_DEC, _base, 64, {}, "iasp_spec_appendix_c_m64_kernel" + AOT, None, None),
    "iasp-iasp_body-hiprtc-m1": (IASP_DEC, _base, 1, {}, "iasp_body" + JIT, None, None),
    "iasp-global-general": (IASP_DEC, _base, 64, {"LDPC_HIP_FORCE_GLOBAL": "1"}, "iasp_global_kernel", None, None),
    "iasp-global-weight2-columns": (IASP_DEC, lambda M: _cw2_code(), 64, {}, "iasp_global_kernel", None, None),
}


def _batch(H, M):
    """The adversarial families plus one AWGN frame: 29 frames, a prime, so every multi-frame wave layout ends ragged."""
    llr, labels = adversarial_llr(H, M, 11)
    return np.concatenate([llr, awgn_llr(np.asarray(H, dtype=np.int32), M, 1.5, 77, 1, burn_codeword=False)]), labels + ["awgn 1.5 dB"]


def _reference(dec_id, H, M, llr, decision, ims):
    """(decword, iters, input as the decoder leaves it) of a fresh reference state (Gallager BP carries its syndrome between calls)."""
    if dec_id == IASP_DEC:
        d, it, after, _ = IaspModel(H, M).decode(llr, MAXITER, decision)
        return d, it, after
    o = Oracle(H, M)
    if dec_id == IMS_DEC and ims is not None:
        thr, qbits, dbits = ims
        after = llr.copy()
        d = np.empty_like(llr)
        it = np.empty(len(llr), dtype=np.int32)
        for f in range(len(llr)):
            it[f] = oracle_lib().orc_imin_sum(o.h, _as_double_p(after[f]), _as_double_p(d[f]), MAXITER, decision, 0.8, thr, qbits, dbits)
        return d, it, after
    return o.decode(dec_id, llr, MAXITER, decision)


def _check_frames(what, got, want, labels):
    for f in range(len(want)):
        assert_bits_equal(got[f], want[f], f"{what}, frame {f} ({labels[f % len(labels)]})")


@pytest.mark.parametrize("cell", list(CELLS))
def test_every_tier_is_bit_exact_on_adversarial_frames(L, torch, monkeypatch, cell):
    dec_id, code, M, env, expect, ims, frames = CELLS[cell]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    H = np.asarray(code(M), dtype=np.int16)
    llr, labels = _batch(H, M)
    d0, it0, after0 = _reference(dec_id, H, M, llr, 0, ims)
    d1, it1, after1 = _reference(dec_id, H, M, llr, 1, ims)
    assert np.array_equal(it0, it1)
    soft_want = d1
    if dec_id == TASP_DEC:          # upstream ignores `decision`: the host call returns hard decisions; the device soft output is the posteriors
        d1, after1 = d0, after0
    idx = np.arange(frames or len(llr)) % len(llr)   # persistent-queue cells: more frames than resident workgroups, pulled from the queue

    def ctx():
        dec = L.LdpcHip(dec_id, H, M)
        if ims is not None:
            dec.set_ims_params(*ims)
        if ims is None or ims[2] <= 8:          # (messages beyond int8 are a per-launch choice: last_launch() below)
            assert dec.kernel_name == expect, dec.kernel_name
        return dec

    with ctx() as dec:
        x = torch.from_numpy(llr[idx]).cuda()
        hard, iters, soft = dec.decode(x, MAXITER, want_soft=True)
        torch.cuda.synchronize()
        assert dec.last_launch() == expect, dec.last_launch()
        it = iters.cpu().numpy()
        bad = np.flatnonzero(it != it0[idx])
        assert not bad.size, [(int(f), labels[f % len(labels)], int(it[f]), int(it0[idx][f])) for f in bad[:8]]
        assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d0[idx]))
        _check_frames("device soft output", soft.cpu().numpy(), soft_want[idx], labels)
        assert_bits_equal(x.cpu().numpy(), llr[idx], "device input after the decode")      # never modified, -0.0 included
    for decision, d_want, a_want in ((0, d0, after0), (1, d1, after1)):
        with ctx() as dec:                          # a fresh context per call, like the fresh reference state
            d, it, after = dec.decode_host(llr, MAXITER, decision=decision)
            assert dec.last_launch() == expect, dec.last_launch()
            assert np.array_equal(it, it0), (decision, it, it0)
            _check_frames(f"decode_host decision {decision} decword", d, d_want, labels)
            _check_frames(f"decode_host decision {decision} clobbered input", after, a_want, labels)


def test_the_matrix_covers_every_decoder_and_shape_unlimited_tier():
    names = {c[4] for c in CELLS.values()}
    for g in ("ms", "lms", "ims", "sp", "asp", "tasp", "bp", "iasp"):
        assert g + "_global_kernel" in names, g
    assert {c[0] for c in CELLS.values()} == {MS_DEC, LMS_DEC, IMS_DEC, SP_DEC, ASP_DEC, TASP_DEC, BP_DEC, IASP_DEC}


_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import ldpc_lib_amd as L
from test_gpu_adversarial import _base, _batch
H = _base(64)
llr, _ = _batch(H, 64)
idx = np.arange(600) %% len(llr)
out = {}
for dec_id in (%d, %d):
    with L.LdpcHip(dec_id, H, 64) as dec:
        hard, iters, soft = dec.decode(torch.from_numpy(llr[idx]).cuda(), %d, want_soft=True)
        torch.cuda.synchronize()
        out["name%%d" %% dec_id] = np.array(dec.kernel_name)
        out["hard%%d" %% dec_id], out["iters%%d" %% dec_id], out["soft%%d" %% dec_id] = hard.cpu().numpy(), iters.cpu().numpy(), soft.cpu().numpy()
np.savez(sys.argv[1], **out)
"""


def test_the_non_persistent_launch_path_on_adversarial_frames(tmp_path):
    """LDPC_HIP_PERSISTENT=0 is read once per process: min-sum and layered min-sum on the ahead-of-time bodies with one workgroup per
    frame, in a fresh child process."""
    out = str(tmp_path / "np.npz")
    script = _CHILD % (ROOT, os.path.join(ROOT, "tests"), MS_DEC, LMS_DEC, MAXITER)
    env = dict(os.environ, LDPC_HIP_PERSISTENT="0")
    subprocess.run([sys.executable, "-c", script, out], env=env, check=True, timeout=300)
    g = np.load(out)
    H = _base(64)
    llr, labels = _batch(H, 64)
    idx = np.arange(600) % len(llr)
    for dec_id, name in ((MS_DEC, "ms_spec_appendix_c_m64_kernel"), (LMS_DEC, "lms_spec_appendix_c_m64_kernel")):
        assert name in str(g["name%d" % dec_id])
        d0, it0, _ = Oracle(H, 64).decode(dec_id, llr, MAXITER, 0)
        d1, _, _ = Oracle(H, 64).decode(dec_id, llr, MAXITER, 1)
        assert np.array_equal(g["iters%d" % dec_id], it0[idx])
        assert np.array_equal(g["hard%d" % dec_id].view(np.uint32), pack_bits(d0[idx]))
        _check_frames("device soft output", g["soft%d" % dec_id], d1[idx], labels)
