"""Integer advanced sum-product decoder (IASP_DEC, decoder id 5) on the GPU: every tier against the compiled reference's golden
vectors (tolerance 0), random shapes against the numpy restatement (tests/iasp_model.py), the decoders.h surface, the host
harness and `ldpc_sim`."""
import glob
import os
import subprocess

import numpy as np
import pytest

from iasp_model import IASP_GOLDEN_DIR, IaspModel, channel_prior
from ldpc_testlib import IASP_DEC, ROOT, assert_bits_equal, awgn_llr, cycle_code, load_base_matrix, pack_bits, random_qc_code, relift, unpack_bits

pytestmark = pytest.mark.gpu

GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(IASP_GOLDEN_DIR, "iasp_*.npz")))
# the tier each golden set lands on without LDPC_HIP_FORCE_GLOBAL
TIER = {"iasp_m64_2p0": "iasp_spec_appendix_c_m64_kernel (ahead of time)", "iasp_m64_1p2": "iasp_spec_appendix_c_m64_kernel (ahead of time)",
        "iasp_m64_0p0": "iasp_spec_appendix_c_m64_kernel (ahead of time)", "iasp_m64_sat": "iasp_spec_appendix_c_m64_kernel (ahead of time)",
        "iasp_m126_1p7": "iasp_body instance (hiprtc)", "iasp_30x60_m67_2p0": "iasp_body instance (hiprtc)", "iasp_m1_4p0": "iasp_body instance (hiprtc)",
        "iasp_cw2_m64_2p0": "iasp_global_kernel", "iasp_cw2_m128_2p0": "iasp_global_kernel"}


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _golden(name):
    g = np.load(os.path.join(IASP_GOLDEN_DIR, name + ".npz"))
    return g["H"], int(g["M"]), g["llr"], int(g["maxiter"]), g


def _check_golden(L, torch, name, expect):
    H, M, llr, maxiter, g = _golden(name)
    with L.LdpcHip(IASP_DEC, H, M) as dec:
        assert dec.kernel_name == expect, dec.kernel_name
        hard, iters, soft = dec.decode(torch.from_numpy(llr).cuda(), maxiter, want_soft=True)
        torch.cuda.synchronize()
        assert np.array_equal(iters.cpu().numpy(), g["iters"])
        assert np.array_equal(hard.cpu().numpy().view(np.uint32), g["hard"])
        assert_bits_equal(soft.cpu().numpy(), g["soft"])
        d1, it1, after = dec.decode_host(llr, maxiter, decision=1)           # upstream's per-frame arrays
        assert np.array_equal(it1, g["iters"])
        assert_bits_equal(d1, g["soft"])
        assert_bits_equal(after, channel_prior(llr))                    # soft[] clobbered like decoders.cpp:3858-3863
        d0, it0, _ = dec.decode_host(llr, maxiter, decision=0)
        assert np.array_equal(it0, g["iters"]) and np.array_equal(pack_bits(d0), g["hard"])


def test_every_golden_set_is_covered():
    assert set(GOLDENS) == set(TIER)


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_vectors_on_the_default_tier(L, torch, name):
    """Appendix C at M = 64: the ahead-of-time instance; M = 126, 1 and the 30 x 60 shape of upstream's input12L.jsonx at M = 67:
    hiprtc instances of the same body; codes whose columns all have weight 2: upstream's own branch on the shape-unlimited tier."""
    _check_golden(L, torch, name, TIER[name])


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_vectors_on_the_forced_global_tier(L, torch, name, monkeypatch):
    monkeypatch.setenv("LDPC_HIP_FORCE_GLOBAL", "1")
    _check_golden(L, torch, name, "iasp_global_kernel")


def _rows_of_weight(rng, rh, nh, M, w):
    H = -np.ones((rh, nh), dtype=np.int16)
    start = 0
    for j in range(rh):
        for q in range(w):
            H[j, (start + q) % nh] = rng.randint(0, M)
        start += max(1, w - 1)
    return H


def _vs_model(L, torch, H, M, llr, maxiter, expect=None):
    H = np.asarray(H, dtype=np.int16)
    soft_m, it_m, _, so_m = IaspModel(H, M).decode(llr, maxiter, 1)
    with L.LdpcHip(IASP_DEC, H, M) as dec:
        if expect:
            assert expect in dec.kernel_name, dec.kernel_name
        hard, iters, soft = dec.decode(torch.from_numpy(llr).cuda(), maxiter, want_soft=True)
        torch.cuda.synchronize()
        assert np.array_equal(iters.cpu().numpy(), it_m)
        assert np.array_equal(unpack_bits(hard.cpu().numpy(), H.shape[1] * M), (so_m >> 15).astype(np.uint8))
        assert_bits_equal(soft.cpu().numpy(), soft_m)
        return dec.kernel_name, it_m


def _llr(H, M, snr, seed, frames):
    return awgn_llr(np.asarray(H, dtype=np.int32), M, snr, seed, frames, burn_codeword=False)


SHAPES = [  # what, factory(rng) -> H, M, snr, frames, expected kernel
    ("row weight 2", lambda r, M: _rows_of_weight(r, 4, 5, M, 2), 33, 3.0, 24, "iasp_body"),
    ("row weight 5", lambda r, M: _rows_of_weight(r, 4, 10, M, 5), 31, 3.0, 24, "iasp_body"),
    ("row weight 8", lambda r, M: _rows_of_weight(r, 4, 16, M, 8), 64, 3.0, 16, "iasp_body"),
    ("row weight 12", lambda r, M: _rows_of_weight(r, 4, 20, M, 12), 100, 3.0, 12, "iasp_body"),
    ("row weight 16", lambda r, M: _rows_of_weight(r, 4, 24, M, 16), 255, 3.0, 8, "iasp_body"),
    ("row weight 20 > 16", lambda r, M: _rows_of_weight(r, 4, 28, M, 20), 32, 4.0, 16, "iasp_global_kernel"),
    ("lifting 1", lambda r, M: random_qc_code(r, 6, 14, M, [2, 3]), 1, 4.0, 64, "iasp_body"),
    ("lifting 5", lambda r, M: random_qc_code(r, 6, 14, M, [2, 3]), 5, 3.0, 48, "iasp_body"),
    ("lifting 67", lambda r, M: random_qc_code(r, 6, 14, M, [2, 3, 4]), 67, 2.0, 16, "iasp_body"),
    ("lifting 512", lambda r, M: random_qc_code(r, 4, 10, M, [2, 3]), 512, 2.5, 6, "iasp_body"),
    ("70 block rows > 64", lambda r, M: random_qc_code(r, 70, 140, M, [2, 3, 3, 4]), 8, 2.5, 8, "iasp_global_kernel"),
    ("weight-2 columns", lambda r, M: cycle_code(r, 5, 10, M), 33, 2.5, 24, "iasp_global_kernel"),
    ("weight-2 columns, lifting 1", lambda r, M: cycle_code(r, 3, 7, M), 1, 3.0, 64, "iasp_global_kernel"),
]


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[s[0] for s in SHAPES])
def test_random_shapes_against_the_model(L, torch, i):
    what, factory, M, snr, frames, expect = SHAPES[i]
    H = factory(np.random.RandomState(900 + i), M)
    _vs_model(L, torch, H, M, _llr(H, M, snr, 40 + i, frames), 30, expect)


def test_an_empty_block_column_runs_on_the_global_tier(L, torch):
    rng = np.random.RandomState(6012)
    H = random_qc_code(rng, 6, 12, 64, [2, 3])
    H[:, 11] = -1
    for j in range(6):
        while (H[j, 6:] >= 0).sum() < 2:
            H[j, 6 + rng.randint(0, 5)] = rng.randint(0, 64)
    _vs_model(L, torch, H, 64, _llr(H, 64, 3.0, 3, 16), 30, "iasp_global_kernel")


@pytest.mark.parametrize("B", [1, 7, 1000])
def test_batch_sizes(L, torch, B):
    """The AOT instance (one frame per workgroup) and the global tier (capped grid striding over the frames) on odd batch sizes."""
    H = relift(load_base_matrix(), 64)
    llr = _llr(H, 64, 1.8, 77, B)
    _vs_model(L, torch, H, 64, llr, 50, "ahead of time")
    os.environ["LDPC_HIP_FORCE_GLOBAL"] = "1"
    try:
        _vs_model(L, torch, H, 64, llr, 50, "iasp_global_kernel")
    finally:
        del os.environ["LDPC_HIP_FORCE_GLOBAL"]


def test_a_row_of_weight_one_is_refused(L, torch):
    H1 = -np.ones((3, 6), dtype=np.int16)
    H1[0, 0] = 0; H1[1, 1] = 0; H1[2, 2] = 0; H1[1, 3] = 5; H1[2, 4] = 7; H1[1, 5] = 2; H1[2, 5] = 3   # block row 0: one circulant
    for M in (1, 64, 600):
        with pytest.raises(L.LdpcHipError):
            L.LdpcHip(IASP_DEC, H1, M)


def test_decode_host_clobbers_the_input_with_the_channel_prior(L, torch):
    H = relift(load_base_matrix(), 64)
    llr = _llr(H, 64, 2.0, 5, 4) * 7.0
    llr[0, :8] = [20.0, -20.0, 0.0, -0.0, 19.999999999999996, -20.000000000000004, 1e-300, -1e-300]
    with L.LdpcHip(IASP_DEC, H, 64) as dec:
        _, _, after = dec.decode_host(llr, 50, decision=0)
        _, _, kept = dec.decode_host(llr, 50, decision=0, clobber_sp_input=False)
    y = np.minimum(np.maximum(llr, -20.0), 20.0)
    assert_bits_equal(after, channel_prior(llr))
    assert np.allclose(after, 1.0 / (1.0 + np.exp(y)), rtol=1e-15, atol=0)
    assert np.array_equal(kept, llr)


def test_decoders_h_surface(L, torch, tmp_path):
    """decod_open(IASP_DEC) / hd fill / decod_init / isum_prod_gf2_decod_qc_lm(st, st->y, st->decword, ...) frame by frame from C++."""
    L.load_library()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = str(tmp_path / "iasp_compat_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "iasp_compat_driver.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_compat", "-lldpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    for name in ("iasp_m64_1p2", "iasp_cw2_m64_2p0"):
        H, M, llr, maxiter, g = _golden(name)
        B, N = llr.shape
        for decision in (0, 1):
            with open(tmp_path / "in.bin", "wb") as f:
                f.write(np.array([H.shape[0], H.shape[1], M, B, maxiter, decision], dtype=np.int32).tobytes())
                f.write(np.ascontiguousarray(H, dtype=np.int16).tobytes())
                f.write(np.ascontiguousarray(llr, dtype=np.float64).tobytes())
            subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
            raw = open(tmp_path / "out.bin", "rb").read()
            iters = np.frombuffer(raw[:4 * B], dtype=np.int32)
            dec = np.frombuffer(raw[4 * B:4 * B + 8 * B * N], dtype=np.float64).reshape(B, N)
            after = np.frombuffer(raw[4 * B + 8 * B * N:], dtype=np.float64).reshape(B, N)
            assert np.array_equal(iters, g["iters"])
            if decision:
                assert_bits_equal(dec, g["soft"])
            else:
                assert np.array_equal(pack_bits(dec), g["hard"])
            assert_bits_equal(after, channel_prior(llr))


def test_ldpc_sim_equals_the_python_host_harness(L, torch, tmp_path):
    """`ldpc_sim simulation examples/simulation_iasp.jsonx`: its frame and bit error rates equal ldpc_lib_amd.host's exact-replay
    harness with decoder_type 5 on the same generator seed."""
    from ldpc_lib_amd.host import bp_simulation
    exe = os.path.join(ROOT, "ldpc-lib_amd", "ldpc_sim")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    out = str(tmp_path / "result.jsonx")
    subprocess.check_call([exe, "simulation", os.path.join(ROOT, "examples", "simulation_iasp.jsonx"), out])

    def get(path):
        return subprocess.check_output([exe, "jsonx-get", out, path], text=True).strip()

    def numbers(path):
        return [float(x) for x in get(path).replace("array {", "").replace("}", "").split()]
    assert int(get("results/0/_decoder_type")) == IASP_DEC
    fer, ber = numbers("results/0/simulation_logs/0/FER"), numbers("results/0/simulation_logs/0/BER")
    H = relift(load_base_matrix(), 64)
    b, f, st = bp_simulation(H, 64, 50, 1000000, 3000, 2.0, 1.0, decoder_type=IASP_DEC, exact_seed=1, return_state=True)
    assert st["experiment"] == 3001
    assert st["nde"] > 0
    assert fer[0] == f and ber[0] == b


def test_logical_shards_give_identical_results(L, torch):
    """n = 1, 2, 8 shards mapped to device 0: the same counters and per-frame records as one context's ldpc_hip_simulate."""
    H = relift(load_base_matrix(), 64)
    snr, seed, first, B = 1.7, 31, 5000, 2000
    with L.LdpcHip(IASP_DEC, H, 64) as dec:
        want = dec.simulate(snr, 50, seed, first, B)
        llr = dec.channel_llr(snr, seed, first, B)
        hard, iters, _ = dec.decode(llr, 50)
        _, info = dec.count_errors(hard, iters, want_frame_info=True, first_frame=first)
        want_info, want_it = info.cpu().numpy(), iters.cpu().numpy()
    assert want["nde"] > 0
    for n, batch in ((1, 1000), (2, 700), (8, 128), (3, 333)):
        with L.LdpcHipMulti(IASP_DEC, H, 64, [0] * n) as m:
            got = m.simulate(snr, 50, seed, first, B, batch, records=True)
            for k in want:
                assert got[k] == want[k], (n, batch, k)
            assert np.array_equal(got["frame_info"], want_info) and np.array_equal(got["iters"], want_it)
