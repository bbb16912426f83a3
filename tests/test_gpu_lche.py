"""Low-complexity high-efficiency decoder (LCHE_DEC, decoder id 9) on the GPU: every tier against the compiled reference's golden
vectors (tolerance 0, soft values as uint64 images), random shapes, adversarial and boundary frames against the numpy restatement
(tests/lche_model.py), the decoders.h surface, the host harness, `ldpc_sim`, exact replay, puncturing and logical shards.
Every cell asserts the kernel it ran on."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from lche_model import LCHE_GOLDEN_DIR, LcheModel
from ldpc_testlib import (LCHE_DEC, ROOT, adversarial_llr, assert_bits_equal, awgn_llr, load_base_matrix, pack_bits, random_qc_code, relift,
                          unpack_bits)

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_lche_goldens  # noqa: E402

pytestmark = pytest.mark.gpu

AOT = "lche_spec_appendix_c_m64_kernel (ahead of time)"
JIT = "lche_body instance (hiprtc)"
GLOBAL = "lche_global_kernel"
GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(LCHE_GOLDEN_DIR, "lche_*.npz")))
# the tier each golden set lands on without LDPC_HIP_FORCE_GLOBAL
TIER = {"lche_m64_2p0": AOT, "lche_m64_1p5": AOT, "lche_m64_1p2": AOT, "lche_m64_0p0": AOT, "lche_m64_boundary": AOT,
        "lche_m126_1p7": JIT, "lche_m1_4p0": JIT, "lche_30x60_m67_2p0": JIT, "lche_rw1_m32_2p5": JIT}


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
    g = np.load(os.path.join(LCHE_GOLDEN_DIR, name + ".npz"))
    return g["H"], int(g["M"]), g["llr"], int(g["maxiter"]), g


def _check_golden(L, torch, name, expect):
    H, M, llr, maxiter, g = _golden(name)
    with L.LdpcHip(LCHE_DEC, H, M) as dec:
        assert dec.kernel_name == expect, dec.kernel_name
        d_llr = torch.from_numpy(llr).cuda()
        hard, iters, soft = dec.decode(d_llr, maxiter, want_soft=True)
        torch.cuda.synchronize()
        assert np.array_equal(iters.cpu().numpy(), g["iters"])
        assert np.array_equal(hard.cpu().numpy().view(np.uint32), g["hard"])
        assert_bits_equal(soft.cpu().numpy(), g["soft"])
        assert_bits_equal(d_llr.cpu().numpy(), llr)                     # the input is never modified
        for decision in (0, 1):                                          # `decision` is dead: always 0.0 / 1.0
            d, it, after = dec.decode_host(llr, maxiter, decision=decision)
            assert np.array_equal(it, g["iters"])
            assert np.array_equal(pack_bits(d), g["hard"]) and set(np.unique(d)) <= {0.0, 1.0}
            assert_bits_equal(after, llr)


def test_every_golden_set_is_covered():
    assert set(GOLDENS) == set(TIER)


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_vectors_on_the_default_tier(L, torch, name):
    """Appendix C at M = 64: the ahead-of-time instance; M = 126, 1, the 30 x 60 shape at M = 67 and the code with a row of weight
    one: hiprtc instances of the same body."""
    _check_golden(L, torch, name, TIER[name])


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_vectors_on_the_forced_global_tier(L, torch, name, monkeypatch):
    monkeypatch.setenv("LDPC_HIP_FORCE_GLOBAL", "1")
    _check_golden(L, torch, name, GLOBAL)


def test_golden_vectors_without_hiprtc(L, torch, monkeypatch):
    """LDPC_HIP_JIT=0: codes without an ahead-of-time instance run on the shape-unlimited tier."""
    monkeypatch.setenv("LDPC_HIP_JIT", "0")
    _check_golden(L, torch, "lche_m126_1p7", GLOBAL)
    _check_golden(L, torch, "lche_m64_1p2", AOT)


def _vs_model(L, torch, H, M, llr, maxiter, expect):
    H = np.asarray(H, dtype=np.int16)
    m_dec, m_it, m_soft = LcheModel(H, M).decode(llr, maxiter)
    with L.LdpcHip(LCHE_DEC, H, M) as dec:
        assert expect in dec.kernel_name, dec.kernel_name
        hard, iters, soft = dec.decode(torch.from_numpy(llr).cuda(), maxiter, want_soft=True)
        torch.cuda.synchronize()
        assert np.array_equal(iters.cpu().numpy(), m_it)
        assert np.array_equal(unpack_bits(hard.cpu().numpy(), H.shape[1] * M), m_dec.astype(np.uint8))
        assert_bits_equal(soft.cpu().numpy(), m_soft)
        return m_it


def _llr(H, M, snr, seed, frames):
    return awgn_llr(np.asarray(H, dtype=np.int32), M, snr, seed, frames, burn_codeword=False)


def _rows_of_weight(rng, rh, nh, M, w):
    H = -np.ones((rh, nh), dtype=np.int16)
    start = 0
    for j in range(rh):
        for q in range(w):
            H[j, (start + q) % nh] = rng.randint(0, M)
        start += max(1, w - 1)
    return H


def _with_weight_one_row(rng, M):
    H = np.asarray(random_qc_code(rng, 6, 14, M, [2, 3]), dtype=np.int16)
    H[2, :] = -1
    H[2, 5] = rng.randint(0, M)
    return H


def _with_empty_row(rng, M):
    H = np.asarray(random_qc_code(rng, 6, 14, M, [2, 3]), dtype=np.int16)
    H[4, :] = -1
    return H


def _with_empty_column(rng, M):
    H = np.asarray(random_qc_code(rng, 6, 12, M, [2, 3]), dtype=np.int16)
    H[:, 11] = -1
    return H


SHAPES = [  # what, factory(rng, M), M, snr, frames, expected kernel
    ("row weight 1", _with_weight_one_row, 40, 3.0, 24, "lche_body"),
    ("row weight 0", _with_empty_row, 40, 3.0, 24, GLOBAL),
    ("empty block column", _with_empty_column, 64, 3.0, 16, GLOBAL),
    ("row weight 3", lambda r, M: _rows_of_weight(r, 4, 8, M, 3), 33, 3.0, 24, "lche_body"),
    ("row weight 16", lambda r, M: _rows_of_weight(r, 4, 24, M, 16), 96, 3.0, 8, "lche_body"),
    ("row weight 20 > 16", lambda r, M: _rows_of_weight(r, 4, 28, M, 20), 32, 4.0, 16, GLOBAL),
    ("lifting 1", lambda r, M: random_qc_code(r, 6, 14, M, [2, 3]), 1, 4.0, 64, "lche_body"),
    ("lifting 5", lambda r, M: random_qc_code(r, 6, 14, M, [2, 3]), 5, 3.0, 48, "lche_body"),
    ("lifting 67", lambda r, M: random_qc_code(r, 6, 14, M, [2, 3, 4]), 67, 2.0, 16, "lche_body"),
    ("lifting 200", lambda r, M: random_qc_code(r, 4, 10, M, [2, 3]), 200, 2.5, 8, "lche_body"),
    ("lifting 300 > 256", lambda r, M: random_qc_code(r, 4, 10, M, [2, 3]), 300, 2.5, 6, GLOBAL),
    ("70 block rows > 64", lambda r, M: random_qc_code(r, 70, 140, M, [2, 3, 3, 4]), 8, 2.5, 8, GLOBAL),
]


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[s[0] for s in SHAPES])
def test_random_shapes_against_the_model(L, torch, i):
    what, factory, M, snr, frames, expect = SHAPES[i]
    H = factory(np.random.RandomState(700 + i), M)
    _vs_model(L, torch, H, M, _llr(H, M, snr, 60 + i, frames), 30, expect)


@pytest.mark.parametrize("i", [0, 3, 6, 9])
def test_random_shapes_on_the_forced_global_tier(L, torch, i, monkeypatch):
    monkeypatch.setenv("LDPC_HIP_FORCE_GLOBAL", "1")
    what, factory, M, snr, frames, _ = SHAPES[i]
    H = factory(np.random.RandomState(700 + i), M)
    _vs_model(L, torch, H, M, _llr(H, M, snr, 60 + i, frames), 30, GLOBAL)


def test_row_weight_above_1024_is_refused(L, torch):
    H = -np.ones((2, 1100), dtype=np.int16)
    H[0, :1025] = 0
    H[1, 1025:] = 0
    with pytest.raises(L.LdpcHipError):
        L.LdpcHip(LCHE_DEC, H, 1)


@pytest.mark.parametrize("M,tier", [(64, AOT), (5, JIT), (33, JIT), (64, GLOBAL), (5, GLOBAL)])
def test_adversarial_and_boundary_frames(L, torch, M, tier, monkeypatch):
    if tier == GLOBAL:
        monkeypatch.setenv("LDPC_HIP_FORCE_GLOBAL", "1")
    H = relift(load_base_matrix(), M)
    adv, _ = adversarial_llr(H, M, 11)
    bnd = make_lche_goldens.boundary(H, M, awgn_llr(H, M, 2.0, 23, 8))
    _vs_model(L, torch, H, M, np.concatenate([adv, bnd]), 30, tier)


@pytest.mark.parametrize("B", [1, 7, 3000])
def test_batch_sizes(L, torch, B, monkeypatch):
    """The AOT instance (one frame per workgroup) and the global tier (capped grid striding over the frames) on odd batch sizes."""
    H = relift(load_base_matrix(), 64)
    llr = _llr(H, 64, 1.8, 77, B)
    _vs_model(L, torch, H, 64, llr, 50, AOT)
    monkeypatch.setenv("LDPC_HIP_FORCE_GLOBAL", "1")
    _vs_model(L, torch, H, 64, llr, 50, GLOBAL)


def test_decoders_h_surface(L, torch, tmp_path):
    """decod_open(LCHE_DEC) / hd fill / decod_init / lche_decod(st, st->y, st->decword, ...) frame by frame from C++."""
    L.load_library()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = str(tmp_path / "lche_compat_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "lche_compat_driver.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_compat", "-lldpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    for name in ("lche_m64_1p2", "lche_m64_boundary", "lche_rw1_m32_2p5"):
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
            assert np.array_equal(pack_bits(dec), g["hard"])
            assert_bits_equal(after, llr)


def test_ldpc_sim_equals_the_python_host_harness(L, torch, tmp_path):
    """`ldpc_sim simulation examples/simulation_lche.jsonx`: its frame and bit error rates equal ldpc_lib_amd.host's exact-replay
    harness with decoder_type 9 on the same generator seed."""
    from ldpc_lib_amd.host import bp_simulation
    exe = os.path.join(ROOT, "ldpc-lib_amd", "ldpc_sim")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    out = str(tmp_path / "result.jsonx")
    subprocess.check_call([exe, "simulation", os.path.join(ROOT, "examples", "simulation_lche.jsonx"), out])

    def get(path):
        return subprocess.check_output([exe, "jsonx-get", out, path], text=True).strip()

    def numbers(path):
        return [float(x) for x in get(path).replace("array {", "").replace("}", "").split()]
    assert int(get("results/0/_decoder_type")) == LCHE_DEC
    fer, ber = numbers("results/0/simulation_logs/0/FER"), numbers("results/0/simulation_logs/0/BER")
    H = relift(load_base_matrix(), 64)
    b, f, st = bp_simulation(H, 64, 50, 1000000, 3000, 1.2, 1.0, decoder_type=LCHE_DEC, exact_seed=1, return_state=True)
    assert st["experiment"] == 3001
    assert st["nde"] > 0
    assert fer[0] == f and ber[0] == b


def _compat(L):
    L.load_library()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    lib = C.CDLL(os.path.join(ROOT, "ldpc-lib_amd", "libldpc_compat.so"))
    lib.ldpc_bp_simulation_exact_perm.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_void_p, C.c_void_p]
    return lib


@pytest.mark.parametrize("punct", [0, 2])
def test_exact_replay_noise_on_the_device_equals_the_host(L, torch, monkeypatch, punct):
    """ldpc::bp_simulation_t with LDPC_HIP_EXACT_NOISE=device and =host: the same counters, BER / FER doubles and next generator word."""
    lib = _compat(L)
    H = np.ascontiguousarray(relift(load_base_matrix(), 64), dtype=np.int32)
    got = []
    for noise in ("device", "host"):
        monkeypatch.setenv("LDPC_HIP_EXACT_NOISE", noise)
        out = (C.c_double * 7)()
        nxt = C.c_uint()
        assert lib.ldpc_bp_simulation_exact_perm(16, 32, H.ctypes.data, 64, 50, 10**9, 600, 1.3, 1.0, LCHE_DEC, 0, 0, 128, 1, punct, 5, 0,
                                                 C.addressof(out), C.addressof(nxt)) == 0
        got.append((tuple(out), nxt.value))
    assert got[0] == got[1]
    assert got[0][0][3] > 0   # some frames failed: the comparison covers errors


def test_punctured_blocks_are_filled_with_zero(L, torch):
    """Upstream's out_type 1 (bp_simulation.cpp:451-466, :700): punctured positions hold 0.0, and the decoder sees them as such."""
    H = relift(load_base_matrix(), 64)
    with L.LdpcHip(LCHE_DEC, H, 64) as dec:
        assert dec.kernel_name == AOT
        llr = dec.channel_llr(2.5, 9, 100, 16, punctured_blocks=2).cpu().numpy()
        assert (llr[:, 2048 - 128:] == 0.0).all() and not (np.signbit(llr[:, 2048 - 128:])).any()
        assert (llr[:, :2048 - 128] != 0.0).all()
    _vs_model(L, torch, H, 64, llr, 50, AOT)


def test_logical_shards_give_identical_results(L, torch):
    """n = 1, 2, 3 shards mapped to device 0: the same counters and per-frame records as one context's ldpc_hip_simulate."""
    H = relift(load_base_matrix(), 64)
    snr, seed, first, B = 1.2, 31, 5000, 2000
    with L.LdpcHip(LCHE_DEC, H, 64) as dec:
        assert dec.kernel_name == AOT
        want = dec.simulate(snr, 50, seed, first, B)
        llr = dec.channel_llr(snr, seed, first, B)
        hard, iters, _ = dec.decode(llr, 50)
        _, info = dec.count_errors(hard, iters, want_frame_info=True, first_frame=first)
        want_info, want_it = info.cpu().numpy(), iters.cpu().numpy()
    assert want["nde"] > 0
    for n, batch in ((1, 1000), (2, 700), (3, 333)):
        with L.LdpcHipMulti(LCHE_DEC, H, 64, [0] * n) as m:
            got = m.simulate(snr, 50, seed, first, B, batch, records=True)
            for k in want:
                assert got[k] == want[k], (n, batch, k)
            assert np.array_equal(got["frame_info"], want_info) and np.array_equal(got["iters"], want_it)
