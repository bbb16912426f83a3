"""The GF(q) transmit chain without a GPU: the numpy encoder model (tests/gfq_chain_model.py) against the compiled upstream
encode_NBQCLDPC where oracle/_ref exists; the golden sets (tests/golden/gfq_chain/, tools/make_gfq_chain_goldens.py) reproduced from
the models; left2right through the C-ABI; the additive C-ABI; the plain-C example."""
import ctypes as C
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gfq_chain_model as cm
from gfq_chain_ref import EncoderReference, chain_ref_available, ref_left2right
from gfq_model import GfqModel
from ldpc_testlib import ROOT, assert_bits_equal

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_gfq_chain_goldens as maker  # noqa: E402

NEW_SYMBOLS = ("ldpc_hip_gfq_left2right", "ldpc_hip_gfq_k", "ldpc_hip_gfq_sigma", "ldpc_hip_encode_gfq_dev", "ldpc_hip_encode_gfq_host",
               "ldpc_hip_gfq_channel_dev", "ldpc_hip_count_errors_gfq_dev", "ldpc_hip_simulate_gfq")


def _golden(name):
    return np.load(os.path.join(cm.CHAIN_GOLDEN_DIR, name + ".npz"))


def _lib():
    import ldpc_lib_amd
    return ldpc_lib_amd.load_library()


def test_golden_sets_exist_and_are_small_data():
    names = {os.path.basename(p)[:-4] for p in glob.glob(os.path.join(cm.CHAIN_GOLDEN_DIR, "*.npz"))}
    want = {"chain_enc_" + n for n in maker.ENC_SETS} | {"chain_channel_" + t for t in ("gf4", "gf16", "gf64", "overflow")} | {"chain_sim_gf16_m8"}
    assert names == want
    biggest = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "gfq", "*.npz")))
    for n in names:
        assert os.path.getsize(os.path.join(cm.CHAIN_GOLDEN_DIR, n + ".npz")) <= biggest, n


@pytest.mark.parametrize("name", sorted(maker.ENC_SETS))
def test_encoder_goldens_reproduce_from_the_model(name):
    g = _golden("chain_enc_" + name)
    q_bits, M, hb, hc, n2c, msg = maker.enc_code(name)
    for key, v in (("hb", hb), ("hc", hc), ("msg", msg)):
        assert np.array_equal(g[key], v), key
    hc_after = GfqModel(q_bits, hb, hc, M, n2c).hc_after
    cw, ok = cm.encode(q_bits, hb, hc_after, M, msg)
    assert np.array_equal(cw, g["codeword"]) and np.array_equal(ok, g["ok"])
    broken = maker.ENC_SETS[name][6]
    assert bool(ok.all()) != broken and not cw[0].any()
    assert np.array_equal(cm.syndrome(q_bits, hb, hc_after, M, cw).any(axis=1), ok == 0)


@pytest.mark.parametrize("tag", ["gf4", "gf16", "gf64", "overflow"])
def test_channel_goldens_reproduce_from_the_model(tag):
    g = _golden("chain_channel_" + tag)
    soft = cm.channel(int(g["q_bits"]), g["codeword"], g["noise"], float(g["sigma"]))
    assert_bits_equal(soft, g["soft"], tag, nan_ok=True)
    assert bool(np.isnan(soft).any()) == (tag == "overflow")
    if tag != "overflow":
        assert float(g["sigma"]) == cm.sigma_of(4, 8, 2.7)


def test_chain_golden_decodes_to_the_transmitted_words():
    g = _golden("chain_sim_gf16_m8")
    q_bits, M = int(g["q_bits"]), int(g["M"])
    cw, ok = cm.encode(q_bits, g["hb"], g["hc"], M, g["msg"])
    assert ok.all() and np.array_equal(cw, g["codeword"])
    rh, nh = g["hb"].shape
    soft = cm.channel(q_bits, cw, g["noise"], cm.sigma_of(rh, nh, float(g["snr"])))
    iters, qhard, _ = GfqModel(q_bits, g["hb"], g["hc"], M).decode(soft, int(g["maxiter"]))
    assert np.array_equal(qhard, cw) and int(np.abs(iters).sum()) == int(g["iters_sum"])
    cnt, info = cm.count(qhard, cw, iters, rh * M)
    assert cnt == [0, 0, 0, 32, int(g["iters_sum"])] and not info.any()


@pytest.mark.skipif(not chain_ref_available(), reason="oracle/_ref (the compiled upstream reference) is absent")
def test_encoder_model_equals_the_compiled_reference(capfd):
    rng = np.random.RandomState(77)
    for q_bits, M, rh, nh in ((2, 1, 2, 4), (4, 8, 3, 6), (6, 67, 4, 8), (8, 5, 4, 8), (10, 3, 3, 6)):
        for scheme in cm.SCHEMES:
            if scheme != "w2" and rh < 3:
                continue
            for brk in (False, True):
                hb, hc = cm.make_code(rng, q_bits, rh, nh, M, scheme, brk)
                msg = rng.randint(0, 1 << q_bits, (6, (nh - rh) * M))
                ref = EncoderReference(q_bits, hb, hc, M)
                cw_r, ok_r = ref.encode(msg)
                ref.close()
                cw, ok = cm.encode(q_bits, hb, hc, M, msg)
                assert np.array_equal(cw, cw_r) and np.array_equal(ok, ok_r), (q_bits, M, rh, nh, scheme, brk)
    for shape in ((2, 2), (2, 5), (4, 8)):
        m = rng.randint(-1, 50, shape)
        assert np.array_equal(ref_left2right(m), cm.left2right(m))


@pytest.mark.parametrize("shape", [(2, 2), (2, 5), (4, 8)])
def test_left2right_through_the_c_abi(shape):
    import ldpc_lib_amd
    m = np.arange(shape[0] * shape[1], dtype=np.int16).reshape(shape) - 1
    out = ldpc_lib_amd.gfq_left2right(m)
    assert np.array_equal(out, cm.left2right(m)) and m[0, 0] == -1   # a copy: the argument is untouched
    lib = _lib()
    buf = np.zeros(8, dtype=np.int16)
    assert lib.ldpc_hip_gfq_left2right(buf.ctypes.data, 3, 2) == -1      # nh < rh
    assert lib.ldpc_hip_gfq_left2right(buf.ctypes.data, 0, 2) == -1
    assert lib.ldpc_hip_gfq_left2right(None, 2, 4) == -1


def test_header_declares_and_library_exports_the_new_entries():
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        header = f.read()
    lib = _lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|double)\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+LDPC_HIP_ABI_VERSION\s+4\b", header)
    assert lib.ldpc_hip_abi_version() == 4
    # binary contexts and null contexts answer the scalar queries with 0
    assert lib.ldpc_hip_gfq_k(None) == 0 and lib.ldpc_hip_gfq_sigma(None, 1.0) == 0.0


def test_gfq_c_example_builds_against_the_header(tmp_path):
    exe = tmp_path / "simulate_gfq"
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "simulate_gfq.c"),
                           "-o", str(exe), "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    assert exe.exists()
    # the example's matrix is one the encoder accepts (checked with the model: no GPU here)
    src = open(os.path.join(ROOT, "examples", "simulate_gfq.c")).read()
    rows = re.findall(r"int16_t (h[bc])\[RH \* NH\] = \{(.*?)\};", src, re.S)
    mats = {k: np.array([int(v) for v in re.findall(r"-?\d+", body)]).reshape(3, 6) for k, body in rows}
    hb, hc = cm.left2right(mats["hb"]), cm.left2right(mats["hc"])
    cw, ok = cm.encode(4, hb, hc, 8, np.random.RandomState(3).randint(0, 16, (4, 24)))
    assert ok.all()
    GfqModel(4, hb, hc, 8)   # and one the decoder opens
