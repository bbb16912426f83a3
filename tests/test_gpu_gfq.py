"""FHT_DEC (decoder id 6, QC-LDPC codes over GF(q)) on the GPU: every golden set of the compiled reference through
ldpc_hip_decode_gfq_dev and _host, tolerance 0 (return values, qhard, and the a-posteriori vectors as uint64 images); fresh frames
against the numpy restatement (tests/gfq_model.py) on further shapes; independence of batch split, frame order and frames in flight;
the q = 16 / q = 64 instances against the generic kernel; refusals; the binary entry points on a GF(q) context.

The one thing not compared is the sign / payload of a NaN, in the boundary set only (ldpc_testlib.assert_bits_equal, nan_ok: x86's
default NaN has the sign bit set, the GPU's does not); NaN positions must match exactly."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest

from gfq_model import GFQ_GOLDEN_DIR, GfqModel, bpsk_symbol_probabilities
from ldpc_testlib import MS_DEC, ROOT, assert_bits_equal

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_gfq_goldens  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GFQ_GOLDEN_DIR, "*.npz")))
EINVAL, EUNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _kernel(q, generic=False):
    if q == 16 and not generic:
        return "gfq_kernel<q=16,16x1>"
    if q == 64 and not generic:
        return "gfq_kernel<q=64,16x4>"
    ql = 4 if q <= 256 else q // 64
    return f"gfq_kernel<generic,q={q},{ql}x{q // ql}>"


def _dev(torch, dec, soft, maxiter):
    d = torch.from_numpy(soft).cuda()
    qhard, iters, post = dec.decode(d, maxiter, want_post=True)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint64), soft.view(np.uint64)), "the input buffer was modified"
    return iters.cpu().numpy(), qhard.cpu().numpy(), post.cpu().numpy()


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_dev_and_host(L, torch, name):
    g = np.load(os.path.join(GFQ_GOLDEN_DIR, name + ".npz"))
    soft, maxiter, nan_ok = g["soft"], int(g["maxiter"]), name.endswith("boundary")
    assert nan_ok or np.isfinite(g["post"]).all()
    with L.LdpcHipGfq(int(g["q_bits"]), g["hb"], g["hc"], int(g["M"]), int(g["ncols2convert"])) as dec:
        assert dec.kernel_name == _kernel(dec.q), dec.kernel_name
        assert (dec.q, dec.N, dec.R) == (1 << int(g["q_bits"]), g["hb"].shape[1] * int(g["M"]), g["hb"].shape[0] * int(g["M"]))
        assert dec.edges == int((g["hb"] >= 0).sum())
        assert np.array_equal(dec.coefficients(), g["hc_after"])
        iters, qhard, post = _dev(torch, dec, soft, maxiter)
        print(name, "dev: iters equal", np.array_equal(iters, g["iters"]), "qhard differing", int((qhard != g["qhard"]).sum()),
              "post differing bits", int((post.view(np.uint64) != g["post"].view(np.uint64)).sum()))
        assert np.array_equal(iters, g["iters"])
        assert np.array_equal(qhard, g["qhard"])
        assert_bits_equal(post, g["post"], name + " post (dev)", nan_ok=nan_ok)
        keep = soft.copy()
        qh, it, po = dec.decode_host(soft, maxiter)
        assert np.array_equal(it, g["iters"]) and np.array_equal(qh, g["qhard"])
        assert_bits_equal(po, g["post"], name + " post (host)", nan_ok=nan_ok)
        assert np.array_equal(soft.view(np.uint64), keep.view(np.uint64))


SHAPES = [("gf16 shipped M=8", 4, "shipped", 8, 2.4, 300), ("gf16 shipped M=128", 4, "shipped", 128, 1.9, 40),
          ("gf16 6x12 M=100", 4, "6x12", 100, 1.5, 24), ("gf16 mixed M=33", 4, "mixed", 33, 1.6, 120),
          ("gf64 shipped M=8", 6, "shipped", 8, 2.4, 200), ("gf64 mixed M=7", 6, "mixed", 7, 2.8, 200),
          ("gf4 mixed M=70", 2, "mixed", 70, 1.8, 200), ("gf8 mixed M=16", 3, "mixed", 16, 3.0, 200),
          ("gf32 shipped M=20", 5, "shipped", 20, 2.4, 100), ("gf128 mixed M=3", 7, "mixed", 3, 2.8, 60),
          ("gf256 shipped M=2", 8, "shipped", 2, 2.4, 60), ("gf512 mixed M=2", 9, "mixed", 2, 3.0, 24), ("gf1024 shipped M=1", 10, "shipped", 1, 2.5, 16)]


def _code(kind, M, q):
    if kind == "shipped":
        return make_gfq_goldens.shipped(M, q)
    if kind == "mixed":
        return make_gfq_goldens.mixed(M, q, seed=11)
    from ldpc_testlib import random_qc_code
    rng = np.random.RandomState(612)
    hb = np.asarray(random_qc_code(rng, 6, 12, M, [2, 3, 5]), dtype=np.int16)
    return hb, np.where(hb >= 0, rng.randint(1, q, hb.shape), -1).astype(np.int16)


@pytest.mark.parametrize("what,q_bits,kind,M,snr,frames", SHAPES, ids=[s[0] for s in SHAPES])
def test_fresh_frames_equal_the_model(L, torch, what, q_bits, kind, M, snr, frames):
    q = 1 << q_bits
    hb, hc = _code(kind, M, q)
    soft = bpsk_symbol_probabilities(np.random.RandomState(900 + q_bits * 7 + M), q_bits, hb.shape[1] * M, make_gfq_goldens.sigma_of(snr, hb), frames)
    mi, mq, mp = GfqModel(q_bits, hb, hc, M).decode(soft, 15)
    with L.LdpcHipGfq(q_bits, hb, hc, M) as dec:
        assert dec.kernel_name == _kernel(q), dec.kernel_name
        iters, qhard, post = _dev(torch, dec, soft, 15)
    print(what, "converged", int((mi > 0).sum()), "of", frames, "| post differing bits", int((post.view(np.uint64) != mp.view(np.uint64)).sum()))
    assert (mi > 0).any() and (mi < 0).any(), "the batch should hold converged and non-converged frames"
    assert np.array_equal(iters, mi) and np.array_equal(qhard, mq)
    assert_bits_equal(post, mp, what)


def test_batch_larger_than_the_slots_split_and_order(L, torch, monkeypatch):
    """Results do not depend on how many frames are in flight (a batch beyond the workspace's slots is worked off inside the launch),
    on the batch split or on the order of the frames."""
    hb, hc = make_gfq_goldens.shipped(8, 16)
    B = 5000
    soft = bpsk_symbol_probabilities(np.random.RandomState(31), 4, 64, make_gfq_goldens.sigma_of(2.3, hb), B)
    with L.LdpcHipGfq(4, hb, hc, 8) as dec:
        it0, qh0, po0 = _dev(torch, dec, soft, 15)                 # 5000 frames: more than the default slots of any device
        monkeypatch.setenv("LDPC_HIP_GFQ_SLOTS", "7")
        it1, qh1, po1 = _dev(torch, dec, soft[:700], 15)           # 7 slots, 100 frames each
        monkeypatch.delenv("LDPC_HIP_GFQ_SLOTS")
        assert np.array_equal(it1, it0[:700]) and np.array_equal(qh1, qh0[:700])
        assert_bits_equal(po1, po0[:700])
        for lo, hi in ((0, 1), (1, 130), (130, 2000), (2000, 5000)):
            it, qh, po = _dev(torch, dec, np.ascontiguousarray(soft[lo:hi]), 15)
            assert np.array_equal(it, it0[lo:hi]) and np.array_equal(qh, qh0[lo:hi])
            assert_bits_equal(po, po0[lo:hi])
        perm = np.random.RandomState(5).permutation(B)
        it, qh, po = _dev(torch, dec, np.ascontiguousarray(soft[perm]), 15)
        assert np.array_equal(it, it0[perm]) and np.array_equal(qh, qh0[perm])
        assert_bits_equal(po, po0[perm])
        qh, it, po = dec.decode_host(soft[:300], 15)
        assert np.array_equal(it, it0[:300]) and np.array_equal(qh, qh0[:300])
        assert_bits_equal(po, po0[:300])
    sub = slice(0, 200)
    mi, mq, mp = GfqModel(4, hb, hc, 8).decode(soft[sub], 15)
    assert np.array_equal(it0[sub], mi) and np.array_equal(qh0[sub], mq)
    assert_bits_equal(po0[sub], mp)
    assert (it0 > 0).any() and (it0 < 0).any()


@pytest.mark.parametrize("q_bits,kind,M", [(4, "shipped", 8), (4, "mixed", 33), (4, "shipped", 100), (6, "shipped", 8), (6, "mixed", 7)])
def test_specialised_and_generic_kernels_agree(L, torch, monkeypatch, q_bits, kind, M):
    q = 1 << q_bits
    hb, hc = _code(kind, M, q)
    soft = bpsk_symbol_probabilities(np.random.RandomState(77 + M), q_bits, hb.shape[1] * M, make_gfq_goldens.sigma_of(2.5, hb), 64)
    with L.LdpcHipGfq(q_bits, hb, hc, M) as dec:
        assert dec.kernel_name == _kernel(q)
        a = _dev(torch, dec, soft, 15)
    monkeypatch.setenv("LDPC_HIP_GFQ_GENERIC", "1")
    with L.LdpcHipGfq(q_bits, hb, hc, M) as dec:
        assert dec.kernel_name == _kernel(q, generic=True), dec.kernel_name
        b = _dev(torch, dec, soft, 15)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert_bits_equal(a[2], b[2])
    mi, mq, mp = GfqModel(q_bits, hb, hc, M).decode(soft, 15)
    assert np.array_equal(a[0], mi) and np.array_equal(a[1], mq)
    assert_bits_equal(a[2], mp)


def test_outputs_are_optional_and_maxiter_is_respected(L, torch):
    hb, hc = make_gfq_goldens.shipped(8, 16)
    soft = bpsk_symbol_probabilities(np.random.RandomState(3), 4, 64, make_gfq_goldens.sigma_of(2.0, hb), 50)
    m = GfqModel(4, hb, hc, 8)
    with L.LdpcHipGfq(4, hb, hc, 8) as dec:
        for maxiter in (1, 2, 7):
            mi, mq, mp = m.decode(soft, maxiter)
            it, qh, po = _dev(torch, dec, soft, maxiter)
            assert np.array_equal(it, mi) and np.array_equal(qh, mq)
            assert_bits_equal(po, mp)
        d = torch.from_numpy(soft).cuda()
        qh, it, po = dec.decode(d, 7, want_qhard=False, want_post=False)
        torch.cuda.synchronize()
        assert qh is None and po is None and np.array_equal(it.cpu().numpy(), mi)
        assert dec.decode(d[:0].contiguous(), 7)[1].numel() == 0
        dec.profile(True)
        dec.decode(d, 7)
        ms, n = dec.profile_read()
        assert n == 1 and ms > 0


def _open(L, q_bits, hb, hc, M, n2c=0):
    lib = L.load_library()
    hb = np.ascontiguousarray(hb, dtype=np.int16)
    hc = np.ascontiguousarray(hc, dtype=np.int16)
    h = C.c_void_p()
    rc = lib.ldpc_hip_open_gfq(q_bits, hb.shape[0], hb.shape[1], M, hb.ctypes.data, hc.ctypes.data, n2c, 0, C.byref(h))
    return rc, h, lib.ldpc_hip_last_error().decode()


def test_refusals(L, torch):
    lib = L.load_library()
    hb, hc = make_gfq_goldens.shipped(8, 16)
    for q_bits in (1, 0, 11):
        rc, h, msg = _open(L, q_bits, hb, hc, 8)
        assert rc == EUNSUPPORTED and not h.value and "q" in msg, (q_bits, msg)
    one = hb.copy()
    one[1, :] = -1
    one[1, 2] = 3                                                  # block row of weight 1
    rc, h, msg = _open(L, 4, one, np.where(one >= 0, 1, -1), 8)
    assert rc == EUNSUPPORTED and "weight 1" in msg, msg
    wide = np.zeros((2, 1025), dtype=np.int16)                     # row weight 1025
    rc, h, msg = _open(L, 4, wide, np.ones_like(wide), 1)
    assert rc == EUNSUPPORTED and "1024" in msg, msg
    zero = hc.copy()
    zero[0, 0] = 0                                                 # coefficient 0: upstream's tables are undefined
    rc, h, msg = _open(L, 4, hb, zero, 8)
    assert rc == EUNSUPPORTED and "coefficient 0" in msg, msg
    big = hc.copy()
    big[0, 0] = 16
    assert _open(L, 4, hb, big, 8)[0] == EINVAL
    assert _open(L, 4, hb, hc, 8, n2c=9)[0] == EINVAL
    h = C.c_void_p()                                               # decoder id 6 through the binary open: no coefficient matrix
    assert lib.ldpc_hip_open(6, 4, 8, 8, hb.ctypes.data, 0, C.byref(h)) == EUNSUPPORTED and not h.value
    with L.LdpcHipGfq(4, hb, hc, 8) as dec:
        d = torch.zeros((2, 16, 64), dtype=torch.float64, device="cuda")
        with pytest.raises(L.LdpcHipError, match="p_thr"):
            dec.decode(d, 15, p_thr=0.01)
        with pytest.raises(L.LdpcHipError, match="maxiter"):
            dec.decode(d, 0)


def test_binary_entry_points_refuse_a_gfq_context(L, torch):
    lib = L.load_library()
    hb, hc = make_gfq_goldens.shipped(8, 16)
    with L.LdpcHipGfq(4, hb, hc, 8) as dec:
        llr = torch.zeros((4, dec.N), dtype=torch.float64, device="cuda")
        hard = torch.zeros((4, 2), dtype=torch.int32, device="cuda")
        iters = torch.zeros((4,), dtype=torch.int32, device="cuda")
        cnt = torch.zeros((5,), dtype=torch.int64, device="cuda")
        host = np.zeros((4, dec.N))
        state = np.zeros(624, dtype=np.uint32)
        c4 = (C.c_ulonglong * 4)()
        calls = {
            "decode_dev": lambda: lib.ldpc_hip_decode_dev(dec.h, llr.data_ptr(), 4, 10, 0.8, hard.data_ptr(), iters.data_ptr(), None, None),
            "decode_host": lambda: lib.ldpc_hip_decode_host(dec.h, host.ctypes.data, 4, 10, 0, 0.8, host.ctypes.data, None, 0),
            "channel": lambda: lib.ldpc_hip_channel_llr_dev(dec.h, 2.0, 0, 0, 26.0, 1, 0, 4, llr.data_ptr(), None),
            "awgn": lambda: lib.ldpc_hip_awgn_llr_dev(dec.h, 2.0, 0, 0, 1, 0, 4, llr.data_ptr(), None),
            "count": lambda: lib.ldpc_hip_count_errors_dev(dec.h, hard.data_ptr(), iters.data_ptr(), 4, None, cnt.data_ptr(), None),
            "simulate": lambda: lib.ldpc_hip_simulate(dec.h, 2.0, 0, 0, 10, 0.8, 1, 0, 4, c4, None),
            "mt_set_state": lambda: lib.ldpc_hip_mt_set_state(dec.h, state.ctypes.data, 624),
            "mt_frames": lambda: lib.ldpc_hip_mt_frames(dec.h, 2.0, 0, 0, 10, 0.8, 4, iters.data_ptr(), iters.data_ptr()),
        }
        for name, call in calls.items():
            assert call() == EINVAL, name
            assert "GF(q)" in lib.ldpc_hip_last_error().decode(), name
        soft = bpsk_symbol_probabilities(np.random.RandomState(1), 4, 64, make_gfq_goldens.sigma_of(3.0, hb), 4)
        assert np.array_equal(dec.decode_host(soft, 15)[1], GfqModel(4, hb, hc, 8).decode(soft, 15)[0])   # the context is still good
    with L.LdpcHip(MS_DEC, np.where(hb >= 0, hb, -1), 8) as b:     # and the GF(q) entries refuse a binary context
        assert lib.ldpc_hip_gfq_q(b.h) == 0
        assert lib.ldpc_hip_decode_gfq_dev(b.h, None, 1, 10, 0.0, None, None, None, None) == EINVAL
