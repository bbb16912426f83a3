"""GPU: the min-sum normalisation factor alpha on every kernel of the single-code path.

alpha is an argument of every decode entry and upstream takes whatever the caller passes (decoders.cpp:4674, :4719-4720; integer
min-sum: ialpha = (int)(alpha * 16), :5458).  The other test files decode at upstream's MS_ALPHA = 0.8 only.  Here every min-sum
kernel a single code can land on -- the code-specialised bodies (ahead of time and hiprtc), the table-driven kernels, the
shape-unlimited tier -- decodes one batch at the factors of ldpc_testlib.MS_ALPHAS and is compared with the CPU oracle bit for bit:
hard words, return values, soft values.  tests/test_oracle_vs_ref.py and the ms_*_a* goldens pin the oracle to the compiled upstream
code at these factors.

What can go wrong, and what the factors aim at: a body that carries c2v values across iterations and takes them out as
keep * |alpha| (ms_m64_body), bodies that form |m * alpha| and put the sign on afterwards (every body of ldpc_spec.hpp,
ms_flood_m64_kernel), a separate instance without soft values, products that are denormal (1e-310) or zero (0.0), messages that
grow into the 32767 clamp on their own (1.25, 2.0), and a sign bit on alpha itself (-0.0, -0.8): upstream's product keeps it, so
the message flips.  And upstream's y + acc * alpha is -0.0 where y is and the product is too: with a negative factor where acc is
+0.0, with a zero factor wherever acc < 0.  The kernels that take |m * alpha| cannot give the first, the kernels that start from
y + 0.0 (all but ms_global_kernel: their sign-bit arithmetic needs the canonical zero) cannot give the second.  So
ldpc_hip_decode_dev sends a launch whose alpha is not above zero to ms_global_kernel, upstream's arithmetic as written
(DESIGN.md 4.1), and last_launch has to name it: the rows of -0.8, -0.0 and 0.0 hold every context to that.  NaN is refused.

No case can pass by ignoring alpha: per code and factor the oracle has converged and failed frames and its soft values differ from
those at 0.8 (the CPU tests at the top, over the same inputs)."""
import numpy as np
import pytest

from ldpc_testlib import (IMS_ALPHAS, IMS_DEC, LMS_DEC, MS_ALPHAS, MS_DEC, TASP_DEC, Oracle, alpha_sweep_llr, assert_bits_equal, load_base_matrix,
                          pack_bits, random_qc_code, relift)
from test_gpu_ms_m64_carry import _all_rows_kept, _twenty_rows
from test_gpu_ms_m64_eqslot import AOT_NAME, _record_rows_last
from test_gpu_ms_m64_local import local_columns

gpu = pytest.mark.gpu   # the tests that decode; the ones that look at the oracle alone run anywhere

MAXITER = 30
JIT0 = {"LDPC_HIP_JIT": "0"}
GLOBAL = {"LDPC_HIP_FORCE_GLOBAL": "1"}


def _random(seed, rh, nh, M, weights):
    return lambda: random_qc_code(np.random.RandomState(seed), rh, nh, M, weights)


# name -> (matrix, lifting).  Small codes, but for the example code and two shapes that ms_m64_body treats in its own ways.
CODES = {
    "example_m64": (lambda: relift(load_base_matrix(), 64), 64),
    "example_m126": (lambda: relift(load_base_matrix(), 126), 126),
    "local_columns_20x40_m64": (_twenty_rows, 64),          # shift-0 columns that bypass LDS, 20 block rows, rows up to 12 wide
    "wide_rows_14x28_m64": (_record_rows_last, 64),         # rows up to 13 wide, carried rows and rows that keep their record
    "dual_diagonal_4x8_m64": (_all_rows_kept, 64),
    "m24_4x8": (_random(2401, 4, 8, 24, [2, 3]), 24),       # two frames per wave
    "m1_8x16": (_random(101, 8, 16, 1, [3, 2, 3]), 1),      # 64 frames per wave
    "m100_4x8": (_random(10001, 4, 8, 100, [2, 3]), 100),
    "m200_4x8": (_random(20001, 4, 8, 200, [2, 3]), 200),
    "m33_3x9": (_random(3301, 3, 9, 33, [2, 3, 2]), 33),
}

# (id, code, environment at open, what kernel_name holds, has an instance without soft values)
MS_CASES = [
    ("flagship ahead of time", "example_m64", {}, (AOT_NAME,), True),
    ("ms_chunk ahead of time", "example_m126", {}, ("ms_chunk_appendix_c_m126_kernel (ahead of time)",), False),
    ("ms_m64_body hiprtc, local columns", "local_columns_20x40_m64", {}, ("ms_m64_body", "hiprtc"), True),
    ("ms_m64_body hiprtc, wide rows", "wide_rows_14x28_m64", {}, ("ms_m64_body", "hiprtc"), True),
    ("ms_small_body M=24", "m24_4x8", {}, ("ms_small_body", "hiprtc"), False),
    ("ms_small_body M=1", "m1_8x16", {}, ("ms_small_body", "hiprtc"), False),
    ("ms_chunk_body M=100", "m100_4x8", {}, ("ms_chunk_body", "hiprtc"), False),
    ("ms_body M=200", "m200_4x8", {}, ("ms_body", "hiprtc"), False),
    ("ms_flood_m64_kernel<atomic>", "dual_diagonal_4x8_m64", JIT0, ("ms_flood_m64_kernel<atomic>",), False),
    ("ms_flood_m64_kernel<rmw>", "dual_diagonal_4x8_m64", dict(JIT0, LDPC_HIP_MS_VARIANT="1"), ("ms_flood_m64_kernel<rmw>",), False),
    ("ms_flood_kernel M=24", "m24_4x8", JIT0, ("ms_flood_kernel",), False),
    ("ms_flood_kernel<multiwave> M=200", "m200_4x8", JIT0, ("ms_flood_kernel<multiwave>",), False),
    ("ms_global_kernel M=64", "dual_diagonal_4x8_m64", GLOBAL, ("ms_global_kernel",), False),
    ("ms_global_kernel M=33", "m33_3x9", GLOBAL, ("ms_global_kernel",), False),
]
MS_CODES = sorted({c[1] for c in MS_CASES})

# (id, code, environment, what kernel_name holds, last_launch when ialpha is beyond [0, 16]: int8 messages do not hold it)
IMS_CASES = [
    ("ims_spec ahead of time M=64", "example_m64", {}, ("ims_spec_appendix_c_m64_kernel (ahead of time)",), "ims_flood_kernel"),
    ("ims_small_body M=24", "m24_4x8", {}, ("ims_small_body", "hiprtc"), "ims_flood_kernel"),
    ("ims_flood_kernel M=64", "dual_diagonal_4x8_m64", JIT0, ("ims_flood_kernel",), "ims_flood_kernel"),
    ("ims_flood_kernel M=24", "m24_4x8", JIT0, ("ims_flood_kernel",), "ims_flood_kernel"),
    ("ims_global_kernel M=64", "dual_diagonal_4x8_m64", GLOBAL, ("ims_global_kernel",), "ims_global_kernel"),
    ("ims_global_kernel M=24", "m24_4x8", GLOBAL, ("ims_global_kernel",), "ims_global_kernel"),
]
IMS_CODES = sorted({c[1] for c in IMS_CASES})

_LLR, _REF = {}, {}


def code(name):
    make, M = CODES[name]
    return np.asarray(make(), dtype=np.int16), M


def inputs(name):
    """25 frames: four each at 1.4, 3, 4.5, 6, 8 and 15 dB, the planted values, the frame of ties (ldpc_testlib.alpha_sweep_llr)"""
    if name not in _LLR:
        H, M = code(name)
        llr = alpha_sweep_llr(H, M, seed=sorted(CODES).index(name))
        llr.setflags(write=False)
        _LLR[name] = llr
    return _LLR[name]


def reference(name, dec_id, alpha, maxiter=MAXITER):
    """(packed hard words, return values, soft values) of the CPU oracle, computed once and left unchanged"""
    key = (name, dec_id, repr(float(alpha)), maxiter)
    if key not in _REF:
        H, M = code(name)
        llr = inputs(name)
        d, it, _ = Oracle(H, M).decode(dec_id, llr, maxiter, 0, alpha=alpha)
        s, it1, after = Oracle(H, M).decode(dec_id, llr, maxiter, 1, alpha=alpha)
        assert np.array_equal(it, it1) and (dec_id == TASP_DEC or np.array_equal(after, llr))   # min-sum leaves its input alone
        out = (pack_bits(d), it, s)
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _ids(seq):
    return [repr(float(a)) for a in seq]


# ---- the oracle alone: the cases below cannot pass by ignoring alpha ----------------------------------------------------------------
def test_the_codes_are_what_the_cases_need():
    H, _ = code("local_columns_20x40_m64")
    assert H.shape[0] > 15 and len(local_columns(H)) > 0
    H, _ = code("wide_rows_14x28_m64")
    assert (H >= 0).sum(axis=1).max() > 8
    for name in ("m24_4x8", "m1_8x16", "m100_4x8", "m200_4x8", "dual_diagonal_4x8_m64"):   # what ims_small_body and ms_flood_m64_kernel take
        H, _ = code(name)
        assert (H >= 0).sum(axis=1).max() <= 8 and ((H >= 0).sum(axis=0) >= 1).all(), name
    assert inputs("example_m64").shape == (25, 2048)
    tie = inputs("example_m64")[24]
    assert (np.abs(tie) == 1.0).all() and (tie < 0).any()


@pytest.mark.parametrize("alpha", MS_ALPHAS, ids=_ids(MS_ALPHAS))
@pytest.mark.parametrize("name", MS_CODES)
def test_min_sum_oracle_has_both_outcomes_and_alpha_matters(name, alpha):
    hard, it, soft = reference(name, MS_DEC, alpha)
    assert (it > 0).any() and (it < 0).any(), it
    if abs(alpha) < 1e-300:   # a zero or denormal factor: the soft values stay the channel's, only what arrives as a codeword returns 1
        assert set(it[it > 0].tolist()) == {1}, it
    assert not np.array_equal(soft, reference(name, MS_DEC, 0.8)[2]), "alpha must matter"
    it1 = reference(name, MS_DEC, alpha, maxiter=1)[1] if name == "example_m64" else None
    assert it1 is None or ((it1 == 1).any() and (it1 == -1).any())


@pytest.mark.parametrize("alpha", IMS_ALPHAS, ids=_ids(IMS_ALPHAS))
@pytest.mark.parametrize("name", IMS_CODES)
def test_integer_min_sum_oracle_has_both_outcomes_and_alpha_matters(name, alpha):
    hard, it, soft = reference(name, IMS_DEC, alpha)
    assert (it > 0).any() and (it < 0).any(), it
    assert not np.array_equal(soft, reference(name, IMS_DEC, 0.8)[2]), "alpha must matter"   # ialpha 12


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
def _open(dec_id, name, env, holds, tmp_path, monkeypatch):
    import ldpc_lib_amd
    monkeypatch.setenv("LDPC_HIP_CACHE_DIR", str(tmp_path))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    H, M = code(name)
    dec = ldpc_lib_amd.LdpcHip(dec_id, H, M)
    assert all(h in dec.kernel_name for h in holds), dec.kernel_name
    if "ms_flood_kernel" in holds or "ims_flood_kernel" in holds:
        assert "multiwave" not in dec.kernel_name, dec.kernel_name
    return dec


def _expect(dec, torch, name, dec_id, alpha, maxiter, want_soft, launch, without_soft=None):
    hard_ref, it_ref, soft_ref = reference(name, dec_id, alpha, maxiter)
    x = torch.from_numpy(np.array(inputs(name))).cuda()   # (a copy: the shared inputs are read-only)
    hard, iters, soft = dec.decode(x, maxiter, alpha=alpha, want_soft=want_soft)
    torch.cuda.synchronize()
    what = f"{name}, alpha {alpha!r}, maxiter {maxiter}, {'with' if want_soft else 'without'} soft values"
    assert dec.last_launch() == launch, (what, dec.last_launch())
    if without_soft is not None:
        assert dec.lib.ldpc_hip_last_launch_without_soft(dec.h) == without_soft, what
    assert np.array_equal(iters.cpu().numpy(), it_ref), (what, iters.cpu().numpy(), it_ref)
    assert np.array_equal(hard.cpu().numpy().view(np.uint32), hard_ref), what
    if want_soft:
        assert_bits_equal(soft.cpu().numpy(), soft_ref, "soft values, " + what)


@gpu
@pytest.mark.parametrize("alpha", MS_ALPHAS, ids=_ids(MS_ALPHAS))
@pytest.mark.parametrize("case", MS_CASES, ids=[c[0] for c in MS_CASES])
def test_min_sum_kernels_equal_the_oracle(case, alpha, tmp_path, monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _, name, env, holds, has_hard = case
    with _open(MS_DEC, name, env, holds, tmp_path, monkeypatch) as dec:
        moved = not alpha > 0   # ldpc_hip_decode_dev: only ms_global_kernel gives upstream's bits then
        launch = "ms_global_kernel" if moved else dec.kernel_name
        _expect(dec, torch, name, MS_DEC, alpha, MAXITER, True, launch, 0 if has_hard else None)
        if has_hard:   # the instance that holds no soft values; a launch that left the body has none
            _expect(dec, torch, name, MS_DEC, alpha, MAXITER, False, launch, 0 if moved else 1)
        _expect(dec, torch, name, MS_DEC, 0.8, MAXITER, True, dec.kernel_name)   # and back: the route is per launch


@gpu
@pytest.mark.parametrize("alpha", MS_ALPHAS, ids=_ids(MS_ALPHAS))
def test_flagship_at_one_iteration(alpha, tmp_path, monkeypatch):
    """maxiter 1: the soft values are the channel's, whatever the factor; the frames that arrive as codewords return 1"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    with _open(MS_DEC, "example_m64", {}, (AOT_NAME,), tmp_path, monkeypatch) as dec:
        moved = not alpha > 0
        launch = "ms_global_kernel" if moved else AOT_NAME
        _expect(dec, torch, "example_m64", MS_DEC, alpha, 1, True, launch, 0)
        _expect(dec, torch, "example_m64", MS_DEC, alpha, 1, False, launch, 0 if moved else 1)


@gpu
@pytest.mark.parametrize("alpha", IMS_ALPHAS, ids=_ids(IMS_ALPHAS))
@pytest.mark.parametrize("case", IMS_CASES, ids=[c[0] for c in IMS_CASES])
def test_integer_min_sum_kernels_equal_the_oracle(case, alpha, tmp_path, monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _, name, env, holds, beyond_int8 = case
    ialpha = int(alpha * 16)
    assert ialpha == {0.5: 8, 0.99: 15, 1.0: 16, 0.03: 0, 1.25: 20, -0.8: -12}[alpha]
    with _open(IMS_DEC, name, env, holds, tmp_path, monkeypatch) as dec:
        _expect(dec, torch, name, IMS_DEC, alpha, MAXITER, True, dec.kernel_name if 0 <= ialpha <= 16 else beyond_int8)


@gpu
@pytest.mark.parametrize("dec_id,name,env,holds", [
    (LMS_DEC, "example_m64", {}, ("lms_spec_appendix_c_m64_kernel (ahead of time)",)),
    (LMS_DEC, "dual_diagonal_4x8_m64", JIT0, ("lms_layered_kernel",)),
    (LMS_DEC, "dual_diagonal_4x8_m64", GLOBAL, ("lms_global_kernel",)),
    (TASP_DEC, "example_m64", {}, ("tasp_spec_appendix_c_m64_kernel (ahead of time)",)),
], ids=["lms_spec", "lms_layered_kernel", "lms_global_kernel", "tasp_spec"])
def test_alpha_is_dead_in_the_layered_decoders(dec_id, name, env, holds, tmp_path, monkeypatch):
    """lmin_sum_decod_qc_lm overwrites its alpha and beta arguments (decoders.cpp:5159-5169) and the TDMP decoder has none: whatever
    the caller passes, NaN included, the bits are those of 0.8."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    maxiter = 15 if dec_id == TASP_DEC else MAXITER
    hard_ref, it_ref, soft_ref = reference(name, dec_id, 0.8, maxiter)
    assert (it_ref > 0).any() and (it_ref < 0).any(), it_ref
    x = torch.from_numpy(np.array(inputs(name))).cuda()
    with _open(dec_id, name, env, holds, tmp_path, monkeypatch) as dec:
        base = None
        for alpha in (0.8, 0.123, -3.0, float("nan")):
            hard, iters, soft = dec.decode(x, maxiter, alpha=alpha, want_soft=True)
            torch.cuda.synchronize()
            assert dec.last_launch() == dec.kernel_name
            assert np.array_equal(iters.cpu().numpy(), it_ref), (alpha, iters.cpu().numpy(), it_ref)
            assert np.array_equal(hard.cpu().numpy().view(np.uint32), hard_ref), alpha
            if dec_id == LMS_DEC:
                assert_bits_equal(soft.cpu().numpy(), soft_ref, f"soft values, alpha {alpha!r}")
            base = soft.cpu().numpy() if base is None else base   # TDMP: the posteriors against those of the first launch
            assert_bits_equal(soft.cpu().numpy(), base, f"soft values against alpha 0.8, alpha {alpha!r}")


@gpu
@pytest.mark.parametrize("case", [MS_CASES[0], MS_CASES[3], MS_CASES[8], MS_CASES[10], MS_CASES[12]], ids=lambda c: c[0])
def test_nan_alpha_is_refused(case, tmp_path, monkeypatch):
    """Every value min-sum forms from a NaN factor is a NaN, and the GPU's default NaN is not the host's: upstream's bits cannot be
    given, so the call is refused -- on every tier, before anything is launched -- and the context decodes as before afterwards."""
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _, name, env, holds, _ = case
    x = torch.from_numpy(np.array(inputs(name))).cuda()
    with _open(MS_DEC, name, env, holds, tmp_path, monkeypatch) as dec:
        for entry in ("decode", "decode_host"):
            with pytest.raises(ldpc_lib_amd.LdpcHipError, match="alpha is NaN"):
                if entry == "decode":
                    dec.decode(x, MAXITER, alpha=float("nan"))
                else:
                    dec.decode_host(inputs(name), MAXITER, alpha=float("nan"))
        _expect(dec, torch, name, MS_DEC, 1.0, MAXITER, True, dec.kernel_name)
    if case is MS_CASES[0]:
        with ldpc_lib_amd.LdpcHip(IMS_DEC, *code(name)) as dec:   # (int)(NaN * 16) is undefined in C
            with pytest.raises(ldpc_lib_amd.LdpcHipError, match="alpha is NaN"):
                dec.decode(x, MAXITER, alpha=float("nan"))


# ---- the host entries: alpha reaches the kernel ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("alpha", [1.25, -0.8], ids=_ids([1.25, -0.8]))
def test_decode_host_passes_alpha_on(alpha):
    import ldpc_lib_amd
    name = "example_m64"
    hard_ref, it_ref, soft_ref = reference(name, MS_DEC, alpha)
    with ldpc_lib_amd.LdpcHip(MS_DEC, *code(name)) as dec:
        assert dec.kernel_name == AOT_NAME
        d0, it0, after = dec.decode_host(inputs(name), MAXITER, decision=0, alpha=alpha)
        assert dec.last_launch() == ("ms_global_kernel" if alpha < 0 else AOT_NAME)
        d1, it1, _ = dec.decode_host(inputs(name), MAXITER, decision=1, alpha=alpha)
    assert np.array_equal(it0, it_ref) and np.array_equal(it1, it_ref), (it0, it1, it_ref)
    assert np.array_equal(pack_bits(d0), hard_ref)
    assert_bits_equal(d1, soft_ref, "soft values")
    assert_bits_equal(after, inputs(name), "the input stays as it was")


@gpu
@pytest.mark.parametrize("alpha", [0.5, -0.8], ids=_ids([0.5, -0.8]))
def test_simulate_passes_alpha_on(alpha):
    """simulate = channel + decode + count with the caller's alpha: its four counters equal those recomputed from the same frames, and
    the return values of those frames are the oracle's."""
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H, M = code("example_m64")
    snr, seed, first, B = 4.5, 31, 1000, 96
    with ldpc_lib_amd.LdpcHip(MS_DEC, H, M) as dec:
        got = dec.simulate(snr, MAXITER, seed, first, B, alpha=alpha)
        assert dec.last_launch() == ("ms_global_kernel" if alpha < 0 else AOT_NAME)
        llr = dec.awgn_llr(snr, seed, first, B)
        hard, iters, _ = dec.decode(llr, MAXITER, alpha=alpha)
        cnt, _ = dec.count_errors(hard, iters, first_frame=first)
        hard8, iters8, _ = dec.decode(llr, MAXITER, alpha=0.8)
        cnt8, _ = dec.count_errors(hard8, iters8, first_frame=first)
        torch.cuda.synchronize()
    cnt, cnt8 = cnt.cpu().numpy().tolist(), cnt8.cpu().numpy().tolist()
    assert [got["nse"], got["nde"], got["nue"], got["frames"], got["sum_abs_iters"]] == cnt, (got, cnt)
    assert cnt[3] == B and 0 < cnt[1] and (alpha < 0 or cnt[1] < B), cnt   # failing frames; at a positive factor converging ones too
    assert cnt != cnt8, "alpha must matter"
    _, it_ref, _ = Oracle(H, M).decode(MS_DEC, llr.cpu().numpy(), MAXITER, 0, alpha=alpha)
    assert np.array_equal(iters.cpu().numpy(), it_ref)
