"""GPU: the device math functions every "bit for bit" claim of the sum-product family rests on, evaluated on the device by a
stand-alone probe (tests/cpp/math_probe.hip, built here with the library's own hipcc flags) and compared on the 64-bit patterns:

  exp_glibc, log_glibc          against the host's libm (ctypes)
  exp_glibc_wide                the same for |x| < 512; beyond, ocml's exp: +inf exactly where glibc overflows, +0 from -746 down,
                                within 2 ulp of glibc on [512, threshold)
  div_ranged                    against IEEE division on each caller's operand domain and on the domain its comment states
  the compiler's a / b, sqrt    against numpy (IEEE) -- special operands, overflowing and underflowing quotients included
  lche::logexp                  against upstream's loop (lche_model.logexp_int), tables in global memory and in LDS
  iasp::prior / q12             against 1 / (1 + exp(clamp(x))) with libm's exp and upstream's rounding

and one decoder case that ties exp_glibc_wide to Gallager BP on LLRs of magnitude 500 .. 745.  Operands, predicates and references
live in tests/device_math_cases.py; tests/test_device_math_cpu.py checks them without a GPU.  The figures each test prints
(operands, mismatches, ulp distances, what came back at div_ranged's poles) are recorded in profiles/r29_device_math.txt."""
import os
import subprocess

import numpy as np
import pytest

import device_math_cases as dm
from lche_model import logexp_int
from ldpc_testlib import BP_DEC, ROOT, Oracle, assert_bits_equal, awgn_llr, load_base_matrix, pack_bits, relift

pytestmark = pytest.mark.gpu

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NOUT = {"exp": 1, "expw": 1, "log": 1, "div": 2, "sqrt": 1, "phi": 1, "phi_lds": 1, "prior": 2}


class Probe:
    """math_probe, one subprocess per call (and per 2^20 operands), one after the other.  After a call that did not exit with 0
    nothing further is started."""

    def __init__(self, exe, tmp):
        self.exe, self.tmp, self.failed, self.calls = str(exe), tmp, None, 0

    def __call__(self, op, *arrays):
        n = arrays[0].size
        outs = [[] for _ in range(NOUT[op])]
        for lo in range(0, n, dm.MAX_OPERANDS):
            if self.failed:
                pytest.fail(f"math_probe not started: an earlier call failed ({self.failed})")
            self.calls += 1
            fin, fout = os.path.join(self.tmp, f"in{self.calls}.bin"), os.path.join(self.tmp, f"out{self.calls}.bin")
            part = [a[lo:lo + dm.MAX_OPERANDS] for a in arrays]
            dm.write_arrays(fin, part)
            try:
                r = subprocess.run([self.exe, op, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
            except subprocess.TimeoutExpired:
                self.failed = f"{op}: no result after 120 s"
                pytest.fail(self.failed)
            if r.returncode != 0:
                self.failed = f"{op}: exit status {r.returncode}: {r.stdout.strip()}"
                pytest.fail(self.failed)
            for o, got in zip(outs, dm.read_arrays(fout, part[0].size, NOUT[op])):
                o.append(got)
            os.remove(fin)
            os.remove(fout)
        return [np.concatenate(o) for o in outs]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    from ldpc_lib_amd.binding import HIPCC_FLAGS          # the library's flags, -ffp-contract=off included: the probe cannot drift from it
    tmp = tmp_path_factory.mktemp("math_probe")
    exe = tmp / "math_probe"
    subprocess.check_call([HIPCC, *HIPCC_FLAGS, os.path.join(ROOT, "tests", "cpp", "math_probe.hip"), "-o", str(exe)])
    return Probe(exe, str(tmp))


def _f(u):
    return dm.from_bits(u)


def _mismatch(got, want, nan_ok=False):
    """indices at which two uint64 images differ (NaN against NaN counts as equal with nan_ok)"""
    bad = got != want
    if nan_ok:
        gn, wn = np.isnan(_f(got)), np.isnan(_f(want))
        bad = (bad & ~(gn & wn)) | (gn != wn)
    return np.flatnonzero(bad)


def _assert_equal(op, x, got, want, nan_ok=False, operands=None):
    bad = _mismatch(got, dm.bits(want), nan_ok)
    print(f"device-math: {op}: {got.size} operands, {bad.size} mismatches")
    if bad.size:
        i = int(bad[0])
        arg = ", ".join(f"{float(a[i])!r} ({float(a[i]).hex()})" for a in (operands or [x]))
        raise AssertionError(f"{op}: {bad.size} of {got.size} values differ; first at operand {arg}: got 0x{int(got[i]):016x} ({_f(got)[i]!r}), "
                             f"want 0x{int(dm.bits(want)[i]):016x} ({np.asarray(want)[i]!r})")


def test_exp_glibc_equals_libm(probe):
    """-512 < x < 709.78: uniform arguments, signed zeros and tiny arguments, +-20 (the callers' clamp), all 257 table index
    boundaries k ln2 / 128 with their neighbours, the largest doubles below 512."""
    x = dm.exp_operands()
    (got,) = probe("exp", x)
    _assert_equal("exp", x, got, dm.libm_exp(x))


def test_exp_glibc_wide_equals_libm_inside_512_and_keeps_its_poles_outside(probe):
    """Inside |x| < 512 the table path, bit for bit.  Outside ocml's exp, of which bp_body needs: +inf exactly where glibc returns
    +inf ((A - 1) / (A + 1) turns from 1 into NaN there), a finite value where glibc's is finite, +0 for every x <= -746.  On
    [512, overflow threshold) ocml (documented 1 ulp) and glibc (below 1 ulp) may differ by 2 ulp at most.  Subnormal results are
    recorded only."""
    x = dm.expw_operands()
    (got,) = probe("expw", x)
    want = dm.libm_exp(x)
    g, w = _f(got), want
    inner = np.abs(x) < 512.0
    mid = (x >= 512.0) & (x < dm.EXP_OVERFLOW)
    low = (x <= -512.0) & (x > -746.0)
    sub = low & (w < np.finfo(np.float64).tiny)
    assert mid.sum() > 100000 and (x >= dm.EXP_OVERFLOW).sum() > 64 and sub.sum() > 64
    d_mid = dm.ulp_distance(g[mid], w[mid]) if np.isfinite(g[mid]).all() else None
    d_low = dm.ulp_distance(g[low], w[low]) if np.isfinite(g[low]).all() else None
    inf_got, inf_want = got == dm.bits(np.inf), np.isinf(w)
    print(f"device-math: expw: {x.size} operands; |x| < 512: {inner.sum()} operands, {_mismatch(got[inner], dm.bits(w[inner])).size} mismatches")
    if d_mid is not None:
        print(f"device-math: expw: [512, threshold): {mid.sum()} operands, {(d_mid != 0).sum()} differ from libm, largest distance {d_mid.max()} ulp")
    if d_low is not None:
        ds = dm.ulp_distance(g[sub], w[sub])
        print(f"device-math: expw: (-746, -512]: {low.sum()} operands, {(d_low != 0).sum()} differ, largest distance {d_low.max()} ulp; "
              f"of these with a subnormal result: {sub.sum()} operands, {(ds != 0).sum()} differ, largest distance {ds.max()} ulp")
    print(f"device-math: expw: +inf at {inf_got.sum()} operands (libm: {inf_want.sum()}); smallest x with +inf: "
          f"{float(x[inf_got].min()).hex() if inf_got.any() else None} (libm: {float(x[inf_want].min()).hex()})")
    _assert_equal("expw, |x| < 512", x[inner], got[inner], w[inner])
    assert not np.isnan(g).any()
    bad = np.flatnonzero(inf_got != inf_want)
    assert bad.size == 0, f"+inf at other arguments than libm's, first x = {float(x[bad[0]]).hex()}: got {g[bad[0]]!r}, libm {w[bad[0]]!r}"
    assert np.isfinite(g[~inf_want]).all()
    assert (got[x <= -746.0] == 0).all() and (x <= -746.0).sum() >= 4, "exp(x) must be +0 for x <= -746"
    assert d_mid.max() <= 2, f"[512, threshold): {d_mid.max()} ulp from libm at x = {float(x[mid][np.argmax(d_mid)]).hex()}"


def test_log_glibc_equals_libm(probe):
    """The CPU test's four families, both ends of the near-1 window with 8 neighbours, 1.0 +- 8 ulp, every power of two from the
    smallest subnormal up, the 128 table-interval boundaries +- 1 ulp (in three binades), and 0, -0, inf, -1, -inf, NaN, DBL_MAX:
    libm's value, and libm's result class (NaN) for negative and NaN arguments."""
    x = dm.log_operands()
    (got,) = probe("log", x)
    _assert_equal("log", x, got, dm.libm_log(x), nan_ok=True)


@pytest.mark.parametrize("name,pairs,inside", dm.DIV_DOMAINS, ids=[d[0] for d in dm.DIV_DOMAINS])
def test_div_ranged_equals_ieee_division_on_its_domains(probe, name, pairs, inside):
    """v_rcp_f64, two Newton steps and the final fma without v_div_scale / v_div_fmas / v_div_fixup: the IEEE quotient on the operand
    domain of each caller (TDMP, ASP, sp_body up to row weight 12, the polar method) and on the domain the comment above div_ranged
    states: 2^18 random pairs each, the domain's corners (exact powers of two, mantissas 1 + ulp and 2 - ulp) and, but for the polar
    method, quotients that miss a rounding boundary by 2^-53 of an ulp (the ones a reciprocal short of one Newton step gets wrong).
    A numerator of -0.0 gives +0.0 (pinned: ldpc_mt.hpp relies on it).  The compiler's own a / b is checked alongside."""
    a, b = pairs()
    assert inside(a, b).all()                                  # before the GPU is touched
    q, qc = probe("div", a, b)
    _assert_equal(f"div_ranged, domain {name}", None, q, dm.div_ranged_expected(a, b), operands=[a, b])
    _assert_equal(f"a / b, domain {name}", None, qc, dm.ieee_div(a, b), operands=[a, b])


def test_div_ranged_zeros_and_poles_and_the_compilers_division_on_special_operands(probe):
    """div_ranged(+0, b) is IEEE's zero (+0 for b > 0), div_ranged(-0, b) is +0 for either sign of b, div_ranged(x, 0) is not finite
    (sp_body's clamp needs no more), div_ranged(0, 0) is NaN.  The compiler's a / b is IEEE's on all of these and on 2^16 pairs with
    denormal, zero, infinite and NaN operands and quotients around the overflow and underflow thresholds."""
    bv = np.array([1e-4, 0.3, 1.0, 2.0, 3.0, 1e7, 2.0 ** -54, 2.0 ** 650, np.nextafter(1.0, 0.0)])
    bv = np.concatenate([bv, -bv])
    xv = np.array([1.0, 1e-6, 0.5, 2.0 ** -650, 2.0 ** 650, 4e-274, 3.0])
    xv = np.concatenate([xv, -xv])
    zero = np.array([0.0, -0.0])
    pa, pb = dm._grid(zero, bv)                                # zeros over finite denominators
    xa, xb = dm._grid(xv, zero)                                # poles
    za, zb = dm._grid(zero, zero)                              # 0 / 0
    sa, sb = dm.div_special_pairs()
    a, b = np.concatenate([pa, xa, za, sa]), np.concatenate([pb, xb, zb, sb])
    q, qc = probe("div", a, b)
    n0, n1, n2 = pa.size, pa.size + xa.size, pa.size + xa.size + za.size
    pole = _f(q[n0:n1])
    kinds = sorted({"NaN" if np.isnan(v) else repr(float(v)) for v in pole})
    print(f"device-math: div_ranged(x, +-0) for x != 0: {pole.size} operands, returned {kinds}; compiler's a / b there: "
          f"{sorted({repr(float(v)) for v in _f(qc[n0:n1])})}")
    print(f"device-math: div_ranged(+-0, +-0): {sorted({'NaN' if np.isnan(v) else repr(float(v)) for v in _f(q[n1:n2])})}")
    _assert_equal("div_ranged(+-0, b)", None, q[:n0], dm.div_ranged_expected(pa, pb), operands=[pa, pb])
    assert (q[:n0][np.signbit(pa)] == 0).all() and (q[:n0][~np.signbit(pa) & (pb > 0)] == 0).all()
    assert not np.isfinite(pole).any(), pole
    assert np.isnan(_f(q[n1:n2])).all()
    _assert_equal("a / b, special operands", None, qc, dm.ieee_div(a, b), nan_ok=True, operands=[a, b])


def test_square_root_is_correctly_rounded(probe):
    """log-uniform positive doubles over the whole range, every power of two, the perfect squares below 2^26 +- 1 ulp, denormals,
    +0, -0 (stays -0), +inf."""
    x = dm.sqrt_operands()
    (got,) = probe("sqrt", x)
    _assert_equal("sqrt", x, got, np.sqrt(x))


def test_phi_lookup_equals_upstreams_loop_from_global_memory_and_from_lds(probe):
    """lche::logexp against logexp_int: every power of two from 2^-1074 to 2^5 +- 1 ulp, the step boundaries 2^-9 32^-k, 1/512, 1/16,
    2, 16, the rounding boundaries of the three tables, +-0, negative arguments, arguments above 16, random arguments."""
    x = dm.phi_operands()
    want = logexp_int(x)
    (g,) = probe("phi", x)
    (l,) = probe("phi_lds", x)
    _assert_equal("phi", x, g, want)
    _assert_equal("phi_lds", x, l, want)
    assert np.array_equal(g, l)


def test_iasp_prior_and_its_quantisation(probe):
    x = dm.prior_operands()
    p, q = probe("prior", x)
    wp, wq = dm.prior_reference(x)
    _assert_equal("prior", x, p, wp)
    bad = np.flatnonzero(q != wq)
    print(f"device-math: q12(prior): {q.size} operands, {bad.size} mismatches")
    assert bad.size == 0, (float(x[bad[0]]).hex(), int(q[bad[0]]), int(wq[bad[0]]))


@pytest.mark.parametrize("tier", ["hiprtc", "_global_kernel"])
def test_gallager_bp_on_llrs_around_the_thresholds_of_exp(probe, tier, monkeypatch):
    """exp_glibc_wide inside a decoder: the 16 x 32 base code at lifting 9, 16 AWGN frames at 2 dB with 8 positions per frame
    overwritten by LLRs of magnitude 500, 511.9, 512, 600, 709, 709.8, 710 and 745 (signs alternating) -- arguments on both sides
    of the switch at 512 and of exp's overflow threshold.  Hard bits, return values and soft values equal the oracle's; where the
    oracle's soft value is NaN the device's is NaN."""
    import torch
    import ldpc_lib_amd as L
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert not probe.failed, f"not started: the probe failed on this GPU ({probe.failed})"
    if tier == "_global_kernel":
        monkeypatch.setenv("LDPC_HIP_FORCE_GLOBAL", "1")
    M, maxiter = 9, 30
    H = relift(load_base_matrix(), M)
    llr = awgn_llr(H, M, 2.0, 512, 16)
    rng = np.random.RandomState(709)
    mags = np.array([500.0, 511.9, 512.0, 600.0, 709.0, 709.8, 710.0, 745.0])
    for f in range(llr.shape[0]):
        pos = rng.choice(llr.shape[1], mags.size, replace=False)
        llr[f, pos] = mags * np.where((np.arange(mags.size) + f) % 2 == 0, 1.0, -1.0)
    with L.LdpcHip(BP_DEC, H, M) as dec:
        assert tier in dec.kernel_name and "bp" in dec.kernel_name, dec.kernel_name
        hard, iters, soft = dec.decode(torch.from_numpy(llr).cuda(), maxiter, want_soft=True)
        torch.cuda.synchronize()
        d_ref, it_ref, _ = Oracle(H, M).decode(BP_DEC, llr, maxiter, 0)
        s_ref, _, _ = Oracle(H, M).decode(BP_DEC, llr, maxiter, 1)       # a fresh state: Gallager BP carries its syndrome from frame to frame
        assert np.array_equal(iters.cpu().numpy(), it_ref)
        assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref))
        assert_bits_equal(soft.cpu().numpy(), s_ref, "soft values", nan_ok=True)
