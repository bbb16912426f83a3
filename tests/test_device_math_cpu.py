"""The device math functions of ldpc_spec.hpp without a GPU: the operand generators of tests/test_gpu_device_math.py against their
domain predicates, the device's phi formula (frexp exponent, C division, ldexp, tables) restated in numpy against upstream's loop
(lche_model.logexp_int), the C transcription of exp_glibc_t against libm over the whole range in which it equals glibc, the
constants the GPU test takes from glibc, and the probe's cross-compilation."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import device_math_cases as dm
from lche_model import logexp_int
from ldpc_testlib import ROOT, assert_bits_equal

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not installed")


@pytest.mark.parametrize("name,pairs,inside", dm.DIV_DOMAINS, ids=[d[0] for d in dm.DIV_DOMAINS])
def test_division_operands_lie_in_their_domain(name, pairs, inside):
    a, b = pairs()
    assert a.shape == b.shape and (1 << 18) < a.size <= dm.MAX_OPERANDS
    ok = inside(a, b)
    assert ok.all(), (name, a[~ok][:4], b[~ok][:4])
    assert (a == 0).any() or name == "stated"                          # the exact zero every caller can produce
    if name != "polar":                                                # the corners: exact powers of two and the mantissas next to them
        m = np.frexp(np.abs(b))[0]
        assert (m == 0.5).any() and (m == np.nextafter(0.5, 1.0)).any() and (m == np.nextafter(1.0, 0.0)).any()


def test_callers_domains_lie_inside_the_stated_one():
    """div_ranged's comment states one domain; every caller's operands with a non-zero numerator must lie inside it."""
    for name, pairs, _ in dm.DIV_DOMAINS[:4]:
        a, b = pairs()
        nz = a != 0
        assert dm.in_stated(a[nz], b[nz]).all(), name


def test_predicates_reject_what_lies_outside():
    one = np.array([1.0])
    assert not dm.in_tdmp(np.array([-0.0]), one)[0] and not dm.in_tdmp(np.array([1e-280]), one)[0] and not dm.in_tdmp(one, np.array([9e-5]))[0]
    assert not dm.in_asp(one, np.array([2e7]))[0] and not dm.in_asp(np.array([1e-260]), one)[0]
    assert not dm.in_sp(np.array([2.0 ** -651]), one)[0] and not dm.in_sp(one, np.array([2.0 ** -55]))[0]
    assert not dm.in_sp(np.array([2.0 ** -56]), np.array([2.0 ** 650]))[0]          # exponents 706 apart
    assert not dm.in_polar(np.array([1.0]), np.array([0.5]))[0] and not dm.in_polar(np.array([0.0]), one)[0]   # -2 log(1) is -0.0
    assert not dm.in_stated(np.array([2.0 ** -970]), one)[0] and not dm.in_stated(one, np.array([2.0 ** 1022]))[0]
    assert not dm.in_stated(np.array([2.0 ** 768]), one)[0] and not dm.in_stated(one, np.array([2.0 ** -1023]))[0]
    assert not dm.in_stated(np.array([0.5]), np.array([1.5 * 2.0 ** 1021]))[0]       # a subnormal quotient
    assert dm.in_stated(np.array([2.0 ** 767]), one)[0] and dm.in_stated(np.array([2.0 ** -969]), np.array([2.0 ** -202]))[0]


def test_operand_sets_fit_the_probe_and_hold_their_edges():
    sets = {"exp": dm.exp_operands(), "expw": dm.expw_operands(), "log": dm.log_operands(), "sqrt": dm.sqrt_operands(), "phi": dm.phi_operands(),
            "prior": dm.prior_operands()}
    for name, x in sets.items():
        # (log: four families of 2^18 plus its edges -- the GPU test sends it to the probe in two calls)
        assert 0 < x.size <= dm.MAX_OPERANDS + (8192 if name == "log" else 0), (name, x.size)
    a, b = dm.div_special_pairs()
    assert (1 << 16) <= a.size <= dm.MAX_OPERANDS
    q = dm.ieee_div(a, b)
    sub = (q != 0) & (np.abs(q) < np.finfo(np.float64).tiny)
    assert np.isnan(a).any() and np.isinf(b).any() and sub.sum() > 1000 and (np.isinf(q) & np.isfinite(a) & (b != 0)).sum() > 1000
    x = sets["exp"]
    assert x.min() > -512 and x.max() < dm.EXP_HI and ((x >= 512).sum() > 100000) and np.nextafter(512.0, 0.0) in x
    assert not np.isnan(sets["phi"]).any() and np.isnan(sets["log"]).sum() == 1
    x = sets["expw"]
    for v in (dm.EXP_OVERFLOW, np.nextafter(dm.EXP_OVERFLOW, np.inf), dm.EXP_UNDERFLOW, 512.0, -512.0, np.inf, -np.inf, -746.0):
        assert v in x


def test_libm_has_the_thresholds_the_gpu_test_names():
    t = dm.EXP_OVERFLOW
    got = dm.libm_exp(np.array([t, np.nextafter(t, np.inf), dm.EXP_UNDERFLOW, np.nextafter(dm.EXP_UNDERFLOW, -np.inf), -746.0, 0.0, -np.inf]))
    assert np.isfinite(got[0]) and got[0] > 1.797e308 and got[1] == np.inf
    assert got[2] == 2.0 ** -1074 and got[3] == 0.0 and got[4] == 0.0 and got[5] == 1.0 and got[6] == 0.0
    lg = dm.libm_log(np.array([0.0, -0.0, np.inf, -1.0, np.nan, 1.0]))
    assert lg[0] == lg[1] == -np.inf and lg[2] == np.inf and np.isnan(lg[3]) and np.isnan(lg[4]) and lg[5] == 0.0


def test_phi_formula_of_the_device_equals_upstreams_loop():
    """lche::logexp replaces `while (x < 1/512) { x *= 32; s -= 3.46; }` by k = (-4 - frexp exponent) / 5 (C division), ldexp and
    kLcheStep[k]: the same value as the loop at every power of two down to the smallest subnormal, at every step boundary
    2^-9 32^-k, at the three tables' rounding boundaries and on random arguments -- and the indices stay inside the tables."""
    x = dm.phi_operands()
    k, idx, base = dm.phi_index(x)
    assert k.min() == 0 and k.max() == 213 and (idx >= base).all() and (idx < base + 32).all()
    assert set(np.unique(k)) == set(range(214))                       # every entry of the step table is reached
    assert {int(v) for v in np.unique(idx)} == set(range(3, 96))      # A[0..2] belong to x < 2, which the B table serves
    assert_bits_equal(dm.phi_device_formula(x), logexp_int(x), "phi")


def test_exp_transcription_equals_libm_between_minus_512_and_the_overflow_threshold(tmp_path):
    """The C transcription of exp_glibc_t (same constants, table and fma placement as the header) returns libm's exp() bit for bit
    for -512 < x < 709.78, the range the header now states: 8 million uniform arguments, the table index boundaries k ln2 / 128
    with their neighbours, and the arguments next to +-512.  (For x <= -512 glibc's special-case path rounds about 0.07 % of the
    arguments differently; that is why exp_glibc_wide switches at 512.)"""
    if " fma" not in open("/proc/cpuinfo").read():
        pytest.skip("host without FMA: glibc selects its non-FMA exp build there")
    src = (dm.exp_transcription_c() +
           "int main(){unsigned long long s=88172645463325252ull;long bad=0,n=8000000;\n"
           " for(long i=0;i<n;i++){s^=s<<13;s^=s>>7;s^=s<<17;double x=((double)(s>>11)/9007199254740992.0)*(709.78+512.0)-512.0;\n"
           "  if(x<=-512.0||x>=709.78) continue; if(asu(exp_glibc(x))!=asu(exp(x))) bad++;}\n"
           " for(int k=-94500;k<=131000;k++){double c=k*0x1.62e42fefa39efp-1/128.0;\n"
           "  double t[3]={nextafter(c,-1e9),c,nextafter(c,1e9)}; for(int j=0;j<3;j++) if(asu(exp_glibc(t[j]))!=asu(exp(t[j]))) bad++;}\n"
           " double e[4]={nextafter(512.0,0.0),nextafter(-512.0,0.0),512.0,nextafter(709.78,0.0)};\n"
           " for(int j=0;j<4;j++) if(asu(exp_glibc(e[j]))!=asu(exp(e[j]))) bad++;\n"
           " printf(\"%ld\\n\",bad);return bad!=0;}\n")
    (tmp_path / "e.c").write_text(src)
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-mfma", str(tmp_path / "e.c"), "-o", str(tmp_path / "e"), "-lm"])
    assert subprocess.run([str(tmp_path / "e")], stdout=subprocess.PIPE, text=True).stdout.strip() == "0"


def test_references_agree_with_numpy_where_both_are_exact():
    p, q = dm.prior_reference(np.array([0.0, -0.0, 25.0, -25.0, 20.0, -20.0]))
    assert p[0] == p[1] == 0.5 and q[0] == 2048 and p[2] == p[4] and p[3] == p[5] and q[2] == 1 and q[3] == 4095
    a = np.array([-0.0, -0.0, 0.0, 0.0, 3.0, -0.0])
    b = np.array([2.0, -2.0, 2.0, -2.0, 2.0, 0.0])
    want = np.array([0.0, 0.0, 0.0, -0.0, 1.5, np.nan])
    assert_bits_equal(dm.div_ranged_expected(a, b), want, "pinned zeros", nan_ok=True)


@needs_hipcc
def test_probe_cross_compiles_with_the_librarys_flags(tmp_path):
    from ldpc_lib_amd.binding import HIPCC_FLAGS
    assert "-ffp-contract=off" in HIPCC_FLAGS and "--offload-arch=gfx950" in HIPCC_FLAGS
    out = tmp_path / "math_probe"
    subprocess.check_call([HIPCC, *HIPCC_FLAGS, os.path.join(ROOT, "tests", "cpp", "math_probe.hip"), "-o", str(out)])
    assert out.exists()
    # no device here or a wrong call: the probe says so and exits non-zero, it never reports success without having computed
    r = subprocess.run([str(out), "nosuchop", str(tmp_path / "in"), str(tmp_path / "o")], stderr=subprocess.PIPE, text=True)
    assert r.returncode != 0 and "unknown op" in r.stderr
