"""Operands, domain predicates and references for the device math functions of ldpc_spec.hpp (exp_glibc, exp_glibc_wide, log_glibc,
div_ranged, lche::logexp, iasp::prior) and for the compiler's own fp64 division and square root.  Shared by
tests/test_device_math_cpu.py (generators against their predicates, the phi formula against logexp_int) and tests/test_gpu_device_math.py
(tests/cpp/math_probe.hip evaluates the functions on the device).

References: exp and log are the host's libm through ctypes (numpy's own are not glibc's, math.exp / math.log raise where libm
returns inf or NaN); division and square root are numpy's fp64 (IEEE, correctly rounded); phi is lche_model.logexp_int.
Everything is seeded: the same operands come out on every machine."""
import ctypes
import ctypes.util
import math
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_lche_table  # noqa: E402

MAX_OPERANDS = 1 << 20                                      # what the probe accepts per call
EXP_OVERFLOW = float.fromhex("0x1.62e42fefa39efp+9")       # glibc: exp(x) is finite up to and including this x, +inf beyond
EXP_UNDERFLOW = float.fromhex("-0x1.74910d52d3051p+9")     # glibc: exp(x) rounds to +0 below this x
EXP_HI = 709.78                                            # upper end of the sampled range of exp_glibc's table path
LOG_OFF = 0x3FE6000000000000                                # log_glibc: x = 2^k z with z in [OFF, 2 OFF), 128 table intervals
LOG_LO, LOG_HI = 0x3FEE000000000000, 0x3FF1090000000000     # log_glibc: the window of the near-1 polynomial

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _name in ("exp", "log"):
    getattr(_libm, _name).restype = ctypes.c_double
    getattr(_libm, _name).argtypes = [ctypes.c_double]


def _map(fn, x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):                       # libm raises the IEEE flags; numpy would turn them into warnings
        return np.frompyfunc(fn, 1, 1)(x).astype(np.float64).reshape(x.shape)


def libm_exp(x):
    return _map(_libm.exp, x)


def libm_log(x):
    return _map(_libm.log, x)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def from_bits(u):
    return np.ascontiguousarray(np.asarray(u, dtype=np.uint64)).view(np.float64)


def around(x, k=1):
    """x and its k neighbours on either side (in value order; steps through zero and the subnormals like nextafter)."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def exponent(x):
    """e with |x| = f 2^e, f in [0.5, 1) (frexp's, defined for subnormals as well)."""
    return np.frexp(np.asarray(x, dtype=np.float64))[1].astype(np.int64)


def ulp_distance(a, b):
    """Distance in representable doubles between two arrays of non-negative finite values."""
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


def log_uniform(rng, lo, hi, n):
    """n doubles with a uniform binary logarithm in [lo, hi] (random mantissas, clipped to the interval)."""
    return np.clip(np.exp2(rng.uniform(math.log2(lo), math.log2(hi), n)), lo, hi)


def _mantissas(e):
    """1, 1 + ulp and 2 - ulp times 2^e for every e of the list."""
    p = np.ldexp(1.0, np.asarray(e, dtype=np.int64))
    return np.concatenate([p, np.nextafter(p, np.inf), np.nextafter(2 * p, 0.0)])


def _grid(a, b):
    a, b = np.meshgrid(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), indexing="ij")
    return a.ravel(), b.ravel()


# ---- exp ---------------------------------------------------------------------------------------------------------------------------
def exp_operands():
    rng = np.random.RandomState(20261020)
    u = rng.uniform(-512.0, 512.0, 1 << 19)
    u = u[np.abs(u) < 512.0]
    hi = rng.uniform(512.0, EXP_HI, 1 << 17)
    hi = hi[hi < EXP_HI]
    tiny = np.array([0.0, 2.0 ** -1074, 2.0 ** -54, 2.0 ** -60, 1e-300])
    k = np.arange(-128, 129, dtype=np.float64)
    edges = np.concatenate([tiny, -tiny, around([20.0, -20.0], 2), around(k * math.log(2.0) / 128.0, 1),       # table index boundaries
                            [np.nextafter(512.0, 0.0), -np.nextafter(512.0, 0.0)]])
    return np.concatenate([edges, u, hi])


def expw_operands():
    extra = np.concatenate([around(EXP_OVERFLOW, 64), [709.0, 710.0, 1e3, 4e4, np.inf, -745.2, -746.0, -1e3, -4e4, -np.inf],
                            around(EXP_UNDERFLOW, 64), around([512.0, -512.0], 2)])
    return np.concatenate([extra, exp_operands()])


# ---- log ---------------------------------------------------------------------------------------------------------------------------
def log_operands():
    rng = np.random.RandomState(20261021)
    n = 1 << 18
    fam = [rng.random_sample(n), 1.0 / (rng.random_sample(n) + 1e-300), 0.9375 + 0.13 * rng.random_sample(n),
           np.ldexp(rng.random_sample(n), -(rng.randint(0, 1 << 30, n) % 1070))]
    window = np.concatenate([from_bits(np.arange(c - 8, c + 9, dtype=np.uint64)) for c in (LOG_LO, LOG_HI)])
    one = around(1.0, 8)
    pow2 = np.ldexp(1.0, np.arange(-1074, 1024))
    z = np.uint64(LOG_OFF) + (np.arange(128, dtype=np.uint64) << np.uint64(45))
    table = from_bits(np.concatenate([z - np.uint64(1), z, z + np.uint64(1)]))
    special = np.array([0.0, -0.0, np.inf, -1.0, -np.inf, np.nan, np.finfo(np.float64).max])
    return np.concatenate([special, window, one, pow2, table, 4.0 * table, table / 1024.0] + fam)


# ---- division ----------------------------------------------------------------------------------------------------------------------
# The callers' domains of div_ranged.  Each predicate takes the operand arrays and says, per pair, whether the pair lies inside.
def in_tdmp(a, b):
    return (((a == 0) & ~np.signbit(a)) | ((a >= 4e-274) & (a <= 2))) & (b >= 1e-4) & (b <= 2)


def in_asp(a, b):
    return (((a == 0) & ~np.signbit(a)) | ((a >= 4e-258) & (a <= 2))) & (b >= 1e-6) & (b <= 1e7)


def in_sp(a, b):
    a, b = np.abs(a), np.abs(b)
    az = a == 0
    return (az | ((a >= 2.0 ** -650) & (a <= 2.0 ** 650))) & (b >= 2.0 ** -54) & (b <= 2.0 ** 650) & (az | (np.abs(exponent(a) - exponent(b)) <= 704))


def in_polar(a, b):
    """b = r2 with 2^-106 <= r2 <= 1, a = -2 log(r2) (libm): -0.0 at r2 == 1, positive below 150 otherwise."""
    return (b >= 2.0 ** -106) & (b <= 1) & (bits(a) == bits(-2.0 * libm_log(b))) & (a >= 0) & (a < 150)


def in_stated(a, b):
    """What the comment above div_ranged states: both operands normal and finite, |a| >= 2^-969, |b| < 2^1022, the numerator's
    exponent less than 768 above the denominator's and the quotient normal (the numerator's exponent at most 1021 below)."""
    a, b = np.abs(a), np.abs(b)
    tiny = np.finfo(np.float64).tiny
    d = exponent(a) - exponent(b)
    return np.isfinite(a) & np.isfinite(b) & (a >= tiny) & (b >= tiny) & (a >= 2.0 ** -969) & (b < 2.0 ** 1022) & (d < 768) & (d >= -1021)


def hard_quotients(rng, n):
    """n pairs of 53-bit integers (A, B) whose quotient lies next to a rounding boundary: B Q = A 2^54 + s for an odd 54-bit Q (the
    midpoint of two neighbouring doubles) and |s| <= 16, so A / B misses the midpoint by |s| / B, about |s| 2^-53 of half an ulp.
    These are the quotients on which a reciprocal that is not accurate to its last bit rounds the wrong way.  Returned as doubles
    in [2^52, 2^53); scaling either by a power of two keeps the property."""
    a, b = [], []
    while len(a) < n:
        q = int(rng.randint(1 << 52, 1 << 53, dtype=np.int64)) * 2 + 1
        sv = int(rng.randint(1, 17)) * (1 if rng.randint(0, 2) else -1)
        bb = (sv * pow(q, -1, 1 << 54)) % (1 << 54)
        aa = (bb * q - sv) >> 54
        if (1 << 52) <= bb < (1 << 53) and (1 << 52) <= aa < (1 << 53):
            assert aa << 54 == bb * q - sv
            a.append(float(aa)); b.append(float(bb))
    return np.array(a), np.array(b)


N_HARD = 1 << 12


def _with_hard(rng, a, b, ea, eb, signs=False):
    """append N_HARD near-midpoint pairs for each (exponent of a, exponent of b) of the lists: A 2^ea / (B 2^eb), A and B in [0.5, 1)"""
    for x, y in zip(ea, eb):
        ha, hb = hard_quotients(rng, N_HARD)
        ha, hb = np.ldexp(ha, x - 53), np.ldexp(hb, y - 53)
        if signs:
            ha, hb = ha * rng.choice([-1.0, 1.0], N_HARD), hb * rng.choice([-1.0, 1.0], N_HARD)
        a, b = np.concatenate([ha, a]), np.concatenate([hb, b])
    return a, b


def _prob_pairs(rng, alo, blo, bhi, n):
    a = np.where(rng.random_sample(n) < 0.5, log_uniform(rng, alo, 2.0, n), rng.uniform(0.0, 2.0, n))
    a = np.where(a < alo, alo, a)
    a[rng.random_sample(n) < 1.0 / 16] = 0.0
    b = np.where(rng.random_sample(n) < 0.5, log_uniform(rng, blo, bhi, n), rng.uniform(blo, min(bhi, 2.0), n))
    ea, eb = exponent(alo), exponent(blo)
    ca = np.concatenate([[0.0, alo, np.nextafter(alo, np.inf), 2.0, np.nextafter(2.0, 0.0)], _mantissas([ea, ea + 1, -1, 0])])
    cb = np.concatenate([[blo, np.nextafter(blo, np.inf), bhi, np.nextafter(bhi, 0.0)], _mantissas([eb, eb + 1, exponent(bhi) - 2, -1, 0])])
    ga, gb = _grid(ca[(ca == 0) | ((ca >= alo) & (ca <= 2))], cb[(cb >= blo) & (cb <= bhi)])
    a, b = _with_hard(rng, a, b, [0, 0, -1, int(ea) + 1], [0, 1, int(eb) + 1, 0])
    return np.concatenate([ga, a]), np.concatenate([gb, b])


def tdmp_pairs():
    return _prob_pairs(np.random.RandomState(20261022), 4e-274, 1e-4, 2.0, 1 << 18)


def asp_pairs():
    return _prob_pairs(np.random.RandomState(20261023), 4e-258, 1e-6, 1e7, 1 << 18)


def sp_pairs():
    rng = np.random.RandomState(20261024)
    n = 1 << 18
    eb = rng.randint(-53, 651, n)                                                 # frexp exponents: |b| in [2^-54, 2^650)
    ea = rng.randint(np.maximum(-649, eb - 704), np.minimum(650, eb + 704) + 1)
    a = np.ldexp(rng.uniform(0.5, 1.0, n), ea) * rng.choice([-1.0, 1.0], n)
    b = np.ldexp(rng.uniform(0.5, 1.0, n), eb) * rng.choice([-1.0, 1.0], n)
    a[rng.random_sample(n) < 1.0 / 32] = 0.0
    a[rng.random_sample(n) < 1.0 / 32] = -0.0
    ca = np.concatenate([[0.0, 2.0 ** 650], _mantissas([-650, -649, -54, -1, 0, 53, 648, 649])])
    cb = np.concatenate([[2.0 ** 650], _mantissas([-54, -53, -1, 0, 53, 648, 649])])
    ga, gb = _grid(np.concatenate([ca, -ca]), np.concatenate([cb, -cb]))
    # the corners of the exponent band: 704 apart, mantissas at both ends
    band_b = _mantissas([-54, -53, 0, 54, 55])
    for sh in (704, 703, -704, -703):
        for mb in band_b:
            ma = _mantissas([int(exponent(mb)) - 1 + sh])
            ga, gb = np.concatenate([ga, ma, -ma]), np.concatenate([gb, np.full(3, mb), np.full(3, mb)])
    a, b = _with_hard(rng, a, b, [0, 0, 650, -649, 300], [0, 1, 10, -53, 650], signs=True)
    keep = in_sp(ga, gb)
    return np.concatenate([ga[keep], a]), np.concatenate([gb[keep], b])


def polar_pairs():
    """The polar method's division -2 log(r2) / r2 (ldpc_mt.hpp): r2 = x^2 + y^2 of two 53-bit canonical values mapped to (-1, 1),
    accepted when 0 < r2 <= 1."""
    rng = np.random.RandomState(20261025)
    n = 3 << 17
    can = lambda: (rng.randint(0, 1 << 53, n, dtype=np.int64).astype(np.float64) / 2.0 ** 53) * 2.0 - 1.0   # noqa: E731
    x, y = can(), can()
    small = rng.random_sample(n) < 0.25                                      # points close to the origin are rare: ask for some
    x[small] = np.ldexp(x[small], -rng.randint(0, 53, int(small.sum())))
    y[small] = np.ldexp(y[small], -rng.randint(0, 53, int(small.sum())))
    r2 = x * x + y * y
    r2 = r2[(r2 > 0) & (r2 <= 1) & (r2 >= 2.0 ** -106)][:1 << 18]
    assert r2.size == 1 << 18
    r2 = np.concatenate([[2.0 ** -106, 2.0 ** -104, 2.0 ** -52, 0.5, np.nextafter(0.5, 0.0), np.nextafter(1.0, 0.0), 1.0], r2])
    return -2.0 * libm_log(r2), r2


def stated_pairs():
    rng = np.random.RandomState(20261026)
    n = 1 << 18
    eb = rng.randint(-1021, 1023, n)                                               # frexp exponents: |b| in [2^-1022, 2^1022)
    ea = rng.randint(np.maximum(-968, eb - 1021), np.minimum(1024, eb + 767) + 1)
    a = np.ldexp(rng.uniform(0.5, 1.0, n), ea) * rng.choice([-1.0, 1.0], n)
    b = np.ldexp(rng.uniform(0.5, 1.0, n), eb) * rng.choice([-1.0, 1.0], n)
    big = np.finfo(np.float64).max
    # on each boundary and one step inside: |a| = 2^-969, |b| just below 2^1022 and at 2^-1022, the numerator's exponent 767 above and 1021
    # below the denominator's, |a| at the largest double
    ga, gb = [], []
    for av in np.concatenate([_mantissas([-969, -968]), [big, np.nextafter(big, 0.0), 2.0 ** 1023], _mantissas([1021, 1022])]):
        e = int(exponent(av)) - 1
        for d in (767, 766, 1, 0, -1, -1020, -1021):
            if -1022 <= e - d <= 1021:
                mb = _mantissas([e - d])
                ga.append(np.full(3, av)); gb.append(mb)
    for bv in np.concatenate([_mantissas([-1022, -1021]), _mantissas([1021, 1020])]):
        e = int(exponent(bv)) - 1
        for d in (767, 766, 1, 0, -1, -1020, -1021):
            if -969 <= e + d <= 1023:
                ma = _mantissas([e + d])
                ga.append(ma); gb.append(np.full(3, bv))
    ga, gb = np.concatenate(ga), np.concatenate(gb)
    ga, gb = np.concatenate([ga, -ga, ga, -ga]), np.concatenate([gb, gb, -gb, -gb])
    a, b = _with_hard(rng, a, b, [0, 0, -968, 1024, -968, 1022], [0, 1, -1021, 1022, 52, 256], signs=True)
    keep = in_stated(ga, gb)
    return np.concatenate([ga[keep], a]), np.concatenate([gb[keep], b])


DIV_DOMAINS = [("tdmp", tdmp_pairs, in_tdmp), ("asp", asp_pairs, in_asp), ("sp", sp_pairs, in_sp), ("polar", polar_pairs, in_polar),
               ("stated", stated_pairs, in_stated)]


def div_special_pairs():
    """For the compiler's a / b only: denormal, zero, infinite and NaN operands, quotients that overflow or underflow."""
    rng = np.random.RandomState(20261027)
    n = 1 << 16
    anyd = lambda: from_bits(rng.randint(0, 1 << 63, n, dtype=np.int64).astype(np.uint64) | (rng.randint(0, 2, n).astype(np.uint64) << np.uint64(63)))   # noqa: E731
    den = lambda: from_bits(rng.randint(1, 1 << 52, n, dtype=np.int64).astype(np.uint64)) * rng.choice([-1.0, 1.0], n)   # noqa: E731
    a, b = anyd(), anyd()                                           # any bit pattern (NaNs of every payload and infinities among them)
    q = n // 8
    a[:q] = den()[:q]                                               # denormal numerators
    b[q:2 * q] = den()[:q]                                          # denormal denominators
    a[2 * q:3 * q], b[2 * q:3 * q] = den()[:q], den()[:q]           # both
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 2.0 ** -1074, -2.0 ** -1074, 2.0 ** -1022, np.finfo(np.float64).max, 3.0, 2.0 ** 1023, 2.0 ** -1000])
    ga, gb = _grid(sp, sp)
    # quotients around the overflow and underflow thresholds
    eb = rng.randint(-1000, 1000, q)
    lo_a = np.ldexp(rng.uniform(0.5, 1.0, q), np.clip(eb - 1022 - rng.randint(-3, 56, q), -1073, 1024))
    lo_b = np.ldexp(rng.uniform(0.5, 1.0, q), eb)
    hi_a = np.ldexp(rng.uniform(0.5, 1.0, q), np.clip(eb + 1024 + rng.randint(-3, 3, q), -1073, 1024))
    a[3 * q:4 * q], b[3 * q:4 * q] = lo_a, lo_b
    a[4 * q:5 * q], b[4 * q:5 * q] = hi_a, lo_b
    return np.concatenate([ga, a]), np.concatenate([gb, b])


def ieee_div(a, b):
    with np.errstate(all="ignore"):
        return np.asarray(a, dtype=np.float64) / np.asarray(b, dtype=np.float64)


def div_ranged_expected(a, b):
    """IEEE a / b, but a numerator of -0.0 gives +0.0 whatever the denominator's sign: -0 * r is a zero, the residual
    fma(-b, q, -0) is +0, and fma(+0, r, q) adds zeros of opposite signs.  (+0 / b keeps IEEE's sign.)  ldpc_mt.hpp relies on it."""
    q = ieee_div(a, b)
    return np.where((a == 0) & np.signbit(a) & (b != 0) & np.isfinite(b), 0.0, q)


# ---- square root -------------------------------------------------------------------------------------------------------------------
def sqrt_operands():
    rng = np.random.RandomState(20261028)
    x = from_bits(rng.randint(1, 0x7FF0000000000000, 1 << 18, dtype=np.int64).astype(np.uint64))      # uniform bit patterns = log-uniform values
    pow2 = np.ldexp(1.0, np.arange(-1074, 1024))
    k = np.arange(1, 1 << 13, dtype=np.float64)
    den = from_bits(rng.randint(1, 1 << 52, 1 << 12, dtype=np.int64).astype(np.uint64))
    return np.concatenate([[0.0, -0.0, np.inf, np.finfo(np.float64).max, 2.0 ** -1022], pow2, around(k * k, 1), den, x])


# ---- phi (lche::logexp) ------------------------------------------------------------------------------------------------------------
def phi_operands():
    """No NaN: logexp is never called with one, and its table index is derived from the operand."""
    rng = np.random.RandomState(20261029)
    pow2 = around(np.ldexp(1.0, np.arange(-1074, 6)), 1)
    steps = around(np.ldexp(1.0, -9 - 5 * np.arange(213)), 2)                     # where upstream's loop takes one more pass
    marks = around([1.0 / 512, 1.0 / 16, 2.0, 16.0], 2)
    i = np.arange(0, 33, dtype=np.float64)
    rounding = np.concatenate([around((i + 0.5) / f, 2) for f in (2.0, 16.0, 512.0)])
    scaled = np.concatenate([around(np.ldexp((i + 0.5) / 512.0, -5 * k), 1) for k in (1, 2, 7, 100, 200)])   # the same boundaries after scaling
    other = np.array([0.0, -0.0, -1.0, -1e-300, -16.0, -1e300, np.nextafter(16.0, np.inf), 17.0, 32.0, 1e300])
    rnd = np.exp2(rng.uniform(-1074.0, 5.0, 1 << 17))
    x = np.concatenate([other, pow2, steps, marks, rounding, scaled, rnd])
    assert not np.isnan(x).any()
    return x


_PHI_T = np.array([v for t in gen_lche_table.tables() for v in t], dtype=np.float64)     # kLcheTab: A, B, C
_PHI_S = np.array(gen_lche_table.steps(), dtype=np.float64)                               # kLcheStep


def phi_index(x):
    """(k, table index) as lche::logexp computes them: frexp exponent, C integer division, ldexp."""
    x = np.array(x, dtype=np.float64, copy=True)
    x = np.where(x <= 0.0, 1.0 / 4096.0, x)
    x = np.where(x > 16.0, 16.0, x)
    t = -4 - exponent(x)
    k = np.where(t < 0, -((-t) // 5), t // 5)                                          # C's division truncates towards zero
    k = np.maximum(k, 0)
    xs = np.ldexp(x, 5 * k)
    f = np.where(x >= 2.0, 2.0, np.where(x > 1.0 / 16.0, 16.0, 512.0))
    base = np.where(x >= 2.0, 0, np.where(x > 1.0 / 16.0, 32, 64))
    return k, base + (f * xs + 0.5).astype(np.int64) - 1, base


def phi_device_formula(x):
    k, idx, _ = phi_index(x)
    return _PHI_S[k] - _PHI_T[idx]


# ---- IASP's channel prior ----------------------------------------------------------------------------------------------------------
def prior_operands():
    rng = np.random.RandomState(20261030)
    return np.concatenate([[0.0, -0.0], around([20.0, -20.0], 2), rng.uniform(-25.0, 25.0, 1 << 17)])


def prior_reference(x):
    """decoders.cpp:3858-3869: p = 1 / (1 + exp(clamp(x, -20, 20))), q = clamp((int)(p * 4096 + 0.5), 1, 4095)."""
    y = np.where(x < 20.0, x, 20.0)
    y = np.where(y < -20.0, -20.0, y)
    p = 1.0 / (1.0 + libm_exp(y))
    q = np.clip((p * 4096.0 + 0.5).astype(np.int64), 1, 4095)
    return p, q.astype(np.uint64)


# ---- the probe's files -------------------------------------------------------------------------------------------------------------
def write_arrays(path, arrays):
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
    n = arrays[0].size
    assert 0 < n <= MAX_OPERANDS and all(a.size == n for a in arrays), [a.size for a in arrays]
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", n, len(arrays)))
        for a in arrays:
            f.write(a.astype("<f8").tobytes())


def read_arrays(path, n, k):
    with open(path, "rb") as f:
        got_n, got_k = struct.unpack("<QQ", f.read(16))
        assert (got_n, got_k) == (n, k), (got_n, got_k, n, k)
        data = np.frombuffer(f.read(), dtype="<u8")
    assert data.size == n * k
    return [data[i * n:(i + 1) * n].copy() for i in range(k)]


# ---- exp_glibc_t as plain C --------------------------------------------------------------------------------------------------------
def exp_transcription_c():
    """C source (helpers asu / asd, the table, `static double exp_glibc(double)`) transcribed from the header's exp_glibc_t: same
    constants, same table, same fma placement.  Compile with -O2 -ffp-contract=off -mfma and append a main()."""
    import gen_exp_table
    tab = gen_exp_table.table()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "ldpc-lib_amd", "csrc", "ldpc_spec.hpp")).read()
    fn = hdr[hdr.index("__device__ __forceinline__ double exp_glibc_t(double x, Tab T) {"):]
    fn = fn[:fn.index("\n}\n") + 3]
    c_fn = (fn.replace("__device__ __forceinline__ double exp_glibc_t(double x, Tab T)", "static double exp_glibc(double x)").replace("__fma_rn", "fma")
              .replace("const ulonglong2 pair = *reinterpret_cast<const ulonglong2 *>(&T[idx]);", "const struct { unsigned long long x, y; } pair = {kExpTab[idx], kExpTab[idx + 1]};")
              .replace("(unsigned long long)__double_as_longlong(kd)", "asu(kd)")
              .replace("__longlong_as_double((long long)pair.x)", "asd(pair.x)")
              .replace("__longlong_as_double((long long)sbits)", "asd(sbits)"))
    return ("#include <math.h>\n#include <stdint.h>\n#include <stdio.h>\n#include <string.h>\n"
            "static unsigned long long asu(double x){unsigned long long u;memcpy(&u,&x,8);return u;}\n"
            "static double asd(unsigned long long u){double x;memcpy(&x,&u,8);return x;}\n"
            "static const unsigned long long kExpTab[256] = {" + ",".join("0x%xull" % v for v in tab) + "};\n" + c_fn)
