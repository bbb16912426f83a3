// ldpc_voltage.hpp -- upstream's equation_builder::check_voltages / check_voltages_and_coefs (equations.cpp:150-267) for a batch of
// labellings on the device: not "does one M divide no equation's sum" (ldpc_label.hpp's check_kernel) but EVERY lifting a labelling
// allows.  Included by ldpc_hip.hip after ldpc_label.hpp, whose equation table it walks; the host half also compiles with a plain C++
// compiler (tests/cpp/voltage_sanitize.cpp), the kernels only under hipcc.
//
//   host    piece_size() and first_bad_value(): the arithmetic of ldpc_voltage_api.hpp that needs no device, here so that it also runs
//           under the sanitizers (tests/cpp/voltage_sanitize.cpp).
//   device  check_kernel: one wave per labelling.  The wave keeps the labelling (and its coefficients) in LDS.
//           Pass 1, lanes over equations: the sums s_e (and c_e), the status and max |s_e|.  A labelling of status 1 ends here.
//           Pass 2, per tile of kTile equations: the lanes write |s_e| (0 where the equation contributes nothing) to LDS, then
//           split into 64 / DL groups of DL lanes, DL the power of two that covers the candidates d <= sqrt(max |s|) (at most 64):
//           a lane holds one candidate d and its reciprocal, its group walks every (64 / DL)-th sum of the tile.  s / d is a float
//           multiply with the reciprocal, exact after one correction step as s < 2^21 (kMaxGirth); no hardware division.  A hit sets
//           bits d and s / d of the LDS bitmap with atomicOr -- OR commutes, the bitmap does not depend on the order.
//           Last, the lanes scan the bitmap for the smallest clear bit >= 2 and the largest set bit and write it out.
//           check_kernel<true> is the alternative that was measured (profiles/r31_voltage_time.txt): lanes over the moduli m, each
//           walking the sums until one is divisible.  It costs up to max_modulo * n_equations / 64 steps per labelling where the
//           candidate layout costs sqrt(max |s|) * n_equations / 64; LDPC_HIP_VOLTAGE_LAYOUT=moduli selects it.
//           bank_kernel: the same check on the attempts of a labelling search's round that have no zero sum (ldpc_label.hpp's
//           check_kernel finds them, one attempt per lane), accepted as upstream's random_search_bank_good_codes accepts.
#pragma once

#include <stdint.h>

namespace ldpc_voltage {

constexpr int kMaxModulo = 65535;   // the LDS bitmap: 8 KiB
constexpr int kMaxEdges = 4096;     // voltages and coefficients in LDS: 32 KiB; an edge index fits the 24 bits of a packed term
constexpr int kTile = 2048;         // sums of one tile in LDS: 8 KiB
constexpr int kMaxValue = 32767;    // voltages and coefficients: |sum| < 62 * 32767 < 2^21

inline int bitmap_words(int max_modulo) { return max_modulo / 64 + 1; }

// the piece size of a batch of K labellings: what fits piece_bytes and piece_max labellings, at least one; forced > 0 (the knob)
// replaces the byte limit.  per-labelling bytes on the device: voltages (and coefficients), the bitmap where the caller wants it, four
// int32 results.
inline long long piece_size(long long K, long long E, bool has_coef, bool has_failed, int W, long long piece_bytes, long long piece_max, long long forced) {
    const long long per = (long long)sizeof(int32_t) * E * (has_coef ? 2 : 1) + (has_failed ? (long long)sizeof(uint64_t) * W : 0) + 4 * (long long)sizeof(int32_t);
    long long piece = forced > 0 ? forced : piece_bytes / per;
    if (piece > piece_max) piece = piece_max;
    if (piece < 1) piece = 1;
    return piece < K ? piece : K;
}

// index of the first of n values outside 0 .. kMaxValue, or -1
inline long long first_bad_value(const int32_t *values, long long n) {
    for (long long i = 0; i < n; ++i)
        if (values[i] < 0 || values[i] > kMaxValue) return i;
    return -1;
}

}  // namespace ldpc_voltage


#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace ldpc_voltage {

struct Equations {
    int n_eq;
    const int32_t *eq_begin;     // [n_eq + 1]
    const int32_t *terms;        // (edge << 8) | (multiplicity & 0xff), as ldpc_label::Args::terms
};

struct Args {
    Equations q;
    int E, max_modulo, W;
    const int32_t *voltages;     // [k][E] of the piece
    const int32_t *coefs;        // [k][E] or NULL
    int32_t *status, *min_ok, *max_nonok, *max_abs_sum;   // [k]
    uint32_t *failed;            // [k][2 * W] (the uint64 words, low half first) or NULL
};

// the bank search: the round of ldpc_label::Args, whose bitmap holds the attempts without a zero sum on entry and the accepted ones
// on return
struct BankArgs {
    ldpc_label::Args l;
    int T, exact_modulo, max_modulo, W;
    int32_t *min_ok_att;         // [n]: written for the accepted attempts
};

// the LDS of one wave: v [E] | coef [E] (with coefficients) | sums [kTile] | bitmap [2 * W]
inline size_t lds_bytes(int E, bool has_coef, int W) { return sizeof(int32_t) * ((size_t)E * (has_coef ? 2 : 1) + kTile + 2 * (size_t)W); }

struct Result { int status, min_ok, max_nonok, max_abs_sum; };

__device__ __forceinline__ int wave_max(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int y = __shfl_xor(x, o); x = y > x ? y : x; }
    return x;
}

__device__ __forceinline__ int wave_min(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int y = __shfl_xor(x, o); x = y < x ? y : x; }
    return x;
}

// the sums of equation eq over the labelling and over the coefficients (cf == nullptr: none) in LDS
__device__ __forceinline__ void eq_sums(const Equations &q, const int32_t *v, const int32_t *cf, int eq, int &s, int &c) {
    s = 0; c = 0;
    const int b = q.eq_begin[eq], e = q.eq_begin[eq + 1];
    for (int t = b; t < e; ++t) {
        const int w = q.terms[t];
        const int mult = (int)(int8_t)(w & 0xff), edge = w >> 8;
        s += mult * v[edge];
        if (cf) c += mult * cf[edge];
    }
}

// q = s / d and whether d divides s, for 0 < d, s < 2^21: float(s) is exact, the reciprocal and the product are each off by a relative
// 2^-23 at most, so the truncated quotient is off by at most one
__device__ __forceinline__ bool divides(uint32_t s, uint32_t d, float rd, uint32_t &q) {
    q = (uint32_t)((float)s * rd);
    int r = (int)s - (int)(q * d);
    if (r < 0) { --q; r += (int)d; }
    else if (r >= (int)d) { ++q; r -= (int)d; }
    return r == 0;
}

// One labelling by one wave (a workgroup of its own: the barriers are the wave's).  v, cf: the labelling in LDS, complete before the
// call; sums [kTile], bits [2 * W]: the wave's scratch; bits holds the set afterwards (all zero for status 1).
template <bool kModuli>
__device__ Result check_labelling(const Equations &q, const int32_t *v, const int32_t *cf, uint32_t *sums, uint32_t *bits, int max_modulo, int W,
                                  int lane) {
    const int n32 = 2 * W;
    for (int w = lane; w < n32; w += 64) bits[w] = 0u;
    // pass 1: status and max |s|
    int smax = 0;
    bool zero_fail = false, zero_rescued = false;
    for (int eq = lane; eq < q.n_eq; eq += 64) {
        int s, c;
        eq_sums(q, v, cf, eq, s, c);
        const int as = s < 0 ? -s : s;
        smax = as > smax ? as : smax;
        if (s == 0) { if (cf && c != 0) zero_rescued = true; else zero_fail = true; }
    }
    Result r;
    r.max_abs_sum = smax = wave_max(smax);
    r.status = __ballot(zero_fail) ? 1 : __ballot(zero_rescued) ? 2 : 0;
    r.min_ok = r.max_nonok = 0;
    __syncthreads();   // the bitmap is clear
    if (r.status == 1) return r;
    // candidates 1 .. dmax = floor(sqrt(smax)): the float root is right to one, the products decide
    int dmax = (int)sqrtf((float)smax);
    while (dmax * dmax > smax) --dmax;
    while ((dmax + 1) * (dmax + 1) <= smax) ++dmax;
    int dl_bits = 0;
    while ((1 << dl_bits) < dmax && dl_bits < 6) ++dl_bits;
    const int DL = 1 << dl_bits, groups = 64 >> dl_bits;
    const int dlane = lane & (DL - 1), glane = lane >> dl_bits;
    for (int t0 = 0; t0 < q.n_eq; t0 += kTile) {
        const int n = q.n_eq - t0 < kTile ? q.n_eq - t0 : kTile;
        __syncthreads();   // the tile before has been read
        for (int i = lane; i < n; i += 64) {
            int s, c;
            eq_sums(q, v, cf, t0 + i, s, c);
            sums[i] = (uint32_t)(s < 0 ? -s : s);   // 0: an equation rescued by its coefficients (status 2), no divisor
        }
        __syncthreads();
        if (!kModuli) {
            for (int d = dlane + 1; d <= dmax; d += DL) {
                const float rd = 1.0f / (float)d;
                const uint32_t dd = (uint32_t)(d * d);
                for (int i = glane; i < n; i += groups) {
                    const uint32_t s = sums[i];
                    uint32_t quot;
                    if (dd <= s && divides(s, (uint32_t)d, rd, quot)) {
                        if (d <= max_modulo) atomicOr(&bits[d >> 5], 1u << (d & 31));
                        if (quot <= (uint32_t)max_modulo) atomicOr(&bits[quot >> 5], 1u << (quot & 31));
                    }
                }
            }
        } else {
            const int top = smax < max_modulo ? smax : max_modulo;   // no modulus above max |s| divides a sum
            for (int m = lane + 1; m <= top; m += 64) {
                if ((bits[m >> 5] >> (m & 31)) & 1u) continue;   // found in an earlier tile; bit m is set by this lane alone
                const float rm = 1.0f / (float)m;
                for (int i = 0; i < n; ++i) {
                    const uint32_t s = sums[i];
                    uint32_t quot;
                    if (s >= (uint32_t)m && divides(s, (uint32_t)m, rm, quot)) {
                        atomicOr(&bits[m >> 5], 1u << (m & 31));
                        break;
                    }
                }
            }
        }
    }
    __syncthreads();
    // the smallest clear bit in 2 .. max_modulo and the largest set bit
    int lo = max_modulo < 2 ? 2 : max_modulo + 1, hi = 1;
    for (int w = lane; w < n32; w += 64) {
        const uint32_t word = bits[w];
        uint32_t clear = ~word;
        if (w == 0) clear &= ~3u;
        if (clear) { const int m = 32 * w + __ffs((int)clear) - 1; if (m <= max_modulo && m < lo) lo = m; }
        if (word) { const int m = 32 * w + 31 - __clz((int)word); if (m > hi) hi = m; }
    }
    r.min_ok = wave_min(lo);
    r.max_nonok = wave_max(hi);
    return r;
}

template <bool kModuli>
__global__ void __launch_bounds__(64) check_kernel(const Args a) {
    extern __shared__ int32_t voltage_lds[];
    const int lane = threadIdx.x;
    const size_t k = blockIdx.x;
    int32_t *v = voltage_lds;
    int32_t *cf = a.coefs ? v + a.E : nullptr;
    uint32_t *sums = (uint32_t *)(v + (a.coefs ? 2 : 1) * a.E);
    uint32_t *bits = sums + kTile;
    for (int e = lane; e < a.E; e += 64) {
        v[e] = a.voltages[k * a.E + e];
        if (cf) cf[e] = a.coefs[k * a.E + e];
    }
    __syncthreads();
    const Result r = check_labelling<kModuli>(a.q, v, cf, sums, bits, a.max_modulo, a.W, lane);
    const int n32 = 2 * a.W;
    if (a.failed)
        for (int w = lane; w < n32; w += 64) a.failed[k * n32 + w] = bits[w];
    if (lane == 0) {
        a.status[k] = r.status;
        a.min_ok[k] = r.min_ok;
        a.max_nonok[k] = r.max_nonok;
        a.max_abs_sum[k] = r.max_abs_sum;
    }
}

// The bank search's second step: one wave per 64 attempts of the round, working through those that ldpc_label::check_kernel left
// (no zero sum).  A survivor's draws are read from the tape (fixed edges have no term in the table: the labelling is the Er draws),
// checked up to max(T, exact_modulo), and accepted as upstream's random_search_bank_good_codes accepts: min_ok <= T and, with an
// exact modulo, check_modulo(exact_modulo) -- exact_modulo >= T >= min_ok, and above max_nonok its bit is clear anyway.
__global__ void __launch_bounds__(64) bank_kernel(const BankArgs b) {
    extern __shared__ int32_t voltage_lds[];
    const ldpc_label::Args &a = b.l;
    const int lane = threadIdx.x;
    int32_t *v = voltage_lds;
    uint32_t *sums = (uint32_t *)(v + a.Er);
    uint32_t *bits = sums + kTile;
    const uint32_t nrej = ldpc_label::rejected_count(a);
    const Equations q{a.n_eq, a.eq_begin, a.terms};
    unsigned long long todo = a.bitmap[blockIdx.x], accepted = 0ull;
    while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const uint32_t att = blockIdx.x * 64u + (uint32_t)l;
        __syncthreads();   // the labelling before has been read
        for (int e = lane; e < a.Er; e += 64) {
            const uint32_t w = ldpc_label::word_of_draw(a, nrej, att * (uint32_t)a.Er + (uint32_t)e);
            v[e] = (int32_t)(((unsigned long long)ldpc_label::temper(a.xw[w]) * (uint32_t)a.M) >> 32);
        }
        __syncthreads();
        const Result r = check_labelling<false>(q, v, nullptr, sums, bits, b.max_modulo, b.W, lane);
        const bool ok = r.status == 0 && r.min_ok <= b.T && (b.exact_modulo == 0 || !((bits[b.exact_modulo >> 5] >> (b.exact_modulo & 31)) & 1u));
        if (ok) {
            accepted |= 1ull << l;
            if (lane == 0) b.min_ok_att[att] = r.min_ok;
        }
    }
    if (lane == 0) a.bitmap[blockIdx.x] = accepted;
}

}  // namespace ldpc_voltage
#endif  // __HIPCC__
