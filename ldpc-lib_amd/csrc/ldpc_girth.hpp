// ldpc_girth.hpp -- girth spectrum and ACE trace of C candidate codes of one shape on the device (gfx950): upstream's
// trace_bound_pol_mon_pm (trace_pm.cpp:58-299, the NATURAL_POLYNOM build), the filter its searches run in front of every bp_simulation
// (search_ggp/scenario_based_code_generation.cpp:527-570) and the source of girth_ / girth_ACE / girth_spectrum in its result records.
//
// The graph: every non-empty circulant (block row j, block column k, shift x) is an edge, numbered column by column with the rows
// ascending (tanner_mon :301-349).  Apm[I][J] (hp2a_mon_pm :352-482) is set for I = (j1, k1), J = (j2, k2) with j1 != j2, k1 != k2 and
// hd[j1][k2] >= 0 -- the walk I, back along (j1, k2), forward along J -- with degree a = ((M - hd[j1][k2]) % M + hd[j2][k2]) % M and
// weight as = 2 * cw[k2].  The host keeps it as per-J predecessor lists (j, a, as), j ascending (girth_graph in ldpc_girth_api.hpp).
//
// The state: B[I][J] is a polynomial of M int32 coefficients with an ace per coefficient (0 where the coefficient is 0; at most
// 20 * rh, so 16 bits hold it).  It starts as Apm (coefficient 1 at position a, ace as), and every step d = 3, 5, .. < gmax is
//     Y[I][J][h] = sum over the predecessors j of J of B[I][j][(h - a) mod M],   aceY = min over the non-zero terms of (aceB + as)
// (mul_mat_mat_mon :658-741, add_pol :631-656).  Integer sums and minima do not depend on the order, and row I of Y depends on row I
// of B only, so:
//   * step_kernel: one workgroup per (code, row I).  It stages row I of B -- E x M coefficients and aces -- in LDS, then walks the J
//     with one lane per coefficient h; the operand is read at the rotated address (h - a) mod M, consecutive lanes on consecutive
//     words (two runs), so the reads are free of bank conflicts.  Lanes = M rounded up to a wave; where that leaves room, several J
//     are in flight per workgroup.  A row beyond 160 KB is read from global memory instead (the kLds = false instance);
//   * trace_kernel: one workgroup per code.  S[d] = sum of the diagonal's constant terms, SA[d] = the smallest ace among the
//     non-zero ones (:183-199); the constant is then removed as upstream removes it (:201-207: pack, clear, pack again, unpack with
//     the aces of the FIRST packing -- the k-th remaining term takes the ace of the (k - 1)-th term of the list before removal, the
//     first one that of the constant); then the stop rule (:248-272) per code on the device.  A finished code is skipped by every
//     later launch, so a set needs 2 launches per step and no host synchronisation, whatever C is.
// Sums wrap in 32 bits as unsigned additions do; a sum of two non-negative values that turns negative sets the code's overflow bit.
#pragma once

#include <cstdint>

namespace ldpc_girth {

enum { kDone = 0, kCnt = 1, kOk = 2, kOverflow = 3, kState = 4 };   // per-code state words
constexpr size_t kLdsLimit = 160 * 1024;
constexpr int kMaxLanes = 1024;

struct Args {
    int32_t *coef[2];            // [codes][Emax][Emax][M], double-buffered
    uint16_t *ace[2];
    const int32_t *E;            // [codes]
    const int32_t *pred_begin;   // [codes][Emax + 1]
    const int32_t *pred;         // [codes][pred_stride][3]: j, a, as
    int32_t *state;              // [codes][kState]
    int32_t *S, *SA;             // [codes][gmax], zero on entry; undivided
    const int32_t *min_ace;      // [gmax] or null
    const int32_t *max_spec;     // [gmax] or null
    long long pred_stride;
    int Emax, M, gmax, gtarget, lanes;
};

__host__ __device__ inline size_t row_bytes(int E, int M) { return (size_t)E * M * (sizeof(int32_t) + sizeof(uint16_t)); }
__host__ __device__ inline size_t code_elems(int Emax, int M) { return (size_t)Emax * Emax * M; }

#if defined(__HIPCC__)

// B = Apm: workgroup (J, code) writes the one term of every predecessor's polynomial into the zeroed buffer 0
__global__ void __launch_bounds__(64) init_kernel(Args a) {
    const int c = blockIdx.y, J = blockIdx.x;
    if (J >= a.E[c]) return;
    const int32_t *pb = a.pred_begin + (size_t)c * (a.Emax + 1);
    const int32_t *pred = a.pred + (size_t)c * a.pred_stride * 3;
    const size_t base = (size_t)c * code_elems(a.Emax, a.M);
    for (int p = pb[J] + (int)threadIdx.x; p < pb[J + 1]; p += (int)blockDim.x) {
        const size_t at = base + ((size_t)pred[3 * p] * a.Emax + J) * a.M + pred[3 * p + 1];
        a.coef[0][at] = 1;
        a.ace[0][at] = (uint16_t)pred[3 * p + 2];
    }
}

template <bool kLds>
__global__ void __launch_bounds__(kMaxLanes) step_kernel(Args a, int src) {
    const int c = blockIdx.y, I = blockIdx.x;
    int32_t *st = a.state + (size_t)c * kState;
    const int E = a.E[c], M = a.M;
    if (st[kDone] || I >= E) return;   // uniform over the workgroup
    const size_t row = (size_t)c * code_elems(a.Emax, M) + (size_t)I * a.Emax * M;
    const int32_t *bc = a.coef[src] + row;
    const uint16_t *ba = a.ace[src] + row;
    int32_t *yc = a.coef[src ^ 1] + row;
    uint16_t *ya = a.ace[src ^ 1] + row;
    if constexpr (kLds) {
        extern __shared__ int32_t girth_lds[];   // coefficients [E * M], then aces [E * M] (16 bits each)
        int32_t *lc = girth_lds;
        uint16_t *la = reinterpret_cast<uint16_t *>(girth_lds + (size_t)E * M);
        for (int i = (int)threadIdx.x; i < E * M; i += (int)blockDim.x) {
            lc[i] = bc[i];
            la[i] = ba[i];
        }
        __syncthreads();
        bc = lc;
        ba = la;
    }
    const int32_t *pb = a.pred_begin + (size_t)c * (a.Emax + 1);
    const int32_t *pred = a.pred + (size_t)c * a.pred_stride * 3;
    const int lanes = a.lanes, groups = (int)blockDim.x / lanes, lane = (int)threadIdx.x % lanes;
    bool overflow = false;
    for (int J = (int)threadIdx.x / lanes; J < E; J += groups) {
        const int p0 = pb[J], p1 = pb[J + 1];
        for (int h = lane; h < M; h += lanes) {
            int32_t sum = 0, amin = 0x7fffffff;
            for (int p = p0; p < p1; ++p) {
                const int j = pred[3 * p], as = pred[3 * p + 2];
                int r = h - pred[3 * p + 1];
                r += r < 0 ? M : 0;
                const int32_t v = bc[j * M + r];
                if (v != 0) {
                    const int32_t s = (int32_t)((uint32_t)sum + (uint32_t)v);
                    overflow |= sum >= 0 && v >= 0 && s < 0;
                    sum = s;
                    amin = min(amin, (int32_t)ba[j * M + r] + as);
                }
            }
            yc[J * M + h] = sum;
            ya[J * M + h] = amin == 0x7fffffff ? (uint16_t)0 : (uint16_t)amin;
        }
    }
    if (overflow) atomicOr(&st[kOverflow], 1);
}

// S[d], SA[d], the removal of the diagonal's constant terms and the stop rule of one code; `buf` holds the step's result
__global__ void __launch_bounds__(256) trace_kernel(Args a, int buf, int d) {
    const int c = blockIdx.x;
    int32_t *st = a.state + (size_t)c * kState;
    if (st[kDone]) return;
    const int E = a.E[c], M = a.M;
    __shared__ unsigned long long s_sum;
    __shared__ int s_min;
    if (threadIdx.x == 0) { s_sum = 0; s_min = 0x7fffffff; }
    __syncthreads();
    for (int I = (int)threadIdx.x; I < E; I += (int)blockDim.x) {
        const size_t at = (size_t)c * code_elems(a.Emax, M) + ((size_t)I * a.Emax + I) * M;
        int32_t *pc = a.coef[buf] + at;
        uint16_t *pa = a.ace[buf] + at;
        const int32_t v = pc[0];
        if (v == 0) continue;
        atomicAdd(&s_sum, (unsigned long long)(long long)v);
        atomicMin(&s_min, (int)pa[0]);
        uint16_t prev = pa[0];   // :201-207
        pc[0] = 0;
        pa[0] = 0;
        for (int h = 1; h < M; ++h)
            if (pc[h] != 0) {
                const uint16_t t = pa[h];
                pa[h] = prev;
                prev = t;
            }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const long long wide = (long long)s_sum;
    const int32_t S = (int32_t)(uint32_t)s_sum, SA = s_min == 0x7fffffff ? 0 : s_min;
    if (wide > 0x7fffffffLL) st[kOverflow] = 1;
    a.S[(size_t)c * a.gmax + d] = S;
    a.SA[(size_t)c * a.gmax + d] = SA;
    int ok = 1;
    if (S > 0) {   // :250-272
        const int cnt = st[kCnt];
        ok = 0;
        if (a.max_spec && S / (d + 1) <= a.max_spec[cnt]) ok = 1;
        if (a.min_ace && SA / 2 >= a.min_ace[cnt]) ok = 1;
        if (!ok || cnt + 1 == a.gtarget) st[kDone] = 1;
        if (ok) st[kCnt] = cnt + 1;
    }
    st[kOk] = ok;
}

#endif  // __HIPCC__

}  // namespace ldpc_girth
