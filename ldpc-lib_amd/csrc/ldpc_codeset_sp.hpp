// Code-set kernels of the two flooding sum-product decoders: sum_prod_decod_qc_lm (SP_DEC, id 1, decoders.cpp:1923-2185; likelihood
// ratios) and sum_prod_gf2_decod_qc_lm (ASP_DEC, id 2, decoders.cpp:2324-2581; probabilities) on work item (c, w) of a code set
// (ldpc_codeset.hpp).  The arithmetic is sp_flood_kernel's (ldpc_sumprod.hpp) and asp_global_kernel's (ldpc_global.hpp), statement by
// statement: the same products in the same order, comparison-form mind / maxd, ldpc_spec::exp_glibc for the input stage, plain IEEE
// divisions, contraction off.  What differs is where the state lives and how a frame is dealt over the lanes.
//
// Table record of a code (the IASP record, for both decoders): row_start[rh+1] | edges[ne] | cw2 | col_start[nh+1] | col_edges[ne],
// col_edges = (row-major edge index << 16) | shift with rows ascending.  It is read through the constant address space; every index
// below is wave-uniform, so every table access is a scalar load.
//
// Launch shape -- a pure function of (M, nh) and of the image:
//   * L lanes serve one block column or block row at a time: L = 64 for M <= 64 (lane = n * F + f: F frames side by side, as in the
//     other set kernels), L = 64 * ceil(M / 64) for M > 64 (F = 1);
//   * a workgroup has G = min(kSpCodesThreads / L, nh) such groups (sp_codes_groups): group g works on block columns g, g + G, ... in the
//     variable phases and on block rows g, g + G, ... in the check phases, with a workgroup barrier between the phases.  A group is
//     whole wavefronts, so the block row / column of a wave is uniform.  Nothing is kept per block row or column in registers;
//   * F = min(floor(64 / M), the largest count whose image fits 160 KiB) (sp_codes_frames): 16 x 32 at M = 64 with 112 circulants is one
//     frame of 82 176 bytes served by 16 waves; at M = 126 one frame of 161 808 bytes served by 8 groups of two waves.
// LDS image per frame, interleaved over the F frames of a workgroup (index * F + f):
//   SP : ZZ[ne_max][M] per-edge messages (indexed by the VARIABLE's position, as sp_flood_kernel), yd[N] channel likelihood ratios,
//        S[R] check products, the hard decisions as bits: 8 * (ne_max * M + N + R) + 4 * ceil(N / 32) bytes;
//   ASP: ST[ne_max][M] per-edge state (indexed by the CHECK's position, as asp_global_kernel), pch[N] channel probabilities, the hard
//        decisions as bits: 8 * (ne_max * M + N) + 4 * ceil(N / 32) bytes;
//   F images rounded up to 16 bytes, then 16 bytes of vote flags.
// There is no a-posteriori array.  SP forms soft in a register in phase C, keeps its hard bit, and recomputes yd * ZZ[e0] * ZZ[e1] ...
// (rows ascending: the operands and the order of `soft *= A`) for d_soft at the end.  ASP forms `so` in a register in the symbol phase,
// keeps its hard bit and stores the value straight to d_soft every iteration when the caller asked for it.
// The hard bits of a word may belong to block columns of different waves: they are set and cleared with LDS atomics.
// A converged frame (and a frame beyond B, which decodes an all-zero LLR word and converges at the input) stores nothing more.
#pragma once

#include "ldpc_codeset.hpp"
#include "ldpc_sumprod.hpp"   // sp_mind, sp_maxd

namespace ldpc {

constexpr int kSpCodesThreads = 1024;
constexpr size_t kSpCodesLdsLimit = 160 * 1024;

__host__ __device__ inline int sp_codes_lanes(int M) { return M > 64 ? ((M + 63) / 64) * 64 : 64; }
__host__ __device__ inline int sp_codes_groups(int M, int nh) {
    const int g = kSpCodesThreads / sp_codes_lanes(M);
    return g < nh ? g : nh;
}
// one frame's image: SP (asp == false) or ASP
__host__ __device__ inline size_t sp_codes_frame_bytes(bool asp, int N, int R, int M, int ne_max) {
    return 8 * ((size_t)ne_max * M + (size_t)N + (asp ? 0 : (size_t)R)) + 4 * (((size_t)N + 31) / 32);
}
__host__ __device__ inline size_t sp_codes_image_bytes(bool asp, int F, int N, int R, int M, int ne_max) {   // in front of the vote flags
    return ((size_t)F * sp_codes_frame_bytes(asp, N, R, M, ne_max) + 15) & ~(size_t)15;
}
// frames per workgroup: floor(64 / M), fewer when their images do not fit; 1 also when one frame does not fit (the caller refuses that)
inline int sp_codes_frames(bool asp, int N, int R, int M, int ne_max) {
    int F = M > 64 ? 1 : 64 / M;
    while (F > 1 && sp_codes_image_bytes(asp, F, N, R, M, ne_max) + 16 > kSpCodesLdsLimit) --F;
    return F;
}

// What the two kernels share: the lane map, the image's bit array and the vote.
struct SpCodesLane {
    int G, g, n, f, F;
    bool valid;
};

template <bool MW>
__device__ __forceinline__ SpCodesLane sp_codes_lane(int M, int F) {
    SpCodesLane q;
    const int L = MW ? ((M + 63) >> 6) << 6 : 64;
    q.G = (int)blockDim.x / L;
    q.g = __builtin_amdgcn_readfirstlane((int)threadIdx.x / L);   // whole waves: uniform
    const int l = (int)threadIdx.x - q.g * L;
    q.F = MW ? 1 : F;
    if (MW) { q.n = l; q.f = 0; }
    else    { q.n = l / F; q.f = l - q.n * F; }
    q.valid = q.n < M;
    if (!q.valid) q.n = 0;   // computes on position 0, never stores, never votes
    return q;
}

__device__ __forceinline__ void sp_codes_set_bit(uint32_t *HB, int v, int F, int f, bool bit) {
    uint32_t *const wp = HB + (v >> 5) * F + f;
    if (bit) atomicOr(wp, 1u << (v & 31));
    else atomicAnd(wp, ~(1u << (v & 31)));
}

// "Which lanes' frames fail?" over the waves of a workgroup: the OR of the waves' ballots.  flag: two 64-bit masks used in turn; the one
// not in use is cleared behind the barrier, and at least one more barrier (a phase of the iteration) lies before its next use.
__device__ __forceinline__ unsigned long long sp_codes_vote(bool fail, int &turn, uint32_t *flag) {
    const unsigned long long b = __ballot(fail);
    uint32_t *const w = flag + 2 * turn;
    if ((threadIdx.x & 63) == 0) {
        if ((uint32_t)b) atomicOr(w, (uint32_t)b);
        if ((uint32_t)(b >> 32)) atomicOr(w + 1, (uint32_t)(b >> 32));
    }
    __syncthreads();
    const unsigned long long m = (unsigned long long)w[0] | ((unsigned long long)w[1] << 32);
    turn ^= 1;
    if (threadIdx.x == 0) { flag[2 * turn] = 0u; flag[2 * turn + 1] = 0u; }
    return m;
}

// the syndrome of the group's block rows over the hard bits (phase D of sp_flood_kernel; check_syndrome_thr :2274-2306)
__device__ __forceinline__ bool sp_codes_syndrome(const SpCodesLane &q, TabPtr rs, int rh, int M, const uint32_t *HB) {
    const int ed = rh + 1;
    uint32_t failw = 0;
    for (int j = q.g; j < rh; j += q.G) {
        const int e0 = rs[j], e1 = rs[j + 1];
        uint32_t sy = 0;
        for (int e = e0; e < e1; ++e) {
            const uint32_t d = (uint32_t)rs[ed + e];
            const int v = (int)(d >> 16) * M + rot_idx(q.n, (int)(d & 0xffffu), M);
            sy ^= HB[(v >> 5) * q.F + q.f] >> (v & 31);
        }
        failw |= sy & 1u;
    }
    return q.valid && failw;
}

// iters and the hard words of a live frame, from the bit array
__device__ __forceinline__ void sp_codes_outputs(const DecArgs &a, const SpCodesLane &q, const uint32_t *HB, long long fr, int res) {
    if (q.g == 0 && q.n == 0 && a.iters) a.iters[fr] = res;
    if (a.hard) {
        for (int wd = q.g * a.M + q.n; wd < a.hard_words; wd += q.G * a.M) {
            uint32_t bits = HB[wd * q.F + q.f];
            if (wd == a.hard_words - 1 && (a.N & 31)) bits &= (1u << (a.N & 31)) - 1u;   // nobody wrote the bits beyond N
            a.hard[fr * a.hard_words + wd] = bits;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// SP_DEC: the four phases of sp_flood_kernel (A variable lanes, B check lanes, C variable lanes, D syndrome)
// ---------------------------------------------------------------------------------------------------------
template <bool MW>
__global__ void __launch_bounds__(kSpCodesThreads) sp_flood_codes_kernel(const CodesetArgs s) {
    extern __shared__ double lds[];
    int w;
    const DecArgs a = codeset_view(s, w);
    const int M = a.M, N = a.N, rh = a.rh, nh = a.nh, R = rh * M;
    const SpCodesLane q = sp_codes_lane<MW>(M, a.F);
    const int F = q.F, G = q.G, g = q.g, n = q.n, f = q.f;
    const bool valid = q.valid;
    const TabPtr rs = tab_ptr(a.row_start);                                         // the code's record; its parts by offset
    const int ne = rs[rh];
    const int ed = rh + 1, cs = ed + ne + 1, ce = cs + nh + 1;                      // edges[], col_start[], col_edges[]
    double *const ZZ = lds, *const yd = ZZ + (size_t)s.ne_max * M * F, *const S = yd + (size_t)N * F;
    uint32_t *const HB = reinterpret_cast<uint32_t *>(S + (size_t)R * F);
    uint32_t *const flag = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(lds) + sp_codes_image_bytes(false, F, N, R, M, s.ne_max));
    const unsigned long long per = MW ? 0ull : slot_mask(F);
    const long long fr = (long long)w * F + f;
    const bool live = valid && fr < a.B;
    auto mine = [&](unsigned long long m) { return MW ? m != 0ull : ((m >> f) & per) != 0ull; };

    if (threadIdx.x == 0) { flag[0] = 0u; flag[1] = 0u; flag[2] = 0u; flag[3] = 0u; }
    for (int k = g; k < nh; k += G) {
        const int v = k * M + n;
        const double yl = sp_maxd(sp_mind(live ? a.llr[fr * N + v] : 0.0, 20.0), -20.0);   // :1949 INPUT_LIMIT
        const double y = ldpc_spec::exp_glibc(yl);
        if (valid) { yd[v * F + f] = y; sp_codes_set_bit(HB, v, F, f, y < 1.0); }
    }
    if (valid)
        for (int e = g; e < ne; e += G) ZZ[(e * M + n) * F + f] = 1.0;              // :1957-1959
    __syncthreads();

    int turn = 0;
    bool done = false;
    int res = -a.maxiter;
    unsigned long long m = sp_codes_vote(sp_codes_syndrome(q, rs, rh, M, HB), turn, flag);   // :1964-2002
    if (!mine(m)) { done = true; res = 0; }
    for (int iter = 0; m != 0ull && iter < a.maxiter; ++iter) {
        const bool wr = !done && valid;
        // ---- phase A: AA_u = yd * zz[0] * .. * zz[u-1] * zz[u+1] * .. in that order (:2027-2041), prefix in a register, tail from
        // the entries not yet overwritten
        for (int k = g; k < nh; k += G) {
            const int c0 = rs[cs + k], c1 = rs[cs + k + 1];
            double prefix = yd[(k * M + n) * F + f];
            for (int u = c0; u < c1; ++u) {
                const int zi = ((int)((uint32_t)rs[ce + u] >> 16) * M + n) * F + f;
                const double orig = ZZ[zi];
                double AA = prefix;
                for (int x = u + 1; x < c1; ++x) AA *= ZZ[((int)((uint32_t)rs[ce + x] >> 16) * M + n) * F + f];
                if (wr) ZZ[zi] = (AA - 1) / (AA + 1);                               // :2044
                prefix *= orig;
            }
        }
        __syncthreads();
        // ---- phase B
        for (int j = g; j < rh; j += G) {
            double sp = 1.0;                                                        // :2010
            for (int e = rs[j]; e < rs[j + 1]; ++e)
                sp *= ZZ[(e * M + rot_idx(n, (int)((uint32_t)rs[ed + e] & 0xffffu), M)) * F + f];   // :2047-2050
            if (wr) S[(j * M + n) * F + f] = sp;
        }
        __syncthreads();
        // ---- phase C
        for (int k = g; k < nh; k += G) {
            const int c0 = rs[cs + k], c1 = rs[cs + k + 1];
            const int v = k * M + n;
            double soft = yd[v * F + f];                                            // :2011
            int j = 0;
            for (int u = c0; u < c1; ++u) {
                const uint32_t d = (uint32_t)rs[ce + u];
                const int e = (int)(d >> 16), c = (int)(d & 0xffffu);
                while (rs[j + 1] <= e) ++j;                                         // the block row of edge e; rows ascend along a column
                int nn = n - c; if (nn < 0) nn += M;                                // rotate by M-circ (:2113)
                const int zi = (e * M + n) * F + f;
                double A = S[(j * M + nn) * F + f] / ZZ[zi];
                A = (1 + A) / (1 - A);
                A = sp_maxd(sp_mind(A, 1.9e+8), -5.2e-9);                           // :2120 (negative lower clamp is upstream's)
                if (wr) ZZ[zi] = A;
                soft *= A;
            }
            if (wr) sp_codes_set_bit(HB, v, F, f, soft < 1.0);
        }
        __syncthreads();
        // ---- phase D
        m = sp_codes_vote(sp_codes_syndrome(q, rs, rh, M, HB), turn, flag);
        if (!done && !mine(m)) { done = true; res = iter + 1; }                     // :2151-2166
    }
    if (!live) return;
    sp_codes_outputs(a, q, HB, fr, res);
    if (a.soft_out) {                                                               // what `soft *= A` left behind, formed again
        for (int k = g; k < nh; k += G) {
            const int v = k * M + n;
            double soft = yd[v * F + f];
            for (int u = rs[cs + k]; u < rs[cs + k + 1]; ++u) soft *= ZZ[((int)((uint32_t)rs[ce + u] >> 16) * M + n) * F + f];
            a.soft_out[fr * N + v] = soft;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// ASP_DEC: asp_global_kernel's check phase (map_bin :2191-2228), symbol phase (the general branch :2482-2556, or upstream's own branch
// :2431-2480 for a code whose block columns all hold two circulants, unclamped) and check_syndrome_thr at 0.5.  map_bin's forward
// products are VGPRs with static indices (the pass is unrolled RWM times under the wave-uniform predicate i < rw); the backward
// product is one register while slot i is finished, and P(i) = 1 - 2 * state is formed again from the slot that is about to be
// overwritten.
// ---------------------------------------------------------------------------------------------------------
template <int RWM, bool MW>
__global__ void __launch_bounds__(kSpCodesThreads) asp_flood_codes_kernel(const CodesetArgs s) {
    extern __shared__ double lds[];
    int w;
    const DecArgs a = codeset_view(s, w);
    const int M = a.M, N = a.N, rh = a.rh, nh = a.nh;
    const SpCodesLane q = sp_codes_lane<MW>(M, a.F);
    const int F = q.F, G = q.G, g = q.g, n = q.n, f = q.f, MF = M * F;
    const bool valid = q.valid;
    const TabPtr rs = tab_ptr(a.row_start);
    const int ne = rs[rh];
    const int ed = rh + 1, cs = ed + ne + 1, ce = cs + nh + 1;
    const bool cw2 = rs[ed + ne] != 0;
    double *const ST = lds, *const pch = ST + (size_t)s.ne_max * M * F;
    uint32_t *const HB = reinterpret_cast<uint32_t *>(pch + (size_t)N * F);
    uint32_t *const flag = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(lds) + sp_codes_image_bytes(true, F, N, 0, M, s.ne_max));
    const unsigned long long per = MW ? 0ull : slot_mask(F);
    const long long fr = (long long)w * F + f;
    const bool live = valid && fr < a.B;
    auto mine = [&](unsigned long long m) { return MW ? m != 0ull : ((m >> f) & per) != 0ull; };
    auto back = [&](int t, int c) { const int x = t - c; return x < 0 ? x + M : x; };   // the check of variable t on an edge of shift c
    double *const soft_fr = (a.soft_out && live) ? a.soft_out + fr * N + n : nullptr;

    if (threadIdx.x == 0) { flag[0] = 0u; flag[1] = 0u; flag[2] = 0u; flag[3] = 0u; }
    for (int k = g; k < nh; k += G) {                                               // :2351-2379
        const int v = k * M + n;
        const double x = (live ? a.llr[fr * N + v] : 0.0) * 0.5;
        const double y = sp_maxd(sp_mind(x, 20.0), -20.0);
        const double x0 = ldpc_spec::exp_glibc(y), x1 = ldpc_spec::exp_glibc(-y);
        const double p = x1 / (x0 + x1);
        if (valid) {
            pch[v * F + f] = p;
            sp_codes_set_bit(HB, v, F, f, p > 0.5);
            if (soft_fr) soft_fr[k * M] = p;
            for (int c = rs[cs + k]; c < rs[cs + k + 1]; ++c) {                     // state <- rotated channel probability
                const uint32_t d = (uint32_t)rs[ce + c];
                ST[((int)(d >> 16) * M + back(n, (int)(d & 0xffffu))) * F + f] = p;
            }
        }
    }
    __syncthreads();

    int turn = 0;
    bool done = false;
    int res = -a.maxiter;
    unsigned long long m = sp_codes_vote(sp_codes_syndrome(q, rs, rh, M, HB), turn, flag);   // :2393-2399
    if (!mine(m)) { done = true; res = 0; }                                         // a codeword at the input: no iteration, 0
    for (int steps = 0; m != 0ull && steps < a.maxiter;) {
        const bool wr = !done && valid;
        for (int j = g; j < rh; j += G) {                                           // map_bin :2191-2228, row weights 2 .. RWM
            const int e0 = rs[j], rw = rs[j + 1] - e0;
            int z = (e0 * M + n) * F + f;                                           // slot i of the check: ST[z], z walks up, then down
            double SF[RWM];
            double fw = 0.0;
#pragma unroll
            for (int i = 0; i < RWM; ++i) {                                         // forward products; SF[rw - 1] is never read
                SF[i] = 0.0;
                if (i < rw) {
                    const double P = 1 - 2 * ST[z];
                    z += MF;
                    fw = i == 0 ? P : P * fw;
                    SF[i] = fw;
                }
            }
            double sb = 0.0;                                                        // backward: SB[i + 1] while slot i is written
#pragma unroll
            for (int i = RWM - 1; i >= 0; --i) {
                if (i < rw) {
                    z -= MF;
                    const double P = 1 - 2 * ST[z];
                    const double sfp = SF[i > 0 ? i - 1 : 0];
                    double out;
                    if (i == 0) out = (1 - sb) / 2;
                    else if (i == rw - 1) { out = (1 - sfp) / 2; sb = P; }          // SF[rw - 2]
                    else { out = (1 - sfp * sb) / 2; sb = P * sb; }
                    if (wr) ST[z] = out;
                }
            }
        }
        __syncthreads();
        if (cw2) {
            for (int k = g; k < nh; k += G) {                                       // :2431-2480: from the channel value and the OTHER edge, unclamped
                const int c0 = rs[cs + k];
                const uint32_t g0 = (uint32_t)rs[ce + c0], g1 = (uint32_t)rs[ce + c0 + 1];   // rows ascending
                const int v = k * M + n;
                const int z0 = ((int)(g0 >> 16) * M + back(n, (int)(g0 & 0xffffu))) * F + f;
                const int z1 = ((int)(g1 >> 16) * M + back(n, (int)(g1 & 0xffffu))) * F + f;
                const double d0 = ST[z0], d1 = ST[z1];                              // data0[k], data1[k] :2449-2450
                double p1 = pch[v * F + f];
                double q10 = p1, q11 = p1, p0 = 1.0 - p1, q00 = 1.0 - p1, q01 = 1.0 - p1;   // :2454-2459
                q10 = q10 * d1;                                                     // :2461-2466
                q00 = q00 * (1 - d1);
                q11 = q11 * d0;
                q01 = q01 * (1 - d0);
                p1 = q10 * d0;
                p0 = q00 * (1 - d0);
                const double so = p1 / (p0 + p1);                                   // :2469
                if (wr) {
                    sp_codes_set_bit(HB, v, F, f, so > 0.5);
                    if (soft_fr) soft_fr[k * M] = so;
                    ST[z0] = q10 / (q10 + q00);                                     // :2471
                    ST[z1] = q11 / (q11 + q01);                                     // :2472
                }
            }
        } else {
            for (int k = g; k < nh; k += G) {                                       // symbol nodes + local data update :2482-2556
                const int c0 = rs[cs + k], c1 = rs[cs + k + 1];
                const int v = k * M + n;
                const double pc = pch[v * F + f];
                double P1 = pc, P0 = 1 - pc;
                for (int c = c0; c < c1; ++c) {                                     // rows ascending
                    const uint32_t d = (uint32_t)rs[ce + c];
                    const double x = ST[((int)(d >> 16) * M + back(n, (int)(d & 0xffffu))) * F + f];
                    P1 *= x;
                    P0 *= 1 - x;
                }
                const double so = P1 / (P0 + P1);
                if (wr) {
                    sp_codes_set_bit(HB, v, F, f, so > 0.5);
                    if (soft_fr) soft_fr[k * M] = so;
                }
                for (int c = c0; c < c1; ++c) {
                    const uint32_t d = (uint32_t)rs[ce + c];
                    const int zi = ((int)(d >> 16) * M + back(n, (int)(d & 0xffffu))) * F + f;
                    const double sos = ST[zi];
                    const double p1 = so / sos;
                    const double p0 = (1 - so) / (1 - sos);
                    const double dd = p1 / (p1 + p0);
                    if (wr) ST[zi] = sp_maxd(sp_mind(dd, 1.0 - 0.000001), 0.000001);   // SP_DEC_MAX_VAL / SP_DEC_MIN_VAL :96-97
                }
            }
        }
        __syncthreads();
        m = sp_codes_vote(sp_codes_syndrome(q, rs, rh, M, HB), turn, flag);         // :2566
        ++steps;
        if (!done && !mine(m)) { done = true; res = steps; }                        // else -steps = -maxiter at the end
    }
    if (!live) return;
    sp_codes_outputs(a, q, HB, fr, res);
}

}  // namespace ldpc
