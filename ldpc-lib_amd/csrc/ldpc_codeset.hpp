// ldpc_codeset.hpp -- C candidate codes of one shape (rh x nh, lifting M) x B frames in ONE launch (gfx950).
//
// The caller is a code search: thousands of base matrices with the same rh, nh and M, each scored by a short Monte-Carlo run over
// the SAME received words.  The table-driven resident kernels of ldpc_kernels.hpp already read the graph from memory, so a code
// set is one more level of indexing:
//   * graph data: one concatenated int32 table; code c owns tab[code_off[c] ...] = row_start[rh+1] (relative to its own edge
//     list) followed by its edges[] in the (block column << 16) | shift row-major format of DecArgs;
//   * work item (c, w): workgroup blockIdx.x = c * blocks_per_code + w decodes frames w*F .. w*F+F-1 of code c.  A packed wave
//     (M <= 64, F = floor(64/M) frames) never mixes codes: the last wave of a code is partly filled when B % F != 0.  The code
//     index comes from blockIdx alone, so the table addresses are wave-uniform and the table loads stay scalar loads;
//   * LLRs: shared [B][N] (llr_code_stride = 0: every code decodes the same B received words; the LLR traffic of C separate
//     runs shrinks to 1/C and the frames of different codes hit the same lines in L2) or per code [C][B][N];
//   * outputs: hard [C][B][hard_words], iters [C][B], soft [C][B][N];
//   * a launch may cover a subset of the codes: code_list[n_active] names the code of every slot blockIdx.x / blocks_per_code (null =
//     the identity).  The graph table and the per-code LLR slice follow the code, the outputs follow the slot ([n_active][B]...).
//   * an SNR grid of P points over one noise draw makes the entries of the list ITEMS i = p * C + c: the table follows the code c, the
//     received words follow the point p (llr + p * llr_point_stride).  With one point an item is its code and the stride is 0.
// The decoder bodies compute what ms_flood_kernel / lms_layered_kernel / tasp_global_kernel / iasp_global_kernel / lche_global_kernel /
// ims_flood_kernel compute (fp64, reference operation order, contraction off; IASP: the integer arithmetic of ldpc_spec::iasp; LCHE:
// ldpc_spec::lche; IMS: integers behind a quantiser that runs once per received word); only the frame index and the table base differ
// (and, for TDMP, IASP, LCHE and IMS, where the state lives), so the results are bit-identical to a single-code context.
// The two flooding sum-product decoders (ids 1 and 2) deal a frame over several waves and live in ldpc_codeset_sp.hpp.
// Structure: the flooding and the layered min-sum set kernels are nothing but codeset_view and the body their single-code kernel runs
// (ms_flood_body, lms_layered_body).  The IASP and integer min-sum set kernels are codeset_view, their own state, and the pieces that
// ldpc_kernels.hpp holds once for every frame-resident kernel -- frame_lane, edge_idx, row_syndrome, stop_vote / stop_all, frame_outputs;
// the integer min-sum kernel calls ims_flood_kernel's row passes (ims_row_add, ims_row_scan) on its halfword image.  Where a shared piece
// cost registers or time its kernel kept its own: iasp_codes_kernel writes its outputs itself (the reason stands in the kernel),
// lms_layered_body has its own syndrome, and tasp_layered_codes_kernel and lche_layered_codes_kernel use none of the pieces: with them
// they were 0.7 % and 1.0 - 1.5 % slower (profiles/kernel_refactor_time.txt).
#pragma once

#include "ldpc_frontend.hpp"   // packed_word_errors, wave_sum_pair, ErrorTally
#include "ldpc_kernels.hpp"
#include "ldpc_spec.hpp"   // exp_glibc, iasp, lche

namespace ldpc {

struct CodesetArgs {
    const double *llr;        // [B][N] (llr_code_stride == 0) or [C][B][N] (llr_code_stride == B * N)
    uint32_t *hard;           // [C][B][hard_words] or null
    int32_t *iters;           // [C][B] or null
    double *soft_out;         // [C][B][N] or null
    const int32_t *tab;       // concatenated per-code tables
    const int32_t *code_off;  // [C] offset of code c's row_start[] in tab
    const int32_t *code_list; // [grid / blocks_per_code] the code of every slot, or null: slot s decodes code s
    long long B;              // frames per code
    long long llr_code_stride;
    int blocks_per_code;      // ceil(B / F)
    int C, rh, nh, M, N, F, maxiter, hard_words;
    double alpha;
    int ne_max;               // tasp_layered_codes_kernel, iasp_codes_kernel, lche_layered_codes_kernel: the largest edge count of the set (size of the per-edge LDS image)
    long long llr_point_stride;   // an SNR grid: the list names ITEMS p * C + c and point p reads llr + p * llr_point_stride; one point: 0
};

// The graph table is read-only for the whole launch and its addresses are wave-uniform: reading it through the constant address
// space makes every table access a scalar load, in the single-wave kernels too (through a plain global pointer the compiler proves
// that only for the multi-wave instances and falls back to 64 identical vector loads otherwise).
typedef const __attribute__((address_space(4))) int32_t *TabPtr;
__device__ __forceinline__ TabPtr tab_ptr(const void *p) { return (TabPtr)(uintptr_t)p; }

// The single-code argument block of work item (c, w): every pointer moved to code c's slice.  All values are functions of
// blockIdx.x and kernel arguments only (wave-uniform); the list of codes is read like the table, so c stays in a scalar register.
__device__ __forceinline__ DecArgs codeset_view(const CodesetArgs &s, int &w) {
    const int slot = blockIdx.x / s.blocks_per_code;
    w = blockIdx.x - slot * s.blocks_per_code;
    const unsigned item = s.code_list ? (unsigned)tab_ptr(s.code_list)[slot] : (unsigned)slot;
    const unsigned p = item / (unsigned)s.C;      // the point of an SNR grid; 0 without one
    const int c = (int)(item - p * (unsigned)s.C);
    const long long fo = (long long)slot * s.B;   // first frame of the slot in the [n_active][B] outputs
    DecArgs a{};
    a.llr = s.llr + (long long)c * s.llr_code_stride + (long long)p * s.llr_point_stride;
    a.hard = s.hard ? s.hard + fo * s.hard_words : nullptr;
    a.iters = s.iters ? s.iters + fo : nullptr;
    a.soft_out = s.soft_out ? s.soft_out + fo * s.N : nullptr;
    a.row_start = s.tab + tab_ptr(s.code_off)[c];
    a.edges = reinterpret_cast<const uint32_t *>(a.row_start + s.rh + 1);
    a.B = s.B; a.rh = s.rh; a.nh = s.nh; a.M = s.M; a.N = s.N; a.F = s.F; a.maxiter = s.maxiter; a.hard_words = s.hard_words;
    a.alpha = s.alpha;
    return a;
}

// ---------------------------------------------------------------------------------------------------------
// Flooding normalised min-sum: ms_flood_kernel's body (ldpc_kernels.hpp; decoders.cpp:4554-4767) on work item (c, w)
// ---------------------------------------------------------------------------------------------------------
template <int RHM, int NHM, bool MW>
__global__ void __launch_bounds__(MW ? 512 : 64) ms_flood_codes_kernel(const CodesetArgs s) {
    extern __shared__ double lds[];
    int w;
    const DecArgs a = codeset_view(s, w);
    ms_flood_body<RHM, NHM, MW>(a, lds, w, tab_ptr(a.row_start), tab_ptr(a.edges));
}

// ---------------------------------------------------------------------------------------------------------
// Layered offset min-sum: lms_layered_kernel's body (ldpc_kernels.hpp; decoders.cpp:5064-5425) on work item (c, w)
// ---------------------------------------------------------------------------------------------------------
template <int RHM, bool MW>
__global__ void __launch_bounds__(MW ? 512 : 64) lms_layered_codes_kernel(const CodesetArgs s) {
    extern __shared__ double lds[];
    int w;
    const DecArgs a = codeset_view(s, w);
    lms_layered_body<RHM, MW>(a, lds, w, tab_ptr(a.row_start), tab_ptr(a.edges));
}

// ---------------------------------------------------------------------------------------------------------
// TDMP sum-product (decoder 7): tdmp_sum_prod_gf2_decod_qc_lm (decoders.cpp:2584-2744, map_bin :2191-2228, check_syndrome_thr at
// 0.5) on work item (c, w), written as tasp_global_kernel (ldpc_global.hpp) writes it -- same expressions, same operand order, the
// compiler's correctly rounded division -- with the state on chip instead of in a workspace:
//   * LDS: the a-posteriori probabilities post[N][F], then the per-edge state Z[ne_max][M][F] (e = edge index inside the frame's own
//     code; Z[e][n] is only ever touched by lane n), then the vote flag: F * 8 * (N + ne_max * M) + 16 bytes;
//   * one lane owns one check of the current layer.  Y[] (the layer's rho values) and map_bin's forward products SF[] are VGPRs:
//     the passes over the row are unrolled RWM times under a predicate on the (wave-uniform) row weight, so the arrays have static
//     indices.  The backward products need no array: the second pass runs from the last edge to the first, carries SB[i + 1] in
//     one register and finishes edge i (q, clamp, Z, gamma) on the way.  The edges of a row lie in distinct block columns, so the
//     order in which a row's a-posteriori values are written does not matter; all of them are read before the first is written.
//   * the two fp64 divisions per edge and layer are chains of about 30 dependent instructions, and the LDS image leaves room for
//     few waves per CU (one workgroup at 16 x 32, M = 126), so nothing hides their latency but the row's other edges: both passes
//     work on groups of G = 4 edges in one basic block (the predicate is per group; slots beyond the row's end recompute its
//     last edge and store nowhere).
// A converged frame of a packed wave (and a frame beyond B) stores nothing more: its state and outputs stay as they were.
// ---------------------------------------------------------------------------------------------------------
template <int RWM, bool MW>
__global__ void __launch_bounds__(MW ? 512 : 64) tasp_layered_codes_kernel(const CodesetArgs s) {
    extern __shared__ double lds[];
    int w;
    const DecArgs a = codeset_view(s, w);
    const TabPtr rs = tab_ptr(a.row_start), ed = tab_ptr(a.edges);
    const int M = a.M, F = a.F, N = a.N, rh = a.rh, nh = a.nh;
    double *const post = lds, *const Z = lds + (size_t)N * F;
    int *const sh_flag = (int *)(Z + (size_t)s.ne_max * M * F);
    const int spare = s.ne_max * M * F + 1;                                         // index into Z of the second half of the flag's 16 bytes
    constexpr int G = 4;                                                            // edges of a row worked on side by side
    static_assert(RWM % G == 0, "tasp_layered_codes_kernel: whole groups");
    const double T = 0.0001, TT = 0;                                                // :2597-2598
    int n, f;
    const bool valid = lane_map<MW>(F, M, n, f);
    const unsigned long long per = MW ? 0ull : slot_mask(F);
    const long long fr = (long long)w * F + f;
    const bool inb = fr < a.B;
    const bool live = valid && inb;
    const int ne = rs[rh];

    if (valid) {
        for (int k = 0; k < nh; ++k) {                                              // :2611-2618
            double p = 0.5;
            if (live) {
                const double x = a.llr[fr * N + k * M + n] * 0.5;
                const double y = x < 20.0 ? (x < -20.0 ? -20.0 : x) : 20.0;         // maxd(mind(x, INPUT_LIMIT), -INPUT_LIMIT)
                const double e0 = ldpc_spec::exp_glibc(y), e1 = ldpc_spec::exp_glibc(-y);
                p = e1 / (e0 + e1);
            }
            post[(k * M + n) * F + f] = p;
        }
        for (int e = 0; e < ne; ++e) Z[(e * M + n) * F + f] = 0.5;                  // :2637
    }
    if (MW) __syncthreads();

    auto syndrome_fail = [&]() -> bool {                                            // check_syndrome_thr :2274-2306, thr 0.5
        uint32_t sy = 0, failw = 0;
        for (int j = 0; j < rh; ++j) {
            const int e0 = rs[j], e1 = rs[j + 1];
            sy = 0;
            for (int e = e0; e < e1; ++e) {
                const uint32_t d = (uint32_t)ed[e];
                const int k = d >> 16, c = d & 0xffffu;
                sy ^= (uint32_t)(post[(k * M + rot_idx(n, c, M)) * F + f] > 0.5);
            }
            failw |= sy;
        }
        return valid && failw;
    };

    bool done = !inb;
    int res = -a.maxiter;
    bool frame_fail = frame_vote<MW>(syndrome_fail(), F, f, per, sh_flag);          // :2653-2660
    if (!done && !frame_fail) { done = true; res = 0; }                             // a codeword at the input: no iteration, 0
    for (int steps = 0; steps < a.maxiter;) {
        if (MW) { if (done) break; }
        else if (__all(done)) break;
        const bool wr = !done && valid;
        for (int j = 0; j < rh; ++j) {                                              // layers in sequence (:2668)
            const int e0 = rs[j], rw = rs[j + 1] - e0;
            double Y[RWM], SF[RWM];
#pragma unroll
            for (int i = 0; i < RWM; ++i) { Y[i] = 0.0; SF[i] = 0.0; }
            double sf = 0.0;
#pragma unroll
            for (int g0 = 0; g0 < RWM; g0 += G) {                                   // :2676-2697 and map_bin's forward products
                if (g0 < rw) {
                    double v[G];
#pragma unroll
                    for (int u = 0; u < G; ++u) {                                   // G independent chains; slots beyond the row repeat its last edge
                        const int i = g0 + u < rw ? g0 + u : rw - 1;
                        const uint32_t d = (uint32_t)ed[e0 + i];
                        const int k = d >> 16, c = d & 0xffffu;
                        const double x = post[(k * M + rot_idx(n, c, M)) * F + f];
                        const double aa = Z[((e0 + i) * M + n) * F + f];
                        double t = x * (1.0 - aa) / (aa + x - 2.0 * aa * x);        // rho = gamma - lambda
                        if (t < TT) t = TT;
                        if (t > 1 - TT) t = 1 - TT;
                        v[u] = t;
                    }
#pragma unroll
                    for (int u = 0; u < G; ++u) {                                   // SF of a slot beyond the row is never read; its Y is 0
                        const int i = g0 + u;
                        Y[i] = i < rw ? v[u] : 0.0;
                        const double P = 1 - 2 * v[u];
                        sf = i == 0 ? P : P * sf;                                   // SF[i] = P[i] * SF[i - 1]
                        SF[i] = sf;
                    }
                }
            }
            // SB[i + 1] while edge i is finished.  It starts at 1.0 and a slot beyond the row has P = 1 - 2 * 0 = 1.0: x * 1.0 is x
            // exactly, so SB[rw - 1] = P[rw - 1] and q[rw - 1] = (1 - SF[rw - 2]) / 2 come out of the general expressions, bit for bit,
            // without a branch on the row weight inside a group.
            double sb = 1.0;
#pragma unroll
            for (int g0 = RWM - G; g0 >= 0; g0 -= G) {
                if (g0 < rw) {
                    double sbn[G], q[G], gm[G];
                    int zi[G], pi[G];
#pragma unroll
                    for (int u = 0; u < G; ++u) {
                        // Where the group's results go, settled before the divisions so that these stay one basic block.  A lane that
                        // must not store (a converged frame, a lane beyond M, a slot beyond the row) aims at the spare word behind the
                        // vote flag, which nothing reads.
                        const int i = g0 + u;
                        const bool ok = wr && i < rw;
                        const int ii = i < rw ? i : rw - 1;
                        const uint32_t d = (uint32_t)ed[e0 + ii];
                        const int k = d >> 16, c = d & 0xffffu;
                        zi[u] = ok ? ((e0 + ii) * M + n) * F + f : spare;
                        pi[u] = ok ? (k * M + rot_idx(n, c, M)) * F + f : N * F + spare;
                    }
#pragma unroll
                    for (int u = G - 1; u >= 0; --u) {                              // the backward products of the group, last edge first
                        const int i = g0 + u;
                        sbn[u] = sb;
                        const double P = 1 - 2 * Y[i];
                        sb = P * sb;                                                // SB[i] = P[i] * SB[i + 1]
                    }
#pragma unroll
                    for (int u = 0; u < G; ++u) {                                   // G independent chains again
                        const int i = g0 + u;
                        const double y = Y[i];
                        double t = sbn[u];                                          // i == 0: (1 - SB[1]) / 2
                        if (i > 0) t = SF[i > 0 ? i - 1 : 0] * sbn[u];                  // (1 - SF[i - 1] * SB[i + 1]) / 2
                        double qv = (1 - t) / 2;
                        if (qv < T) qv = T;                                         // :2703-2704
                        if (qv > 1.0 - T) qv = 1.0 - T;
                        q[u] = qv;
                        gm[u] = y * qv / (1.0 - y - qv + 2 * y * qv);               // :2707-2720 gamma = rho + lambda
                    }
#pragma unroll
                    for (int u = 0; u < G; ++u) { Z[zi[u]] = q[u]; post[pi[u]] = gm[u]; }
                }
            }
            if (MW) __syncthreads();
        }
        frame_fail = frame_vote<MW>(syndrome_fail(), F, f, per, sh_flag);           // :2723 (the value after the last layer)
        ++steps;
        if (!done && !frame_fail) { done = true; res = steps; }                     // else -steps = -maxiter at the end
    }
    // glob_outputs<1>: decword[k] = soft[k] > 0.5 (:2734), the a-posteriori probabilities as the soft output
    if (!live) return;
    if (n == 0 && a.iters) a.iters[fr] = res;
    if (a.hard) {
        for (int wd = n; wd < a.hard_words; wd += M) {
            uint32_t bits = 0;
            for (int b = 0; b < 32; ++b) {
                const int v = 32 * wd + b;
                if (v < N) bits |= (uint32_t)(post[v * F + f] > 0.5) << b;
            }
            a.hard[fr * a.hard_words + wd] = bits;
        }
    }
    if (a.soft_out)
        for (int k = 0; k < nh; ++k) a.soft_out[fr * N + k * M + n] = post[(k * M + n) * F + f];
}

// ---------------------------------------------------------------------------------------------------------
// Integer advanced sum-product (decoder 5): isum_prod_gf2_decod_qc_lm (decoders.cpp:3822-4121, imap_bin :2235-2271, icheck_syndrome
// :3772-3803) on work item (c, w), written as iasp_global_kernel (ldpc_global.hpp) writes it -- the same calls of ldpc_spec::iasp
// in the same order -- with the state on chip instead of in a workspace:
//   * table record of a code: row_start[rh+1] | edges[ne] | cw2 | col_start[nh+1] | col_edges[ne], col_edges = (slot << 16) | shift
//     with rows ascending, slot = the edge's row-major index inside its own code; cw2 = every block column holds two circulants;
//   * LDS, all u16 and interleaved over the F frames of a packed wave: the per-edge state ST[ne_max][M][F] (ST[e][n] belongs to check
//     n of edge e's block row), the a-posteriori word so[N][F], the channel word ych[N][F], then the vote flag:
//     F * 2 * (ne_max * M + 2 * N) bytes, rounded up to 16, + 16 (iasp_codes_words_bytes).  Lanes n and n + 1 of a frame share a dword
//     when F = 1, frames f and f + 1 of a check otherwise: consecutive lanes read and write consecutive halfwords either way;
//   * check phase: lane n owns check n of block row j, j in a run-time loop -- nothing of a row outlives it, so rh is unbounded.
//     P[] and imap_bin's forward products SF[] are VGPRs with static indices (the pass is unrolled RWM times under the wave-uniform
//     predicate i < rw); the backward product is one register while slot i is finished.  The rows touch disjoint edges;
//   * variable phase: lane t owns variable t of block column k, k in a run-time loop; the column's edges in a run-time loop (any
//     column weight), or upstream's own branch for a code whose columns all have weight 2 (the flag is per code, wave-uniform).
// A converged frame of a packed wave (and a frame beyond B) stores nothing more: its state and outputs stay as they were.
// ---------------------------------------------------------------------------------------------------------
__host__ __device__ inline size_t iasp_codes_words_bytes(int F, int M, int N, int ne_max) {   // the u16 arrays in front of the vote flag
    return ((size_t)F * 2 * ((size_t)ne_max * M + 2 * (size_t)N) + 15) & ~(size_t)15;
}

template <int RWM, bool MW>
__global__ void __launch_bounds__(MW ? 512 : 64) iasp_codes_kernel(const CodesetArgs s) {
    namespace I = ldpc_spec::iasp;
    extern __shared__ double lds[];
    int w;
    const DecArgs a = codeset_view(s, w);
    const int M = a.M, F = MW ? 1 : a.F, N = a.N, rh = a.rh, nh = a.nh;             // one frame per multi-wave workgroup
    const TabPtr rs = tab_ptr(a.row_start);                                         // the code's record; its parts by offset
    const int ne = rs[rh], MF = M * F;
    const int ed = rh + 1, cs = ed + ne + 1, ce = cs + nh + 1;                      // edges[], col_start[], col_edges[]
    const bool cw2 = rs[ed + ne] != 0;
    uint16_t *const ST = reinterpret_cast<uint16_t *>(lds);
    uint16_t *const so = ST + s.ne_max * M * F, *const ych = so + N * F;
    int *const sh_flag = reinterpret_cast<int *>(reinterpret_cast<char *>(lds) + iasp_codes_words_bytes(F, M, N, s.ne_max));
    const Lane l = frame_lane<MW>(F, M, a.B, w);
    const int n = l.n, f = l.f;
    const bool valid = l.valid;
    auto back = [&](int t, int c) { const int x = t - c; return x < 0 ? x + M : x; };   // the check of variable t on an edge of shift c
    // where the frame's outputs go, per lane (VGPRs): the scalar registers are the scarce ones in the loops below.  That is why this
    // kernel writes its outputs itself: frame_outputs forms these addresses at the end, from values that stay in scalar registers
    // through the iteration loop, and the kernel then spills scalar registers, which it does not do this way.
    uint32_t *const hard_fr = a.hard ? a.hard + l.fr * a.hard_words : nullptr;
    int32_t *const iters_fr = a.iters ? a.iters + l.fr : nullptr;
    double *const soft_fr = a.soft_out ? a.soft_out + l.fr * N + n : nullptr;

    if (valid) {                                                                    // :3858-3897
        for (int k = 0; k < nh; ++k) {
            const uint32_t q = I::q12(I::prior(l.live ? a.llr[l.fr * N + k * M + n] : 0.0));
            for (int c = rs[cs + k]; c < rs[cs + k + 1]; ++c) {                     // state <- rotated Q12 value
                const uint32_t d = (uint32_t)rs[ce + c];
                ST[((int)(d >> 16) * M + back(n, (int)(d & 0xffffu))) * F + f] = (uint16_t)q;
            }
            so[(k * M + n) * F + f] = ych[(k * M + n) * F + f] = (uint16_t)(q << 4);   // then the words, Q16
        }
    }
    if (MW) __syncthreads();

    auto syndrome_fail = [&]() -> bool {                                            // icheck_syndrome :3772-3803
        return valid && row_syndrome(rs, rs + ed, rh, l, M, F, [=](int i) { return (uint32_t)so[i] >> 15; }) != 0;
    };

    FrameStop st = stop_init(l, a.maxiter);
    stop_vote<MW>(st, syndrome_fail(), l, F, sh_flag, 0);                           // :3899-3906; a codeword at the input: no iteration, 0
    for (int steps = 0; steps < a.maxiter;) {
        if (stop_all<MW>(st)) break;
        const bool wr = !st.done && valid;
        for (int j = 0; j < rh; ++j) {                                              // imap_bin :2235-2271, row weights 2 .. RWM
            const int e0 = rs[j], rw = rs[j + 1] - e0;
            int z = (e0 * M + n) * F + f;                                           // slot i of the check: ST[z], z walks up, then down
            int P[RWM], SF[RWM];
            int fw = 0;
#pragma unroll
            for (int i = 0; i < RWM; ++i) {                                         // forward products; SF[rw - 1] is never read
                P[i] = 0; SF[i] = 0;
                if (i < rw) {
                    P[i] = I::chk_p(ST[z]);
                    z += MF;
                    fw = i == 0 ? P[i] : I::i16(I::chk_mul(P[i], fw));
                    SF[i] = fw;
                }
            }
            int sb = 0;                                                             // backward: SB[i + 1] while slot i is written
#pragma unroll
            for (int i = RWM - 1; i >= 0; --i) {
                if (i < rw) {
                    uint32_t out;
                    z -= MF;
                    if (i == 0) out = I::chk_out(sb);
                    else if (i == rw - 1) { out = I::chk_out(SF[i - 1]); sb = P[i]; }   // SF[rw - 2]
                    else { out = I::chk_out(I::chk_mul(SF[i - 1], sb)); sb = I::i16(I::chk_mul(P[i], sb)); }
                    if (wr) ST[z] = (uint16_t)out;
                }
            }
        }
        if (MW) __syncthreads();
        if (cw2) {
            for (int k = 0; k < nh; ++k) {                                          // :3915-3977
                const int c0 = rs[cs + k];
                const uint32_t g0 = (uint32_t)rs[ce + c0], g1 = (uint32_t)rs[ce + c0 + 1];   // rows ascending
                const int v = (k * M + n) * F + f;
                const int z0 = ((int)(g0 >> 16) * M + back(n, (int)(g0 & 0xffffu))) * F + f;
                const int z1 = ((int)(g1 >> 16) * M + back(n, (int)(g1 & 0xffffu))) * F + f;
                uint32_t sv, d0, d1;
                I::cw2(ych[v], ST[z0], ST[z1], sv, d0, d1);
                if (wr) { so[v] = (uint16_t)sv; ST[z0] = (uint16_t)d0; ST[z1] = (uint16_t)d1; }
            }
        } else {
            for (int k = 0; k < nh; ++k) {                                          // :3978-4100
                const int c0 = rs[cs + k], c1 = rs[cs + k + 1];
                const int v = (k * M + n) * F + f;
                const uint32_t y = ych[v];
                uint32_t P1 = y << 16, P0 = (65536u - y) << 16;
                for (int c = c0; c < c1; ++c) {                                     // rows ascending
                    const uint32_t d = (uint32_t)rs[ce + c];
                    I::col_mul(P1, P0, ST[((int)(d >> 16) * M + back(n, (int)(d & 0xffffu))) * F + f]);
                }
                const uint32_t sv = I::col_soft(P1, P0);
                if (wr) so[v] = (uint16_t)sv;
                for (int c = c0; c < c1; ++c) {
                    const uint32_t d = (uint32_t)rs[ce + c];
                    const int zi = ((int)(d >> 16) * M + back(n, (int)(d & 0xffffu))) * F + f;
                    const uint32_t nd = I::local_update(sv, ST[zi]);
                    if (wr) ST[zi] = (uint16_t)nd;
                }
            }
        }
        if (MW) __syncthreads();
        ++steps;                                                                    // a frame that never passes keeps -steps = -maxiter
        stop_vote<MW>(st, syndrome_fail(), l, F, sh_flag, steps);                   // :4104-4113
    }
    // hard bit = so >> 15, soft output = so / 65536 (imake_output :3805-3820, decision 1)
    if (!l.live) return;
    if (n == 0 && iters_fr) *iters_fr = st.res;
    if (hard_fr) {
        for (int wd = n; wd < a.hard_words; wd += M) {
            uint32_t bits = 0;
            for (int b = 0; b < 32; ++b) {
                const int v = 32 * wd + b;
                if (v < N) bits |= (uint32_t)(so[v * F + f] >> 15) << b;
            }
            hard_fr[wd] = bits;
        }
    }
    if (soft_fr)
        for (int k = 0; k < nh; ++k) soft_fr[k * M] = (double)so[(k * M + n) * F + f] / 65536.0;
}

// ---------------------------------------------------------------------------------------------------------
// Low-complexity high-efficiency decoder (decoder 9): lche_decod (decoders.cpp:2899-3012, map_bin_llr :2815-2890, logexp_int
// :2777-2813, check_syndrome :793-814 on L < 0) on work item (c, w), written as lche_global_kernel (ldpc_global.hpp) writes it -- the
// same statements in the same order through ldpc_spec::lche::logexp -- with the state on chip instead of in a workspace:
//   * LDS: the a-posteriori LLRs L[N][F], then the per-edge state Z[ne_max][M][F] (e = edge index inside the frame's own code;
//     Z[e][n] is only ever touched by lane n), then the 96 + 214 table words of logexp (divergent indices, copied in at the start as
//     lche_body does), then the vote flag: F * 8 * (N + ne_max * M) + 8 * (kTabWords + kStepWords) bytes (lche_codes_image_bytes) + 16;
//   * one lane owns one check of the current layer, the block rows in a run-time loop: nothing of a row outlives it, so rh is
//     unbounded.  u[] and p[] are VGPRs with static indices (the passes are unrolled RWM times under a predicate on the wave-uniform
//     row weight).  lche_global_kernel forms u = L - Z and p = logexp(|u|) again in its second pass; L and Z of the check's edges are
//     unchanged until the check itself writes them (a row's edges lie in distinct block columns and the checks of a layer touch
//     disjoint variables), so the second evaluation has the first one's operands and gives its bits: keeping the values changes no
//     result and saves one of the three logexp per edge and layer.  All of a row's L values are read before the first is written;
//   * a logexp is a chain of dependent compares, exponent arithmetic and two LDS lookups, and nothing hides its latency but the
//     row's other edges: both passes work on groups of G = 4 edges in one basic block, as in the TDMP kernel (the predicate is per
//     group; slots beyond the row's end recompute its last edge, add nothing to the parity or the sum and store nowhere).
// A converged frame of a packed wave (and a frame beyond B) stores nothing more: its state and outputs stay as they were.  A lane that
// must not store aims at the spare word behind the vote flag, which nothing reads.
// ---------------------------------------------------------------------------------------------------------
__host__ __device__ inline size_t lche_codes_image_bytes(int F, int M, int N, int ne_max) {   // L, Z and the tables, in front of the vote flag
    return (size_t)F * 8 * ((size_t)N + (size_t)ne_max * M) + 8 * (size_t)(ldpc_spec::lche::kTabWords + ldpc_spec::lche::kStepWords);
}

template <int RWM, bool MW>
__global__ void __launch_bounds__(MW ? 512 : 64) lche_layered_codes_kernel(const CodesetArgs s) {
    namespace E = ldpc_spec::lche;
    extern __shared__ double lds[];
    int w;
    const DecArgs a = codeset_view(s, w);
    const TabPtr rs = tab_ptr(a.row_start), ed = tab_ptr(a.edges);
    const int M = a.M, F = a.F, N = a.N, rh = a.rh, nh = a.nh;
    double *const L = lds, *const Z = lds + (size_t)N * F;
    double *const tab = Z + (size_t)s.ne_max * M * F;
    const double *const T = tab, *const S = tab + E::kTabWords;
    int *const sh_flag = reinterpret_cast<int *>(reinterpret_cast<char *>(lds) + lche_codes_image_bytes(F, M, N, s.ne_max));
    const int spare = s.ne_max * M * F + E::kTabWords + E::kStepWords + 1;          // index into Z of the second half of the flag's 16 bytes
    constexpr int G = 4;                                                            // edges of a row worked on side by side
    static_assert(RWM % G == 0, "lche_layered_codes_kernel: whole groups");
    int n, f;
    const bool valid = lane_map<MW>(F, M, n, f);
    const unsigned long long per = MW ? 0ull : slot_mask(F);
    const long long fr = (long long)w * F + f;
    const bool inb = fr < a.B;
    const bool live = valid && inb;
    const int ne = rs[rh];

    for (int i = threadIdx.x; i < E::kTabWords + E::kStepWords; i += (int)blockDim.x)
        tab[i] = i < E::kTabWords ? E::kLcheTab[i] : E::kLcheStep[i - E::kTabWords];
    if (valid) {
        for (int k = 0; k < nh; ++k) L[(k * M + n) * F + f] = live ? a.llr[fr * N + k * M + n] : 0.0;   // :2923-2924, the input as it is
        for (int e = 0; e < ne; ++e) Z[(e * M + n) * F + f] = 0.0;                  // :2919-2921
    }
    __syncthreads();

    auto syndrome_fail = [&]() -> bool {                                            // check_syndrome :793-814 on L < 0
        uint32_t failw = 0;
        for (int j = 0; j < rh; ++j) {
            const int e0 = rs[j], e1 = rs[j + 1];
            uint32_t sy = 0;
            for (int e = e0; e < e1; ++e) {
                const uint32_t d = (uint32_t)ed[e];
                const int k = d >> 16, c = d & 0xffffu;
                sy ^= (uint32_t)(L[(k * M + rot_idx(n, c, M)) * F + f] < 0);
            }
            failw |= sy;
        }
        return valid && failw;
    };

    bool done = !inb;
    int res = -a.maxiter;
    bool frame_fail = frame_vote<MW>(syndrome_fail(), F, f, per, sh_flag);          // :2928-2937
    if (!done && !frame_fail) { done = true; res = 0; }                             // a codeword at the input: no iteration, 0
    for (int steps = 0; steps < a.maxiter;) {
        if (MW) { if (done) break; }
        else if (__all(done)) break;
        const bool wr = !done && valid;
        for (int j = 0; j < rh; ++j) {                                              // layers in sequence (:2946)
            const int e0 = rs[j], rw = rs[j + 1] - e0;
            double u[RWM], p[RWM];
#pragma unroll
            for (int i = 0; i < RWM; ++i) { u[i] = 0.0; p[i] = 0.0; }
            bool par = false;
            double sum = 0.0;
#pragma unroll
            for (int g0 = 0; g0 < RWM; g0 += G) {                                   // map_bin_llr :2836-2855
                if (g0 < rw) {
#pragma unroll
                    for (int q = 0; q < G; ++q) {                                   // G independent chains; slots beyond the row repeat its last edge
                        const int i = g0 + q < rw ? g0 + q : rw - 1;
                        const uint32_t d = (uint32_t)ed[e0 + i];
                        const int k = d >> 16, c = d & 0xffffu;
                        const double uu = L[(k * M + rot_idx(n, c, M)) * F + f] - Z[((e0 + i) * M + n) * F + f];
                        u[g0 + q] = uu;
                        p[g0 + q] = E::logexp(uu < 0.0 ? -uu : uu, T, S);
                    }
#pragma unroll
                    for (int q = 0; q < G; ++q) {                                   // parity and sum in edge order, over the row's own edges
                        const bool in_row = g0 + q < rw;
                        par ^= in_row && u[g0 + q] < 0;
                        sum = in_row ? sum + p[g0 + q] : sum;
                    }
                }
            }
#pragma unroll
            for (int g0 = 0; g0 < RWM; g0 += G) {                                   // :2857-2863, :2974-2988
                if (g0 < rw) {
                    double cv[G];
                    int zi[G], li[G];
#pragma unroll
                    for (int q = 0; q < G; ++q) {                                   // where the group's results go, settled before the chains
                        const int i = g0 + q;
                        const bool ok = wr && i < rw;
                        const int ii = i < rw ? i : rw - 1;
                        const uint32_t d = (uint32_t)ed[e0 + ii];
                        const int k = d >> 16, c = d & 0xffffu;
                        zi[q] = ok ? ((e0 + ii) * M + n) * F + f : spare;
                        li[q] = ok ? (k * M + rot_idx(n, c, M)) * F + f : N * F + spare;
                    }
#pragma unroll
                    for (int q = 0; q < G; ++q) {
                        const double av = E::logexp(p[g0 + q] - sum, T, S);
                        cv[q] = ((u[g0 + q] < 0) != par) ? av : -av;
                    }
#pragma unroll
                    for (int q = 0; q < G; ++q) { L[li[q]] = cv[q] + u[g0 + q]; Z[zi[q]] = cv[q]; }
                }
            }
            if (MW) __syncthreads();
        }
        frame_fail = frame_vote<MW>(syndrome_fail(), F, f, per, sh_flag);           // :2995-3001 (the value after the last layer)
        ++steps;
        if (!done && !frame_fail) { done = true; res = steps; }                     // else -steps = -maxiter at the end
    }
    // glob_outputs: decword[k] = L[k] < 0 (:3005-3006), the final L as the soft output
    if (!live) return;
    if (n == 0 && a.iters) a.iters[fr] = res;
    if (a.hard) {
        for (int wd = n; wd < a.hard_words; wd += M) {
            uint32_t bits = 0;
            for (int b = 0; b < 32; ++b) {
                const int v = 32 * wd + b;
                if (v < N) bits |= (uint32_t)(L[v * F + f] < 0) << b;
            }
            a.hard[fr * a.hard_words + wd] = bits;
        }
    }
    if (a.soft_out)
        for (int k = 0; k < nh; ++k) a.soft_out[fr * N + k * M + n] = L[(k * M + n) * F + f];
}

// ---------------------------------------------------------------------------------------------------------
// Integer min-sum (decoder 4): imin_sum_decod_qc_lm (decoders.cpp:5430-5690) on work item (c, w), ims_flood_kernel's arithmetic
// (ldpc_kernels.hpp) in two parts.
//
// The input stage does not depend on the code: coef = sqrt(N / sum y^2) (ims_coef_kernel, ldpc_frontend.hpp: the sum is sequential
// and its rounding is part of the result) and the quantised channel word are functions of the received word alone.
// ims_flood_kernel lets every lane walk the N LLRs of its frame; over shared LLRs that would be repeated per code.  Here
// ims_quantise_kernel writes the int16 word once per received word ([B][N], or [C][B][N] for per-code LLRs) and every code reads
// 2 bytes per variable instead of 8.
//
// ims_flood_codes_kernel keeps the whole state of a frame in LDS, so neither rh nor nh is bounded:
//   * rec[R][F], R = rh * M: per check one 8-byte record {u16 m1, u16 m2, u32 meta}, meta = the 16 edge-sign bits | pos << kRowBits as
//     in ims_flood_kernel's registers; rec[(j * M + n) * F + f] is only ever touched by lane n of frame f;
//   * soft[N][F] int16: the accumulator of STATE1, then the a-posteriori value;
//   * iy[N][F] int16: the quantised channel word, loaded once; iy[(k * M + n) * F + f] is only read by lane n;
//   * F * (4 * N + 8 * R) bytes, rounded up to 16 (ims_codes_image_bytes), then the vote flag's 16.
// Stored values never leave [-max_data, max_data] (max_data <= 16383; |iy| <= max_quant <= 16383, m1, m2 in [0, max_data]): halfwords
// hold them exactly; sums and scaled magnitudes are 32-bit registers.  STATE1 adds the block rows in ascending order and saturates
// after every add, as the reference does (saturating adds do not commute).
// A converged frame of a packed wave (and a frame beyond B) stores nothing more: its state and outputs stay as they were.
// ---------------------------------------------------------------------------------------------------------
struct ImsQuantArgs {
    const double *llr;   // [frames][N]
    const double *coef;  // [frames] from ims_coef_kernel
    int16_t *q;          // [frames][N]
    long long total;     // frames * N
    int N;
    double thr;
    int max_quant;
};

// ims_flood_kernel's quantiser (decoders.cpp:5483-5500): magnitude, scale, clamp, round, sign -- in that order
__device__ __forceinline__ int ims_quantise(double val, double coef, double thr, int max_quant) {
    int sign = 0;
    if (val < 0) { val = -val; sign = 1; }
    val *= coef;
    if (val > thr) val = thr;
    const int ival = (int)(short)floor(val * max_quant / thr + 0.5);
    return sign ? -ival : ival;
}

__global__ void __launch_bounds__(256) ims_quantise_kernel(const ImsQuantArgs a) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.total; i += (long long)gridDim.x * blockDim.x)
        a.q[i] = (int16_t)ims_quantise(a.llr[i], a.coef[i / a.N], a.thr, a.max_quant);
}

struct ImsCodesArgs {
    const int16_t *q;    // the quantised channel words, laid out like CodesetArgs::llr
    int max_data;        // (1 << (dbits - 1)) - 1, decoders.cpp:5445
    int ialpha;          // (int)(alpha * 16), :5458
};

__host__ __device__ inline size_t ims_codes_image_bytes(int F, int N, int R) {   // rec, soft and iy, in front of the vote flag
    return ((size_t)F * (4 * (size_t)N + 8 * (size_t)R) + 15) & ~(size_t)15;
}

template <bool MW>
__global__ void __launch_bounds__(MW ? 512 : 64) ims_flood_codes_kernel(const CodesetArgs s, const ImsCodesArgs q) {
    extern __shared__ double lds[];
    int w;
    const DecArgs a = codeset_view(s, w);
    const TabPtr rs = tab_ptr(a.row_start), ed = tab_ptr(a.edges);
    const int M = a.M, F = MW ? 1 : a.F, N = a.N, rh = a.rh, nh = a.nh, R = rh * M;
    uint2 *const rec = reinterpret_cast<uint2 *>(lds);
    int16_t *const soft = reinterpret_cast<int16_t *>(rec + (size_t)R * F), *const iy = soft + (size_t)N * F;
    int *const sh_flag = reinterpret_cast<int *>(reinterpret_cast<char *>(lds) + ims_codes_image_bytes(F, N, R));
    const int max_data = q.max_data, ialpha = q.ialpha;
    const Lane l = frame_lane<MW>(F, M, a.B, w);
    const int n = l.n, f = l.f;
    const bool valid = l.valid;

    if (valid) {
        const int16_t *const qf = q.q + (a.llr - s.llr) + (l.inb ? l.fr : 0) * (long long)N;   // the code's slice, as for the LLRs
        for (int k = 0; k < nh; ++k) iy[(k * M + n) * F + f] = l.live ? qf[k * M + n] : (int16_t)0;
        for (int j = 0; j < rh; ++j) rec[(j * M + n) * F + f] = make_uint2(0u, 0u);        // :5462-5470
    }

    FrameStop st = stop_init(l, a.maxiter);
    for (int iter = 0; iter < a.maxiter; ++iter) {
        const bool wr = !st.done && valid;
        if (wr)
            for (int k = 0; k < nh; ++k) soft[(k * M + n) * F + f] = 0;
        if (MW) __syncthreads();
        for (int j = 0; j < rh; ++j) {   // STATE1
            const int e0 = rs[j], rw = rs[j + 1] - e0;
            const uint2 rc = rec[(j * M + n) * F + f];
            const int c1 = ((int)(rc.x & 0xffffu) * ialpha) >> 4, c2 = ((int)(rc.x >> 16) * ialpha) >> 4;
            ims_row_add(ed, e0, rw, RowRec<int>{c1, c2, rc.y, 0u}, wr, soft, max_data, l, M, F);
            if (MW) __syncthreads();     // the next block row adds into the same variables
        }
        if (wr) {                        // STATE2 :5579-5604
            for (int k = 0; k < nh; ++k) {
                const int o = (k * M + n) * F + f;
                soft[o] = (int16_t)ims_sat((int)iy[o] + (int)soft[o], max_data);
            }
        }
        if (MW) __syncthreads();
        uint32_t failw = 0;
        for (int j = 0; j < rh; ++j) {   // STATE3
            const int e0 = rs[j], rw = rs[j + 1] - e0;
            const int ri = (j * M + n) * F + f;
            const uint2 rc = rec[ri];
            const int c1 = ((int)(rc.x & 0xffffu) * ialpha) >> 4, c2 = ((int)(rc.x >> 16) * ialpha) >> 4;
            const RowRec<int> nr = ims_row_scan(ed, e0, rw, RowRec<int>{c1, c2, rc.y, 0u}, soft, max_data, l, M, F);
            failw |= nr.sy;
            if (wr) rec[ri] = make_uint2((uint32_t)nr.m1 | ((uint32_t)nr.m2 << 16), nr.meta);
        }
        stop_vote<MW>(st, valid && (failw >> 31), l, F, sh_flag, iter + 1);  // :5684-5689
        if (stop_all<MW>(st)) break;
    }
    frame_outputs(a, F, l, st.res, [=](int i) { return (uint32_t)(int)soft[i] >> 31; }, [=](int i) { return (double)soft[i]; });
}

// ---------------------------------------------------------------------------------------------------------
// Error accounting against the all-zero codeword per code, with the shared count of ldpc_frontend.hpp: one wavefront per (slot, frame),
// blocks_per_code workgroups per slot; a workgroup works on one slot only, so its totals go to the row of the slot's code.
// ---------------------------------------------------------------------------------------------------------
struct CodesetCountArgs {
    const uint32_t *hard;          // [n_active][B][hard_words]
    const int32_t *iters;          // [n_active][B]
    int32_t *frame_info;           // [n_active][B] or null
    unsigned long long *counters;  // [C][5]: nse, nde, nue, frames, sum |iters|; the row of a slot is its code's
    const int32_t *code_list;      // [n_active] or null (slot s holds code s), as in CodesetArgs
    long long B;
    int blocks_per_code;
    int hard_words, R;
};

__global__ void __launch_bounds__(256) count_errors_codes_kernel(const CodesetCountArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int cs = blockIdx.x / a.blocks_per_code, slot = blockIdx.x - cs * a.blocks_per_code;
    const int c = a.code_list ? tab_ptr(a.code_list)[cs] : cs;
    ErrorTally tally;
    for (long long fr = (long long)slot * 4 + wv; fr < a.B; fr += (long long)a.blocks_per_code * 4) {
        const long long g = (long long)cs * a.B + fr;
        uint32_t all = 0, info = 0;
        packed_word_errors(a.hard + g * a.hard_words, nullptr, a.hard_words, a.R, lane, all, info);
        wave_sum_pair(all, info);
        if (lane == 0) tally.add(all, info, a.iters[g], a.frame_info ? a.frame_info + g : nullptr);
    }
    tally.flush(a.counters + (size_t)c * 5);
}

// ---------------------------------------------------------------------------------------------------------
// Upstream's sequential stopping rule (bp_simulation.cpp:591, :805-823) over the ordered records of one piece, one wavefront per
// running slot.  Per code and frame, in frame order:
//     stop unless nde < n_frame_errors && experiment <= n_experiments;  ++experiment;
//     a non-zero record:  nse += record & (2^30 - 1), ++nde, stop if nde >= 10 && (double)nde / experiment > 2.5 * reference_frame_error.
// 64 frames per step: the error flags are one ballot, so lane l knows the nde it would see (the carry + the errors below it) and the
// experiment it would see (the carry + l) if no frame before it stopped the run, and evaluates both conditions for its own frame;
// the first lane whose frame stops the run is exact (nothing stopped before it), and it is the find-first-set of the ballot of stop
// flags.  Frames behind the stop do not reach the state.  frames_decoded grows by B: the piece was decoded for this code.
// ---------------------------------------------------------------------------------------------------------
struct CodesetRuleArgs {
    const int32_t *frame_info;     // [n_active][B]
    const int32_t *code_list;      // [n_active]
    unsigned long long *state;     // [C][4]: experiment, nse, nde, frames_decoded
    int32_t *running;              // [C]: cleared when the code stops
    long long B;
    long long n_frame_errors, n_experiments;
    double reference_frame_error;
};

struct CodesetRuleFullArgs : CodesetRuleArgs {   // state is [C][6]
    const int32_t *iters;          // [n_active][B]
};

// FULL: the whole SimCounters of an exact replay.  The state is [C][6] = experiment, nse, nde, nue, sum |iters|, frames_decoded, and
// the slot's iteration counts iters [n_active][B] are read next to its records: nue counts the error frames with iters >= 0
// (:809-810) and sum |iters| every frame (:799), both over exactly the frames that reach the state (`take`), with the ballot and the
// 64-bit sum of nse.  !FULL is the rule of the Philox entry points, state [C][4], and reads no iteration count.
// GRID: the rule on an SNR grid.  The list holds items p * C + c, the state and the flags have P * C rows, and point p has a reference
// of its own, reference[item / C] (upstream's best_errors[s], main_simulation.cpp:510); reference_frame_error is not read.  The kernel
// itself is the template (a body in a __device__ function that both forms call gave the existing instances another order of the
// 64-bit additions, profiles/r21_codeset_exact_resource_usage.txt): <FULL, false> is the kernel of the existing entry points.
template <bool FULL>
struct CodesetRuleGridArgs : std::conditional_t<FULL, CodesetRuleFullArgs, CodesetRuleArgs> {
    const double *reference;       // [P]
    int C;
};

template <bool FULL, bool GRID = false>
__global__ void __launch_bounds__(64)
stop_rule_codes_kernel(const std::conditional_t<GRID, CodesetRuleGridArgs<FULL>, std::conditional_t<FULL, CodesetRuleFullArgs, CodesetRuleArgs>> a) {
    constexpr int kWords = FULL ? 6 : 4;
    const int lane = threadIdx.x;
    const int code = tab_ptr(a.code_list)[blockIdx.x];   // GRID: the item
    double reference_frame_error = a.reference_frame_error;
    if constexpr (GRID) reference_frame_error = a.reference[(unsigned)code / (unsigned)a.C];
    const int32_t *const rec = a.frame_info + (long long)blockIdx.x * a.B;
    unsigned long long *const st = a.state + kWords * (size_t)code;
    long long experiment = (long long)st[0], nde = (long long)st[2];
    unsigned long long nse = st[1];
    unsigned long long nue = 0, sit = 0;   // FULL: what this piece adds
    const double thr = 2.5 * reference_frame_error;
    const unsigned long long below = (1ull << lane) - 1;
    bool stopped = false;
    for (long long base = 0; base < a.B && !stopped; base += 64) {
        const bool act = base + lane < a.B;
        const int32_t r = act ? rec[base + lane] : 0;
        int32_t it = 0;
        if constexpr (FULL) it = act ? a.iters[(long long)blockIdx.x * a.B + base + lane] : 0;
        const bool err = r != 0;                                                     // bit 30: any wrong bit (:805)
        const unsigned long long em = __ballot(err);
        const long long d0 = nde + __popcll(em & below);                             // nde and experiment before this lane's frame
        const long long e0 = experiment + lane;
        const bool pre = act && !(d0 < a.n_frame_errors && e0 <= a.n_experiments);   // :591, the frame is not consumed
        const long long d1 = d0 + 1, e1 = e0 + 1;
        const bool post = act && !pre && err && d1 >= 10 && (double)d1 / (double)e1 > thr;   // :820, the frame is consumed
        const unsigned long long pm = __ballot(pre), sm = __ballot(pre || post);
        const long long left = a.B - base;
        int n = left < 64 ? (int)left : 64;                                          // frames of this step that reach the state
        if (sm) {
            const int p = __ffsll((long long)sm) - 1;
            n = p + (((pm >> p) & 1ull) ? 0 : 1);
            stopped = true;
        }
        const unsigned long long take = n >= 64 ? ~0ull : (1ull << n) - 1;
        experiment += n;
        if (em & take) {
            nde += __popcll(em & take);
            unsigned long long s = lane < n ? (unsigned long long)(r & ((1 << 30) - 1)) : 0ull;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            nse += s;
        }
        if (FULL) {
            nue += (unsigned long long)__popcll(__ballot(err && it >= 0) & take);
            unsigned long long s = lane < n ? (unsigned long long)(it < 0 ? -(long long)it : (long long)it) : 0ull;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            sit += s;
        }
    }
    if (!(nde < a.n_frame_errors && experiment <= a.n_experiments)) stopped = true;   // :591 fails before the next frame
    if (lane == 0) {
        st[0] = (unsigned long long)experiment; st[1] = nse; st[2] = (unsigned long long)nde;
        if (FULL) { st[3] += nue; st[4] += sit; }
        st[kWords - 1] += (unsigned long long)a.B;
        if (stopped) a.running[code] = 0;
    }
}

// The codes still running, in ascending order, and their number: one wavefront, 64 codes per step.
__global__ void __launch_bounds__(64) running_codes_kernel(const int32_t *running, int C, int32_t *code_list, int32_t *n_active) {
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1;
    int n = 0;
    for (int base = 0; base < C; base += 64) {
        const int c = base + lane;
        const bool on = c < C && running[c] != 0;
        const unsigned long long m = __ballot(on);
        if (on) code_list[n + __popcll(m & below)] = c;
        n += __popcll(m);
    }
    if (lane == 0) *n_active = n;
}

}  // namespace ldpc
