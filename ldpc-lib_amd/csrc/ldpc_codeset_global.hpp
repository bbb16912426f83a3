// ldpc_codeset_global.hpp -- the global-memory tier of a code set: C candidate codes of one shape x B frames in one launch with the
// message state in a per-workgroup slice of a workspace in HBM, so that a set is never refused for its shape (any lifting, any
// number of block rows and columns, any image size).  What ldpc_global.hpp is to a single code, for the sets of ldpc_codeset.hpp.
//
//   * work item (slot, frame): item = slot * B + frame; a slot is a code of CodesetArgs::code_list (null: the identity).  The grid is
//     capped and a workgroup strides over the n_slots * B items, so the workspace -- one slice per workgroup, sized for the set's
//     ne_max -- grows with neither B nor C.  Workgroups are glob_threads(N) threads.
//   * codeset_glob_view does for a *_global_kernel body what codeset_view does for a resident one: the table pointers go to the
//     code's own record, the LLR pointer to the item's received word (shared [B][N] or the code's slice of [C][B][N]), the outputs to
//     [slot][frame].  The record of this route (ldpc_codeset_api.hpp, CS_SLOTS) holds everything DecArgs names for the tier:
//     row_start[rh+1], edges[ne], cw2, col_start[nh+1], col_edges[ne], col_slot[ne].  It is read through the constant address
//     space (tab_ptr): the addresses are wave-uniform.
//   * what belongs to a CODE comes from its record and never from the launch: its edge count ne (the slice is laid out for it; it
//     fits, ne <= ne_max), its row and column weights, and cw2 -- every block column holds exactly two circulants, upstream's own
//     branch of decoders 2 and 5 -- so one set may mix both kinds.  A workgroup that moves on to another code reads nothing its
//     previous item left in the slice: every body initialises what it reads, as the bodies of ldpc_global.hpp do per frame.
//
// The eight bodies below compute exactly what ms_ / lms_ / tasp_ / lche_ / sp_ / ims_ / asp_ / iasp_global_kernel of ldpc_global.hpp
// compute: the same expressions in the same operand order, contraction off, upstream's comparisons and branches; only where the
// tables, the received word and the outputs are found differs (and, for integer min-sum, that the quantiser has run once per
// received word before the launch, codeset_ims_quantise: the int16 words are the values ims_global_kernel forms itself).  They are
// functions of their own and share with ldpc_global.hpp the slice layout and the addressing helpers only, so that no kernel of that
// header changes (its header notes that shared pieces have cost time before).  Gallager BP has no set: its frames are not independent.
// Bit-identical to one LdpcHip per matrix and to the CPU oracle (tests/test_gpu_codeset_global.py).
#pragma once

#include "ldpc_codeset.hpp"
#include "ldpc_global.hpp"

namespace ldpc {

struct CodesetGlobArgs {
    CodesetArgs s;      // inputs, outputs, table, list of codes and shape as for the resident set kernels (F and blocks_per_code unused)
    char *ws;           // gridDim.x slices of ws_stride bytes, each glob_ws_bytes(N, R, ne_max, M, the decoder's edge arrays)
    size_t ws_stride;
    long long items;    // n_slots * B
};

// One work item as its body sees it
struct GlobCode {
    GlobFrame w;                                               // the workgroup's slice laid out for THIS code's ne, and the sizes
    const double *llr;                                         // [N] the item's received word
    uint32_t *hard; int32_t *iters; double *soft_out;          // the item's outputs, or null
    TabPtr row_start, edges, col_start, col_edges, col_slot;   // the code's record
    long long word;                                            // index of the received word among all of CodesetArgs::llr
    int rh, maxiter, hard_words, cw2;
    double alpha;
};

__device__ __forceinline__ GlobCode codeset_glob_view(const CodesetGlobArgs &g, long long item, int edge_arrays) {
    const CodesetArgs &s = g.s;
    const int slot = (int)(item / s.B);
    const long long fr = item - (long long)slot * s.B;
    const int c = s.code_list ? tab_ptr(s.code_list)[slot] : slot;
    const TabPtr rec = tab_ptr(s.tab + tab_ptr(s.code_off)[c]);
    const int ne = rec[s.rh];
    GlobCode a;
    a.w = GlobFrame{glob_view(g.ws + (size_t)blockIdx.x * g.ws_stride, s.N, s.rh * s.M, ne, s.M, edge_arrays), s.M, s.N, s.rh * s.M, ne};
    a.word = (long long)c * (s.llr_code_stride / s.N) + fr;
    a.llr = s.llr + (long long)c * s.llr_code_stride + fr * s.N;
    a.hard = s.hard ? s.hard + item * s.hard_words : nullptr;
    a.iters = s.iters ? s.iters + item : nullptr;
    a.soft_out = s.soft_out ? s.soft_out + item * s.N : nullptr;
    a.row_start = rec;
    a.edges = rec + s.rh + 1;
    a.cw2 = rec[s.rh + 1 + ne];
    a.col_start = rec + s.rh + 2 + ne;
    a.col_edges = a.col_start + s.nh + 1;
    a.col_slot = a.col_edges + ne;
    a.rh = s.rh; a.maxiter = s.maxiter; a.hard_words = s.hard_words;
    a.alpha = s.alpha;
    return a;
}

// glob_syndrome and glob_outputs of ldpc_global.hpp on a work item
template <class Bit>
__device__ __forceinline__ int codes_glob_syndrome(const GlobCode &a, Bit bit) {
    const GlobFrame &w = a.w;
    const int M = w.M;
    int fail = 0;
    for (int chk = threadIdx.x; chk < w.R; chk += (int)blockDim.x) {
        const int j = chk / M, n = chk - j * M;
        int synd = 0;
        for (int e = a.row_start[j]; e < a.row_start[j + 1]; ++e) synd ^= (int)bit(var_idx((uint32_t)a.edges[e], n, M));
        fail |= synd;
    }
    return __syncthreads_or(fail);
}

template <class Bit, class Soft>
__device__ __forceinline__ void codes_glob_outputs(const GlobCode &a, int res, Bit bit, Soft soft) {
    const int N = a.w.N;
    if (threadIdx.x == 0 && a.iters) a.iters[0] = res;
    if (a.hard) {
        for (int wd = threadIdx.x; wd < a.hard_words; wd += (int)blockDim.x) {
            uint32_t bits = 0;
            for (int b = 0; b < 32; ++b) {
                const int v = 32 * wd + b;
                if (v < N) bits |= (uint32_t)bit(v) << b;
            }
            a.hard[wd] = bits;
        }
    }
    if (a.soft_out)
        for (int v = threadIdx.x; v < N; v += (int)blockDim.x) a.soft_out[v] = soft(v);
}

// ms_global_kernel's frame (min_sum_decod_qc_lm, decoders.cpp:4554-4767)
__device__ __forceinline__ void ms_global_item(const GlobCode &a) {
    const GlobFrame &w = a.w;
    const int M = w.M, N = w.N, R = w.R;
    const double alpha = a.alpha;
    const double *y = a.llr;
    glob_reset_records(w, w.m1, w.m2);                                            // :4579-4596
    __syncthreads();
    int res = -a.maxiter;
    for (int iter = 0; iter < a.maxiter; ++iter) {
        for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {                  // STATE1 + STATE2 from the variable side (:4633-4685)
            const int k = v / M, i = v - k * M;
            double acc = 0.0;                                                     // memset(soft, 0) :4630
            for (int q = a.col_start[k]; q < a.col_start[k + 1]; ++q) {           // block rows ascending
                const uint32_t d = (uint32_t)a.col_edges[q];
                const int j = (int)(d >> 16), e = (int)a.col_slot[q], n = chk_pos(d, i, M);
                const int chk = j * M + n;
                const double tmp = w.pos[chk] == e - a.row_start[j] ? w.m2[chk] : w.m1[chk];
                const double cv = (w.sgn[(size_t)e * M + n] ^ w.par[chk]) ? -tmp : tmp;
                acc = acc + cv;                                                   // :4660
            }
            w.soft[v] = y[v] + acc * alpha;                                       // :4674 / :4682, two roundings
        }
        __syncthreads();
        int fail = 0;
        for (int chk = threadIdx.x; chk < R; chk += (int)blockDim.x) {            // STATE3 from the check side (:4690-4755)
            const int j = chk / M, n = chk - j * M;
            const int e0 = a.row_start[j], e1 = a.row_start[j + 1];
            const int po = w.pos[chk];
            const uint8_t pa = w.par[chk];
            const double o1 = w.m1[chk], o2 = w.m2[chk];
            double nm1 = kMaxVal, nm2 = kMaxVal;
            int np = 0, synd = 0;
            uint8_t npar = 0;
            for (int e = e0; e < e1; ++e) {
                const double r = w.soft[var_idx((uint32_t)a.edges[e], n, M)];
                synd ^= (int)(r < 0);                                             // :4712
                double val = (po == e - e0 ? o2 : o1) * alpha;                   // :4720
                double t = (w.sgn[(size_t)e * M + n] ^ pa) ? -val : val;
                t = r - t;
                const uint8_t sign = t < 0;
                w.sgn[(size_t)e * M + n] = sign;
                npar ^= sign;
                val = t < 0.0 ? -t : t;
                val = (val > kMaxVal) ? kMaxVal : val;                            // :4730
                if (val < nm1) { np = e - e0; nm2 = nm1; nm1 = val; }
                else if (val < nm2) nm2 = val;
            }
            w.m1[chk] = nm1; w.m2[chk] = nm2; w.pos[chk] = np; w.par[chk] = npar;
            fail |= synd;
        }
        if (!__syncthreads_or(fail)) { res = iter + 1; break; }                   // :4757-4766
    }
    codes_glob_outputs(a, res, [=](int v) { return w.soft[v] < 0; }, [=](int v) { return w.soft[v]; });   // decword[k] = soft[k] < 0 (:4683)
    __syncthreads();                                                              // the slice is reused by this workgroup's next item
}

// lms_global_kernel's frame (lmin_sum_decod_qc_lm, decoders.cpp:5064-5425, MY_VERSION branch)
__device__ __forceinline__ void lms_global_item(const GlobCode &a) {
    const GlobFrame &w = a.w;
    const int M = w.M, N = w.N;
    const auto bit = [=](int v) { return w.soft[v] < 0; };                         // check_syndrome :793-814; decword[] :5418
    const double *y = a.llr;
    for (int v = threadIdx.x; v < N; v += (int)blockDim.x) w.soft[v] = y[v];        // :5088
    glob_reset_records(w, w.m1, w.m2);
    __syncthreads();
    int parity = codes_glob_syndrome(a, bit);                                      // :5111-5115
    int iter = 0;
    for (; iter < a.maxiter; ++iter) {
        if (parity == 0) break;                                                    // :5119
        for (int j = 0; j < a.rh; ++j) {                                           // layers in sequence
            const int e0 = a.row_start[j], e1 = a.row_start[j + 1];
            for (int n = threadIdx.x; n < M; n += (int)blockDim.x) {
                const int chk = j * M + n;
                const int po = w.pos[chk];
                const uint8_t pa = w.par[chk];
                const double o1 = w.m1[chk], o2 = w.m2[chk];
                double nm1 = kMaxVal, nm2 = kMaxVal;                               // :5133-5134
                int np = 0;
                uint8_t npar = 0;
                for (int e = e0; e < e1; ++e) {                                    // :5141-5177
                    const double prev_abs = po == e - e0 ? o2 : o1;
                    const double prev_val = (w.sgn[(size_t)e * M + n] ^ pa) ? -prev_abs : prev_abs;
                    const double t = w.soft[var_idx((uint32_t)a.edges[e], n, M)] - prev_val;
                    const uint8_t sign = t < 0;
                    double mag = t < 0.0 ? -t : t;
                    mag -= 0.4;                                                     // beta :5163
                    mag = mag < 0 ? 0 : mag;
                    w.tmp[(size_t)e * M + n] = t;
                    w.sgn[(size_t)e * M + n] = sign;
                    npar ^= sign;                                                  // process_check_node :5009-5027
                    if (mag < nm1) { np = e - e0; nm2 = nm1; nm1 = mag; }
                    else if (mag < nm2) nm2 = mag;
                }
                w.m1[chk] = nm1; w.m2[chk] = nm2; w.pos[chk] = np; w.par[chk] = npar;
                for (int e = e0; e < e1; ++e) {                                    // :5182-5206
                    const double c_abs = np == e - e0 ? nm2 : nm1;
                    const double c_val = (w.sgn[(size_t)e * M + n] ^ npar) ? -c_abs : c_abs;
                    w.soft[var_idx((uint32_t)a.edges[e], n, M)] = w.tmp[(size_t)e * M + n] + c_val;
                }
            }
            __syncthreads();
        }
        parity = codes_glob_syndrome(a, bit);                                      // :5281-5288
        if (parity == 0) break;
    }
    codes_glob_outputs(a, parity ? -iter : iter + 1, bit, [=](int v) { return w.soft[v]; });   // :5424
    __syncthreads();
}

// tasp_global_kernel's frame (tdmp_sum_prod_gf2_decod_qc_lm, decoders.cpp:2584-2744)
__device__ __forceinline__ void tasp_global_item(const GlobCode &a) {
    const GlobFrame &w = a.w;
    const int M = w.M, N = w.N, ne = w.ne;
    const double T = 0.0001, TT = 0;                                                // :2597-2598
    const size_t EM = glob_align(sizeof(double) * (size_t)ne * M) / sizeof(double);
    double *const Z = w.tmp, *const Y = w.tmp + EM, *const SF = w.tmp + 2 * EM, *const SB = w.tmp + 3 * EM;   // [e * M + k]
    const auto bit = [=](int v) { return w.soft[v] > 0.5; };                        // check_syndrome_thr :2274-2306, thr 0.5; decword[] :2734
    for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {                       // :2611-2618
        const double x = a.llr[v] * 0.5;
        const double y = x < 20.0 ? (x < -20.0 ? -20.0 : x) : 20.0;                 // maxd(mind(x, INPUT_LIMIT), -INPUT_LIMIT)
        const double e0 = ldpc_spec::exp_glibc(y), e1 = ldpc_spec::exp_glibc(-y);
        w.soft[v] = e1 / (e0 + e1);
    }
    for (size_t i = threadIdx.x; i < (size_t)ne * M; i += (int)blockDim.x) Z[i] = 0.5;   // :2637
    __syncthreads();
    int synd = codes_glob_syndrome(a, bit);                                         // :2653-2660
    int steps = 0;
    if (synd != 0) {
        while (steps < a.maxiter) {
            for (int j = 0; j < a.rh; ++j) {                                        // layers in sequence (:2668)
                const int e0 = a.row_start[j], e1 = a.row_start[j + 1], rw = e1 - e0;
                for (int k = threadIdx.x; k < M; k += (int)blockDim.x) {
                    for (int e = e0; e < e1; ++e) {                                 // :2676-2697
                        const double x = w.soft[var_idx((uint32_t)a.edges[e], k, M)];
                        const double aa = Z[(size_t)e * M + k];
                        double v = x * (1.0 - aa) / (aa + x - 2.0 * aa * x);        // rho = gamma - lambda
                        if (v < TT) v = TT;
                        if (v > 1 - TT) v = 1 - TT;
                        Y[(size_t)e * M + k] = v;
                    }
                    // map_bin(a, cnt, 1) :2191-2228 with P[i] = 1 - 2 * y[i]
                    auto P = [&](int i) { return 1 - 2 * Y[(size_t)(e0 + i) * M + k]; };
                    auto sf = [&](int i) -> double & { return SF[(size_t)(e0 + i) * M + k]; };
                    auto sb = [&](int i) -> double & { return SB[(size_t)(e0 + i) * M + k]; };
                    sf(0) = P(0);
                    for (int i = 1; i < rw - 1; ++i) sf(i) = P(i) * sf(i - 1);
                    sb(rw - 1) = P(rw - 1);
                    for (int i = rw - 2; i > 0; --i) sb(i) = P(i) * sb(i + 1);
                    for (int i = 0; i < rw; ++i) {
                        double q;
                        if (i == 0) q = (1 - sb(1)) / 2;
                        else if (i == rw - 1) q = (1 - sf(rw - 2)) / 2;
                        else q = (1 - sf(i - 1) * sb(i + 1)) / 2;
                        if (q < T) q = T;                                            // :2703-2704
                        if (q > 1.0 - T) q = 1.0 - T;
                        Z[(size_t)(e0 + i) * M + k] = q;
                    }
                    for (int e = e0; e < e1; ++e) {                                 // :2707-2720
                        const double y = Y[(size_t)e * M + k], q = Z[(size_t)e * M + k];
                        w.soft[var_idx((uint32_t)a.edges[e], k, M)] = y * q / (1.0 - y - q + 2 * y * q);   // gamma = rho + lambda
                    }
                }
                __syncthreads();
            }
            synd = codes_glob_syndrome(a, bit);                                     // :2723 (the value after the last layer)
            steps = steps + 1;
            if (synd == 0) break;
        }
    }
    codes_glob_outputs(a, synd ? -steps : steps, bit, [=](int v) { return w.soft[v]; });   // :2734-2743 (0 when the input was a codeword)
    __syncthreads();
}

// lche_global_kernel's frame (lche_decod, decoders.cpp:2899-3012): the arithmetic of ldpc_spec::lche
__device__ __forceinline__ void lche_global_item(const GlobCode &a) {
    namespace E = ldpc_spec::lche;
    const GlobFrame &w = a.w;
    const int M = w.M, N = w.N, ne = w.ne;
    double *const Z = w.tmp;
    const double *const T = E::kLcheTab, *const S = E::kLcheStep;
    const auto bit = [=](int v) { return w.soft[v] < 0; };                          // check_syndrome :793-814 on L < 0
    for (int v = threadIdx.x; v < N; v += (int)blockDim.x) w.soft[v] = a.llr[v];    // :2923-2924
    for (size_t i = threadIdx.x; i < (size_t)ne * M; i += (int)blockDim.x) Z[i] = 0.0;   // :2919-2921
    __syncthreads();
    int synd = codes_glob_syndrome(a, bit);                                         // :2928-2937
    int steps = 0;
    if (synd != 0) {
        while (steps < a.maxiter) {
            for (int j = 0; j < a.rh; ++j) {                                        // layers in sequence (:2946)
                const int e0 = a.row_start[j], e1 = a.row_start[j + 1];
                for (int k = threadIdx.x; k < M; k += (int)blockDim.x) {
                    auto var = [&](int e) -> double & { return w.soft[var_idx((uint32_t)a.edges[e], k, M)]; };
                    bool par = false;
                    double sum = 0.0;
                    for (int e = e0; e < e1; ++e) {                                 // map_bin_llr :2836-2855
                        const double u = var(e) - Z[(size_t)e * M + k];
                        par ^= u < 0;
                        sum += E::logexp(u < 0.0 ? -u : u, T, S);
                    }
                    for (int e = e0; e < e1; ++e) {                                 // :2857-2863, :2974-2988
                        double &x = var(e);
                        const double u = x - Z[(size_t)e * M + k];
                        const double p = E::logexp(u < 0.0 ? -u : u, T, S);
                        const double av = E::logexp(p - sum, T, S);
                        const double c2v = ((u < 0) != par) ? av : -av;
                        x = c2v + u;
                        Z[(size_t)e * M + k] = c2v;
                    }
                }
                __syncthreads();
            }
            synd = codes_glob_syndrome(a, bit);                                     // :2995-3001
            steps = steps + 1;
            if (synd == 0) break;
        }
    }
    codes_glob_outputs(a, synd ? -steps : steps, bit, [=](int v) { return w.soft[v]; });   // :3005-3011 (0 when the input was a codeword)
    __syncthreads();
}

// sp_global_kernel's frame (sum_prod_decod_qc_lm, decoders.cpp:1923-2185)
__device__ __forceinline__ void sp_global_item(const GlobCode &a) {
    const GlobFrame &w = a.w;
    const int M = w.M, N = w.N, R = w.R, ne = w.ne;
    double *const ZZ = w.tmp, *const yd = w.aux, *const S = w.m1;
    const auto bit = [=](int v) { return w.soft[v] < 1.0; };                        // the syndromes :1964-2002 / :2129-2149; decword[] :2172
    for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {                       // :1947-1951
        const double yl = maxd(mind(a.llr[v], 20.0), -20.0);
        yd[v] = w.soft[v] = ldpc_spec::exp_glibc(yl);
    }
    for (size_t i = threadIdx.x; i < (size_t)ne * M; i += (int)blockDim.x) ZZ[i] = 1.0;   // :1957-1959
    __syncthreads();
    int res = -a.maxiter;
    bool conv = codes_glob_syndrome(a, bit) == 0;
    if (conv) res = 0;
    for (int iter = 0; !conv && iter < a.maxiter; ++iter) {
        for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {                   // phase A :2017-2060
            const int k = v / M, t = v - k * M;
            const int c0 = a.col_start[k], c1 = a.col_start[k + 1];
            double prefix = yd[v];
            for (int u = c0; u < c1; ++u) {
                const size_t zi = (size_t)a.col_slot[u] * M + t;
                const double orig = ZZ[zi];
                double AA = prefix;
                for (int x = u + 1; x < c1; ++x) AA *= ZZ[(size_t)a.col_slot[x] * M + t];
                ZZ[zi] = (AA - 1) / (AA + 1);
                prefix *= orig;
            }
        }
        __syncthreads();
        for (int chk = threadIdx.x; chk < R; chk += (int)blockDim.x) {             // phase B :2047-2050
            const int j = chk / M, n = chk - j * M;
            double s = 1.0;
            for (int e = a.row_start[j]; e < a.row_start[j + 1]; ++e) s *= ZZ[(size_t)e * M + var_pos((uint32_t)a.edges[e], n, M)];
            S[chk] = s;
        }
        __syncthreads();
        for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {                   // phase C :2103-2127
            const int k = v / M, t = v - k * M;
            double soft = yd[v];
            for (int u = a.col_start[k]; u < a.col_start[k + 1]; ++u) {
                const uint32_t d = (uint32_t)a.col_edges[u];
                const int j = (int)(d >> 16), nn = chk_pos(d, t, M);
                const size_t zi = (size_t)a.col_slot[u] * M + t;
                double A = S[j * M + nn] / ZZ[zi];
                A = (1 + A) / (1 - A);
                A = maxd(mind(A, 1.9e+8), -5.2e-9);                                 // :2120 (the negative lower clamp is upstream's)
                ZZ[zi] = A;
                soft *= A;
            }
            w.soft[v] = soft;
        }
        __syncthreads();
        if (codes_glob_syndrome(a, bit) == 0) { conv = true; res = iter + 1; }      // :2151-2166
    }
    codes_glob_outputs(a, res, bit, [=](int v) { return w.soft[v]; });
    __syncthreads();
}

// ims_global_kernel's frame (imin_sum_decod_qc_lm, decoders.cpp:5430-5690) behind the set's quantiser: iy is the int16 word that
// codeset_ims_quantise left for the item's received word (:5472-5500, once per word)
__device__ __forceinline__ void ims_global_item(const GlobCode &a, const ImsCodesArgs &q) {
    const GlobFrame &w = a.w;
    const int M = w.M, N = w.N, R = w.R;
    int *const soft = reinterpret_cast<int *>(w.soft), *const iy = reinterpret_cast<int *>(w.aux);
    int *const m1 = reinterpret_cast<int *>(w.m1), *const m2 = reinterpret_cast<int *>(w.m2);
    const int max_data = q.max_data, ialpha = q.ialpha;                             // :5445, :5458
    auto sat = [&](int x) { return x > max_data ? max_data : (x < -max_data ? -max_data : x); };   // limit_val :4308
    const int16_t *const qw = q.q + a.word * (long long)N;
    for (int v = threadIdx.x; v < N; v += (int)blockDim.x) iy[v] = (int)qw[v];
    glob_reset_records(w, m1, m2);                                                  // :5462-5470
    __syncthreads();
    int res = -a.maxiter;
    for (int iter = 0; iter < a.maxiter; ++iter) {
        for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {                    // STATE1 + STATE2 from the variable side (:5540-5604)
            const int k = v / M, i = v - k * M;
            int acc = 0;
            for (int c = a.col_start[k]; c < a.col_start[k + 1]; ++c) {             // block rows ascending: saturation after EVERY add (:5568)
                const uint32_t d = (uint32_t)a.col_edges[c];
                const int j = (int)(d >> 16), e = (int)a.col_slot[c], n = chk_pos(d, i, M);
                const int chk = j * M + n;
                int tmp = w.pos[chk] == e - a.row_start[j] ? m2[chk] : m1[chk];
                tmp = (tmp * ialpha) >> 4;                                           // :5554
                const int cv = (w.sgn[(size_t)e * M + n] ^ w.par[chk]) ? -tmp : tmp;
                acc = sat(acc + cv);
            }
            soft[v] = sat(iy[v] + acc);                                             // :5590-5601
        }
        __syncthreads();
        int fail = 0;
        for (int chk = threadIdx.x; chk < R; chk += (int)blockDim.x) {              // STATE3 (:5610-5678)
            const int j = chk / M, n = chk - j * M;
            const int e0 = a.row_start[j], e1 = a.row_start[j + 1];
            const int po = w.pos[chk], o1 = m1[chk], o2 = m2[chk];
            const uint8_t pa = w.par[chk];
            int nm1 = max_data, nm2 = max_data, np = 0, synd = 0;
            uint8_t npar = 0;
            for (int e = e0; e < e1; ++e) {
                const int r = soft[var_idx((uint32_t)a.edges[e], n, M)];
                synd ^= (int)(r < 0);
                const int val = ((po == e - e0 ? o2 : o1) * ialpha) >> 4;           // :5640
                const int t = (w.sgn[(size_t)e * M + n] ^ pa) ? -val : val;
                const int msg = r - t;
                const uint8_t sign = msg < 0;
                w.sgn[(size_t)e * M + n] = sign;
                npar ^= sign;
                int v = msg < 0 ? -msg : msg;
                v = v > max_data ? max_data : v;
                if (v < nm1) { np = e - e0; nm2 = nm1; nm1 = v; }
                else if (v < nm2) nm2 = v;
            }
            m1[chk] = nm1; m2[chk] = nm2; w.pos[chk] = np; w.par[chk] = npar;
            fail |= synd;
        }
        if (!__syncthreads_or(fail)) { res = iter + 1; break; }                     // :5684-5689
    }
    codes_glob_outputs(a, res, [=](int v) { return soft[v] < 0; }, [=](int v) { return (double)soft[v]; });
    __syncthreads();
}

// asp_global_kernel's frame (sum_prod_gf2_decod_qc_lm, decoders.cpp:2324-2581): the general branch, and for a cw2 CODE upstream's own
__device__ __forceinline__ void asp_global_item(const GlobCode &a) {
    const GlobFrame &w = a.w;
    const int M = w.M, N = w.N, R = w.R, ne = w.ne;
    const size_t EM = glob_align(sizeof(double) * (size_t)ne * M) / sizeof(double);
    double *const ST = w.tmp, *const SF = w.tmp + EM, *const SB = w.tmp + 2 * EM, *const p1ch = w.aux;
    const auto bit = [=](int v) { return w.soft[v] > 0.5; };                        // check_syndrome_thr :2274-2306, thr 0.5; the decision too
    for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {                        // :2351-2379
        const int k = v / M, t = v - k * M;
        const double x = a.llr[v] * 0.5;
        const double y = maxd(mind(x, 20.0), -20.0);
        const double e0 = ldpc_spec::exp_glibc(y), e1 = ldpc_spec::exp_glibc(-y);
        const double p = e1 / (e0 + e1);
        p1ch[v] = w.soft[v] = p;
        for (int q = a.col_start[k]; q < a.col_start[k + 1]; ++q)                   // state <- rotated channel probability
            ST[(size_t)a.col_slot[q] * M + chk_pos((uint32_t)a.col_edges[q], t, M)] = p;
    }
    __syncthreads();
    int synd = codes_glob_syndrome(a, bit);                                         // :2393-2399
    int steps = 0;
    while (synd != 0 && steps < a.maxiter) {
        for (int chk = threadIdx.x; chk < R; chk += (int)blockDim.x) {              // check nodes: map_bin(&state[0][i*m+k], rw, r) :2191-2228
            const int j = chk / M, n = chk - j * M;
            const int e0 = a.row_start[j], rw = a.row_start[j + 1] - e0;
            auto st = [&](int i) -> double & { return ST[(size_t)(e0 + i) * M + n]; };
            auto sf = [&](int i) -> double & { return SF[(size_t)(e0 + i) * M + n]; };
            auto sb = [&](int i) -> double & { return SB[(size_t)(e0 + i) * M + n]; };
            auto P = [&](int i) { return 1 - 2 * st(i); };
            sf(0) = P(0);
            for (int i = 1; i < rw - 1; ++i) sf(i) = P(i) * sf(i - 1);
            sb(rw - 1) = P(rw - 1);
            for (int i = rw - 2; i > 0; --i) sb(i) = P(i) * sb(i + 1);
            st(0) = (1 - sb(1)) / 2;
            for (int i = 1; i < rw - 1; ++i) st(i) = (1 - sf(i - 1) * sb(i + 1)) / 2;
            st(rw - 1) = (1 - sf(rw - 2)) / 2;
        }
        __syncthreads();
        if (a.cw2) {
            // every block column of this code has exactly two circulants: upstream's own branch (:2431-2480) -- the messages are formed
            // from the channel value and the OTHER edge directly, and nothing is clamped
            for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {
                const int k = v / M, t = v - k * M;
                const int q0 = a.col_start[k], q1 = q0 + 1;                         // hci[i][0] < hci[i][1]: rows ascending
                const int n0 = chk_pos((uint32_t)a.col_edges[q0], t, M), n1 = chk_pos((uint32_t)a.col_edges[q1], t, M);
                const size_t z0 = (size_t)a.col_slot[q0] * M + n0, z1 = (size_t)a.col_slot[q1] * M + n1;
                const double d0 = ST[z0], d1 = ST[z1];                              // data0[k], data1[k] :2449-2450
                double p1 = p1ch[v];
                double q10 = p1, q11 = p1, p0 = 1.0 - p1, q00 = 1.0 - p1, q01 = 1.0 - p1;   // :2454-2459
                q10 = q10 * d1;                                                     // :2461-2466
                q00 = q00 * (1 - d1);
                q11 = q11 * d0;
                q01 = q01 * (1 - d0);
                p1 = q10 * d0;
                p0 = q00 * (1 - d0);
                w.soft[v] = p1 / (p0 + p1);                                         // :2469
                ST[z0] = q10 / (q10 + q00);                                         // :2471
                ST[z1] = q11 / (q11 + q01);                                         // :2472
            }
        } else
        for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {                    // symbol nodes + local data update :2482-2556
            const int k = v / M, t = v - k * M;
            double P1 = p1ch[v], P0 = 1 - p1ch[v];
            for (int q = a.col_start[k]; q < a.col_start[k + 1]; ++q) {             // rows ascending
                const double d = ST[(size_t)a.col_slot[q] * M + chk_pos((uint32_t)a.col_edges[q], t, M)];
                P1 *= d;
                P0 *= 1 - d;
            }
            const double so = P1 / (P0 + P1);
            w.soft[v] = so;
            for (int q = a.col_start[k]; q < a.col_start[k + 1]; ++q) {
                const size_t zi = (size_t)a.col_slot[q] * M + chk_pos((uint32_t)a.col_edges[q], t, M);
                const double sos = ST[zi];
                const double p1 = so / sos;
                const double p0 = (1 - so) / (1 - sos);
                const double dd = p1 / (p1 + p0);
                ST[zi] = maxd(mind(dd, 1.0 - 0.000001), 0.000001);                  // SP_DEC_MAX_VAL / SP_DEC_MIN_VAL :96-97
            }
        }
        __syncthreads();
        synd = codes_glob_syndrome(a, bit);                                         // :2566
        steps = steps + 1;
    }
    codes_glob_outputs(a, synd ? -steps : steps, bit, [=](int v) { return w.soft[v]; });   // 0: codeword at the input; converged after `steps`; else -steps
    __syncthreads();
}

// iasp_global_kernel's frame (isum_prod_gf2_decod_qc_lm, decoders.cpp:3822-4121): the arithmetic of ldpc_spec::iasp, both branches
__device__ __forceinline__ void iasp_global_item(const GlobCode &a) {
    namespace I = ldpc_spec::iasp;
    const GlobFrame &w = a.w;
    const int M = w.M, N = w.N, R = w.R, ne = w.ne;
    uint16_t *const ST = reinterpret_cast<uint16_t *>(w.tmp);
    int16_t *const SF = reinterpret_cast<int16_t *>(ST + (size_t)ne * M);          // 4 B per slot of the 8 B edge array
    uint16_t *const so = reinterpret_cast<uint16_t *>(w.soft), *const ych = reinterpret_cast<uint16_t *>(w.aux);
    const auto bit = [=](int v) { return so[v] >> 15; };                            // icheck_syndrome :3772-3803; decision 1 of imake_output
    for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {                        // :3858-3897
        const int k = v / M, t = v - k * M;
        const uint32_t q = I::q12(I::prior(a.llr[v]));
        for (int c = a.col_start[k]; c < a.col_start[k + 1]; ++c)                   // state <- rotated Q12 value
            ST[(size_t)a.col_slot[c] * M + chk_pos((uint32_t)a.col_edges[c], t, M)] = (uint16_t)q;
        so[v] = ych[v] = (uint16_t)(q << 4);                                        // then the words, Q16
    }
    __syncthreads();
    int synd = codes_glob_syndrome(a, bit);                                         // :3899-3906
    int steps = 0;
    while (synd != 0 && steps < a.maxiter) {
        for (int chk = threadIdx.x; chk < R; chk += (int)blockDim.x) {              // imap_bin :2235-2271, any row weight >= 2
            const int j = chk / M, n = chk - j * M;
            const int e0 = a.row_start[j], rw = a.row_start[j + 1] - e0;
            auto st = [&](int i) -> uint16_t & { return ST[(size_t)(e0 + i) * M + n]; };
            auto sf = [&](int i) -> int16_t & { return SF[(size_t)(e0 + i) * M + n]; };
            int f = I::chk_p(st(0));                                                // forward products SF[0 .. rw-2]
            sf(0) = (int16_t)f;
            for (int i = 1; i < rw - 1; ++i) { f = I::i16(I::chk_mul(I::chk_p(st(i)), f)); sf(i) = (int16_t)f; }
            int sb = 0;                                                             // backward: SB[i+1] while slot i is written
            for (int i = rw - 1; i >= 0; --i) {
                const int p = I::chk_p(st(i));
                uint32_t out;
                if (i == rw - 1) { out = I::chk_out(sf(rw - 2)); sb = p; }
                else if (i == 0) out = I::chk_out(sb);
                else { out = I::chk_out(I::chk_mul(sf(i - 1), sb)); sb = I::i16(I::chk_mul(p, sb)); }
                st(i) = (uint16_t)out;
            }
        }
        __syncthreads();
        if (a.cw2) {
            for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {                // :3915-3977
                const int k = v / M, t = v - k * M;
                const int c0 = a.col_start[k], c1 = c0 + 1;                         // hci[i][0] < hci[i][1]: rows ascending
                const int n0 = chk_pos((uint32_t)a.col_edges[c0], t, M), n1 = chk_pos((uint32_t)a.col_edges[c1], t, M);
                const size_t z0 = (size_t)a.col_slot[c0] * M + n0, z1 = (size_t)a.col_slot[c1] * M + n1;
                uint32_t s, d0, d1;
                I::cw2(ych[v], ST[z0], ST[z1], s, d0, d1);
                so[v] = (uint16_t)s;
                ST[z0] = (uint16_t)d0;
                ST[z1] = (uint16_t)d1;
            }
        } else
        for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {                    // :3978-4100
            const int k = v / M, t = v - k * M;
            uint32_t P1 = (uint32_t)ych[v] << 16, P0 = (65536u - ych[v]) << 16;
            for (int c = a.col_start[k]; c < a.col_start[k + 1]; ++c)               // rows ascending
                I::col_mul(P1, P0, ST[(size_t)a.col_slot[c] * M + chk_pos((uint32_t)a.col_edges[c], t, M)]);
            const uint32_t s = I::col_soft(P1, P0);
            so[v] = (uint16_t)s;
            for (int c = a.col_start[k]; c < a.col_start[k + 1]; ++c) {
                const size_t zi = (size_t)a.col_slot[c] * M + chk_pos((uint32_t)a.col_edges[c], t, M);
                ST[zi] = (uint16_t)I::local_update(s, ST[zi]);
            }
        }
        __syncthreads();
        synd = codes_glob_syndrome(a, bit);                                         // :4104-4113
        steps = steps + 1;
    }
    codes_glob_outputs(a, synd ? -steps : steps, bit, [=](int v) { return (double)so[v] / 65536.0; });   // imake_output :3805-3820, decision 1
    __syncthreads();
}

// The kernels: a workgroup walks its items; the second argument is the number of per-edge arrays of the decoder's slice (glob_ws_bytes)
#define LDPC_CODES_GLOBAL_KERNEL(name, item, edge_arrays)                                                      \
    __global__ void __launch_bounds__(kGlobThreads) name(const CodesetGlobArgs g) {                            \
        for (long long it = blockIdx.x; it < g.items; it += gridDim.x) item(codeset_glob_view(g, it, edge_arrays)); \
    }
LDPC_CODES_GLOBAL_KERNEL(sp_global_codes_kernel, sp_global_item, 1)
LDPC_CODES_GLOBAL_KERNEL(asp_global_codes_kernel, asp_global_item, 3)
LDPC_CODES_GLOBAL_KERNEL(ms_global_codes_kernel, ms_global_item, 0)
LDPC_CODES_GLOBAL_KERNEL(iasp_global_codes_kernel, iasp_global_item, 1)
LDPC_CODES_GLOBAL_KERNEL(tasp_global_codes_kernel, tasp_global_item, 4)
LDPC_CODES_GLOBAL_KERNEL(lms_global_codes_kernel, lms_global_item, 1)
LDPC_CODES_GLOBAL_KERNEL(lche_global_codes_kernel, lche_global_item, 1)
#undef LDPC_CODES_GLOBAL_KERNEL

__global__ void __launch_bounds__(kGlobThreads) ims_global_codes_kernel(const CodesetGlobArgs g, const ImsCodesArgs q) {
    for (long long it = blockIdx.x; it < g.items; it += gridDim.x) ims_global_item(codeset_glob_view(g, it, 0), q);
}

}  // namespace ldpc
