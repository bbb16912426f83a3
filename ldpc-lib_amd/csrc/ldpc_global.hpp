// ldpc_global.hpp -- the shape-unlimited tier: min-sum, integer min-sum, layered min-sum, sum-product and TDMP sum-product with the message state in
// GLOBAL memory.
//
// The LDS/VGPR-resident kernels (ldpc_spec.hpp, ldpc_kernels.hpp) need the a-posteriori values of a frame in one CU's LDS
// (N * 8 B <= 160 KiB), M <= 512, <= 64 block rows / columns, row weight <= 16 and no empty block column.  Upstream's decod_open
// (decoders.cpp:348-791) has none of these limits, so any other valid binary QC-LDPC code runs HERE instead of being refused:
// one workgroup of 256 threads per frame, soft values / check records / edge signs in a per-workgroup slice of a workspace in
// HBM (it is re-read every iteration, so it lives in L2 / Infinity Cache for the usual sizes), workgroup barriers between the
// phases.  The grid is capped and strides over the frames, so the workspace does not grow with the batch.
//
//   sp_global_kernel   sum_prod_decod_qc_lm  decoders.cpp:1923-2185: the four phases of ldpc_sumprod.hpp, arrays in the workspace.
//   ims_global_kernel  imin_sum_decod_qc_lm  decoders.cpp:5430-5690: min-sum on ints, saturation after every add of STATE1 (:5568).
//   bp_global_kernel   bp_decod_qc_lm        decoders.cpp:1708-1920, with the frame chain of the resident kernel.
//   asp_global_kernel  sum_prod_gf2_decod_qc_lm  decoders.cpp:2324-2581 (the general branch, and the branch for codes whose block
//                      columns all hold exactly two circulants, :2431-2480).
//   iasp_global_kernel isum_prod_gf2_decod_qc_lm  decoders.cpp:3822-4121 (integer advanced sum-product, decoder 5; both branches,
//                      u16 / i16 state in the workspace).
//   lche_global_kernel lche_decod  decoders.cpp:2899-3012 (decoder 9): per-edge Z in the workspace, any row weight up to 1024
//                      (0 and 1 included), any number of block rows, any lifting.
//   tasp_global_kernel tdmp_sum_prod_gf2_decod_qc_lm  decoders.cpp:2584-2744 (decoder 7, the decoder of upstream's shipped scenarios):
//                      per-edge lambda / rho / forward / backward products in the workspace instead of VGPRs, so row weight and
//                      the number of circulants are unbounded (the resident tasp_body holds the Z state of ~300 circulants in the registers of two lanes per check).
// The arithmetic is upstream's, literally (comparisons `< 0`, explicit branches, additions in upstream's order):
//   ms_global_kernel   min_sum_decod_qc_lm   decoders.cpp:4554-4767.  STATE1 is done from the VARIABLE side (a thread walks its
//                      column's circulants in ascending block row = upstream's order of additions into soft[], :4633-4667), which
//                      needs no atomics and no zeroing pass; STATE3 from the check side.
//   lms_global_kernel  lmin_sum_decod_qc_lm  decoders.cpp:5064-5425 (MY_VERSION branch): layers strictly in sequence, inside a
//                      layer every variable belongs to exactly one check.
// Bit-identical hard decisions, return values and soft values (tests/test_gpu_shapes.py: against the CPU oracle on shapes the
// resident kernels refuse, and against the golden vectors of the compiled reference with the tier forced on).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ldpc_kernels.hpp"
#include "ldpc_spec.hpp"   // exp_glibc

namespace ldpc {

constexpr int kGlobThreads = 1024;   // launch bound; the host launches 256 threads per frame for small codes, 1024 for large ones
inline int glob_threads(int N) { return N >= 16384 ? 1024 : 256; }

struct GlobArgs {
    DecArgs d;          // tables: row_start, edges, col_start, col_edges, col_slot
    char *ws;           // gridDim.x slices of ws_stride bytes
    size_t ws_stride;
    int ne;             // circulants
    // bp_global_kernel only: the frame chain (see SpecArgs in ldpc_spec.hpp; same layouts)
    const uint32_t *stale;    // [B][rh * ceil(M/64)] u64 words, bit = lane: syndrome the previous frame left behind, or null
    uint32_t *synd_out;       // same layout: what this frame leaves behind, or null
    const int *frame_idx;     // [slots] frame decoded by each workgroup slot, or null = the slot index
    long long slots;          // workgroup slots of this launch (B, or the number of frames of a re-decode pass)
    int asp_cw2;              // asp_global_kernel / iasp_global_kernel: every block column holds exactly two circulants -> upstream's own branch
                              // (decoders.cpp:2431-2480 / :3915-3977)
    const double *ims_coef;   // ims_global_kernel: [B] sqrt(N / sum y^2) per frame (ims_coef_kernel: the sum is sequential, its rounding is part of the result)
};

// slice layout (all offsets 16-byte aligned)
struct GlobView {
    double *soft, *aux, *m1, *m2, *tmp;   // aux: [N]; tmp: `edge_arrays` arrays of ne * M doubles, one after the other
    int32_t *pos;
    uint8_t *par, *sgn;
};
__host__ __device__ inline size_t glob_align(size_t x) { return (x + 15) & ~(size_t)15; }
__host__ __device__ inline size_t glob_ws_bytes(int N, int R, int ne, int M, int edge_arrays) {
    return 2 * glob_align(sizeof(double) * (size_t)N) + 2 * glob_align(sizeof(double) * (size_t)R) + glob_align(sizeof(int32_t) * (size_t)R) +
           glob_align((size_t)R) + glob_align((size_t)ne * M) + (size_t)edge_arrays * glob_align(sizeof(double) * (size_t)ne * M);
}
__device__ inline GlobView glob_view(char *p, int N, int R, int ne, int M, int edge_arrays) {
    GlobView v;
    v.soft = reinterpret_cast<double *>(p); p += glob_align(sizeof(double) * (size_t)N);
    v.aux = reinterpret_cast<double *>(p); p += glob_align(sizeof(double) * (size_t)N);
    v.m1 = reinterpret_cast<double *>(p); p += glob_align(sizeof(double) * (size_t)R);
    v.m2 = reinterpret_cast<double *>(p); p += glob_align(sizeof(double) * (size_t)R);
    v.pos = reinterpret_cast<int32_t *>(p); p += glob_align(sizeof(int32_t) * (size_t)R);
    v.par = reinterpret_cast<uint8_t *>(p); p += glob_align((size_t)R);
    v.sgn = reinterpret_cast<uint8_t *>(p); p += glob_align((size_t)ne * M);
    v.tmp = edge_arrays ? reinterpret_cast<double *>(p) : nullptr;
    return v;
}

// What every kernel of this tier does the same way stands once, here: the frame-invariant values of a workgroup (GlobFrame,
// glob_frame), the two directions of edge addressing (var_pos / var_idx, chk_pos), check_syndrome (glob_syndrome), the reset of the
// min-sum records (glob_reset_records), upstream's clamps (mind, maxd) and the outputs of a frame (glob_outputs).  What differs
// between decoders -- the test that decides a bit, the conversion of the a-posteriori word -- arrives as a functor.  The functors
// capture the pointers they read by value ([=]), as in ldpc_kernels.hpp (profiles/kernel_refactor_resources.txt).
//
// The frame of a decoder -- initialisation, iterations, outputs, closing barrier -- stands once as well: *_global_frame, a template on
// the view of one frame (GlobCode).  The kernels of this header call it for frame fr of one code, with the tables of DecArgs behind
// plain pointers; the *_global_codes_kernel of ldpc_codeset_global.hpp call it for one (code, frame) item of a set, with the code's
// record behind the constant address space.  Neither side's loads change kind, and there is one text of upstream's arithmetic.
// A frame takes its view BY VALUE: by reference every single-code kernel but the two flooding min-sums came out 23 - 53
// instructions longer, with more SGPR spills (profiles/global_frame_refactor_resources.txt).
// lche_global_frame keeps its own syndrome and edge decode and calls only glob_outputs: with glob_syndrome and var_idx the
// single-code kernel measured slower (profiles/global_tier_refactor_time.txt).  Gallager BP has no set (its frames are chained); its
// kernel holds its own frame and builds the view for glob_syndrome and glob_outputs.

// what a workgroup keeps over all its frames: its workspace slice and the sizes (lifting, variables, checks, circulants)
struct GlobFrame : GlobView {
    int M, N, R, ne;
};
__device__ __forceinline__ GlobFrame glob_frame(const GlobArgs &g, int edge_arrays) {
    const int M = g.d.M, N = g.d.N, R = g.d.rh * M, ne = g.ne;
    return GlobFrame{glob_view(g.ws + (size_t)blockIdx.x * g.ws_stride, N, R, ne, M, edge_arrays), M, N, R, ne};
}

// One frame as its body sees it.  Idx is how row_start / col_start are addressed and Words how the three tables of edge words are:
// both index to an int and a uint32_t, `const int32_t *` and `const uint32_t *` for a single code, TabPtr and TabWords for a set.
template <class Idx, class Words>
struct GlobCode {
    GlobFrame w;                                               // the workgroup's slice laid out for this code's ne, and the sizes
    const double *llr;                                         // [N] the frame's received word
    uint32_t *hard; int32_t *iters; double *soft_out;          // the launch's output arrays, or null
    long long out;                                             // the frame's row in them; glob_outputs forms the addresses (offset here, the
                                                               // three pointers stay live over the iterations: more SGPR spills in every kernel)
    Idx row_start, col_start;
    Words edges, col_edges, col_slot;
    int rh, maxiter, hard_words;
    int cw2;                                                   // every block column holds exactly two circulants (GlobArgs::asp_cw2)
    double alpha;
};
// frame fr of the launch's one code; w is the workgroup's glob_frame
__device__ __forceinline__ GlobCode<const int32_t *, const uint32_t *> glob_code(const GlobArgs &g, const GlobFrame &w, long long fr) {
    const DecArgs &d = g.d;
    return {w, d.llr + fr * d.N, d.hard, d.iters, d.soft_out, fr, d.row_start, d.col_start, d.edges, d.col_edges, d.col_slot,
            d.rh, d.maxiter, d.hard_words, g.asp_cw2, d.alpha};
}

// Check n of a block row reaches over edge word d = (block column k << 16) | shift c the variable (k, (n + c) mod M): its position
// inside the block column, and its index among the N variables.
__device__ __forceinline__ int var_pos(uint32_t d, int n, int M) {
    int i = n + (int)(d & 0xffffu);
    if (i >= M) i -= M;
    return i;
}
__device__ __forceinline__ int var_idx(uint32_t d, int n, int M) { return (int)(d >> 16) * M + var_pos(d, n, M); }
// The mirror: position i of a block column is seen over column edge word d = (block row j << 16) | shift c by check (i - c) mod M of row j.
__device__ __forceinline__ int chk_pos(uint32_t d, int i, int M) {
    int n = i - (int)(d & 0xffffu);
    if (n < 0) n += M;
    return n;
}

__device__ __forceinline__ double mind(double x, double y) { return x < y ? x : y; }   // decoders.cpp:104-105
__device__ __forceinline__ double maxd(double x, double y) { return x < y ? y : x; }

// check_syndrome (decoders.cpp:793-814; check_syndrome_thr :2274-2306, icheck_syndrome :3772-3803) for the whole workgroup: the OR over
// all checks of the XOR over a check's variables of bit(variable index).  sink(chk, synd) receives a check's result and start(j, n) is
// the value its XOR begins with (bp_global_kernel: left[] and the stale bit).  Ends in a barrier; every thread returns the OR.
template <class Code, class Bit, class Sink, class Start>
__device__ __forceinline__ int glob_syndrome(const Code &a, Bit bit, Sink sink, Start start) {
    const GlobFrame &w = a.w;
    const int M = w.M;
    int fail = 0;
    for (int chk = threadIdx.x; chk < w.R; chk += (int)blockDim.x) {
        const int j = chk / M, n = chk - j * M;
        int synd = start(j, n);
        for (int e = a.row_start[j]; e < a.row_start[j + 1]; ++e) synd ^= (int)bit(var_idx(a.edges[e], n, M));
        sink(chk, synd);
        fail |= synd;
    }
    return __syncthreads_or(fail);
}
template <class Code, class Bit>
__device__ __forceinline__ int glob_syndrome(const Code &a, Bit bit) {
    return glob_syndrome(a, bit, [](int, int) {}, [](int, int) { return 0; });
}

// The min-sum records at the start of a frame: min1 = min2 = 0, position 0, parity and edge signs 0 (:4579-4596, :5462-5470).  m1 / m2
// are the kernel's own view of w.m1 / w.m2, doubles or -- ims_global_kernel -- ints.  The caller's barrier follows.
template <class T>
__device__ __forceinline__ void glob_reset_records(const GlobFrame &w, T *m1, T *m2) {
    for (int c = threadIdx.x; c < w.R; c += (int)blockDim.x) { m1[c] = 0; m2[c] = 0; w.pos[c] = 0; w.par[c] = 0; }
    for (size_t i = threadIdx.x; i < (size_t)w.ne * w.M; i += (int)blockDim.x) w.sgn[i] = 0;
}

// The outputs of a frame, called by the whole workgroup: the iteration result, the hard decisions bit(variable) packed 32 to a word
// and the soft values soft(variable).
template <class Code, class Bit, class Soft>
__device__ __forceinline__ void glob_outputs(const Code &a, int res, Bit bit, Soft soft) {
    const int N = a.w.N;
    const long long fr = a.out;
    if (threadIdx.x == 0 && a.iters) a.iters[fr] = res;
    if (a.hard) {
        for (int wd = threadIdx.x; wd < a.hard_words; wd += (int)blockDim.x) {
            uint32_t bits = 0;
            for (int b = 0; b < 32; ++b) {
                const int v = 32 * wd + b;
                if (v < N) bits |= (uint32_t)bit(v) << b;
            }
            a.hard[fr * a.hard_words + wd] = bits;
        }
    }
    if (a.soft_out)
        for (int v = threadIdx.x; v < N; v += (int)blockDim.x) a.soft_out[fr * N + v] = soft(v);
}

// min_sum_decod_qc_lm, decoders.cpp:4554-4767
template <class Code>
__device__ __forceinline__ void ms_global_frame(const Code a) {
    const GlobFrame &w = a.w;
    const int M = w.M, N = w.N, R = w.R;
    const double alpha = a.alpha;
    const double *y = a.llr;
    glob_reset_records(w, w.m1, w.m2);                                            // :4579-4596
    __syncthreads();
    int res = -a.maxiter;
    for (int iter = 0; iter < a.maxiter; ++iter) {
        // ---- STATE1 + STATE2 from the variable side (:4633-4685)
        for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {
            const int k = v / M, i = v - k * M;
            double acc = 0.0;                                                     // memset(soft, 0) :4630
            for (int q = a.col_start[k]; q < a.col_start[k + 1]; ++q) {           // block rows ascending
                const uint32_t d = a.col_edges[q];
                const int j = (int)(d >> 16), e = (int)a.col_slot[q], n = chk_pos(d, i, M);
                const int chk = j * M + n;
                const double tmp = w.pos[chk] == e - a.row_start[j] ? w.m2[chk] : w.m1[chk];
                const double cv = (w.sgn[(size_t)e * M + n] ^ w.par[chk]) ? -tmp : tmp;
                acc = acc + cv;                                                   // :4660
            }
            w.soft[v] = y[v] + acc * alpha;                                       // :4674 / :4682, two roundings
        }
        __syncthreads();
        // ---- STATE3 from the check side (:4690-4755)
        int fail = 0;
        for (int chk = threadIdx.x; chk < R; chk += (int)blockDim.x) {
            const int j = chk / M, n = chk - j * M;
            const int e0 = a.row_start[j], e1 = a.row_start[j + 1];
            const int po = w.pos[chk];
            const uint8_t pa = w.par[chk];
            const double o1 = w.m1[chk], o2 = w.m2[chk];
            double nm1 = kMaxVal, nm2 = kMaxVal;
            int np = 0, synd = 0;
            uint8_t npar = 0;
            for (int e = e0; e < e1; ++e) {
                const double r = w.soft[var_idx(a.edges[e], n, M)];
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
        if (!__syncthreads_or(fail)) { res = iter + 1; break; }                   // :4757-4766 (the barrier also fences the next STATE1)
    }
    glob_outputs(a, res, [=](int v) { return w.soft[v] < 0; }, [=](int v) { return w.soft[v]; });   // decword[k] = soft[k] < 0 (:4683)
    __syncthreads();                                                              // the slice is reused by this workgroup's next frame
}

// lmin_sum_decod_qc_lm, decoders.cpp:5064-5425 (MY_VERSION branch)
template <class Code>
__device__ __forceinline__ void lms_global_frame(const Code a) {
    const GlobFrame &w = a.w;
    const int M = w.M, N = w.N;
    const auto bit = [=](int v) { return w.soft[v] < 0; };                         // check_syndrome, decoders.cpp:793-814; decword[] :5418
    const double *y = a.llr;
    for (int v = threadIdx.x; v < N; v += (int)blockDim.x) w.soft[v] = y[v];        // :5088
    glob_reset_records(w, w.m1, w.m2);
    __syncthreads();
    int parity = glob_syndrome(a, bit);                                            // :5111-5115
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
                    const double t = w.soft[var_idx(a.edges[e], n, M)] - prev_val;
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
                    w.soft[var_idx(a.edges[e], n, M)] = w.tmp[(size_t)e * M + n] + c_val;
                }
            }
            __syncthreads();
        }
        parity = glob_syndrome(a, bit);                                            // :5281-5288
        if (parity == 0) break;
    }
    glob_outputs(a, parity ? -iter : iter + 1, bit, [=](int v) { return w.soft[v]; });   // :5424
    __syncthreads();
}

// tdmp_sum_prod_gf2_decod_qc_lm, decoders.cpp:2584-2744
template <class Code>
__device__ __forceinline__ void tasp_global_frame(const Code a) {
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
    int synd = glob_syndrome(a, bit);                                               // :2653-2660
    int steps = 0;
    if (synd != 0) {
        while (steps < a.maxiter) {
            for (int j = 0; j < a.rh; ++j) {                                        // layers in sequence (:2668)
                const int e0 = a.row_start[j], e1 = a.row_start[j + 1], rw = e1 - e0;
                for (int k = threadIdx.x; k < M; k += (int)blockDim.x) {
                    for (int e = e0; e < e1; ++e) {                                 // :2676-2697
                        const double x = w.soft[var_idx(a.edges[e], k, M)];
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
                        w.soft[var_idx(a.edges[e], k, M)] = y * q / (1.0 - y - q + 2 * y * q);   // gamma = rho + lambda
                    }
                }
                __syncthreads();
            }
            synd = glob_syndrome(a, bit);                                           // :2723 (the value after the last layer)
            steps = steps + 1;
            if (synd == 0) break;
        }
    }
    glob_outputs(a, synd ? -steps : steps, bit, [=](int v) { return w.soft[v]; });   // :2734-2743 (0 when the input was a codeword)
    __syncthreads();
}

// lche_decod, decoders.cpp:2899-3012 (low-complexity high-efficiency decoder, decoder 9): the arithmetic of ldpc_spec::lche
// (shared with the resident lche_body), tables read from global memory.  Workspace (glob_ws_bytes with one edge array): the
// a-posteriori LLRs L [N] in soft, Z [e * M + k] in tmp.  A thread owns a check of the current layer and walks its edges twice:
// the first pass forms the hard-bit parity and `sum` in edge order, the second recomputes u and p (L is unchanged until the
// check writes it, and the checks of a layer touch disjoint variables) and writes L and Z.
// This frame keeps its own syndrome and edge decode: with glob_syndrome and var_idx lche_global_kernel was 1 % slower
// (profiles/global_tier_refactor_time.txt).  The set kernel runs this text too.
template <class Code>
__device__ __forceinline__ void lche_global_frame(const Code a) {
    namespace E = ldpc_spec::lche;
    const GlobFrame &w = a.w;
    const int M = w.M, N = w.N, R = w.R, ne = w.ne;
    double *const Z = w.tmp;
    const double *const T = E::kLcheTab, *const S = E::kLcheStep;
    auto syndrome = [&]() -> int {                                                  // check_syndrome :793-814 on L < 0
        int fail = 0;
        for (int chk = threadIdx.x; chk < R; chk += (int)blockDim.x) {
            const int j = chk / M, n = chk - j * M;
            int synd = 0;
            for (int e = a.row_start[j]; e < a.row_start[j + 1]; ++e) {
                const uint32_t d = a.edges[e];
                int i = n + (int)(d & 0xffffu);
                if (i >= M) i -= M;
                synd ^= (int)(w.soft[(int)(d >> 16) * M + i] < 0);
            }
            fail |= synd;
        }
        return __syncthreads_or(fail);
    };
    for (int v = threadIdx.x; v < N; v += (int)blockDim.x) w.soft[v] = a.llr[v];    // :2923-2924
    for (size_t i = threadIdx.x; i < (size_t)ne * M; i += (int)blockDim.x) Z[i] = 0.0;   // :2919-2921
    __syncthreads();
    int synd = syndrome();                                                          // :2928-2937
    int steps = 0;
    if (synd != 0) {
        while (steps < a.maxiter) {
            for (int j = 0; j < a.rh; ++j) {                                        // layers in sequence (:2946)
                const int e0 = a.row_start[j], e1 = a.row_start[j + 1];
                for (int k = threadIdx.x; k < M; k += (int)blockDim.x) {
                    auto var = [&](int e) -> double & {
                        const uint32_t d = a.edges[e];
                        int i = k + (int)(d & 0xffffu);
                        if (i >= M) i -= M;
                        return w.soft[(int)(d >> 16) * M + i];
                    };
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
            synd = syndrome();                                                      // :2995-3001
            steps = steps + 1;
            if (synd == 0) break;
        }
    }
    glob_outputs(a, synd ? -steps : steps, [=](int v) { return w.soft[v] < 0; }, [=](int v) { return w.soft[v]; });   // :3005-3011 (0 when the input was a codeword)
    __syncthreads();
}

// sum_prod_decod_qc_lm, decoders.cpp:1923-2185 (likelihood-ratio domain), the four phases of ldpc_sumprod.hpp with every array in
// the workspace: ZZ[e][t] per edge and variable position, yd / soft per variable, the check products in m1[].
template <class Code>
__device__ __forceinline__ void sp_global_frame(const Code a) {
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
    bool conv = glob_syndrome(a, bit) == 0;
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
            for (int e = a.row_start[j]; e < a.row_start[j + 1]; ++e) s *= ZZ[(size_t)e * M + var_pos(a.edges[e], n, M)];
            S[chk] = s;
        }
        __syncthreads();
        for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {                   // phase C :2103-2127
            const int k = v / M, t = v - k * M;
            double soft = yd[v];
            for (int u = a.col_start[k]; u < a.col_start[k + 1]; ++u) {
                const uint32_t d = a.col_edges[u];
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
        if (glob_syndrome(a, bit) == 0) { conv = true; res = iter + 1; }            // :2151-2166
    }
    glob_outputs(a, res, bit, [=](int v) { return w.soft[v]; });
    __syncthreads();
}

// imin_sum_decod_qc_lm, decoders.cpp:5430-5690 (MS_MUL_CORRECTION build: c2v magnitude (min * ialpha) >> 4 in STATE1 and STATE3).
// IMS_DATA is a short upstream; every intermediate fits (|values| <= 2 * max_data < 2^15), so int arithmetic gives the same numbers.
// Workspace: soft / iy as ints in the soft / aux arrays, min1 / min2 as ints in m1 / m2.  channel(v) is the quantised channel word
// of variable v (:5472-5500): ims_global_kernel quantises in place, a set reads what codeset_ims_quantise left behind.
template <class Code, class Channel>
__device__ __forceinline__ void ims_global_frame(const Code a, int max_data, int ialpha, Channel channel) {
    const GlobFrame &w = a.w;
    const int M = w.M, N = w.N, R = w.R;
    int *const soft = reinterpret_cast<int *>(w.soft), *const iy = reinterpret_cast<int *>(w.aux);
    int *const m1 = reinterpret_cast<int *>(w.m1), *const m2 = reinterpret_cast<int *>(w.m2);
    auto sat = [&](int x) { return x > max_data ? max_data : (x < -max_data ? -max_data : x); };   // limit_val :4308
    for (int v = threadIdx.x; v < N; v += (int)blockDim.x) iy[v] = channel(v);
    glob_reset_records(w, m1, m2);                                                  // :5462-5470
    __syncthreads();
    int res = -a.maxiter;
    for (int iter = 0; iter < a.maxiter; ++iter) {
        for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {                    // STATE1 + STATE2 from the variable side (:5540-5604)
            const int k = v / M, i = v - k * M;
            int acc = 0;
            for (int q = a.col_start[k]; q < a.col_start[k + 1]; ++q) {             // block rows ascending: saturation after EVERY add (:5568)
                const uint32_t d = a.col_edges[q];
                const int j = (int)(d >> 16), e = (int)a.col_slot[q], n = chk_pos(d, i, M);
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
                const int r = soft[var_idx(a.edges[e], n, M)];
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
    glob_outputs(a, res, [=](int v) { return soft[v] < 0; }, [=](int v) { return (double)soft[v]; });
    __syncthreads();
}

// sum_prod_gf2_decod_qc_lm, decoders.cpp:2324-2581 (probability domain, flooding): the general branch :2482-2556 and -- GlobCode::cw2
// -- the branch upstream takes for codes whose block columns ALL hold exactly two circulants (:2431-2480; only this tier runs it).
// Workspace: state[e][n] per circulant and check (upstream's state[slot][row*m + n]) + two scratch arrays for map_bin's forward /
// backward products; channel P(bit = 1) in aux, a-posteriori values in soft.
template <class Code>
__device__ __forceinline__ void asp_global_frame(const Code a) {
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
            ST[(size_t)a.col_slot[q] * M + chk_pos(a.col_edges[q], t, M)] = p;
    }
    __syncthreads();
    int synd = glob_syndrome(a, bit);                                               // :2393-2399
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
            // every block column has exactly two circulants: upstream's own branch (:2431-2480) -- the messages are formed from the
            // channel value and the OTHER edge directly, and nothing is clamped
            for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {
                const int k = v / M, t = v - k * M;
                const int q0 = a.col_start[k], q1 = q0 + 1;                         // hci[i][0] < hci[i][1]: rows ascending
                const int n0 = chk_pos(a.col_edges[q0], t, M), n1 = chk_pos(a.col_edges[q1], t, M);
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
                const double d = ST[(size_t)a.col_slot[q] * M + chk_pos(a.col_edges[q], t, M)];
                P1 *= d;
                P0 *= 1 - d;
            }
            const double so = P1 / (P0 + P1);
            w.soft[v] = so;
            for (int q = a.col_start[k]; q < a.col_start[k + 1]; ++q) {
                const size_t zi = (size_t)a.col_slot[q] * M + chk_pos(a.col_edges[q], t, M);
                const double sos = ST[zi];
                const double p1 = so / sos;
                const double p0 = (1 - so) / (1 - sos);
                const double dd = p1 / (p1 + p0);
                ST[zi] = maxd(mind(dd, 1.0 - 0.000001), 0.000001);                  // SP_DEC_MAX_VAL / SP_DEC_MIN_VAL :96-97
            }
        }
        __syncthreads();
        synd = glob_syndrome(a, bit);                                               // :2566
        steps = steps + 1;
    }
    glob_outputs(a, synd ? -steps : steps, bit, [=](int v) { return w.soft[v]; });   // 0: codeword at the input; converged after `steps`; else -steps
    __syncthreads();
}

// isum_prod_gf2_decod_qc_lm, decoders.cpp:3822-4121 (integer advanced sum-product, decoder 5): the general branch :3978-4100 and --
// GlobCode::cw2 -- the branch for codes whose block columns all hold exactly two circulants (:3915-3977).  The arithmetic is
// ldpc_spec::iasp (shared with the resident iasp_body).  Workspace (glob_ws_bytes with one edge array): state u16 [ne][M] and
// imap_bin's forward products i16 [ne][M] in tmp, the a-posteriori word u16 [N] in soft, the channel word u16 [N] in aux.
template <class Code>
__device__ __forceinline__ void iasp_global_frame(const Code a) {
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
            ST[(size_t)a.col_slot[c] * M + chk_pos(a.col_edges[c], t, M)] = (uint16_t)q;
        so[v] = ych[v] = (uint16_t)(q << 4);                                        // then the words, Q16
    }
    __syncthreads();
    int synd = glob_syndrome(a, bit);                                               // :3899-3906
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
                const int n0 = chk_pos(a.col_edges[c0], t, M), n1 = chk_pos(a.col_edges[c1], t, M);
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
                I::col_mul(P1, P0, ST[(size_t)a.col_slot[c] * M + chk_pos(a.col_edges[c], t, M)]);
            const uint32_t s = I::col_soft(P1, P0);
            so[v] = (uint16_t)s;
            for (int c = a.col_start[k]; c < a.col_start[k + 1]; ++c) {
                const size_t zi = (size_t)a.col_slot[c] * M + chk_pos(a.col_edges[c], t, M);
                ST[zi] = (uint16_t)I::local_update(s, ST[zi]);
            }
        }
        __syncthreads();
        synd = glob_syndrome(a, bit);                                               // :4104-4113
        steps = steps + 1;
    }
    glob_outputs(a, synd ? -steps : steps, bit, [=](int v) { return (double)so[v] / 65536.0; });   // imake_output :3805-3820, decision 1
    __syncthreads();
}

// The single-code kernels: the workgroup's slice once, then its frames; the third argument is the number of per-edge arrays of the
// decoder's slice (glob_ws_bytes)
#define LDPC_GLOBAL_KERNEL(name, frame, edge_arrays)                                                       \
    __global__ void __launch_bounds__(kGlobThreads) name(const GlobArgs g) {                               \
        const GlobFrame w = glob_frame(g, edge_arrays);                                                    \
        for (long long fr = blockIdx.x; fr < g.d.B; fr += gridDim.x) frame(glob_code(g, w, fr));            \
    }
LDPC_GLOBAL_KERNEL(ms_global_kernel, ms_global_frame, 0)
LDPC_GLOBAL_KERNEL(lms_global_kernel, lms_global_frame, 1)
LDPC_GLOBAL_KERNEL(tasp_global_kernel, tasp_global_frame, 4)
LDPC_GLOBAL_KERNEL(lche_global_kernel, lche_global_frame, 1)
LDPC_GLOBAL_KERNEL(sp_global_kernel, sp_global_frame, 1)
LDPC_GLOBAL_KERNEL(asp_global_kernel, asp_global_frame, 3)
LDPC_GLOBAL_KERNEL(iasp_global_kernel, iasp_global_frame, 1)
#undef LDPC_GLOBAL_KERNEL

// integer min-sum quantises the received word itself (:5472-5500), with the frame's coefficient of GlobArgs::ims_coef
__global__ void __launch_bounds__(kGlobThreads) ims_global_kernel(const GlobArgs g) {
    const DecArgs &d = g.d;
    const GlobFrame w = glob_frame(g, 0);
    const int max_data = (1 << (d.ims_dbits - 1)) - 1;   // :5445
    const int max_quant = (1 << (d.ims_qbits - 1)) - 1;  // :5446
    const int ialpha = (int)(d.alpha * (1 << 4));         // :5458 MS_ALPHA_FPP = 4
    const double ims_thr = d.ims_thr;
    for (long long fr = blockIdx.x; fr < d.B; fr += gridDim.x) {
        const auto a = glob_code(g, w, fr);
        const double *const y = a.llr;
        const double coef = g.ims_coef[fr];
        ims_global_frame(a, max_data, ialpha, [=](int v) {
            double val = y[v];
            int sign = 0;
            if (val < 0) { val = -val; sign = 1; }
            val *= coef;
            if (val > ims_thr) val = ims_thr;
            const int ival = (int)(short)floor(val * max_quant / ims_thr + 0.5);
            return sign ? -ival : ival;
        });
    }
}

// bp_decod_qc_lm, decoders.cpp:1708-1920 (Gallager BP in the log domain), the phases of bp_body (ldpc_spec.hpp) with every array in
// the workspace: ZZ[e][t] per edge and variable position (tmp), BB in sgn, the check sums s in m1 and their signs in par, yd in aux,
// the a-posteriori LLRs in soft.  exp / log are glibc's algorithms (tables read from global memory here).  The frame chain
// (stale syndrome in, syndrome left behind out, re-decode passes) works exactly as in the resident kernel.
__global__ void __launch_bounds__(kGlobThreads) bp_global_kernel(const GlobArgs g) {
    const DecArgs &a = g.d;
    const GlobFrame w = glob_frame(g, 1);
    const int M = w.M, N = w.N, R = w.R, ne = w.ne, CH = (M + 63) / 64, SW = a.rh * CH;
    double *const ZZ = w.tmp, *const yd = w.aux, *const S = w.m1;
    uint8_t *const BB = w.sgn, *const bs = w.par;
    uint8_t *const left = reinterpret_cast<uint8_t *>(w.pos);                       // [R] syndrome bits as last computed (upstream's st->syndr)
    const unsigned long long *const stale = reinterpret_cast<const unsigned long long *>(g.stale);
    const auto bit = [=](int v) { return w.soft[v] < 0; };                          // the syndromes :1742-1766 / :1869-1893 and the decision
    const auto keep = [=](int chk, int sy) { left[chk] = (uint8_t)sy; };
    for (long long slot = blockIdx.x; slot < g.slots; slot += gridDim.x) {
        const long long fr = g.frame_idx ? g.frame_idx[slot] : slot;
        const auto c = glob_code(g, w, fr);                                         // the frame as glob_syndrome and glob_outputs see it
        for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {
            const double y = maxd(mind(a.llr[fr * N + v], 20.0), -20.0);            // :1738 INPUT_LIMIT
            yd[v] = w.soft[v] = y;
        }
        for (size_t i = threadIdx.x; i < (size_t)ne * M; i += (int)blockDim.x) ZZ[i] = 0.0;   // :1731-1733
        __syncthreads();
        int fail = glob_syndrome(c, bit, keep,                                      // :1742-1766, on top of what the previous frame left behind
                                 [=](int j, int n) { return stale ? (int)((stale[fr * SW + j * CH + (n >> 6)] >> (n & 63)) & 1ull) : 0; });
        // re-decode pass: nothing can change unless the frame was a codeword at its input (see bp_body)
        if (g.frame_idx && fail && a.iters && a.iters[fr] != 0) { __syncthreads(); continue; }
        int iter = 0;
        while (fail && iter < a.maxiter) {
            for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {                // A: variable-node activation :1803-1812
                const int k = v / M, t = v - k * M;
                const double so = w.soft[v];
                for (int q = a.col_start[k]; q < a.col_start[k + 1]; ++q) {
                    const size_t zi = (size_t)a.col_slot[q] * M + t;
                    const double A = ldpc_spec::exp_glibc_wide(so - ZZ[zi], ldpc_spec::kExpTab);
                    ZZ[zi] = ldpc_spec::log_glibc(fabs((A - 1) / (A + 1)));
                    BB[zi] = A < 1;
                }
            }
            __syncthreads();
            for (int chk = threadIdx.x; chk < R; chk += (int)blockDim.x) {          // A': check sums :1815-1824, columns ascending
                const int j = chk / M, n = chk - j * M;
                double s = 0.0;
                unsigned b = 0;
                for (int e = a.row_start[j]; e < a.row_start[j + 1]; ++e) {
                    const int i = var_pos(a.edges[e], n, M);
                    s += ZZ[(size_t)e * M + i];
                    b ^= BB[(size_t)e * M + i];
                }
                S[chk] = s;
                bs[chk] = (uint8_t)b;
            }
            __syncthreads();
            for (int v = threadIdx.x; v < N; v += (int)blockDim.x) {                // B: check-node activation seen from the variable :1834-1866
                const int k = v / M, t = v - k * M;
                double soft = yd[v];
                for (int q = a.col_start[k]; q < a.col_start[k + 1]; ++q) {         // rows ascending
                    const uint32_t d = a.col_edges[q];
                    const int j = (int)(d >> 16), nn = chk_pos(d, t, M);
                    const size_t zi = (size_t)a.col_slot[q] * M + t;
                    double A = ldpc_spec::exp_glibc_wide(S[j * M + nn] - ZZ[zi], ldpc_spec::kExpTab);
                    const int b = bs[j * M + nn] ^ BB[zi];
                    A = (double)(1 - 2 * b) * ldpc_spec::log_glibc((1 + A) / (1 - A));
                    const double zn = maxd(mind(A, 19.07), -19.07);
                    ZZ[zi] = zn;
                    soft += zn;
                }
                w.soft[v] = soft;
            }
            __syncthreads();
            fail = glob_syndrome(c, bit, keep, [](int, int) { return 0; });         // :1869-1893
            iter = iter + 1;
        }
        if (g.synd_out) {
            for (int u = threadIdx.x; u < SW; u += (int)blockDim.x) {               // one u64 per block row and 64-lane chunk
                const int j = u / CH, ch = u - j * CH;
                unsigned long long bits = 0;
                for (int l = 0; l < 64 && ch * 64 + l < M; ++l) bits |= (unsigned long long)left[j * M + ch * 64 + l] << l;
                reinterpret_cast<unsigned long long *>(g.synd_out)[fr * SW + u] = bits;
            }
        }
        glob_outputs(c, fail ? -iter : iter, bit, [=](int v) { return w.soft[v]; });
        __syncthreads();
    }
}

}  // namespace ldpc

