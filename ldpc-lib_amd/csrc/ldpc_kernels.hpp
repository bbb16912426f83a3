// ldpc_kernels.hpp -- hand-written gfx950 (CDNA4) kernels for the QC-LDPC belief-propagation hot path.
//
// Work decomposition (all decoders):
//   * a codeword ("frame") never leaves the CU: its whole message-passing state is on chip for all
//     iterations.  HBM carries only the compulsory traffic (LLR in, packed hard bits / iteration count out).
//   * one lane = one check row n of every circulant (the "check lane" view); the same lane is also
//     variable i = n of every block column (the "variable lane" view).  With lifting M = 64 a frame is exactly
//     one wavefront.  M < 64 packs F = floor(64/M) frames into one wavefront; 64 < M <= 512 spreads one frame
//     over ceil(M/64) wavefronts of one workgroup (barriers between dependent phases).
//   * a-posteriori values `soft[N]` live in LDS (fp64, 8 B per variable).  A circulant shift c is an indexed LDS
//     access at ((n+c) mod M): consecutive lanes -> consecutive 8-byte words -> bank-conflict free, and it
//     replaces the two memcpy rotations per edge of the CPU code (decoders.cpp:327-346).
//   * per-check records {min1,min2,pos,sign} and per-edge sign bits never touch memory: they are VGPRs of
//     the check lane (min1/min2 fp64, pos + the row's edge-sign bits packed in one dword per block row).
//     Because a lane owns a whole check row, min1/min2 is a serial in-register scan over the row's <= 16
//     circulants: no cross-lane reduction is needed at all; the only cross-lane traffic is the rotation
//     (LDS) and the syndrome vote (ballot).
//   * arithmetic is IEEE fp64 in the reference's exact operation order with contraction OFF
//     (-ffp-contract=off): the hard decisions are bit-identical to the CPU code, not approximately equal.
//
// Sign tests use the sign BIT of the high dword.  That equals the reference's `x < 0` for every value except
// -0.0 (and NaN); inputs are canonicalised (y + 0.0) on load, after which no intermediate of the algorithms
// can be -0.0 (x - y is -0.0 only for x = -0.0, y = +0.0; x + y only for x = y = -0.0), and the sign of a
// zero never influences a non-zero value or a comparison.  Inputs must be finite.
//
// What every frame-resident kernel does the same way is written once, here, for this file and for the code-set
// kernels of ldpc_codeset.hpp: who a lane is (Lane, frame_lane), the LDS index behind an edge (edge_idx), the
// per-row syndrome (row_syndrome), the stop bookkeeping (FrameStop, stop_vote, stop_all) and the frame's
// outputs (frame_outputs).  What differs between decoders -- the word whose bit decides, the result a clean
// vote stores, the conversion of the soft value -- arrives as a functor or a value.  The functors capture their
// LDS pointer by value ([=]): captured by reference it sits in a stack slot until the functor is inlined, and the
// register allocation of the whole kernel moves (profiles/kernel_refactor_resources.txt).
//
// The reference-exact arithmetic of the min-sum family is written once per decoder as well, as the work of one lane
// on one block row: ms_row_add / ms_row_scan (flooding, STATE1 / STATE3), lms_row_layer (both passes of a layer),
// ims_row_add / ims_row_scan (integer, templated on the LDS word).  Every LDS-tier kernel of the family -- this file,
// ldpc_codeset.hpp, ldpc_codeset_wide.hpp -- calls them from its own block-row loop (unrolled over VGPR records, or
// run-time over LDS records) and stores the returned record (RowRec) under its own condition.  Records go in and
// come out as values; the edge table is a template parameter (plain pointer or TabPtr), handed over with the row's
// first edge as an index, as the kernels addressed it before (profiles/lds_minsum_rows_resources.txt).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ldpc {

constexpr double kMaxVal = 32767.0;  // decoders.cpp:4299-4301 MAX_VAL = (1L<<15)-1
constexpr int kRowBits = 16;         // edge-sign bits per block row kept in the low half of `meta`

struct DecArgs {
    const double *llr;        // [B][N]
    uint32_t *hard;           // [B][hard_words] or null
    int32_t *iters;           // [B] or null
    double *soft_out;         // [B][N] or null
    const int32_t *row_start; // [rh+1]
    const uint32_t *edges;    // [ne]  (block column << 16) | shift, row-major order (rows asc, columns asc)
    const int32_t *col_start; // [nh+1]           (sum-product only)
    const uint32_t *col_edges;// [ne] (block row << 16) | shift, column-major order (columns asc, rows asc)
    const uint32_t *col_slot; // [ne] for the q-th entry of a column: row-major id of that edge
    const uint32_t *edge_row; // [ne] block row of each row-major edge
    long long B;
    int rh, nh, M, N, F, maxiter, hard_words;
    double alpha;
    double ims_thr;           // integer min-sum quantiser (decoders.h:46-48): threshold, bits of the input, bits of the data path
    int ims_qbits, ims_dbits;
};

__device__ __forceinline__ uint32_t hi32(double x) { return (uint32_t)__double2hiint(x); }
__device__ __forceinline__ uint32_t lo32(double x) { return (uint32_t)__double2loint(x); }
__device__ __forceinline__ double mkdouble(uint32_t hi, uint32_t lo) { return __hiloint2double((int)hi, (int)lo); }
// x with its sign flipped when bit0 of s is set
__device__ __forceinline__ double flip_if(double x, uint32_t s) { return mkdouble(hi32(x) ^ (s << 31), lo32(x)); }

// Lane -> (check row n, frame slot f).  Single-wave kernels interleave the F frames of a wave across lanes
// (lane = n*F + f) so that the LDS image ((k*M+i)*F + f) is hit with consecutive addresses by consecutive lanes.
// Lanes beyond the last check row of the wave/workgroup are "invalid": they compute on row 0 (so every address
// stays in range) but never store and never vote.
template <bool MW>
__device__ __forceinline__ bool lane_map(int F, int M, int &n, int &f) {
    if (MW) { n = threadIdx.x; f = 0; }
    else    { n = threadIdx.x / F; f = threadIdx.x - n * F; }
    const bool valid = n < M;
    if (!valid) n = 0;
    return valid;
}

// bit q*F set for every q: the lanes of frame slot 0 in a single-wave kernel (slot f = same mask << f)
__device__ __forceinline__ unsigned long long slot_mask(int F) {
    unsigned long long per = 0ull;
    for (int q = 0; q < 64; q += F) per |= 1ull << q;
    return per;
}

// Who a lane is in work item w (the w-th wave or workgroup of a code's frames): lane_map's (n, f, valid), the lane
// mask of frame slot 0, the frame, whether the frame exists (uniform per frame, and per workgroup when MW) and
// whether the lane has a frame and a row of it to store for.
// The kernels copy n, f and valid into locals, so that their arithmetic lines read as they always did, and read the
// rest (fr, inb, live) through the struct.
struct Lane {
    int n, f;
    bool valid;
    unsigned long long per;
    long long fr;
    bool inb, live;
};

template <bool MW>
__device__ __forceinline__ Lane frame_lane(int F, int M, long long B, int w) {
    Lane l;
    l.valid = lane_map<MW>(F, M, l.n, l.f);
    l.per = MW ? 0ull : slot_mask(F);
    l.fr = (long long)w * F + l.f;
    l.inb = l.fr < B;
    l.live = l.valid && l.inb;
    return l;
}

__device__ __forceinline__ int rot_idx(int n, int c, int M) {
    int t = n + c;
    return t >= M ? t - M : t;
}

// The LDS index of the variable that check n reaches over edge d = (block column << 16) | shift
__device__ __forceinline__ int edge_idx(uint32_t d, int n, int M, int F, int f) {
    const int k = d >> 16, c = d & 0xffffu;
    return (k * M + rot_idx(n, c, M)) * F + f;
}

// check_syndrome's double loop (decoders.cpp:793-814) for the lane's check of every block row: the OR over the
// block rows of the XOR over the row's variables of word(LDS index).  The caller picks the deciding bit of the
// result and masks it with the lane's validity.
template <class RowStart, class Edges, class Word>
__device__ __forceinline__ uint32_t row_syndrome(RowStart rs, Edges ed, int rh, const Lane &l, int M, int F, Word word) {
    uint32_t failw = 0;
    for (int j = 0; j < rh; ++j) {
        const int e0 = rs[j], e1 = rs[j + 1];
        uint32_t sy = 0;
        for (int e = e0; e < e1; ++e) sy ^= word(edge_idx((uint32_t)ed[e], l.n, M, F, l.f));
        failw |= sy;
    }
    return failw;
}

// "Does any check of MY frame fail?"  fail/valid are per lane.  Returns a per-lane bool (uniform per frame).
template <bool MW>
__device__ __forceinline__ bool frame_vote(bool fail, int F, int f, unsigned long long per, int *sh_flag) {
    if (MW) {
        // several waves, one frame: OR through LDS.  sh_flag is reset by the barrier protocol below.
        if (threadIdx.x == 0) *sh_flag = 0;
        __syncthreads();
        if (__any(fail) && (threadIdx.x & 63) == 0) atomicOr(sh_flag, 1);
        __syncthreads();
        bool r = *sh_flag != 0;
        __syncthreads();
        return r;
    } else {
        const unsigned long long b = __ballot(fail);
        if (F == 1) return b != 0ull;
        return ((b >> f) & per) != 0ull;  // lanes of frame slot f are f, f+F, f+2F, ...
    }
}

// Stop bookkeeping, per FRAME: every lane of a frame (valid or not) carries the same values.  A frame beyond B is
// done from the start; res stays -maxiter for a frame that the iteration loop leaves unconverged.
struct FrameStop {
    bool done;
    int res;
};

__device__ __forceinline__ FrameStop stop_init(const Lane &l, int maxiter) { return FrameStop{!l.inb, -maxiter}; }

// Vote on the lanes' failing checks; a running frame without one stops with the result res_clean.
template <bool MW>
__device__ __forceinline__ void stop_vote(FrameStop &st, bool fail, const Lane &l, int F, int *sh_flag, int res_clean) {
    const bool frame_fail = frame_vote<MW>(fail, F, l.f, l.per, sh_flag);
    if (!st.done && !frame_fail) { st.done = true; st.res = res_clean; }
}

// all frames of this wave (MW: the frame of this workgroup) are done
template <bool MW>
__device__ __forceinline__ bool stop_all(const FrameStop &st) { return MW ? st.done : __all(st.done); }

// The outputs of a frame, called by all its lanes: the iteration result, the hard decisions hard(LDS index of the
// variable) packed 32 to a word, and the soft values soft(LDS index).
template <class Hard, class Soft>
__device__ __forceinline__ void frame_outputs(const DecArgs &a, int F, const Lane &l, int res, Hard hard, Soft soft) {
    const int M = a.M, N = a.N;
    if (!l.live) return;
    if (l.n == 0 && a.iters) a.iters[l.fr] = res;
    if (a.hard) {
        for (int wd = l.n; wd < a.hard_words; wd += M) {
            uint32_t bits = 0;
            for (int b = 0; b < 32; ++b) {
                const int v = 32 * wd + b;
                if (v < N) bits |= (uint32_t)hard(v * F + l.f) << b;
            }
            a.hard[l.fr * a.hard_words + wd] = bits;
        }
    }
    if (a.soft_out)
        for (int k = 0; k < a.nh; ++k) a.soft_out[l.fr * N + k * M + l.n] = soft((k * M + l.n) * F + l.f);
}

// MS / LMS: hard bit = soft < 0 (the sign bit; soft is never -0.0), soft output = the LDS-resident value
__device__ __forceinline__ void write_outputs(const DecArgs &a, const double *lds, const Lane &l, int res) {
    frame_outputs(a, a.F, l, res, [=](int i) { return hi32(lds[i]) >> 31; }, [=](int i) { return lds[i]; });
}

// The min-sum record of one check row, as the row passes below take and return it: the two smallest magnitudes and
// meta = [15:0] v2c sign bit of the row's idx-th edge, [23:16] idx of the min1 edge.  sy is set by the flooding row
// scans only: the xor over the row's edges of the a-posteriori word.  Where a kernel keeps its records (VGPRs under an
// unrolled block-row loop, LDS words under a run-time loop, packed halfwords) is its own business; the passes get and
// give values, never a reference to a kernel's locals (profiles/lds_minsum_rows_resources.txt).
template <class T>
struct RowRec {
    T m1, m2;
    uint32_t meta, sy;
};

// ---------------------------------------------------------------------------------------------------------
// Flooding normalised min-sum  (min_sum_decod_qc_lm, decoders.cpp:4554-4767; semantics SURVEY Appendix A.1)
//
// per iteration:  STATE1  acc[v] = sum_j c2v(j,v)   (check lanes scatter-add into LDS in ascending block row)
//                 STATE2  soft = y + acc*alpha       (variable lanes, y in VGPRs, two roundings)
//                 STATE3  new records per check row from v2c = soft - alpha*c2v_old ; syndrome = xor of signs
// Algorithmic state traffic that the CPU code moves through memory every iteration (4.25*E + 30*R + 8.125*N
// bytes at 4-byte LLR width) stays in VGPRs/LDS here.
//
// The body serves ms_flood_kernel (work item blockIdx.x, the graph through plain global pointers) and
// ms_flood_codes_kernel (ldpc_codeset.hpp: work item w of a code, the graph through the constant address space).
// The two row passes below are the arithmetic of one block row for one lane; ms_flood_body calls them with its records in VGPRs,
// ms_flood_wide_codes_kernel (ldpc_codeset_wide.hpp) with its records in LDS.
// ---------------------------------------------------------------------------------------------------------
// STATE1 of a row: add the c2v value of each of the row's rw edges ed[e0 .. e0 + rw) into lds
template <class Edges>
__device__ __forceinline__ void ms_row_add(Edges ed, int e0, int rw, RowRec<double> o, bool wr, double *lds, Lane l, int M, int F) {
    const uint32_t mt = o.meta;
    const uint32_t par = __popc(mt & 0xffffu) & 1u;  // row sign = xor of the row's edge signs
    const uint32_t pos = mt >> kRowBits;
    for (int idx = 0; idx < rw; ++idx) {
        const int addr = edge_idx((uint32_t)ed[e0 + idx], l.n, M, F, l.f);
        const double aa = (pos == (uint32_t)idx) ? o.m2 : o.m1;
        const double cv = flip_if(aa, ((mt >> idx) ^ par) & 1u);
        if (wr) lds[addr] = lds[addr] + cv;
    }
}

// STATE3 of a row: the new record from v2c = soft - old c2v, o = the old record with m1 and m2 already multiplied by alpha;
// sy = the xor of the row's a-posteriori words (the sign bit is the syndrome)
template <class Edges>
__device__ __forceinline__ RowRec<double> ms_row_scan(Edges ed, int e0, int rw, RowRec<double> o, const double *lds, Lane l, int M, int F) {
    const uint32_t mt = o.meta;
    const uint32_t par = __popc(mt & 0xffffu) & 1u;
    const uint32_t pos = mt >> kRowBits;
    double nm1 = kMaxVal, nm2 = kMaxVal;
    uint32_t npos = 0, nS = 0, sy = 0;
    for (int idx = 0; idx < rw; ++idx) {
        const double r = lds[edge_idx((uint32_t)ed[e0 + idx], l.n, M, F, l.f)];
        sy ^= hi32(r);
        const double aa = (pos == (uint32_t)idx) ? o.m2 : o.m1;
        const double x = flip_if(aa, ((mt >> idx) ^ par) & 1u);
        const double t = r - x;                       // v2c
        nS |= (hi32(t) >> 31) << idx;
        const double v = fmin(fabs(t), kMaxVal);      // :4729-4730
        const bool c1 = v < nm1;                      // strict: first minimum keeps the position
        nm2 = fmin(fmax(v, nm1), nm2);                // = c1 ? nm1 : min(v, nm2)
        npos = c1 ? (uint32_t)idx : npos;
        nm1 = fmin(v, nm1);
    }
    return RowRec<double>{nm1, nm2, nS | (npos << kRowBits), sy};
}

template <int RHM, int NHM, bool MW, class RowStart, class Edges>
__device__ __forceinline__ void ms_flood_body(const DecArgs &a, double *lds, int w, RowStart rs, Edges ed) {
    // lds: [N][F] soft / acc, then one flag word (kept behind, so the base stays aligned)
    const int M = a.M, F = a.F, N = a.N, rh = a.rh, nh = a.nh;
    int *const sh_flag = (int *)(lds + (size_t)N * F);
    const double alpha = a.alpha;
    const Lane l = frame_lane<MW>(F, M, a.B, w);
    const int n = l.n, f = l.f;
    const bool valid = l.valid;

    double y[NHM];
#pragma unroll
    for (int k = 0; k < NHM; ++k) y[k] = (k < nh && l.live) ? a.llr[l.fr * N + k * M + n] + 0.0 : 0.0;

    double m1[RHM], m2[RHM];
    uint32_t meta[RHM];  // [15:0] v2c sign bit of the row's idx-th edge, [23:16] idx of the min1 edge
#pragma unroll
    for (int j = 0; j < RHM; ++j) { m1[j] = 0.0; m2[j] = 0.0; meta[j] = 0u; }  // :4579-4596

    FrameStop st = stop_init(l, a.maxiter);

    for (int iter = 0; iter < a.maxiter; ++iter) {
        const bool wr = !st.done && valid;  // this lane may store
        // ---- STATE1 (:4633-4667)
        if (wr) {
#pragma unroll
            for (int k = 0; k < NHM; ++k) if (k < nh) lds[(k * M + n) * F + f] = 0.0;
        }
        if (MW) __syncthreads();
#pragma unroll
        for (int j = 0; j < RHM; ++j) {
            if (j < rh) {
                const int e0 = rs[j], rw = rs[j + 1] - e0;
                ms_row_add(ed, e0, rw, RowRec<double>{m1[j], m2[j], meta[j], 0u}, wr, lds, l, M, F);
                if (MW) __syncthreads();  // the next block row adds into the same variables
            }
        }
        // ---- STATE2 (:4670-4685): multiply, then add -- two roundings (no FMA)
        if (wr) {
#pragma unroll
            for (int k = 0; k < NHM; ++k) {
                if (k < nh) {
                    const int o = (k * M + n) * F + f;
                    const double p = lds[o] * alpha;
                    lds[o] = y[k] + p;
                }
            }
        }
        if (MW) __syncthreads();
        // ---- STATE3 (:4690-4755)
        uint32_t failw = 0;
#pragma unroll
        for (int j = 0; j < RHM; ++j) {
            if (j < rh) {
                const int e0 = rs[j], rw = rs[j + 1] - e0;
                const RowRec<double> nr = ms_row_scan(ed, e0, rw, RowRec<double>{m1[j] * alpha, m2[j] * alpha, meta[j], 0u}, lds, l, M, F);
                failw |= nr.sy;
                if (!st.done) { m1[j] = nr.m1; m2[j] = nr.m2; meta[j] = nr.meta; }
            }
        }
        stop_vote<MW>(st, valid && (failw >> 31), l, F, sh_flag, iter + 1);  // :4761-4766
        if (stop_all<MW>(st)) break;
    }
    write_outputs(a, lds, l, st.res);
}

template <int RHM, int NHM, bool MW>
__global__ void __launch_bounds__(MW ? 512 : 64) ms_flood_kernel(const DecArgs a) {
    extern __shared__ double lds[];
    ms_flood_body<RHM, NHM, MW>(a, lds, blockIdx.x, a.row_start, a.edges);
}

// ---------------------------------------------------------------------------------------------------------
// Layered offset min-sum  (lmin_sum_decod_qc_lm, decoders.cpp:5064-5425, active branch :5106-5290 with
// MY_VERSION; semantics SURVEY Appendix A.3).  Block rows (layers) are strictly sequential; inside a layer
// every variable is touched by exactly one check, so the layer needs no synchronisation of its own.
//
// lms_row_layer is one layer for one lane.  Its two passes are run-time loops over the row's edges; nothing but the
// new record is carried from the first to the second, which reads the a-posteriori value again and repeats the
// subtraction (same operands, same rounding).  No variable of the layer has been written by then: a lane writes only
// the variable it has just read, and the block columns of a row are distinct.  The caller stores the record under
// its own condition.  Callers: lms_layered_body (records in VGPRs) and lms_layered_wide_codes_kernel
// (ldpc_codeset_wide.hpp, records in LDS).
// ---------------------------------------------------------------------------------------------------------
template <class Edges>
__device__ __forceinline__ RowRec<double> lms_row_layer(Edges ed, int e0, int rw, RowRec<double> o, bool wr, double *lds, Lane l, int M, int F) {
    const double beta = 0.4;  // :5163 (the alpha/beta arguments are dead upstream)
    const uint32_t mt = o.meta;
    const uint32_t par = __popc(mt & 0xffffu) & 1u;
    const uint32_t pos = mt >> kRowBits;
    double nm1 = kMaxVal, nm2 = kMaxVal;  // :5133-5134
    uint32_t npos = 0, nS = 0;
    for (int idx = 0; idx < rw; ++idx) {  // :5141-5177
        const double r = lds[edge_idx((uint32_t)ed[e0 + idx], l.n, M, F, l.f)];
        const double aa = (pos == (uint32_t)idx) ? o.m2 : o.m1;
        const double pc = flip_if(aa, ((mt >> idx) ^ par) & 1u);
        const double t = r - pc;
        nS |= (hi32(t) >> 31) << idx;   // sign kept even when the magnitude clips to 0 (:5164-5168)
        double mag = fabs(t) - beta;
        mag = mag < 0 ? 0 : mag;
        const bool c1 = mag < nm1;      // process_check_node :5012-5027
        nm2 = fmin(fmax(mag, nm1), nm2);
        npos = c1 ? (uint32_t)idx : npos;
        nm1 = fmin(mag, nm1);
    }
    const uint32_t npar = __popc(nS) & 1u;
    for (int idx = 0; idx < rw; ++idx) {  // :5182-5206
        const int addr = edge_idx((uint32_t)ed[e0 + idx], l.n, M, F, l.f);
        const double ao = (pos == (uint32_t)idx) ? o.m2 : o.m1;
        const double t = lds[addr] - flip_if(ao, ((mt >> idx) ^ par) & 1u);
        const double aa = (npos == (uint32_t)idx) ? nm2 : nm1;
        const double cv = flip_if(aa, ((nS >> idx) ^ npar) & 1u);
        if (wr) lds[addr] = t + cv;
    }
    return RowRec<double>{nm1, nm2, nS | (npos << kRowBits), 0u};
}

// The body serves lms_layered_kernel (work item blockIdx.x, plain global pointers) and lms_layered_codes_kernel
// (ldpc_codeset.hpp: work item w of a code, the constant address space).  The block-row loop unrolls RHM times and the
// per-row records stay in VGPRs: no scratch.  The syndrome is written out here; with row_syndrome the set kernel
// measured slower (profiles/kernel_refactor_time.txt).
template <int RHM, bool MW, class RowStart, class Edges>
__device__ __forceinline__ void lms_layered_body(const DecArgs &a, double *lds, int w, RowStart rs, Edges ed) {
    const int M = a.M, F = a.F, N = a.N, rh = a.rh, nh = a.nh;
    int *const sh_flag = (int *)(lds + (size_t)N * F);
    const Lane l = frame_lane<MW>(F, M, a.B, w);
    const int n = l.n, f = l.f;
    const bool valid = l.valid;

    if (valid) {
        for (int k = 0; k < nh; ++k)  // :5088 soft = y
            lds[(k * M + n) * F + f] = l.live ? a.llr[l.fr * N + k * M + n] + 0.0 : 0.0;
    }
    double m1[RHM], m2[RHM];
    uint32_t meta[RHM];
#pragma unroll
    for (int j = 0; j < RHM; ++j) { m1[j] = 0.0; m2[j] = 0.0; meta[j] = 0u; }
    if (MW) __syncthreads();

    // syndrome of the current soft values (check_syndrome, decoders.cpp:793-814)
    auto syndrome_fail = [&]() -> bool {
        uint32_t failw = 0;
        for (int j = 0; j < rh; ++j) {
            const int e0 = rs[j], e1 = rs[j + 1];
            uint32_t sy = 0;
            for (int e = e0; e < e1; ++e) {
                const uint32_t d = (uint32_t)ed[e];
                const int k = d >> 16, c = d & 0xffffu;
                sy ^= hi32(lds[(k * M + rot_idx(n, c, M)) * F + f]);
            }
            failw |= sy;
        }
        return valid && (failw >> 31);
    };

    FrameStop st = stop_init(l, a.maxiter);                            // res: :5424 when the loop runs dry
    stop_vote<MW>(st, syndrome_fail(), l, F, sh_flag, 1);              // :5111-5115; :5119 at iter 0 -> returns 0+1
    const bool at_entry = st.done && l.inb;                            // no layer ran: upstream's soft[] is y itself, -0.0 included
    for (int iter = 0; iter < a.maxiter; ++iter) {
        if (stop_all<MW>(st)) break;
        const bool wr = !st.done && valid;
#pragma unroll
        for (int j = 0; j < RHM; ++j) {
            if (j < rh) {
                const int e0 = rs[j], rw = rs[j + 1] - e0;
                const RowRec<double> nr = lms_row_layer(ed, e0, rw, RowRec<double>{m1[j], m2[j], meta[j], 0u}, wr, lds, l, M, F);
                if (!st.done) { m1[j] = nr.m1; m2[j] = nr.m2; meta[j] = nr.meta; }
                if (MW) __syncthreads();  // the next layer reads what this one wrote
            }
        }
        stop_vote<MW>(st, syndrome_fail(), l, F, sh_flag, iter + 1);   // :5281-5284; :5287, returns iter+1
    }
    write_outputs(a, lds, l, st.res);
    if (l.live && at_entry && a.soft_out)
        for (int k = 0; k < a.nh; ++k) a.soft_out[l.fr * N + k * M + n] = a.llr[l.fr * N + k * M + n];
}

template <int RHM, bool MW>
__global__ void __launch_bounds__(MW ? 512 : 64) lms_layered_kernel(const DecArgs a) {
    extern __shared__ double lds[];
    lms_layered_body<RHM, MW>(a, lds, blockIdx.x, a.row_start, a.edges);
}

// ---------------------------------------------------------------------------------------------------------
// Integer min-sum (imin_sum_decod_qc_lm, decoders.cpp:5430-5690; semantics SURVEY Appendix A.4): the flooding
// schedule of ms_flood_kernel on int16 values.  Input quantiser: coef = sqrt(N / sum y^2) with the sum taken in
// index order (a parallel reduction would round differently and could move a value across a quantiser boundary),
// q = floor(min(|y|*coef, thr)*max_quant/thr + 0.5) with the sign of y; c2v magnitudes are scaled (a*ialpha)>>4 in
// STATE1 and STATE3, STATE1 saturates at +-max_data after every add, STATE2 is sat(iy + acc) (no alpha).  Everything
// after the quantiser is integer arithmetic, so the GPU result is exact by construction; values never leave
// [-2*max_data, 2*max_data], so 32-bit lanes reproduce the reference's int16 arithmetic without wrap-around.
// LDS: one int32 per variable.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ims_sat(int x, int max_data) { return x > max_data ? max_data : (x < -max_data ? -max_data : x); }  // limit_val :4308

// The two row passes of integer min-sum for one lane, W = the LDS word of a variable: int in ims_flood_kernel, int16_t in
// ims_flood_codes_kernel (ldpc_codeset.hpp).  Both take the old record with m1 and m2 already scaled, (m * ialpha) >> 4.
// STATE1 of a row (:5540-5576): add the c2v value of each edge into lds, saturating after every add
template <class W, class Edges>
__device__ __forceinline__ void ims_row_add(Edges ed, int e0, int rw, RowRec<int> o, bool wr, W *lds, int max_data, Lane l, int M, int F) {
    const uint32_t mt = o.meta;
    const uint32_t par = __popc(mt & 0xffffu) & 1u;
    const uint32_t pos = mt >> kRowBits;
    for (int idx = 0; idx < rw; ++idx) {
        const int addr = edge_idx((uint32_t)ed[e0 + idx], l.n, M, F, l.f);
        const int tmp = (pos == (uint32_t)idx) ? o.m2 : o.m1;
        const int cv = (((mt >> idx) ^ par) & 1u) ? -tmp : tmp;
        if (wr) lds[addr] = (W)ims_sat((int)lds[addr] + cv, max_data);
    }
}

// STATE3 of a row (:5610-5678): the new record (unscaled) and sy = the xor of the row's a-posteriori words
template <class W, class Edges>
__device__ __forceinline__ RowRec<int> ims_row_scan(Edges ed, int e0, int rw, RowRec<int> o, const W *lds, int max_data, Lane l, int M, int F) {
    const uint32_t mt = o.meta;
    const uint32_t par = __popc(mt & 0xffffu) & 1u;
    const uint32_t pos = mt >> kRowBits;
    int nm1 = max_data, nm2 = max_data;
    uint32_t npos = 0, nS = 0, sy = 0;
    for (int idx = 0; idx < rw; ++idx) {
        const int r = lds[edge_idx((uint32_t)ed[e0 + idx], l.n, M, F, l.f)];
        sy ^= (uint32_t)r;
        const int val = (pos == (uint32_t)idx) ? o.m2 : o.m1;
        const int t = (((mt >> idx) ^ par) & 1u) ? -val : val;
        const int msg = r - t;
        nS |= ((uint32_t)msg >> 31) << idx;
        int v = msg < 0 ? -msg : msg;
        v = v > max_data ? max_data : v;
        if (v < nm1) { npos = idx; nm2 = nm1; nm1 = v; }
        else if (v < nm2) nm2 = v;
    }
    return RowRec<int>{nm1, nm2, nS | (npos << kRowBits), sy};
}

template <int RHM, int NHM, bool MW>
__global__ void __launch_bounds__(MW ? 512 : 64) ims_flood_kernel(const DecArgs a) {
    extern __shared__ double lds_raw[];
    int *const lds = reinterpret_cast<int *>(lds_raw);  // [N][F] soft / acc
    const int M = a.M, F = a.F, N = a.N, rh = a.rh, nh = a.nh;
    int *const sh_flag = lds + (size_t)N * F;
    const int max_data = (1 << (a.ims_dbits - 1)) - 1;   // :5445
    const int max_quant = (1 << (a.ims_qbits - 1)) - 1;  // :5446
    const int ialpha = (int)(a.alpha * (1 << 4));         // :5458 MS_ALPHA_FPP = 4
    const Lane l = frame_lane<MW>(F, M, a.B, blockIdx.x);
    const int n = l.n, f = l.f;
    const bool valid = l.valid;

    // :5472-5500 energy-normalised quantiser.  Every lane of a frame walks the frame's LLRs in index order (same
    // addresses within the frame: broadcast loads), so all of them hold the identical, sequentially rounded sum.
    int iy[NHM];
    {
        double en = 0;
        const double *yf = a.llr + (l.inb ? l.fr : 0) * (long long)N;
        for (int i = 0; i < N; ++i) { const double v = yf[i]; en += v * v; }
        const double coef = sqrt((double)N / en);
#pragma unroll
        for (int k = 0; k < NHM; ++k) {
            iy[k] = 0;
            if (k < nh && l.live) {
                double val = yf[k * M + n];
                int sign = 0;
                if (val < 0) { val = -val; sign = 1; }
                val *= coef;
                if (val > a.ims_thr) val = a.ims_thr;
                const int ival = (int)(short)floor(val * max_quant / a.ims_thr + 0.5);
                iy[k] = sign ? -ival : ival;
            }
        }
    }
    int m1[RHM], m2[RHM];
    uint32_t meta[RHM];
#pragma unroll
    for (int j = 0; j < RHM; ++j) { m1[j] = 0; m2[j] = 0; meta[j] = 0u; }

    FrameStop st = stop_init(l, a.maxiter);
    for (int iter = 0; iter < a.maxiter; ++iter) {
        const bool wr = !st.done && valid;
        if (wr) {
#pragma unroll
            for (int k = 0; k < NHM; ++k) if (k < nh) lds[(k * M + n) * F + f] = 0;
        }
        if (MW) __syncthreads();
#pragma unroll
        for (int j = 0; j < RHM; ++j) {   // STATE1
            if (j < rh) {
                const int e0 = a.row_start[j], rw = a.row_start[j + 1] - e0;
                ims_row_add(a.edges, e0, rw, RowRec<int>{(m1[j] * ialpha) >> 4, (m2[j] * ialpha) >> 4, meta[j], 0u}, wr, lds, max_data, l, M, F);
                if (MW) __syncthreads();
            }
        }
        if (wr) {                          // STATE2 :5579-5604
#pragma unroll
            for (int k = 0; k < NHM; ++k) {
                if (k < nh) {
                    const int o = (k * M + n) * F + f;
                    lds[o] = ims_sat(iy[k] + lds[o], max_data);
                }
            }
        }
        if (MW) __syncthreads();
        uint32_t failw = 0;
#pragma unroll
        for (int j = 0; j < RHM; ++j) {   // STATE3
            if (j < rh) {
                const int e0 = a.row_start[j], rw = a.row_start[j + 1] - e0;
                const RowRec<int> nr = ims_row_scan(a.edges, e0, rw, RowRec<int>{(m1[j] * ialpha) >> 4, (m2[j] * ialpha) >> 4, meta[j], 0u}, lds, max_data, l, M, F);
                failw |= nr.sy;
                if (!st.done) { m1[j] = nr.m1; m2[j] = nr.m2; meta[j] = nr.meta; }
            }
        }
        stop_vote<MW>(st, valid && (failw >> 31), l, F, sh_flag, iter + 1);  // :5684-5689
        if (stop_all<MW>(st)) break;
    }
    frame_outputs(a, F, l, st.res, [=](int i) { return (uint32_t)lds[i] >> 31; }, [=](int i) { return (double)lds[i]; });
}

}  // namespace ldpc
