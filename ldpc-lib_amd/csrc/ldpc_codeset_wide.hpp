// ldpc_codeset_wide.hpp -- min-sum and layered min-sum code sets at any number of block rows and columns (gfx950).
//
// ms_flood_codes_kernel and lms_layered_codes_kernel (ldpc_codeset.hpp) keep the per-check records m1 / m2 / meta of all block rows in
// VGPRs under an unrolled block-row loop (16 rows), and the flooding kernel the channel LLRs of 32 block columns.  The kernels here
// call the same row passes (ms_row_add, ms_row_scan, lms_row_layer) with the records in LDS, so every loop over block rows or block
// columns is a run-time loop:
//   * soft[N][F] fp64 at the front of the image, as in the register-resident kernels (write_outputs reads it there);
//   * m1[R][F], m2[R][F] fp64 and meta[R][F], R = rh * M: the record of check n of block row j is entry (j * M + n) * F + f of each
//     array, so consecutive lanes touch consecutive words.  meta is the u32 of the registers ([15:0] sign bit of the row's idx-th v2c
//     value, [23:16] slot of min1) in an 8-byte slot: all three arrays are read and written as b64 words under one index;
//   * F * (8 * N + 24 * R) bytes, rounded up to 16 (wide_codes_image_bytes), then the vote flag's 16.
// A record is read and written only by lane n of frame f: it needs no barrier beyond those the soft values need.
// The flooding kernel reads the channel LLRs from memory again in STATE2 of every iteration (the + 0.0 canonicalisation with them): a
// set's shared LLRs are read by every code and stay in L2, and a second [N][F] array would take 8 * N * F bytes more of the image
// (112 576 instead of 80 416 bytes at 30 x 60, M = 67).  Both were measured on 30 x 60 at M = 67, 4096 frames per code,
// 50 iterations: 354 ms re-read against 667 ms in LDS at 16 codes, 2806 against 5343 ms at 128 -- the 112 576-byte image leaves one
// workgroup per CU where 80 416 bytes leave two -- and the LDS variant was removed (profiles/r22_codeset_wide_time.txt).
// Measured against what these shapes ran on before (one context per code on the shape-unlimited tier): 30 x 60, M = 67: MS 1.29x as
// fast at 16 and at 256 codes, LMS 2.23x and 2.25x.  Where the register-resident set kernels fit (16 x 32, M = 64) these kernels are
// 3.1 - 3.4x SLOWER than they: three workgroups per CU instead of nine, loops not unrolled.  They are the route beyond the limits only.
// A converged frame of a packed wave (and a frame beyond B) stores nothing more: its records and outputs stay as they were.
// Row weight stays 1 .. 16 (the sign bits of meta), M <= 512.
#pragma once

#include "ldpc_codeset.hpp"

namespace ldpc {

__host__ __device__ inline size_t wide_codes_image_bytes(int F, int N, int R) {   // soft, m1, m2 and meta, in front of the vote flag
    return ((size_t)F * (8 * (size_t)N + 24 * (size_t)R) + 15) & ~(size_t)15;
}

// The records of a workgroup's frames behind soft[N][F]
struct WideRecords {
    double *m1, *m2;
    uint2 *meta;
    int *sh_flag;
};

__device__ __forceinline__ WideRecords wide_records(double *lds, int F, int N, int R) {
    WideRecords r;
    r.m1 = lds + (size_t)N * F;
    r.m2 = r.m1 + (size_t)R * F;
    r.meta = reinterpret_cast<uint2 *>(r.m2 + (size_t)R * F);
    r.sh_flag = reinterpret_cast<int *>(reinterpret_cast<char *>(lds) + wide_codes_image_bytes(F, N, R));
    return r;
}

// ---------------------------------------------------------------------------------------------------------
// Flooding normalised min-sum (decoders.cpp:4554-4767) on work item (c, w): ms_flood_body's frame (ldpc_kernels.hpp) around the same
// two row passes, ms_row_add and ms_row_scan, with the records read from and stored to LDS under wr and the channel value of
// STATE2 (two roundings) read from memory.
// ---------------------------------------------------------------------------------------------------------
template <bool MW>
__global__ void __launch_bounds__(MW ? 512 : 64) ms_flood_wide_codes_kernel(const CodesetArgs s) {
    extern __shared__ double lds[];
    int w;
    const DecArgs a = codeset_view(s, w);
    const TabPtr rs = tab_ptr(a.row_start), ed = tab_ptr(a.edges);
    const int M = a.M, F = a.F, N = a.N, rh = a.rh, nh = a.nh;
    const WideRecords rec = wide_records(lds, F, N, rh * M);
    const double alpha = a.alpha;
    const Lane l = frame_lane<MW>(F, M, a.B, w);
    const int n = l.n, f = l.f;
    const bool valid = l.valid;

    if (valid) {
        for (int j = 0; j < rh; ++j) {                                              // :4579-4596
            const int ri = (j * M + n) * F + f;
            rec.m1[ri] = 0.0; rec.m2[ri] = 0.0; rec.meta[ri] = make_uint2(0u, 0u);
        }
    }

    FrameStop st = stop_init(l, a.maxiter);
    for (int iter = 0; iter < a.maxiter; ++iter) {
        const bool wr = !st.done && valid;  // this lane may store; its frame exists
        // ---- STATE1 (:4633-4667)
        if (wr)
            for (int k = 0; k < nh; ++k) lds[(k * M + n) * F + f] = 0.0;
        if (MW) __syncthreads();
        for (int j = 0; j < rh; ++j) {
            const int e0 = rs[j], rw = rs[j + 1] - e0;
            const int ri = (j * M + n) * F + f;
            ms_row_add(ed, e0, rw, RowRec<double>{rec.m1[ri], rec.m2[ri], rec.meta[ri].x, 0u}, wr, lds, l, M, F);
            if (MW) __syncthreads();  // the next block row adds into the same variables
        }
        // ---- STATE2 (:4670-4685): multiply, then add -- two roundings (no FMA); the channel value from memory, canonicalised
        if (wr) {
            const double *const yf = a.llr + l.fr * N + n;
            for (int k = 0; k < nh; ++k) {
                const int o = (k * M + n) * F + f;
                const double y = yf[k * M] + 0.0;
                const double p = lds[o] * alpha;
                lds[o] = y + p;
            }
        }
        if (MW) __syncthreads();
        // ---- STATE3 (:4690-4755)
        uint32_t failw = 0;
        for (int j = 0; j < rh; ++j) {
            const int e0 = rs[j], rw = rs[j + 1] - e0;
            const int ri = (j * M + n) * F + f;
            const RowRec<double> nr = ms_row_scan(ed, e0, rw, RowRec<double>{rec.m1[ri] * alpha, rec.m2[ri] * alpha, rec.meta[ri].x, 0u}, lds, l, M, F);
            failw |= nr.sy;
            if (wr) { rec.m1[ri] = nr.m1; rec.m2[ri] = nr.m2; rec.meta[ri] = make_uint2(nr.meta, 0u); }
        }
        stop_vote<MW>(st, valid && (failw >> 31), l, F, rec.sh_flag, iter + 1);  // :4761-4766
        if (stop_all<MW>(st)) break;
    }
    write_outputs(a, lds, l, st.res);
}

// ---------------------------------------------------------------------------------------------------------
// Layered offset min-sum (decoders.cpp:5064-5425) on work item (c, w): lms_layered_body's frame (ldpc_kernels.hpp) around the same
// lms_row_layer, one call per layer, with the records read from and stored to LDS under wr; result 1 at entry, then iter + 1; the
// soft output is the LLR itself, -0.0 included, when no layer ran.
// ---------------------------------------------------------------------------------------------------------
template <bool MW>
__global__ void __launch_bounds__(MW ? 512 : 64) lms_layered_wide_codes_kernel(const CodesetArgs s) {
    extern __shared__ double lds[];
    int w;
    const DecArgs a = codeset_view(s, w);
    const TabPtr rs = tab_ptr(a.row_start), ed = tab_ptr(a.edges);
    const int M = a.M, F = a.F, N = a.N, rh = a.rh, nh = a.nh;
    const WideRecords rec = wide_records(lds, F, N, rh * M);
    const Lane l = frame_lane<MW>(F, M, a.B, w);
    const int n = l.n, f = l.f;
    const bool valid = l.valid;

    if (valid) {
        for (int k = 0; k < nh; ++k)
            lds[(k * M + n) * F + f] = l.live ? a.llr[l.fr * N + k * M + n] + 0.0 : 0.0;
        for (int j = 0; j < rh; ++j) {
            const int ri = (j * M + n) * F + f;
            rec.m1[ri] = 0.0; rec.m2[ri] = 0.0; rec.meta[ri] = make_uint2(0u, 0u);
        }
    }
    if (MW) __syncthreads();

    auto syndrome_fail = [&]() -> bool {
        return valid && (row_syndrome(rs, ed, rh, l, M, F, [=](int i) { return hi32(lds[i]); }) >> 31);
    };

    FrameStop st = stop_init(l, a.maxiter);
    stop_vote<MW>(st, syndrome_fail(), l, F, rec.sh_flag, 1);
    const bool at_entry = st.done && l.inb;   // no layer ran: upstream's soft[] is y itself, -0.0 included
    for (int iter = 0; iter < a.maxiter; ++iter) {
        if (stop_all<MW>(st)) break;
        const bool wr = !st.done && valid;
        for (int j = 0; j < rh; ++j) {
            const int e0 = rs[j], rw = rs[j + 1] - e0;
            const int ri = (j * M + n) * F + f;
            const RowRec<double> nr = lms_row_layer(ed, e0, rw, RowRec<double>{rec.m1[ri], rec.m2[ri], rec.meta[ri].x, 0u}, wr, lds, l, M, F);
            if (wr) { rec.m1[ri] = nr.m1; rec.m2[ri] = nr.m2; rec.meta[ri] = make_uint2(nr.meta, 0u); }
            if (MW) __syncthreads();   // the next layer reads what this one wrote
        }
        stop_vote<MW>(st, syndrome_fail(), l, F, rec.sh_flag, iter + 1);
    }
    write_outputs(a, lds, l, st.res);
    if (l.live && at_entry && a.soft_out)
        for (int k = 0; k < nh; ++k) a.soft_out[l.fr * N + k * M + n] = a.llr[l.fr * N + k * M + n];
}

}  // namespace ldpc
