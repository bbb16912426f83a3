// FHT_DEC (decoder id 6): sum-product decoding of QC-LDPC codes over GF(q), q = 2^p, with the check nodes in the Walsh-Hadamard
// domain -- upstream's sum_prod_gfq_decod_lm (decoders.cpp:7036-7694, the SUM_PROD_GFQ_ORIG build) with map_graph (:6269-6391).
//
// One workgroup decodes one frame at a time, all iterations, in one launch.  The frame is decode_frame<QL, LPC>, written once; two
// schedulers hand it frames: gfq_kernel here (one code: workgroup w takes frames w, w + grid, ...) and gfq_codes_kernel of
// ldpc_gfq_codeset.hpp (a set of codes: work items (code, frame), each on the Args view of its code).  The message
// state of a frame does not fit a CU's LDS in general, so it lives in a per-workgroup slot of a workspace in global memory (L2 /
// Infinity Cache resident for the codes this decoder is used on), laid out for the machine and not like upstream:
//   win  [E][M][q]   upstream's fht_soft_in   (symbol -> check), edge e = row_start[j] + slot, check lane k, q values contiguous
//   wout [E][M][q]   upstream's fht_soft_outs (check -> symbol), same indexing
//   post [N][q]      upstream's fht_soft_out  (a-posteriori vectors)
//   qh   [N]         upstream's qhard
// so that a check node or a symbol node moves whole q * 8 byte vectors.
//
// Check node (the hot path): LPC lanes share one check, each lane keeps QL = q / LPC consecutive values of a vector in VGPRs under
// static indices.  Butterfly stages below QL run inside the lane, the log2(LPC) stages above it exchange with lane ^ 1, ^ 2, ...
// (quad-perm DPP for distances 1 and 2, ds_bpermute beyond); stage order and the a - b orientation are upstream's, so every sum is
// the same IEEE operation on the same operands.  The two permutations of map_graph (by the division table before the transform, by
// the multiplication table after the inverse one) are folded into the addresses of the loads and stores -- both are gathers /
// scatters with the division table, because mul and div by one coefficient are inverse permutations -- so no register is ever
// indexed at run time.  The rw transformed vectors of a check go to the check's own wout vectors (which the second pass overwrites
// with the results anyway) and the forward products to its own win vectors (which the symbol nodes rewrite in full afterwards): the
// second pass finds both in the cache of the CU that wrote them.
//   q = 16: QL 16, LPC 1 (no cross-lane traffic at all);  q = 64: QL 16, LPC 4 (two DPP stages);
//   generic: QL 4 (q <= 256), 8 (q = 512), 16 (q = 1024) with LPC = q / QL <= 64 read at run time.
//
// Arithmetic: IEEE fp64, no contraction (the library is built with -ffp-contract=off), correctly rounded division, every compare
// written as upstream writes it (`max < x`, `x < 0.00001`) so that Inf / NaN take upstream's path too.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ldpc_gfq {

struct Args {
    const double *soft;   // [B][q][N]
    int16_t *qhard;       // [B][N] or null
    int32_t *iters;       // [B] or null
    double *post;         // [B][q][N] or null
    char *ws;
    size_t ws_stride;     // bytes per workgroup slot
    long long B;
    int maxiter;
    int rh, nh, M, N, R, E, q, lpc, cw2;
    const int32_t *row_start;   // [rh + 1]
    const int32_t *e_col;       // [E] block column of edge e
    const int32_t *e_circ;      // [E] shift
    const int32_t *e_rl;        // [E] index of the edge's coefficient in the tables (upstream's hc_rl)
    const int32_t *col_start;   // [nh + 1]
    const int32_t *ce_edge;     // [E] edges of a block column in ascending row order (upstream's hb_ci + posh)
    const int16_t *mul;         // [ncoef][q] mul[c][s] = s * coef_c
    const int16_t *div;         // [ncoef][q] div[c][s] = s / coef_c
};

// bytes of the four arrays of one slot, each aligned to 256
__host__ __device__ inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
__host__ __device__ inline size_t msg_bytes(int E, int M, int q) { return align256(sizeof(double) * (size_t)E * M * q); }
__host__ __device__ inline size_t post_bytes(int N, int q) { return align256(sizeof(double) * (size_t)N * q); }
__host__ __device__ inline size_t slot_bytes(int E, int M, int N, int q) {
    return 2 * msg_bytes(E, M, q) + post_bytes(N, q) + align256(sizeof(int16_t) * (size_t)N);
}

#if defined(__HIPCC__)

// value of lane ^ D (D = 1, 2: quad-perm DPP on the two halves; else ds_bpermute through __shfl_xor)
template <int D>
__device__ __forceinline__ double lane_xor_dpp(double x) {
    static_assert(D == 1 || D == 2, "quad perm reaches lane ^ 1 and lane ^ 2");
    constexpr int ctrl = D == 1 ? 0xB1 : 0x4E;   // quad_perm [1,0,3,2] / [2,3,0,1]
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(b & 0xffffffffLL), ctrl, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), ctrl, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// Walsh-Hadamard transform of a q = QL * lpc vector spread over lpc lanes, y[r] = element sub * QL + r: stage i pairs the indices
// that differ in bit i, low stage first; the lower index receives a + b, the upper a - b (decoders.cpp:5742-6111).
template <int QL, int LPC>
__device__ __forceinline__ void fht(double (&y)[QL], int sub, int lpc) {
#pragma unroll
    for (int f = 1; f < QL; f <<= 1) {
#pragma unroll
        for (int j0 = 0; j0 < QL; ++j0) {
            if (j0 & f) continue;
            const double a = y[j0], b = y[j0 + f];
            y[j0] = a + b;
            y[j0 + f] = a - b;
        }
    }
    if constexpr (LPC == 4) {
#pragma unroll
        for (int r = 0; r < QL; ++r) { const double o = lane_xor_dpp<1>(y[r]); y[r] = (sub & 1) ? o - y[r] : y[r] + o; }
#pragma unroll
        for (int r = 0; r < QL; ++r) { const double o = lane_xor_dpp<2>(y[r]); y[r] = (sub & 2) ? o - y[r] : y[r] + o; }
    } else if constexpr (LPC == 0) {
        for (int d = 1; d < lpc; d <<= 1) {
#pragma unroll
            for (int r = 0; r < QL; ++r) { const double o = __shfl_xor(y[r], d); y[r] = (sub & d) ? o - y[r] : y[r] + o; }
        }
    }
}

// map_graph for every check of the frame.  LPC == 0: lanes per check from a.lpc.
template <int QL, int LPC>
__device__ __forceinline__ void check_nodes(const Args &a, double *win, double *wout) {
    const int lpc = LPC ? LPC : a.lpc;
    const int q = QL * lpc;
    const int sub = (int)threadIdx.x % lpc;
    const int per_pass = (int)blockDim.x / lpc;
    const double qinv = 1.0 / (double)q;
    for (int c = (int)threadIdx.x / lpc; c < a.R; c += per_pass) {   // the lanes of a check stay together: every exchange is inside the group
        const int j = c / a.M, k = c - j * a.M;
        const int e0 = a.row_start[j], rw = a.row_start[j + 1] - e0;
        double F[QL], S[QL];
        // permute, transform, forward products F[s] = S[s] * F[s-1]
        for (int s = 0; s < rw; ++s) {
            const int e = e0 + s;
            const int16_t *dv = a.div + (size_t)a.e_rl[e] * q + sub * QL;
            double *v = win + ((size_t)e * a.M + k) * q;
            double *o = wout + ((size_t)e * a.M + k) * q + sub * QL;
#pragma unroll
            for (int r = 0; r < QL; ++r) S[r] = v[dv[r]];
            fht<QL, LPC>(S, sub, lpc);
#pragma unroll
            for (int r = 0; r < QL; ++r) o[r] = S[r];
            if (s == 0) {
#pragma unroll
                for (int r = 0; r < QL; ++r) F[r] = S[r];
            } else {
#pragma unroll
                for (int r = 0; r < QL; ++r) F[r] = S[r] * F[r];
            }
            if (s < rw - 1) {   // every lane of the group has read v before any of them gets here: the stored values depend on the loads
#pragma unroll
                for (int r = 0; r < QL; ++r) v[sub * QL + r] = F[r];
            }
        }
        // backward products B[s] = S[s] * B[s+1], Z = F[s-1] * B[s+1], transform back, un-permute, scale, clamp
        double Bk[QL], Z[QL];
        for (int s = rw - 1; s >= 0; --s) {
            const int e = e0 + s;
            const int16_t *dv = a.div + (size_t)a.e_rl[e] * q + sub * QL;
            double *o = wout + ((size_t)e * a.M + k) * q;
            const double *fp = win + ((size_t)(e - 1) * a.M + k) * q + sub * QL;
#pragma unroll
            for (int r = 0; r < QL; ++r) S[r] = o[sub * QL + r];
            if (s == rw - 1) {
#pragma unroll
                for (int r = 0; r < QL; ++r) Z[r] = fp[r];
            } else if (s == 0) {
#pragma unroll
                for (int r = 0; r < QL; ++r) Z[r] = Bk[r];
            } else {
#pragma unroll
                for (int r = 0; r < QL; ++r) Z[r] = fp[r] * Bk[r];
            }
            fht<QL, LPC>(Z, sub, lpc);
            if (lpc > 1) __builtin_amdgcn_s_waitcnt(0);   // the group's loads of S have landed before its scatter rewrites the vector
#pragma unroll
            for (int r = 0; r < QL; ++r) {
                double x = Z[r] * qinv;
                if (x < 0.00001) x = 0.00001;
                o[dv[r]] = x;   // out[i] = s[mul[i]]  <=>  out[div[t]] = s[t]
            }
            if (s == rw - 1) {
#pragma unroll
                for (int r = 0; r < QL; ++r) Bk[r] = S[r];
            } else {
#pragma unroll
                for (int r = 0; r < QL; ++r) Bk[r] = S[r] * Bk[r];
            }
        }
    }
}

// symbol nodes, one variable per lane; sums over the q symbols ascend from 0 (decoders.cpp:7309-7597, COLUMN_BY_COLUMN)
__device__ __forceinline__ void symbol_nodes(const Args &a, const double *soft, double *win, const double *wout, double *post) {
    const int q = a.q, M = a.M, N = a.N;
    for (int i = (int)threadIdx.x; i < N; i += (int)blockDim.x) {
        const int col = i / M, k = i - col * M;
        const int c0 = a.col_start[col], cw = a.col_start[col + 1] - c0;
        const double *x = soft + i;
        double *p = post + (size_t)i * q;
        auto vec = [&](int kk) -> size_t {   // the vector of this variable on the kk-th edge of its block column
            const int e = a.ce_edge[c0 + kk];
            int idx = k - a.e_circ[e];
            if (idx < 0) idx += M;
            return ((size_t)e * M + idx) * q;
        };
        if (a.cw2) {   // every block column has weight 2 (:7310-7432)
            const size_t d0 = vec(0), d1 = vec(1);
            double sa = 0, sb = 0, sc = 0;
            for (int j = 0; j < q; ++j) {
                const double b0 = wout[d0 + j], b1 = wout[d1 + j], xv = x[(size_t)j * N];
                const double y0 = xv * b0, y1 = xv * b1;
                const double so = y1 * b0;
                win[d0 + j] = y1;
                win[d1 + j] = y0;
                p[j] = so;
                sa += so; sb += y1; sc += y0;
            }
            sa = 1.0 / sa; sb = 1.0 / sb; sc = 1.0 / sc;
            for (int j = 0; j < q; ++j) {
                p[j] *= sa;
                win[d0 + j] *= sb;
                win[d1 + j] *= sc;
            }
        } else if (cw == 2) {   // (:7446-7518)
            const size_t d0 = vec(0), d1 = vec(1);
            double sum = 0;
            for (int j = 0; j < q; ++j) { const double v = x[(size_t)j * N] * wout[d0 + j] * wout[d1 + j]; p[j] = v; sum += v; }
            sum = 1.0 / sum;
            for (int j = 0; j < q; ++j) p[j] *= sum;
            sum = 0;
            for (int j = 0; j < q; ++j) { const double v = x[(size_t)j * N] * wout[d1 + j]; win[d0 + j] = v; sum += v; }
            sum = 1.0 / sum;
            for (int j = 0; j < q; ++j) win[d0 + j] *= sum;
            sum = 0;
            for (int j = 0; j < q; ++j) { const double v = x[(size_t)j * N] * wout[d0 + j]; win[d1 + j] = v; sum += v; }
            sum = 1.0 / sum;
            for (int j = 0; j < q; ++j) win[d1 + j] *= sum;
        } else {   // (:7520-7590)
            double sum = 0;
            for (int j = 0; j < q; ++j) {
                double v = x[(size_t)j * N];
                for (int kk = 0; kk < cw; ++kk) v *= wout[vec(kk) + j];
                p[j] = v;
                sum += v;
            }
            sum = 1.0 / sum;
            for (int j = 0; j < q; ++j) p[j] *= sum;
            for (int kk = 0; kk < cw; ++kk) {
                const size_t d = vec(kk);
                double s2 = 0;
                for (int j = 0; j < q; ++j) { const double v = p[j] / wout[d + j]; win[d + j] = v; s2 += v; }
                s2 = 1.0 / s2;
                for (int j = 0; j < q; ++j) win[d + j] *= s2;
            }
        }
    }
}

// The four arrays of a workgroup's slot of the workspace (slot_bytes), for a code with a.E edges.
struct Slot {
    double *win, *wout, *post;
    int16_t *qh;
};
__device__ __forceinline__ Slot carve_slot(const Args &a, char *slot) {
    return {(double *)slot, (double *)(slot + msg_bytes(a.E, a.M, a.q)), (double *)(slot + 2 * msg_bytes(a.E, a.M, a.q)),
            (int16_t *)(slot + 2 * msg_bytes(a.E, a.M, a.q) + post_bytes(a.N, a.q))};
}

// One frame, start to end, by the whole workgroup: soft [q][N] is the frame's input, st the workgroup's slot, and the frame's results
// go to row `item` of the outputs that a has (a.qhard, a.iters, a.post; null = not wanted).  Both schedulers -- gfq_kernel below and
// gfq_codes_kernel (ldpc_gfq_codeset.hpp, on the view of one code of a set) -- decode through this function, which is why a code
// gives the same bits in a set as alone.  The output addresses are formed at the end, from a and item, and the slot is carved by
// the caller (once per launch here, once per item in a set): either one done the other way costs scalar registers through the
// iteration loop (profiles/frame_tally_refactor_resources.txt).
template <int QL, int LPC>
__device__ __forceinline__ void decode_frame(const Args &a, const double *soft, const Slot &st, size_t item) {
    double *const win = st.win, *const wout = st.wout, *const post = st.post;
    int16_t *const qh = st.qh;
    const int q = a.q, M = a.M, N = a.N;
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;

    // symbol -> check messages and a-posteriori vectors start as the input (:7081-7104)
    for (int t = tid; t < a.E * M; t += nt) {
        const int e = t / M, k = t - e * M;
        int n = k + a.e_circ[e];
        if (n >= M) n -= M;
        const double *x = soft + a.e_col[e] * M + n;
        double *v = win + (size_t)t * q;
        for (int j = 0; j < q; ++j) v[j] = x[(size_t)j * N];
    }
    for (int i = tid; i < N; i += nt)
        for (int j = 0; j < q; ++j) post[(size_t)i * q + j] = soft[(size_t)j * N + i];
    __syncthreads();

    int result = -a.maxiter;
    for (int iter = 0; iter < a.maxiter; ++iter) {
        for (int i = tid; i < N; i += nt) {   // hard decision: first index of the strict maximum (:7124-7143)
            double mx = 0.0;
            int pos = 0;
            const double *p = post + (size_t)i * q;
            for (int j = 0; j < q; ++j)
                if (mx < p[j]) { mx = p[j]; pos = j; }
            qh[i] = (int16_t)pos;
        }
        __syncthreads();
        int syn = 0;   // syndrome over GF(q) (:5695-5736)
        for (int c = tid; c < a.R; c += nt) {
            const int j = c / M, k = c - j * M;
            int acc = 0;
            for (int e = a.row_start[j]; e < a.row_start[j + 1]; ++e) {
                int n = k + a.e_circ[e];
                if (n >= M) n -= M;
                acc ^= a.mul[(size_t)a.e_rl[e] * q + qh[a.e_col[e] * M + n]];
            }
            syn |= acc;
        }
        if (!__syncthreads_or(syn)) { result = iter; break; }
        check_nodes<QL, LPC>(a, win, wout);
        __syncthreads();
        symbol_nodes(a, soft, win, wout, post);
        __syncthreads();
    }
    if (tid == 0 && a.iters) a.iters[item] = result;
    if (a.qhard)
        for (int i = tid; i < N; i += nt) a.qhard[item * N + i] = qh[i];
    if (a.post) {
        double *po = a.post + item * q * N;
        for (int i = tid; i < N; i += nt)
            for (int j = 0; j < q; ++j) po[(size_t)j * N + i] = post[(size_t)i * q + j];
    }
    __syncthreads();   // the slot is free for the workgroup's next frame, which in a set may belong to another code
}

// The single-code scheduler: workgroup w decodes frames w, w + grid, ... in its slot.
template <int QL, int LPC>
__global__ __launch_bounds__(256) void gfq_kernel(const Args a) {
    const Slot st = carve_slot(a, a.ws + (size_t)blockIdx.x * a.ws_stride);
    for (long long b = blockIdx.x; b < a.B; b += gridDim.x)
        decode_frame<QL, LPC>(a, a.soft + (size_t)b * a.q * a.N, st, (size_t)b);
}

#endif  // __HIPCC__

}  // namespace ldpc_gfq
