// ldpc_gfq_codeset.hpp -- C candidate codes over GF(q) of one shape (rh x nh, lifting M) x B frames in ONE launch (gfx950): the
// code-set layer of ldpc_codeset.hpp for FHT_DEC (ldpc_gfq.hpp).
//
// The caller is upstream's second search driver (search_ggp/scenario_based_code_generation.cpp:692-940): candidates that differ in
// the shifts and the coefficients of one pattern, each scored over the SAME noise.  A candidate is tiny (the shipped one is a
// 64-symbol code), so the cost per call -- launches, a synchronisation, the same channel output drawn again -- is what a set saves.
//   * graph data: one concatenated int32 table; code c owns the record tab[code_off[c] ...] =
//         E, cw2, row_start[rh+1], col_start[nh+1], e_col[E], e_circ[E], e_rl[E], ce_edge[E]
//     -- everything ldpc_gfq::Args holds per code.  e_rl = coefficient - 1: the multiplication and division tables are made once per
//     set for all q - 1 coefficients, so a record holds no coefficient list;
//   * work item w in [0, n_active * B): slot s = w / B, frame f = w % B, code c = code_list ? code_list[s] : s.  Workgroup g takes
//     items g, g + grid, ... as gfq_kernel takes frames, and finds the state of the item in its own slot of the workspace (sized by
//     the largest E of the set).  The code index is uniform over the workgroup: the list, the offset and the record's header are
//     read through the constant address space, so they are scalar loads and the view of the code stays in scalar registers;
//   * the record and a per-code soft slice follow the code; qhard, iters and post follow the slot ([n_active][B]..., which is
//     index w itself);
//   * a workgroup that moves on to an item of another code builds that code's view -- record, E, cw2 -- and carves its slot by that
//     E before the item's first instruction, and the barrier that ends an item stands between the two.
// gfq_codes_kernel is only this scheduler.  The frame itself -- initial messages, hard decision, syndrome, check nodes, symbol nodes,
// outputs -- is decode_frame<QL, LPC> of ldpc_gfq.hpp on that view, the function gfq_kernel calls for a single code: one statement
// of the frame, hence bit-identical to a single-code context.
#pragma once

#include "ldpc_codeset.hpp"   // TabPtr
#include "ldpc_gfq.hpp"
#include "ldpc_gfq_chain.hpp" // gfq_symbol_probabilities

namespace ldpc_gfq {

struct CodesArgs {
    const double *soft;           // [B][q][N] (soft_code_stride == 0) or [C][B][q][N] (soft_code_stride == B * q * N)
    int16_t *qhard;               // [n_active][B][N] or null
    int32_t *iters;               // [n_active][B] or null
    double *post;                 // [n_active][B][q][N] or null
    char *ws;
    size_t ws_stride;             // bytes per workgroup slot, for the largest E of the set
    const int32_t *tab;           // concatenated per-code records
    const int32_t *code_off;      // [C] offset of code c's record in tab
    const int32_t *code_list;     // [n_active] the code of every slot, or null: slot s decodes code s
    long long soft_code_stride;
    unsigned B, items;            // frames per code, n_active * B
    int maxiter;
    int rh, nh, M, N, R, q, lpc;
    const int16_t *mul;           // [q - 1][q] mul[coef - 1][s]
    const int16_t *div;           // [q - 1][q]
};

constexpr int kRecHeader = 2;     // E, cw2
__host__ __device__ inline size_t record_length(int rh, int nh, int E) { return (size_t)kRecHeader + rh + 1 + nh + 1 + 4 * (size_t)E; }

#if defined(__HIPCC__)

// The single-code argument block of code c.  Everything is a function of kernel arguments and of c, which is wave-uniform.  The
// outputs are the set's, rows by work item; soft stays null: the caller chooses the item's slice.
__device__ __forceinline__ Args codes_view(const CodesArgs &s, int c) {
    const int off = ldpc::tab_ptr(s.code_off)[c];
    const ldpc::TabPtr rec = ldpc::tab_ptr(s.tab + off);
    Args a{};
    a.qhard = s.qhard; a.iters = s.iters; a.post = s.post;
    a.E = rec[0]; a.cw2 = rec[1];
    a.row_start = s.tab + off + kRecHeader;
    a.col_start = a.row_start + s.rh + 1;
    a.e_col = a.col_start + s.nh + 1;
    a.e_circ = a.e_col + a.E;
    a.e_rl = a.e_circ + a.E;
    a.ce_edge = a.e_rl + a.E;
    a.ws = s.ws; a.ws_stride = s.ws_stride; a.B = s.B; a.maxiter = s.maxiter;
    a.rh = s.rh; a.nh = s.nh; a.M = s.M; a.N = s.N; a.R = s.R; a.q = s.q; a.lpc = s.lpc;
    a.mul = s.mul; a.div = s.div;
    return a;
}

// The set scheduler: workgroup g decodes items g, g + grid, ... in its slot, each on the view of the item's code.
template <int QL, int LPC>
__global__ __launch_bounds__(256) void gfq_codes_kernel(const CodesArgs s) {
    char *slot = s.ws + (size_t)blockIdx.x * s.ws_stride;
    for (unsigned w = blockIdx.x; w < s.items; w += gridDim.x) {
        const unsigned sl = w / s.B, f = w - sl * s.B;
        const int c = s.code_list ? ldpc::tab_ptr(s.code_list)[sl] : (int)sl;
        const Args a = codes_view(s, c);
        const Slot st = carve_slot(a, slot);   // by the E of this code
        decode_frame<QL, LPC>(a, s.soft + (long long)c * s.soft_code_stride + (size_t)f * s.q * s.N, st, w);
    }
}

// The channel of a set whose codes each carry a word of their own (exact replay of upstream's harness, which encodes a message per
// candidate): the noise is the same for every code, the transmitted symbol is not, so the soft values are per code.  Work item
// (frame, position) with lane = position as in gfq_channel_kernel, so that for a fixed symbol s a wave stores 64 consecutive doubles;
// the q_bits Gaussians of the position are read once into registers, and for every slot of the launch the symbol of the slot's code goes
// through gfq_symbol_probabilities, the arithmetic of the single-code channel.  The soft values of code c are written at
// soft[c][f][q][N] -- by code, not by slot: that is where gfq_codes_kernel reads the per-code input of a launch over B frames.
// A launch over the slots of a stop loop writes the regions of the codes still running and leaves the others as an earlier launch left
// them (with another B: at other offsets, so they hold no frame's values); nothing reads them, the decode launch covers the same slots.
struct CodesChanArgs {
    const int16_t *words;          // [C][N]
    const double *noise;           // [B][N * q_bits]
    double *soft;                  // [C][B][q][N]
    const int32_t *code_list;      // [n_slots] or null (slot s holds code s)
    long long B;
    int n_slots, N;
    double sigma;
};

template <int QB>
__global__ __launch_bounds__(256) void gfq_channel_codes_kernel(const CodesChanArgs a) {
    constexpr int q = 1 << QB;
    const int N = a.N;
    const long long total = a.B * (long long)N;
    const double s2 = a.sigma * a.sigma;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long b = t / N;
        const int i = (int)(t - b * N);
        double g[QB];
#pragma unroll
        for (int k = 0; k < QB; ++k) g[k] = a.noise[t * QB + k];   // bit i * q_bits + k of frame b
        for (int sl = 0; sl < a.n_slots; ++sl) {
            const int c = a.code_list ? ldpc::tab_ptr(a.code_list)[sl] : sl;
            gfq_symbol_probabilities<QB>(a.words[(size_t)c * N + i], g, a.sigma, s2, a.soft + ((size_t)c * a.B + b) * q * N + i, N);
        }
    }
}

// Symbol errors per code against the code's word (words [C][N]) or, words = null, against the all-zero word, with the shared count of
// ldpc_frontend.hpp.  One wavefront per (slot, frame), blocks_per_code workgroups per slot; a workgroup works on one slot only, so its
// totals go to the row of the slot's code.
struct CodesCountArgs {
    const int16_t *qhard;          // [n_active][B][N]
    const int32_t *iters;          // [n_active][B]
    int32_t *frame_info;           // [n_active][B] or null
    unsigned long long *counters;  // [C][5]: nse, nde, nue, frames, sum |iters|; the row of a slot is its code's
    const int32_t *code_list;      // [n_active] or null (slot s holds code s)
    long long B;
    int blocks_per_code;
    int N, R;
    const int16_t *words;          // [C][N] the word code c sent, or null = the all-zero word
};

__global__ __launch_bounds__(256) void gfq_count_codes_kernel(const CodesCountArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int cs = blockIdx.x / a.blocks_per_code, blk = blockIdx.x - cs * a.blocks_per_code;
    const int c = a.code_list ? ldpc::tab_ptr(a.code_list)[cs] : cs;
    ldpc::ErrorTally tally;
    for (long long fr = (long long)blk * 4 + wv; fr < a.B; fr += (long long)a.blocks_per_code * 4) {
        const long long g = (long long)cs * a.B + fr;
        uint32_t all = 0, info = 0;
        ldpc::symbol_errors(a.qhard + g * a.N, a.words ? a.words + (size_t)c * a.N : nullptr, a.N, a.R, lane, all, info);
        ldpc::wave_sum_pair(all, info);
        if (lane == 0) tally.add(all, info, a.iters[g], a.frame_info ? a.frame_info + g : nullptr);
    }
    tally.flush(a.counters + (size_t)c * 5);
}

#endif  // __HIPCC__

}  // namespace ldpc_gfq
