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
// This header holds no arithmetic.  The frame of each decoder -- initialisation, iterations, outputs, closing barrier -- is
// ms_ / lms_ / tasp_ / lche_ / sp_ / ims_ / asp_ / iasp_global_frame of ldpc_global.hpp, a template on the view of one frame
// (GlobCode), and the same text runs in the single code's *_global_kernel; only where the tables, the received word and the outputs
// are found differs, and that is what codeset_glob_view fills in.  For integer min-sum the quantiser has run once per received word
// before the launch (codeset_ims_quantise: the int16 words are the values ims_global_kernel forms itself), so the kernel hands
// the frame a read of that word where ims_global_kernel hands it its quantiser.  lche_global_frame carries its own syndrome and edge
// decode because the single-code kernel measured slower with the shared ones (profiles/global_tier_refactor_time.txt); what merging
// the two texts did to the seventeen kernels: profiles/global_frame_refactor_resources.txt, global_frame_refactor_time.txt.
// Gallager BP has no set: its frames are not independent.
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

// The edge words of a record: int32 in the constant address space, read as the uint32_t a frame body expects
struct TabWords {
    TabPtr p;
    __device__ __forceinline__ uint32_t operator[](int i) const { return (uint32_t)p[i]; }
};

// One work item as the frame bodies of ldpc_global.hpp see it: the slice laid out for THIS code's ne, the item's received word and
// outputs, the tables and cw2 of the code's record
__device__ __forceinline__ GlobCode<TabPtr, TabWords> codeset_glob_view(const CodesetGlobArgs &g, long long item, int edge_arrays) {
    const CodesetArgs &s = g.s;
    const int slot = (int)(item / s.B);
    const long long fr = item - (long long)slot * s.B;
    const unsigned list_item = s.code_list ? (unsigned)tab_ptr(s.code_list)[slot] : (unsigned)slot;   // p * C + c on an SNR grid
    const unsigned p = __builtin_amdgcn_readfirstlane(list_item / (unsigned)s.C);   // wave-uniform, like the list itself
    const int c = (int)(list_item - p * (unsigned)s.C);
    const TabPtr rec = tab_ptr(s.tab + tab_ptr(s.code_off)[c]);
    const int ne = rec[s.rh];
    GlobCode<TabPtr, TabWords> a;
    a.w = GlobFrame{glob_view(g.ws + (size_t)blockIdx.x * g.ws_stride, s.N, s.rh * s.M, ne, s.M, edge_arrays), s.M, s.N, s.rh * s.M, ne};
    a.llr = s.llr + (long long)c * s.llr_code_stride + (long long)p * s.llr_point_stride + fr * s.N;
    a.hard = s.hard; a.iters = s.iters; a.soft_out = s.soft_out;   // [slot][frame]: row `item`
    a.out = item;
    a.row_start = rec;
    a.edges = {rec + s.rh + 1};
    a.cw2 = rec[s.rh + 1 + ne];
    a.col_start = rec + s.rh + 2 + ne;
    a.col_edges = {a.col_start + s.nh + 1};
    a.col_slot = {a.col_edges.p + ne};
    a.rh = s.rh; a.maxiter = s.maxiter; a.hard_words = s.hard_words;
    a.alpha = s.alpha;
    return a;
}

// The kernels: a workgroup walks its items; the third argument is the number of per-edge arrays of the decoder's slice (glob_ws_bytes)
#define LDPC_CODES_GLOBAL_KERNEL(name, frame, edge_arrays)                                                      \
    __global__ void __launch_bounds__(kGlobThreads) name(const CodesetGlobArgs g) {                            \
        for (long long it = blockIdx.x; it < g.items; it += gridDim.x) frame(codeset_glob_view(g, it, edge_arrays)); \
    }
LDPC_CODES_GLOBAL_KERNEL(sp_global_codes_kernel, sp_global_frame, 1)
LDPC_CODES_GLOBAL_KERNEL(asp_global_codes_kernel, asp_global_frame, 3)
LDPC_CODES_GLOBAL_KERNEL(ms_global_codes_kernel, ms_global_frame, 0)
LDPC_CODES_GLOBAL_KERNEL(iasp_global_codes_kernel, iasp_global_frame, 1)
LDPC_CODES_GLOBAL_KERNEL(tasp_global_codes_kernel, tasp_global_frame, 4)
LDPC_CODES_GLOBAL_KERNEL(lms_global_codes_kernel, lms_global_frame, 1)
LDPC_CODES_GLOBAL_KERNEL(lche_global_codes_kernel, lche_global_frame, 1)
#undef LDPC_CODES_GLOBAL_KERNEL

// integer min-sum behind the set's quantiser: the channel word is the int16 that codeset_ims_quantise left for the item's received
// word (once per word), at the offset the word has in CodesetArgs::llr
__global__ void __launch_bounds__(kGlobThreads) ims_global_codes_kernel(const CodesetGlobArgs g, const ImsCodesArgs q) {
    for (long long it = blockIdx.x; it < g.items; it += gridDim.x) {
        const auto a = codeset_glob_view(g, it, 0);
        const int16_t *const qw = q.q + (a.llr - g.s.llr);
        ims_global_frame(a, q.max_data, q.ialpha, [=](int v) { return (int)qw[v]; });
    }
}

}  // namespace ldpc

