// Host side of the code-set kernels (ldpc_codeset.hpp): the concatenated graph table, the ldpc_hip_*codes* entry points and the
// shared-noise Monte-Carlo pass.  What a binary and a GF(q) code set (ldpc_gfq_codeset_api.hpp) keep and do alike -- the tables, the
// per-code outputs of a piece, the fixed-length and the stopping-rule loop -- is codeset_common and the functions around it.
// Included at the end of ldpc_hip.hip.
#pragma once

// ldpc_hip_simulate_codes_stop and its GF(q) twin: the per-code state of the stopping rule and the list of the codes still running
struct codeset_rule_ws {
    unsigned long long *rule = nullptr;              // [C][4]: experiment, nse, nde, frames_decoded; the exact-replay run: [C][6] (room for 6)
    int32_t *running = nullptr, *list = nullptr;     // [C] each
    int32_t *nactive = nullptr;                      // [1]
    double *reference = nullptr;                     // an SNR grid (ldpc_codeset_grid_api.hpp): [64], one reference frame error per point
    size_t rows = 0;                                 // the rows rule, running and list hold: C, or P * C once a grid has run
};

// what every code-set state holds
struct codeset_common {
    int C = 0;
    int ne_max = 0;                    // the largest edge count of a code of the set
    std::vector<int32_t> off, tab;     // host copies of the device tables
    int32_t *d_off = nullptr, *d_tab = nullptr;
    // workspace of the simulate entry points for w_frames frames per code, next to the decoder's own input and decisions
    int32_t *w_iters = nullptr, *w_info = nullptr;   // [C][w_frames]
    unsigned long long *w_cnt = nullptr;             // [C][5]
    long long w_frames = 0;                          // input rows the workspace holds: frames per code, times the points of an SNR grid
    int w_points = 1;                                // the points w_cnt holds rows for: [w_points * C][5]
    codeset_rule_ws stop;                            // the *_stop entry points
};

struct ldpc_codeset_state : codeset_common {
    double *w_llr = nullptr;           // [w_frames][N], shared by the codes
    uint32_t *w_hard = nullptr;        // [C][w_frames][hard_words]
    // an IMS set: the quantiser's results for the received words of one decode launch (grown on demand, never shrunk)
    double *w_coef = nullptr;          // [w_q_frames]
    int16_t *w_q = nullptr;            // [w_q_frames][N]
    long long w_q_frames = 0;
    int route = 0;                     // the record of codeset_kinds[] the set was opened with: (decoder_id, route)
    // ROUTE_GLOBAL: one slice of glob_stride bytes per workgroup of a decode launch (grown on demand, never shrunk)
    char *w_glob = nullptr;
    size_t glob_stride = 0;
    int glob_grid = 0;
};

void codeset_common_release(codeset_common &s) {
    void *dev[] = {s.d_off, s.d_tab, s.w_iters, s.w_info, s.w_cnt, s.stop.rule, s.stop.running, s.stop.list, s.stop.nactive, s.stop.reference};
    for (void *p : dev)
        if (p) (void)hipFree(p);
}

void ldpc_codeset_release(ldpc_codeset_state *s) {
    if (!s) return;
    if (s->w_llr) (void)hipFree(s->w_llr);
    if (s->w_hard) (void)hipFree(s->w_hard);
    if (s->w_coef) (void)hipFree(s->w_coef);
    if (s->w_q) (void)hipFree(s->w_q);
    if (s->w_glob) (void)hipFree(s->w_glob);
    codeset_common_release(*s);
    delete s;
}

namespace {

// Dynamic LDS of the code-set kernels for F frames per workgroup: the image that the kernel's header describes (ldpc_codeset.hpp,
// ldpc_codeset_sp.hpp, ldpc_codeset_wide.hpp) + 16 for the vote flags.  MS / LMS: the a-posteriori values alone, on the wide route the
// per-check records next to them; TDMP: the per-edge state Z[ne_max][M] next to them.
size_t codeset_lds_apost(int F, int, int nh, int M, int) { return sizeof(double) * ((size_t)nh * M) * (size_t)F + 16; }
size_t codeset_lds_tdmp(int F, int, int nh, int M, int ne_max) { return sizeof(double) * ((size_t)nh * M + (size_t)ne_max * M) * (size_t)F + 16; }
size_t codeset_lds_iasp(int F, int, int nh, int M, int ne_max) { return ldpc::iasp_codes_words_bytes(F, M, nh * M, ne_max) + 16; }
size_t codeset_lds_lche(int F, int, int nh, int M, int ne_max) { return ldpc::lche_codes_image_bytes(F, M, nh * M, ne_max) + 16; }
size_t codeset_lds_ims(int F, int rh, int nh, int M, int) { return ldpc::ims_codes_image_bytes(F, nh * M, rh * M) + 16; }
size_t codeset_lds_sp(int F, int rh, int nh, int M, int ne_max) { return ldpc::sp_codes_image_bytes(false, F, nh * M, rh * M, M, ne_max) + 16; }
size_t codeset_lds_asp(int F, int rh, int nh, int M, int ne_max) { return ldpc::sp_codes_image_bytes(true, F, nh * M, rh * M, M, ne_max) + 16; }
size_t codeset_lds_wide(int F, int rh, int nh, int M, int) { return ldpc::wide_codes_image_bytes(F, nh * M, rh * M) + 16; }
size_t codeset_lds_none(int, int, int, int, int) { return 0; }   // ROUTE_GLOBAL: the state is in the workspace

enum codeset_lds_text { LDS_NONE, LDS_LENGTH, LDS_IMS, LDS_IASP, LDS_TDMP, LDS_LCHE, LDS_FLOOD, LDS_WIDE };   // the refusals of codeset_lds_refusal

enum : int { ROUTE_RESIDENT = 0, ROUTE_WIDE = 1, ROUTE_GLOBAL = 2 };   // ldpc_hip_open_codes and its kin; ldpc_hip_open_codes_wide; ldpc_hip_open_codes_global

enum : unsigned {
    CS_COLS = 1,     // the record goes on with cw2, col_start and col_edges, and a column entry names its edge in 16 bits
    CS_FLOOD = 2,    // a frame's state is in LDS and dealt over the waves of a workgroup (ldpc_codeset_sp.hpp): frames and threads are
                     // sp_codes_frames and sp_codes_groups x sp_codes_lanes, and a set is refused only when ONE frame's image does not fit
    CS_CHECKS = 4,   // that image holds the R check products
    CS_QUANT = 8,    // the kernel reads the quantiser's int16 words through a second argument (ImsCodesArgs)
    CS_SLOTS = 16,   // the record goes on with cw2, col_start, col_edges ((block ROW << 16) | shift) and col_slot (the row-major index of the
                     // edge, a word of its own): the five tables of DecArgs, as the kernels of ldpc_codeset_global.hpp read them
    CS_GLOBAL = 32,  // the state is in a workspace in global memory (ldpc_codeset_global.hpp): one frame per workgroup of glob_threads(N)
                     // threads, the grid capped and striding over the n_slots * B items, the argument block a CodesetGlobArgs
};

// What a set decoder is on the host: the one place where the limits of the set kernels live
struct codeset_kind {
    int id;
    const char *kernel;                // kernel_name, "<multiwave>" appended when M > 64
    const void *wave, *multiwave;      // its instance for M <= 64 and the one for M > 64
    int rh_max, nh_max, rw_max;        // block rows and block columns (the kernel holds them, or their channel LLRs, in registers) and row weight; 0: any
    const char *min_rw2;               // row weight at least 2 (map_bin and imap_bin read SB[1], decoders.cpp:2191-2271), under this name; null: 1 is legal
    unsigned is;                       // CS_*
    size_t (*lds)(int F, int rh, int nh, int M, int ne_max);
    codeset_lds_text early, late;      // the image is checked before the table is built (with ne_max = 0) and once ne_max is known
    int route = ROUTE_RESIDENT;        // ROUTE_WIDE: the same decoder with its per-check records in LDS, or launched without a block-row limit
    int M_max = 512;                   // the lifting its lanes and LDS image take; 0: any
    int glob_edge_arrays = 0;          // CS_GLOBAL: the per-edge arrays of a workspace slice (glob_ws_bytes), those of its decoder_kind
};

const codeset_kind codeset_kinds[] = {
    {LDPC_HIP_SP_DEC, "sp_flood_codes_kernel", (const void *)ldpc::sp_flood_codes_kernel<false>, (const void *)ldpc::sp_flood_codes_kernel<true>,
     0, 0, 0, nullptr, CS_COLS | CS_FLOOD | CS_CHECKS, codeset_lds_sp, LDS_NONE, LDS_FLOOD},
    {LDPC_HIP_ASP_DEC, "asp_flood_codes_kernel", (const void *)ldpc::asp_flood_codes_kernel<kRWM, false>, (const void *)ldpc::asp_flood_codes_kernel<kRWM, true>,
     0, 0, kRWM, "advanced sum-product", CS_COLS | CS_FLOOD, codeset_lds_asp, LDS_NONE, LDS_FLOOD},
    {LDPC_HIP_MS_DEC, "ms_flood_codes_kernel", (const void *)ldpc::ms_flood_codes_kernel<kRHM, kNHM, false>, (const void *)ldpc::ms_flood_codes_kernel<kRHM, kNHM, true>,
     kRHM, kNHM, kRWM, nullptr, 0, codeset_lds_apost, LDS_LENGTH, LDS_NONE},
    {LDPC_HIP_IMS_DEC, "ims_flood_codes_kernel", (const void *)ldpc::ims_flood_codes_kernel<false>, (const void *)ldpc::ims_flood_codes_kernel<true>,
     0, 0, kRWM, nullptr, CS_QUANT, codeset_lds_ims, LDS_IMS, LDS_NONE},
    {LDPC_HIP_IASP_DEC, "iasp_codes_kernel", (const void *)ldpc::iasp_codes_kernel<kRWM, false>, (const void *)ldpc::iasp_codes_kernel<kRWM, true>,
     0, 0, kRWM, "integer advanced sum-product", CS_COLS, codeset_lds_iasp, LDS_NONE, LDS_IASP},
    {LDPC_HIP_TASP_DEC, "tasp_layered_codes_kernel", (const void *)ldpc::tasp_layered_codes_kernel<kRWM, false>, (const void *)ldpc::tasp_layered_codes_kernel<kRWM, true>,
     kRHM, 0, kRWM, "TDMP sum-product", 0, codeset_lds_tdmp, LDS_LENGTH, LDS_TDMP},
    {LDPC_HIP_LMS_DEC, "lms_layered_codes_kernel", (const void *)ldpc::lms_layered_codes_kernel<kRHM, false>, (const void *)ldpc::lms_layered_codes_kernel<kRHM, true>,
     kRHM, 0, kRWM, nullptr, 0, codeset_lds_apost, LDS_LENGTH, LDS_NONE},
    {LDPC_HIP_LCHE_DEC, "lche_layered_codes_kernel", (const void *)ldpc::lche_layered_codes_kernel<kRWM, false>, (const void *)ldpc::lche_layered_codes_kernel<kRWM, true>,
     0, 0, kRWM, nullptr, 0, codeset_lds_lche, LDS_NONE, LDS_LCHE},
    // ldpc_hip_open_codes_wide: any number of block rows and columns.  TDMP's kernel walks the block rows in a run-time loop and keeps
    // nothing of a row: the same instances, without the limit
    {LDPC_HIP_MS_DEC, "ms_flood_wide_codes_kernel", (const void *)ldpc::ms_flood_wide_codes_kernel<false>, (const void *)ldpc::ms_flood_wide_codes_kernel<true>,
     0, 0, kRWM, nullptr, 0, codeset_lds_wide, LDS_WIDE, LDS_NONE, ROUTE_WIDE},
    {LDPC_HIP_TASP_DEC, "tasp_layered_codes_kernel", (const void *)ldpc::tasp_layered_codes_kernel<kRWM, false>, (const void *)ldpc::tasp_layered_codes_kernel<kRWM, true>,
     0, 0, kRWM, "TDMP sum-product", 0, codeset_lds_tdmp, LDS_NONE, LDS_TDMP, ROUTE_WIDE},
    {LDPC_HIP_LMS_DEC, "lms_layered_wide_codes_kernel", (const void *)ldpc::lms_layered_wide_codes_kernel<false>, (const void *)ldpc::lms_layered_wide_codes_kernel<true>,
     0, 0, kRWM, nullptr, 0, codeset_lds_wide, LDS_WIDE, LDS_NONE, ROUTE_WIDE},
    // ldpc_hip_open_codes_global: any shape the single-code shape-unlimited tier takes.  No LDS, no limit on M, rh, nh or the row weight
    // (LCHE: 1024, upstream's map_bin_llr); one instance per decoder
#define LDPC_GLOBAL_SET(id, kernel, rw_max, min_rw2, is, edge_arrays)                                                                       \
    {id, #kernel, (const void *)ldpc::kernel, (const void *)ldpc::kernel, 0, 0, rw_max, min_rw2, CS_SLOTS | CS_GLOBAL | (is), codeset_lds_none, \
     LDS_NONE, LDS_NONE, ROUTE_GLOBAL, 0, edge_arrays}
    LDPC_GLOBAL_SET(LDPC_HIP_SP_DEC, sp_global_codes_kernel, 0, nullptr, 0, 1),
    LDPC_GLOBAL_SET(LDPC_HIP_ASP_DEC, asp_global_codes_kernel, 0, "advanced sum-product", 0, 3),
    LDPC_GLOBAL_SET(LDPC_HIP_MS_DEC, ms_global_codes_kernel, 0, nullptr, 0, 0),
    LDPC_GLOBAL_SET(LDPC_HIP_IMS_DEC, ims_global_codes_kernel, 0, nullptr, CS_QUANT, 0),
    LDPC_GLOBAL_SET(LDPC_HIP_IASP_DEC, iasp_global_codes_kernel, 0, "integer advanced sum-product", 0, 1),
    LDPC_GLOBAL_SET(LDPC_HIP_TASP_DEC, tasp_global_codes_kernel, 0, "TDMP sum-product", 0, 4),
    LDPC_GLOBAL_SET(LDPC_HIP_LMS_DEC, lms_global_codes_kernel, 0, nullptr, 0, 1),
    LDPC_GLOBAL_SET(LDPC_HIP_LCHE_DEC, lche_global_codes_kernel, 1024, nullptr, 0, 1),
#undef LDPC_GLOBAL_SET
};

// ROUTE_GLOBAL: a launch takes at most this many workgroups, halved while their slices exceed kGlobSetBytes but not below
// kGlobSetMinGrid -- the rule of launch_global.  A set whose kGlobSetMinGrid slices exceed kGlobSetBytes is refused when it is opened.
constexpr int kGlobSetGrid = 1024, kGlobSetMinGrid = 16;
constexpr size_t kGlobSetBytes = (size_t)8 << 30;

// The entry points come here with an id that their route serves
const codeset_kind *codeset_find(int decoder_id, int route = ROUTE_RESIDENT) {
    for (const codeset_kind &k : codeset_kinds)
        if (k.id == decoder_id && k.route == route) return &k;
    return nullptr;
}

// the record a set context was opened with
const codeset_kind &codeset_kind_of(const ldpc_hip_ctx *c) { return *codeset_find(c->decoder_id, c->codes->route); }

// An image beyond 160 KiB, in the words of its kernel
int codeset_lds_refusal(const codeset_kind &k, codeset_lds_text text, const char *who, int F, int rh, int nh, int M, int ne_max) {
    const int N = nh * M;
    const size_t bytes = k.lds(F, rh, nh, M, ne_max);
    switch (text) {
    case LDS_LENGTH: return fail(LDPC_HIP_EUNSUPPORTED, "%s: code length %d x %d frames per wave does not fit the 160 KiB LDS image", who, N, F);
    case LDS_IMS: return fail(LDPC_HIP_EUNSUPPORTED, "%s: %d frame(s) per wave x (4 x %d variables + 8 x %d checks) bytes, rounded up to 16, + 16 need an LDS image of %zu bytes; the limit is 160 KiB", who, F, N, rh * M, bytes);
    case LDS_IASP: return fail(LDPC_HIP_EUNSUPPORTED, "%s: %d frame(s) per wave x (%d circulants x %d checks + 2 x %d variables) halfwords need an LDS image of %zu bytes; the limit is 160 KiB", who, F, ne_max, M, N, bytes);
    case LDS_TDMP: return fail(LDPC_HIP_EUNSUPPORTED, "%s: %d frame(s) per wave x (%d a-posteriori values + %d circulants x %d checks) need an LDS image of %zu bytes; the limit is 160 KiB", who, F, N, ne_max, M, bytes);
    case LDS_WIDE: return fail(LDPC_HIP_EUNSUPPORTED, "%s: %d frame(s) per wave x (8 x %d variables + 24 x %d checks) bytes, rounded up to 16, + 16 need an LDS image of %zu bytes; the limit is 160 KiB", who, F, N, rh * M, bytes);
    case LDS_LCHE: return fail(LDPC_HIP_EUNSUPPORTED, "%s: %d frame(s) per wave x (%d a-posteriori LLRs + %d circulants x %d checks) and the tables of logexp need an LDS image of %zu bytes; the limit is 160 KiB", who, F, N, ne_max, M, bytes);
    default: return fail(LDPC_HIP_EUNSUPPORTED, "%s: one frame's image, 8 x (%d circulants x %d + %d variables%s) + 4 x %d bytes, rounded up to 16, + 16 is %zu bytes; the limit is 160 KiB", who, ne_max, M, N, k.is & CS_CHECKS ? " + the checks" : "", (N + 31) / 32, bytes);
    }
}

// Checks a code set against the limits of its kernel and builds its table: per code row_start[rh+1] (relative to the code's own edge
// list) then edges[] ((block column << 16) | shift, rows ascending, columns ascending); off[c] = index of code c's row_start[0].  A
// CS_COLS record goes on with cw2 (1: every block column holds exactly two circulants, upstream's own branch), col_start[nh+1] and
// col_edges[] ((row-major index of the edge inside its code << 16) | shift, columns ascending, rows ascending).  A CS_SLOTS record goes
// on instead with cw2, col_start[nh+1], col_edges[ne] ((block row << 16) | shift, columns ascending, rows ascending) and col_slot[ne]
// (the row-major index of that edge inside its code): rh + nh + 3 + 3 ne entries per code.
int codeset_build(const char *who, const codeset_kind &kind, int rh, int nh, int M, const int16_t *hd, int C, std::vector<int32_t> &off,
                  std::vector<int32_t> &tab, int *ne_max_out = nullptr) {
    if (!hd || rh <= 0 || nh <= 0 || M <= 0) return fail(LDPC_HIP_EINVAL, "%s: bad argument", who);
    if (C < 1) return fail(LDPC_HIP_EINVAL, "%s: C = %d, a code set holds at least one code", who, C);
    if (kind.M_max && M > kind.M_max) return fail(LDPC_HIP_EINVAL, "%s: M = %d, the resident table kernels take M <= %d", who, M, kind.M_max);
    if (kind.is & CS_GLOBAL) {   // what an edge word and the 32-bit indices of the tier hold, as ldpc_hip_open has it
        if (M >= 65536 || nh >= 65536 || rh >= 65536)
            return fail(LDPC_HIP_EUNSUPPORTED, "%s: M = %d, rh = %d, nh = %d; an edge word holds a shift and a block row or column in 16 bits each: all below 65536", who, M, rh, nh);
        if ((long long)nh * M >= (1LL << 28))
            return fail(LDPC_HIP_EUNSUPPORTED, "%s: code length nh * M = %lld: at most 2^28 - 1 is supported (32-bit indices)", who, (long long)nh * M);
    }
    if (kind.rh_max && rh > kind.rh_max) return fail(LDPC_HIP_EINVAL, "%s: rh = %d, the resident table kernels take %d block rows", who, rh, kind.rh_max);
    if (kind.nh_max && nh > kind.nh_max)
        return fail(LDPC_HIP_EINVAL, "%s: nh = %d, the flooding table kernel keeps the channel LLRs of %d block columns in registers", who, nh, kind.nh_max);
    const int F = kind.is & CS_FLOOD ? 1 : M > 64 ? 1 : 64 / M;   // the frames whose images have to fit
    if (kind.early && kind.lds(F, rh, nh, M, 0) > 160 * 1024) return codeset_lds_refusal(kind, kind.early, who, F, rh, nh, M, 0);
    off.clear(); tab.clear();
    std::vector<int> col_w((size_t)nh);
    int ne_max = 0;
    for (int c = 0; c < C; ++c) {
        const int16_t *h = hd + (size_t)c * rh * nh;
        if (tab.size() + (size_t)rh + 1 + (size_t)rh * nh + (kind.is & (CS_COLS | CS_SLOTS) ? (size_t)nh + 2 + (size_t)rh * nh : 0) +
                (kind.is & CS_SLOTS ? (size_t)rh * nh : 0) >= ((size_t)1 << 31))
            return fail(LDPC_HIP_EINVAL, "%s: the table of %d codes exceeds 2^31 entries", who, C);
        off.push_back((int32_t)tab.size());
        const size_t rs = tab.size();
        tab.resize(rs + (size_t)rh + 1);
        std::fill(col_w.begin(), col_w.end(), 0);
        int ne = 0;
        for (int j = 0; j < rh; ++j) {
            tab[rs + j] = ne;
            int rw = 0;
            for (int k = 0; k < nh; ++k) {
                const int v = h[(size_t)j * nh + k];
                if (v < -1 || v >= M) return fail(LDPC_HIP_EINVAL, "%s: code %d, shift %d at (%d, %d) is outside [-1, %d)", who, c, v, j, k, M);
                if (v == -1) continue;
                tab.push_back((int32_t)(((uint32_t)k << 16) | (uint32_t)v));
                ++col_w[(size_t)k];
                ++rw; ++ne;
            }
            if (rw == 0) return fail(LDPC_HIP_EINVAL, "%s: code %d, block row %d is empty", who, c, j);
            if (kind.rw_max && rw > kind.rw_max)   // a resident kernel's registers; CS_GLOBAL: upstream's own arrays (map_bin_llr, decoders.cpp:2818-2822)
                return fail(kind.is & CS_GLOBAL ? LDPC_HIP_EUNSUPPORTED : LDPC_HIP_EINVAL, "%s: code %d, block row %d has weight %d; at most %d", who, c, j, rw, kind.rw_max);
            if (kind.min_rw2 && rw < 2)
                return fail(LDPC_HIP_EINVAL, "%s: code %d, block row %d has weight %d; %s needs at least 2", who, c, j, rw, kind.min_rw2);
        }
        tab[rs + rh] = ne;
        ne_max = ne > ne_max ? ne : ne_max;
        for (int k = 0; k < nh; ++k)
            if (!col_w[(size_t)k]) return fail(LDPC_HIP_EINVAL, "%s: code %d, block column %d is empty", who, c, k);
        if (kind.is & CS_SLOTS) {
            bool cw2 = true;   // the rule of ldpc_hip_open, per code
            for (int k = 0; k < nh; ++k) cw2 = cw2 && col_w[(size_t)k] == 2;
            tab.push_back(cw2 ? 1 : 0);
            const size_t cst = tab.size(), ed = rs + (size_t)rh + 1, ce = cst + (size_t)nh + 1, sl = ce + (size_t)ne;
            tab.resize(sl + (size_t)ne);
            int q = 0;
            for (int k = 0; k < nh; ++k) { tab[cst + k] = q; q += col_w[(size_t)k]; }
            tab[cst + nh] = q;
            std::vector<int> fill(tab.begin() + (long)cst, tab.begin() + (long)cst + nh);
            for (int j = 0; j < rh; ++j)   // row-major order: the rows of a column come out ascending
                for (int e = tab[rs + j]; e < tab[rs + j + 1]; ++e) {
                    const uint32_t d = (uint32_t)tab[ed + (size_t)e];
                    const int at = fill[d >> 16]++;
                    tab[ce + (size_t)at] = (int32_t)(((uint32_t)j << 16) | (d & 0xffffu));
                    tab[sl + (size_t)at] = e;
                }
        }
        if (kind.is & CS_COLS) {
            if (ne > 65535) return fail(LDPC_HIP_EINVAL, "%s: code %d has %d circulants; a column entry names its edge in 16 bits", who, c, ne);
            bool cw2 = true;   // the rule of ldpc_hip_open, per code
            for (int k = 0; k < nh; ++k) cw2 = cw2 && col_w[(size_t)k] == 2;
            tab.push_back(cw2 ? 1 : 0);
            const size_t cst = tab.size(), ed = rs + (size_t)rh + 1;
            tab.resize(cst + (size_t)nh + 1 + (size_t)ne);
            int q = 0;
            for (int k = 0; k < nh; ++k) { tab[cst + k] = q; q += col_w[(size_t)k]; }
            tab[cst + nh] = q;
            std::vector<int> fill(tab.begin() + (long)cst, tab.begin() + (long)cst + nh);
            for (int e = 0; e < ne; ++e) {   // row-major order: the rows of a column come out ascending
                const uint32_t d = (uint32_t)tab[ed + (size_t)e];
                tab[cst + (size_t)nh + 1 + (size_t)fill[d >> 16]++] = (int32_t)(((uint32_t)e << 16) | (d & 0xffffu));
            }
        }
    }
    if (kind.late && kind.lds(F, rh, nh, M, ne_max) > 160 * 1024) return codeset_lds_refusal(kind, kind.late, who, F, rh, nh, M, ne_max);
    if (kind.is & CS_GLOBAL) {
        const size_t slice = ldpc::glob_ws_bytes(nh * M, rh * M, ne_max, M, kind.glob_edge_arrays);
        if (slice > kGlobSetBytes / kGlobSetMinGrid)
            return fail(LDPC_HIP_EUNSUPPORTED, "%s: a workgroup's workspace slice for %d variables, %d checks and %d circulants x %d is %zu bytes; the limit is %zu (%d slices within 8 GiB)",
                        who, nh * M, rh * M, ne_max, M, slice, kGlobSetBytes / kGlobSetMinGrid, kGlobSetMinGrid);
    }
    if (ne_max_out) *ne_max_out = ne_max;
    return 0;
}

int codeset_ctx(const ldpc_hip_ctx *c, const char *who) {
    if (!c || !c->codes) return fail(LDPC_HIP_EINVAL, "%s: not a code-set context (ldpc_hip_open_codes)", who);
    return 0;
}

// Workgroups per code of the count kernels: four frames (waves) each, fewer when there are many codes
int codeset_count_blocks(long long B, int C) {
    const long long bpc = (B + 3) / 4, cap = 2048 / C > 1 ? 2048 / C : 1;
    return (int)(bpc > cap ? cap : bpc);
}

// code_list / n_slots: the codes of the [n_slots][B] inputs (null: all C codes in order), see ldpc_codeset.hpp.  points: an SNR grid,
// the list names items and a null list stands for all points * C of them
int codeset_count_launch(const ldpc_hip_ctx *c, const uint32_t *d_hard, const int32_t *d_iters, long long B, int32_t *d_frame_info,
                         unsigned long long *d_counters, hipStream_t stream, const int32_t *code_list = nullptr, int n_slots = 0, int points = 1) {
    const int C = code_list ? n_slots : c->codes->C * points;
    const int bpc = codeset_count_blocks(B, C);
    ldpc::CodesetCountArgs a{d_hard, d_iters, d_frame_info, d_counters, code_list, B, bpc, c->hard_words, c->R};
    hipLaunchKernelGGL(ldpc::count_errors_codes_kernel, dim3((unsigned)((long long)bpc * C)), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The result of a *_table_host entry point: any of length, offsets [C] and table [capacity] may be null
int codeset_table_out(const char *who, const std::vector<int32_t> &off, const std::vector<int32_t> &tab, int32_t *offsets, int32_t *table,
                      long long capacity, long long *length) {
    if (length) *length = (long long)tab.size();
    if (offsets) std::memcpy(offsets, off.data(), sizeof(int32_t) * off.size());
    if (table) {
        if (capacity < (long long)tab.size())
            return fail(LDPC_HIP_EINVAL, "%s: the table has %lld entries, room for %lld", who, (long long)tab.size(), capacity);
        std::memcpy(table, tab.data(), sizeof(int32_t) * tab.size());
    }
    return 0;
}

// Takes the built tables into the state and onto the current device, with the counters of the simulate entry points
int codeset_upload(codeset_common &s, int C, int ne_max, std::vector<int32_t> &off, std::vector<int32_t> &tab) {
    s.off.swap(off); s.tab.swap(tab);
    s.C = C; s.ne_max = ne_max;
    HIP_TRY(hipMalloc(&s.d_off, sizeof(int32_t) * s.off.size()));
    HIP_TRY(hipMemcpy(s.d_off, s.off.data(), sizeof(int32_t) * s.off.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&s.d_tab, sizeof(int32_t) * s.tab.size()));
    HIP_TRY(hipMemcpy(s.d_tab, s.tab.data(), sizeof(int32_t) * s.tab.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&s.w_cnt, sizeof(unsigned long long) * 5 * (size_t)C));
    return 0;
}

int codeset_table_host(const char *who, int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int32_t *offsets, int32_t *table,
                       long long capacity, long long *length, int route = ROUTE_RESIDENT) {
    std::vector<int32_t> off, tab;
    if (int rc = codeset_build(who, *codeset_find(decoder_id, route), rh, nh, M, hd, C, off, tab)) return rc;
    return codeset_table_out(who, off, tab, offsets, table, capacity, length);
}

// what the two wide entry points say to any other id
int codeset_wide_id(const char *who, int decoder_id) {
    if (decoder_id == LDPC_HIP_MS_DEC || decoder_id == LDPC_HIP_TASP_DEC || decoder_id == LDPC_HIP_LMS_DEC) return 0;
    return fail(LDPC_HIP_EINVAL, "%s: decoder id %d; MS_DEC (3), TASP_DEC (7) or LMS_DEC (8)", who, decoder_id);
}

// what the two global entry points say to any other id
int codeset_global_id(const char *who, int decoder_id) {
    if (codeset_find(decoder_id, ROUTE_GLOBAL)) return 0;
    return fail(LDPC_HIP_EINVAL, "%s: decoder id %d; SP_DEC (1), ASP_DEC (2), MS_DEC (3), IMS_DEC (4), IASP_DEC (5), TASP_DEC (7), LMS_DEC (8) or LCHE_DEC (9)", who, decoder_id);
}

}  // namespace

extern "C" {

int ldpc_hip_codes_table_host(int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int32_t *offsets, int32_t *table,
                              long long capacity, long long *length) {
    if (decoder_id != LDPC_HIP_MS_DEC && decoder_id != LDPC_HIP_IASP_DEC && decoder_id != LDPC_HIP_TASP_DEC && decoder_id != LDPC_HIP_LMS_DEC)
        return fail(LDPC_HIP_EINVAL, "%s: decoder id %d; a code set decodes with MS_DEC (3), IASP_DEC (5), TASP_DEC (7) or LMS_DEC (8), with LCHE_DEC (9) through ldpc_hip_open_codes_lche / ldpc_hip_codes_table_lche_host and with IMS_DEC (4) through ldpc_hip_open_codes_ims / ldpc_hip_codes_table_ims_host, and with SP_DEC (1) or ASP_DEC (2) through ldpc_hip_open_codes_sp / ldpc_hip_codes_table_sp_host", "ldpc_hip_codes_table_host", decoder_id);
    return codeset_table_host("ldpc_hip_codes_table_host", decoder_id, rh, nh, M, hd, C, offsets, table, capacity, length);
}

int ldpc_hip_codes_table_lche_host(int rh, int nh, int M, const int16_t *hd, int C, int32_t *offsets, int32_t *table, long long capacity,
                                   long long *length) {
    return codeset_table_host("ldpc_hip_codes_table_lche_host", LDPC_HIP_LCHE_DEC, rh, nh, M, hd, C, offsets, table, capacity, length);
}

int ldpc_hip_codes_table_ims_host(int rh, int nh, int M, const int16_t *hd, int C, int32_t *offsets, int32_t *table, long long capacity,
                                  long long *length) {
    return codeset_table_host("ldpc_hip_codes_table_ims_host", LDPC_HIP_IMS_DEC, rh, nh, M, hd, C, offsets, table, capacity, length);
}

int ldpc_hip_codes_table_wide_host(int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int32_t *offsets, int32_t *table,
                                   long long capacity, long long *length) {
    if (int rc = codeset_wide_id("ldpc_hip_codes_table_wide_host", decoder_id)) return rc;
    return codeset_table_host("ldpc_hip_codes_table_wide_host", decoder_id, rh, nh, M, hd, C, offsets, table, capacity, length, ROUTE_WIDE);
}

int ldpc_hip_codes_table_global_host(int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int32_t *offsets, int32_t *table,
                                     long long capacity, long long *length) {
    if (int rc = codeset_global_id("ldpc_hip_codes_table_global_host", decoder_id)) return rc;
    return codeset_table_host("ldpc_hip_codes_table_global_host", decoder_id, rh, nh, M, hd, C, offsets, table, capacity, length, ROUTE_GLOBAL);
}

int ldpc_hip_codes_table_sp_host(int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int32_t *offsets, int32_t *table,
                                 long long capacity, long long *length) {
    if (decoder_id != LDPC_HIP_SP_DEC && decoder_id != LDPC_HIP_ASP_DEC)
        return fail(LDPC_HIP_EINVAL, "ldpc_hip_codes_table_sp_host: decoder id %d; SP_DEC (1) or ASP_DEC (2)", decoder_id);
    return codeset_table_host("ldpc_hip_codes_table_sp_host", decoder_id, rh, nh, M, hd, C, offsets, table, capacity, length);
}

}  // extern "C"

namespace {

int codeset_open(const char *who, int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int device, ldpc_hip_ctx **out,
                 int route = ROUTE_RESIDENT) {
    if (out) *out = nullptr;
    if (!out) return fail(LDPC_HIP_EINVAL, "%s: bad argument", who);
    std::vector<int32_t> off, tab;
    int ne_max = 0;
    const codeset_kind &kind = *codeset_find(decoder_id, route);
    if (int rc = codeset_build(who, kind, rh, nh, M, hd, C, off, tab, &ne_max)) return rc;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(LDPC_HIP_EINVAL, "%s: device %d of %d", who, device, ndev);
    std::unique_ptr<ldpc_hip_ctx, void (*)(ldpc_hip_ctx *)> c(new ldpc_hip_ctx(), ldpc_hip_close);
    ldpc_codeset_state *s = c->codes = new ldpc_codeset_state();
    s->route = route;
    c->decoder_id = decoder_id; c->device = device;
    c->rh = rh; c->nh = nh; c->M = M; c->N = nh * M; c->R = rh * M;
    c->ne = kind.is & CS_SLOTS  ? (int)((tab.size() - (size_t)C * (rh + nh + 3)) / 3)   // edges of the whole set
            : kind.is & CS_COLS ? (int)((tab.size() - (size_t)C * (rh + nh + 3)) / 2)
                                : (int)(tab.size() - (size_t)C * (rh + 1));
    c->hard_words = (c->N + 31) / 32;
    c->multiwave = M > 64;
    c->F = c->multiwave ? 1 : 64 / M;
    c->threads = c->multiwave ? ((M + 63) / 64) * 64 : 64;
    if (kind.is & CS_FLOOD) {   // fewer frames when their images do not fit, several groups of lanes per frame
        c->F = ldpc::sp_codes_frames(!(kind.is & CS_CHECKS), c->N, c->R, M, ne_max);
        c->threads = ldpc::sp_codes_groups(M, nh) * ldpc::sp_codes_lanes(M);
    }
    if (kind.is & CS_GLOBAL) {   // one frame per workgroup, whatever the lifting; one instance
        c->multiwave = false; c->F = 1;
        c->threads = ldpc::glob_threads(c->N);
        s->glob_stride = ldpc::glob_ws_bytes(c->N, c->R, ne_max, M, kind.glob_edge_arrays);
    }
    c->lds_bytes = kind.lds(c->F, rh, nh, M, ne_max);
    c->kernel_name = std::string(kind.kernel) + (c->multiwave ? "<multiwave>" : "");
    HIP_TRY(hipSetDevice(device));
    if (int rc = codeset_upload(*s, C, ne_max, off, tab)) return rc;
    *out = c.release();
    return 0;
}

// An IMS set: the quantiser over the `frames` received words of a decode launch, into the context's workspace, on `stream`.
// ims_coef_kernel's sequential energy sum, then one coalesced stream fp64 -> int16.
int codeset_ims_quantise(ldpc_hip_ctx *c, const double *d_llr, long long frames, hipStream_t stream) {
    ldpc_codeset_state *s = c->codes;
    if (frames > s->w_q_frames) {
        if (s->w_coef) (void)hipFree(s->w_coef);
        if (s->w_q) (void)hipFree(s->w_q);
        s->w_coef = nullptr; s->w_q = nullptr; s->w_q_frames = 0;
        HIP_TRY(hipMalloc(&s->w_coef, sizeof(double) * (size_t)frames));
        HIP_TRY(hipMalloc(&s->w_q, sizeof(int16_t) * (size_t)frames * (size_t)c->N));
        s->w_q_frames = frames;
    }
    if ((frames + 63) / 64 > 0x7fffffffLL) return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_codes_dev: %lld received words are more than one launch takes", frames);
    if (int rc = ims_coef_launch(d_llr, s->w_coef, frames, c->N, stream)) return rc;
    ldpc::ImsQuantArgs qa{d_llr, s->w_coef, s->w_q, frames * (long long)c->N, c->N, c->ims_thr, (1 << (c->ims_qbits - 1)) - 1};
    long long blocks = (qa.total + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(ldpc::ims_quantise_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, qa);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ROUTE_GLOBAL: the workgroups of a launch over `grid` items -- at most kGlobSetGrid, halved while their slices exceed kGlobSetBytes, and
// at most LDPC_HIP_CODES_GLOBAL_GRID = n (read per call: the tests make a handful of workgroups walk many items) -- and their workspace.
// A launch that needs more slices than the context holds frees the workspace and allocates a larger one: hipFree waits for the device,
// so earlier launches that use the old one have finished, and that call is not asynchronous (as launch_global's first calls are not).
int codeset_glob_reserve(ldpc_codeset_state *s, long long &grid) {
    long long cap = kGlobSetGrid;
    while (cap > kGlobSetMinGrid && (size_t)cap * s->glob_stride > kGlobSetBytes) cap /= 2;
    if (const char *e = getenv("LDPC_HIP_CODES_GLOBAL_GRID")) {
        const long long n = atoll(e);
        if (n > 0 && n < cap) cap = n;
    }
    if (grid > cap) grid = cap;
    if (grid > s->glob_grid) {
        if (s->w_glob) (void)hipFree(s->w_glob);
        s->w_glob = nullptr; s->glob_grid = 0;
        HIP_TRY(hipMalloc(&s->w_glob, (size_t)grid * s->glob_stride));
        s->glob_grid = (int)grid;
    }
    return 0;
}

// The decode launch over n_slots codes: code_list [n_slots] (DEVICE) names them, null = all C codes in order.  Outputs [n_slots][B]...
// points > 1: an SNR grid on shared LLRs [points][B][N]; the list names items p * C + c, null = all points * C in order.
int codeset_decode_launch(ldpc_hip_ctx *c, const double *d_llr, int shared_llr, long long B, int maxiter, double alpha, uint32_t *d_hard,
                          int32_t *d_iters, double *d_soft, hipStream_t stream, const int32_t *code_list, int n_slots, int points = 1) {
    if (B < 0) return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_codes_dev: bad argument");
    if (maxiter < 1) return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_codes_dev: maxiter must be >= 1 (got %d)", maxiter);
    if (int rc = alpha_refusal("ldpc_hip_decode_codes_dev", c->decoder_id, alpha)) return rc;
    // MS_DEC with an alpha that is not above zero (ms_alpha_not_positive): ms_flood_codes_kernel and ms_flood_wide_codes_kernel keep the
    // sign of m * alpha as upstream does, but start from y + 0.0 and return +0.0 where upstream's y + acc * alpha is -0.0.
    // ms_global_codes_kernel (ms_global_frame) is upstream's arithmetic as written; a set's tables are those of its route, so the other
    // routes refuse
    if (ms_alpha_not_positive(c->decoder_id, alpha) && !(codeset_kind_of(c).is & CS_GLOBAL))
        return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_codes_dev: alpha = %g is not above zero; %s gives upstream's bits for alpha > 0 only, "
                    "a set opened with ldpc_hip_open_codes_global takes any alpha", alpha, c->kernel_name.c_str());
    if (B == 0) return 0;
    if (!d_llr) return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_codes_dev: null llr");
    ldpc_codeset_state *s = c->codes;
    if (!code_list) n_slots = s->C * points;
    if (n_slots < 1) return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_codes_dev: a launch covers at least one code");   // never a grid of 0 blocks
    const long long bpc = (B + c->F - 1) / c->F;
    if (bpc * n_slots > 0x7fffffffLL) return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_codes_dev: %d codes x %lld frames is more than one launch takes", n_slots, B);
    HIP_TRY(hipSetDevice(c->device));
    ldpc::CodesetArgs a{};
    a.llr = d_llr; a.hard = d_hard; a.iters = d_iters; a.soft_out = d_soft;
    a.tab = s->d_tab; a.code_off = s->d_off; a.code_list = code_list;
    a.B = B; a.llr_code_stride = shared_llr ? 0 : B * (long long)c->N; a.blocks_per_code = (int)bpc;
    a.llr_point_stride = points > 1 ? B * (long long)c->N : 0;
    a.C = s->C; a.rh = c->rh; a.nh = c->nh; a.M = c->M; a.N = c->N; a.F = c->F; a.maxiter = maxiter; a.hard_words = c->hard_words;
    a.alpha = alpha; a.ne_max = s->ne_max;
    const codeset_kind &kind = codeset_kind_of(c);
    const void *k = c->multiwave ? kind.multiwave : kind.wave;
    if (int rc = set_lds_limit(k, c->lds_bytes)) return rc;
    ProfTimer timer;
    if (int rc = timer.begin(c, stream)) return rc;
    ldpc::ImsCodesArgs ia{};   // the second argument of a CS_QUANT kernel; the others take the first alone
    if (kind.is & CS_QUANT) {   // once per received word: B of them when the codes share the LLRs, C * B otherwise
        if (int rc = codeset_ims_quantise(c, d_llr, shared_llr ? B * points : B * (long long)s->C, stream)) return rc;
        ia.q = s->w_q; ia.max_data = (1 << (c->ims_dbits - 1)) - 1; ia.ialpha = (int)(alpha * (1 << 4));   // decoders.cpp:5445, :5458
    }
    long long grid = bpc * n_slots;
    ldpc::CodesetGlobArgs ga{};   // the first argument of a CS_GLOBAL kernel
    if (kind.is & CS_GLOBAL) {
        if (int rc = codeset_glob_reserve(s, grid)) return rc;
        ga.s = a; ga.ws = s->w_glob; ga.ws_stride = s->glob_stride; ga.items = bpc * n_slots;
    }
    void *kargs[] = {kind.is & CS_GLOBAL ? (void *)&ga : (void *)&a, &ia};
    c->last_launch = c->kernel_name.c_str();
    HIP_TRY(hipLaunchKernel(k, dim3((unsigned)grid), dim3((unsigned)c->threads), kargs, c->lds_bytes, stream));
    HIP_TRY(hipGetLastError());
    return timer.end();
}

// Frames per piece of the simulate entry points: at most 65536, the buffers of a piece (bytes_per_frame) within 1 GiB, the environment
// variable `cap_env` = n caps it (read per call).
long long codeset_piece(size_t bytes_per_frame, const char *cap_env, long long B) {
    long long piece = (long long)(((size_t)1 << 30) / bytes_per_frame);
    piece = piece > (1 << 16) ? (1 << 16) : (piece < 1 ? 1 : piece);
    if (const char *e = getenv(cap_env)) { if (atoll(e) > 0 && atoll(e) < piece) piece = atoll(e); }
    return piece > B ? B : piece;
}

long long codeset_piece(const ldpc_hip_ctx *c, long long B, int points = 1) {
    size_t per_frame = (size_t)c->codes->C * (sizeof(uint32_t) * (size_t)c->hard_words + 2 * sizeof(int32_t)) + sizeof(double) * (size_t)c->N;
    if (codeset_kind_of(c).is & CS_QUANT) per_frame += sizeof(double) + sizeof(int16_t) * (size_t)c->N;   // the quantiser's coef and int16 word
    return codeset_piece(per_frame * (size_t)points, "LDPC_HIP_CODES_PIECE", B);   // an SNR grid: the bytes of every point's frame
}

// The workspace for `piece` frames per code (grown, never shrunk): the decoder's input [piece] of in_bytes per frame, shared by the
// codes, its decisions [C][piece] of out_bytes per frame, and the iteration counts and records [C][piece].  points > 1 (an SNR grid):
// the call needs points * piece input rows and C times as many rows of the rest.  w_frames counts INPUT ROWS, so the capacity is
// that of the largest call so far and a single-SNR call after a grid call is sized by its own piece, as it always was; only the
// counters [points * C][5] keep the largest grid's rows.
int codeset_reserve(codeset_common &s, long long piece, void **w_in, size_t in_bytes, void **w_out, size_t out_bytes, int points = 1) {
    if (points > s.w_points) {
        if (s.w_cnt) (void)hipFree(s.w_cnt);
        s.w_cnt = nullptr;
        HIP_TRY(hipMalloc(&s.w_cnt, sizeof(unsigned long long) * 5 * (size_t)s.C * (size_t)points));
        s.w_points = points;
    }
    const long long rows = piece * points;
    if (rows <= s.w_frames) return 0;
    const size_t C = (size_t)s.C;
    void *old[] = {*w_in, *w_out, s.w_iters, s.w_info};
    for (void *p : old)
        if (p) (void)hipFree(p);
    *w_in = nullptr; *w_out = nullptr; s.w_iters = nullptr; s.w_info = nullptr; s.w_frames = 0;
    HIP_TRY(hipMalloc(w_in, in_bytes * (size_t)rows));
    HIP_TRY(hipMalloc(w_out, out_bytes * C * (size_t)rows));
    HIP_TRY(hipMalloc(&s.w_iters, sizeof(int32_t) * C * (size_t)rows));
    HIP_TRY(hipMalloc(&s.w_info, sizeof(int32_t) * C * (size_t)rows));
    s.w_frames = rows;
    return 0;
}

int codeset_reserve(ldpc_hip_ctx *c, long long piece, int points = 1) {
    ldpc_codeset_state *s = c->codes;
    return codeset_reserve(*s, piece, (void **)&s->w_llr, sizeof(double) * (size_t)c->N, (void **)&s->w_hard, sizeof(uint32_t) * (size_t)c->hard_words, points);
}

// The channel of ldpc_hip_channel_llr_dev with modulation 0 on the all-zero word for the simulate entry points: noise keyed by
// (seed, global frame, position), written to the workspace's [piece][N] LLRs (after codeset_reserve).  sigma is the caller's.
void codeset_channel_args(const ldpc_hip_ctx *c, int punctured_blocks, uint64_t seed, ldpc::ChannelArgs &ch) {
    ch.llr = c->codes->w_llr; ch.N = c->N; ch.T = 26.0; ch.seed = seed;
    ch.tx = nullptr; ch.ncw = 1; ch.ntx = c->N; ch.scatter = nullptr;
    ch.punct_start = c->N - c->M * punctured_blocks;
    ch.punct_val = punctured_llr(c->decoder_id);
}

int codeset_channel_launch(const ldpc_hip_ctx *c, ldpc::ChannelArgs &ch, long long first_frame, long long nb) {
    ch.B = nb; ch.first_frame = first_frame;
    long long blocks = (nb * (long long)((c->N + 1) / 2) + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(ldpc::channel_llr_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, nullptr, ch);
    HIP_TRY(hipGetLastError());
    return 0;
}

// channel -> set decode on the shared LLRs -> set count, for frames [first_frame, first_frame + nb) and the n_active codes of `list`
// (null: all)
int codeset_piece_launch(ldpc_hip_ctx *c, ldpc::ChannelArgs &ch, int maxiter, double alpha, long long first_frame, long long nb, bool want_info,
                         const int32_t *list, int n_active) {
    ldpc_codeset_state *s = c->codes;
    if (int rc = codeset_channel_launch(c, ch, first_frame, nb)) return rc;
    if (int rc = codeset_decode_launch(c, s->w_llr, 1, nb, maxiter, alpha, s->w_hard, s->w_iters, nullptr, nullptr, list, n_active)) return rc;
    return codeset_count_launch(c, s->w_hard, s->w_iters, nb, want_info ? s->w_info : nullptr, s->w_cnt, nullptr, list, n_active);
}

// The fixed-length run of the simulate entry points in pieces: run_piece(first, nb) draws, decodes and counts frames [first, first + nb)
// of the call for all codes, leaving their records in w_info [C][nb] where frame_info is asked for.  The device is the caller's
// current one; counters [C][5] and frame_info [C][B] (may be null) are the HOST results.
// points > 1: an SNR grid, P * C rows everywhere: counters [P][C][5], frame_info [P][C][B].
template <class Piece>
int codeset_simulate_loop(codeset_common &s, long long piece, long long B, unsigned long long *counters, int32_t *frame_info, Piece run_piece,
                          int points = 1) {
    const size_t C = (size_t)s.C * (size_t)points;
    HIP_TRY(hipMemsetAsync(s.w_cnt, 0, sizeof(unsigned long long) * 5 * C, nullptr));
    for (long long done = 0; done < B; done += piece) {
        const long long nb = (B - done) < piece ? (B - done) : piece;
        if (int rc = run_piece(done, nb)) return rc;
        if (frame_info)   // [C][nb] on the device -> columns [done, done + nb) of the caller's [C][B]
            HIP_TRY(hipMemcpy2D(frame_info + done, sizeof(int32_t) * (size_t)B, s.w_info, sizeof(int32_t) * (size_t)nb, sizeof(int32_t) * (size_t)nb, C,
                                hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipMemcpy(counters, s.w_cnt, sizeof(unsigned long long) * 5 * C, hipMemcpyDeviceToHost));
    return 0;
}

// What the two *_stop entry points ask of their arguments
int codeset_stop_args(const char *who, const unsigned long long *state, long long first_frame, long long first_batch, long long max_batch, int maxiter) {
    if (!state || first_frame < 0) return fail(LDPC_HIP_EINVAL, "%s: bad argument", who);
    if (first_batch < 1 || max_batch < first_batch)
        return fail(LDPC_HIP_EINVAL, "%s: batches of %lld .. %lld frames; 1 <= first_batch <= max_batch", who, first_batch, max_batch);
    if (maxiter < 1) return fail(LDPC_HIP_EINVAL, "%s: maxiter must be >= 1 (got %d)", who, maxiter);
    return 0;
}

// The batch schedule and the stopping rule of the *_stop entry points around the launches of one piece: run_piece(first, nb, list,
// n_active) draws, decodes and counts frames [first, first + nb) of the run for the n_active codes of `list` (DEVICE), leaving their
// records in w_info [n_active][nb].  The device is the caller's current one; w_cnt [C][5] is cleared; state [C][4] is the HOST result.
// full: the rule of an exact replay (stop_rule_codes_kernel<true>), which reads w_iters [n_active][nb] too; state is [C][6].
// references [points] (HOST), points >= 1: an SNR grid -- the rows are the P * C items, point p's rule reads references[p]
// (stop_rule_codes_kernel<FULL, true>) and reference_frame_error is not read; state is [P][C][4 or 6].
template <class Piece>
int codeset_stop_loop(codeset_common &s, long long piece, int n_frame_errors, long long n_experiments, double reference_frame_error, long long first_batch,
                      long long max_batch, unsigned long long *state, Piece run_piece, bool full = false, const double *references = nullptr,
                      int points = 1) {
    const size_t C = (size_t)s.C * (size_t)points, words = full ? 6 : 4;
    codeset_rule_ws &w = s.stop;
    if (C > w.rows) {
        void *old[] = {w.rule, w.running, w.list};
        for (void *p : old)
            if (p) (void)hipFree(p);
        w.rule = nullptr; w.running = nullptr; w.list = nullptr; w.rows = 0;
        HIP_TRY(hipMalloc(&w.rule, sizeof(unsigned long long) * 6 * C));
        HIP_TRY(hipMalloc(&w.running, sizeof(int32_t) * C));
        HIP_TRY(hipMalloc(&w.list, sizeof(int32_t) * C));
        if (!w.nactive) HIP_TRY(hipMalloc(&w.nactive, sizeof(int32_t)));
        w.rows = C;
    }
    if (references) {
        if (!w.reference) HIP_TRY(hipMalloc(&w.reference, sizeof(double) * ldpc::kGridPoints));
        HIP_TRY(hipMemcpy(w.reference, references, sizeof(double) * (size_t)points, hipMemcpyHostToDevice));
    }
    std::vector<int32_t> ident(C), ones(C, 1);
    for (size_t q = 0; q < C; ++q) ident[q] = (int32_t)q;
    HIP_TRY(hipMemcpy(w.list, ident.data(), sizeof(int32_t) * C, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(w.running, ones.data(), sizeof(int32_t) * C, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(w.rule, 0, sizeof(unsigned long long) * words * C, nullptr));
    HIP_TRY(hipMemsetAsync(s.w_cnt, 0, sizeof(unsigned long long) * 5 * C, nullptr));
    int32_t n_active = (int32_t)C;
    long long first = 0, batch = first_batch;   // every running code has consumed the same number of frames: `first`
    while (n_active > 0) {
        const long long room = n_experiments + 1 - first;
        const long long B = batch < room ? batch : room;
        if (B <= 0) break;
        for (long long done = 0; done < B && n_active > 0; done += piece) {
            const long long nb = (B - done) < piece ? (B - done) : piece;
            if (int rc = run_piece(first + done, nb, w.list, n_active)) return rc;
            const ldpc::CodesetRuleArgs ra{s.w_info, w.list, w.rule, w.running, nb, n_frame_errors, n_experiments, reference_frame_error};
            const ldpc::CodesetRuleFullArgs fa{ra, s.w_iters};
            if (references && full) {
                ldpc::CodesetRuleGridArgs<true> ga{};
                static_cast<ldpc::CodesetRuleFullArgs &>(ga) = fa; ga.reference = w.reference; ga.C = s.C;
                hipLaunchKernelGGL((ldpc::stop_rule_codes_kernel<true, true>), dim3((unsigned)n_active), dim3(64), 0, nullptr, ga);
            } else if (references) {
                ldpc::CodesetRuleGridArgs<false> ga{};
                static_cast<ldpc::CodesetRuleArgs &>(ga) = ra; ga.reference = w.reference; ga.C = s.C;
                hipLaunchKernelGGL((ldpc::stop_rule_codes_kernel<false, true>), dim3((unsigned)n_active), dim3(64), 0, nullptr, ga);
            }
            else if (full) hipLaunchKernelGGL(ldpc::stop_rule_codes_kernel<true>, dim3((unsigned)n_active), dim3(64), 0, nullptr, fa);
            else hipLaunchKernelGGL(ldpc::stop_rule_codes_kernel<false>, dim3((unsigned)n_active), dim3(64), 0, nullptr, ra);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(ldpc::running_codes_kernel, dim3(1), dim3(64), 0, nullptr, w.running, (int)C, w.list, w.nactive);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(&n_active, w.nactive, sizeof(int32_t), hipMemcpyDeviceToHost));   // the one value the host needs per piece
        }
        first += B;
        if (batch < max_batch) batch = batch * 4 < max_batch ? batch * 4 : max_batch;
    }
    HIP_TRY(hipMemcpy(state, w.rule, sizeof(unsigned long long) * words * C, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

extern "C" {

int ldpc_hip_open_codes(int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int device, ldpc_hip_ctx **out) {
    if (out) *out = nullptr;
    if (decoder_id != LDPC_HIP_MS_DEC && decoder_id != LDPC_HIP_LMS_DEC)   // TDMP, IASP, LCHE and IMS sets open through ldpc_hip_open_codes_tdmp / _iasp / _lche / _ims
        return fail(LDPC_HIP_EINVAL, "ldpc_hip_open_codes: decoder id %d; a code set decodes with MS_DEC (3) or LMS_DEC (8)", decoder_id);
    return codeset_open("ldpc_hip_open_codes", decoder_id, rh, nh, M, hd, C, device, out);
}

int ldpc_hip_open_codes_tdmp(int rh, int nh, int M, const int16_t *hd, int C, int device, ldpc_hip_ctx **out) {
    return codeset_open("ldpc_hip_open_codes_tdmp", LDPC_HIP_TASP_DEC, rh, nh, M, hd, C, device, out);
}

int ldpc_hip_open_codes_iasp(int rh, int nh, int M, const int16_t *hd, int C, int device, ldpc_hip_ctx **out) {
    return codeset_open("ldpc_hip_open_codes_iasp", LDPC_HIP_IASP_DEC, rh, nh, M, hd, C, device, out);
}

int ldpc_hip_open_codes_lche(int rh, int nh, int M, const int16_t *hd, int C, int device, ldpc_hip_ctx **out) {
    return codeset_open("ldpc_hip_open_codes_lche", LDPC_HIP_LCHE_DEC, rh, nh, M, hd, C, device, out);
}

int ldpc_hip_open_codes_ims(int rh, int nh, int M, const int16_t *hd, int C, int device, ldpc_hip_ctx **out) {
    return codeset_open("ldpc_hip_open_codes_ims", LDPC_HIP_IMS_DEC, rh, nh, M, hd, C, device, out);
}

int ldpc_hip_open_codes_sp(int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int device, ldpc_hip_ctx **out) {
    if (out) *out = nullptr;
    if (decoder_id != LDPC_HIP_SP_DEC && decoder_id != LDPC_HIP_ASP_DEC)
        return fail(LDPC_HIP_EINVAL, "ldpc_hip_open_codes_sp: decoder id %d; SP_DEC (1) or ASP_DEC (2)", decoder_id);
    return codeset_open("ldpc_hip_open_codes_sp", decoder_id, rh, nh, M, hd, C, device, out);
}

int ldpc_hip_open_codes_global(int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int device, ldpc_hip_ctx **out) {
    if (out) *out = nullptr;
    if (int rc = codeset_global_id("ldpc_hip_open_codes_global", decoder_id)) return rc;
    return codeset_open("ldpc_hip_open_codes_global", decoder_id, rh, nh, M, hd, C, device, out, ROUTE_GLOBAL);
}

int ldpc_hip_open_codes_wide(int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int device, ldpc_hip_ctx **out) {
    if (out) *out = nullptr;
    if (int rc = codeset_wide_id("ldpc_hip_open_codes_wide", decoder_id)) return rc;
    return codeset_open("ldpc_hip_open_codes_wide", decoder_id, rh, nh, M, hd, C, device, out, ROUTE_WIDE);
}

int ldpc_hip_decode_codes_dev(ldpc_hip_ctx *c, const double *d_llr, int shared_llr, long long B, int maxiter, double alpha, uint32_t *d_hard,
                              int32_t *d_iters, double *d_soft, void *stream_) {
    if (int rc = codeset_ctx(c, "ldpc_hip_decode_codes_dev")) return rc;
    return codeset_decode_launch(c, d_llr, shared_llr, B, maxiter, alpha, d_hard, d_iters, d_soft, (hipStream_t)stream_, nullptr, 0);
}

int ldpc_hip_count_errors_codes_dev(ldpc_hip_ctx *c, const uint32_t *d_hard, const int32_t *d_iters, long long B, int32_t *d_frame_info,
                                    unsigned long long *d_counters, void *stream_) {
    if (int rc = codeset_ctx(c, "ldpc_hip_count_errors_codes_dev")) return rc;
    if (!d_hard || !d_iters || !d_counters || B < 0) return fail(LDPC_HIP_EINVAL, "ldpc_hip_count_errors_codes_dev: bad argument");
    if (B == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    return codeset_count_launch(c, d_hard, d_iters, B, d_frame_info, d_counters, (hipStream_t)stream_);
}

int ldpc_hip_simulate_codes(ldpc_hip_ctx *c, double snr_db, int punctured_blocks, int maxiter, double alpha, uint64_t seed, long long first_frame,
                            long long B, unsigned long long *counters, int32_t *frame_info) {
    if (int rc = codeset_ctx(c, "ldpc_hip_simulate_codes")) return rc;
    if (!counters || B < 0 || first_frame < 0) return fail(LDPC_HIP_EINVAL, "ldpc_hip_simulate_codes: bad argument");
    if (maxiter < 1) return fail(LDPC_HIP_EINVAL, "ldpc_hip_simulate_codes: maxiter must be >= 1 (got %d)", maxiter);
    ldpc::ChannelArgs ch{};
    if (int rc = awgn_sigma(c, snr_db, 0, punctured_blocks, &ch.sigma)) return rc;   // the common rate (nh - rh) / (nh - punctured_blocks)
    HIP_TRY(hipSetDevice(c->device));
    const long long piece = codeset_piece(c, B);
    if (int rc = codeset_reserve(c, piece)) return rc;
    codeset_channel_args(c, punctured_blocks, seed, ch);
    return codeset_simulate_loop(*c->codes, piece, B, counters, frame_info, [&](long long first, long long nb) -> int {
        return codeset_piece_launch(c, ch, maxiter, alpha, first_frame + first, nb, frame_info != nullptr, nullptr, 0);
    });
}

int ldpc_hip_simulate_codes_stop(ldpc_hip_ctx *c, double snr_db, int punctured_blocks, int maxiter, double alpha, uint64_t seed, long long first_frame,
                                 int n_frame_errors, long long n_experiments, double reference_frame_error, long long first_batch,
                                 long long max_batch, unsigned long long *state) {
    if (int rc = codeset_ctx(c, "ldpc_hip_simulate_codes_stop")) return rc;
    if (int rc = codeset_stop_args("ldpc_hip_simulate_codes_stop", state, first_frame, first_batch, max_batch, maxiter)) return rc;
    ldpc::ChannelArgs ch{};
    if (int rc = awgn_sigma(c, snr_db, 0, punctured_blocks, &ch.sigma)) return rc;   // the common rate (nh - rh) / (nh - punctured_blocks)
    std::memset(state, 0, sizeof(unsigned long long) * 4 * (size_t)c->codes->C);
    if (n_frame_errors <= 0 || n_experiments < 0) return 0;   // :591 fails before the first frame
    HIP_TRY(hipSetDevice(c->device));
    const long long piece = codeset_piece(c, max_batch < n_experiments + 1 ? max_batch : n_experiments + 1);
    if (int rc = codeset_reserve(c, piece)) return rc;
    codeset_channel_args(c, punctured_blocks, seed, ch);
    return codeset_stop_loop(*c->codes, piece, n_frame_errors, n_experiments, reference_frame_error, first_batch, max_batch, state,
                             [&](long long first, long long nb, const int32_t *list, int n_active) -> int {
                                 return codeset_piece_launch(c, ch, maxiter, alpha, first_frame + first, nb, true, list, n_active);
                             });
}

}  // extern "C"

// ---- exact replay on a binary code set (ldpc_hip_mt_*_codes): the generator of ldpc_mt_api.hpp draws the [piece][N] LLRs of upstream's
// own stream ONCE into the set's workspace and every code decodes them -- what a search that calls reset_random() before each
// candidate computes, in one launch per piece.
namespace {

int mt_codes_ctx(const ldpc_hip_ctx *c, const char *who) {
    if (!c || !c->codes) return fail(LDPC_HIP_EINVAL, "%s: not a binary code-set context (ldpc_hip_open_codes and its kin)", who);
    return 0;
}

// the next nb frames of the stream -> w_llr (after codeset_reserve) -> set decode -> set count, for the n_active codes of `list` (null: all)
int mt_codes_piece_launch(ldpc_hip_ctx *c, double snr_db, int punctured_blocks, int maxiter, double alpha, long long nb, bool want_info,
                          const int32_t *list, int n_active) {
    ldpc_codeset_state *s = c->codes;
    if (int rc = mt_llr_rows(c, snr_db, 0, punctured_blocks, nb, 0, nb, s->w_llr, nullptr)) return rc;
    if (int rc = codeset_decode_launch(c, s->w_llr, 1, nb, maxiter, alpha, s->w_hard, s->w_iters, nullptr, nullptr, list, n_active)) return rc;
    return codeset_count_launch(c, s->w_hard, s->w_iters, nb, want_info ? s->w_info : nullptr, s->w_cnt, nullptr, list, n_active);
}

// what mt_frame_proto refuses, before anything is drawn or reserved
int mt_codes_channel_check(ldpc_hip_ctx *c, double snr_db, int punctured_blocks) {
    ldpc_mt::PolarArgs a{};
    return mt_frame_proto(c, snr_db, 0, punctured_blocks, a);
}

}  // namespace

extern "C" {

int ldpc_hip_mt_set_state_codes(ldpc_hip_ctx *c, const uint32_t state[624], int pos) {
    if (int rc = mt_codes_ctx(c, "ldpc_hip_mt_set_state_codes")) return rc;
    if (!state || pos < 0 || pos > 624) return fail(LDPC_HIP_EINVAL, "ldpc_hip_mt_set_state_codes: bad argument");
    return mt_state_store(c, state, pos);
}

int ldpc_hip_mt_get_state_codes(ldpc_hip_ctx *c, uint32_t state[624], int *pos) {
    if (int rc = mt_codes_ctx(c, "ldpc_hip_mt_get_state_codes")) return rc;
    if (!state || !pos) return fail(LDPC_HIP_EINVAL, "ldpc_hip_mt_get_state_codes: bad argument");
    return mt_state_load(c, "ldpc_hip_mt_set_state", state, pos);
}

int ldpc_hip_mt_advance_codes(ldpc_hip_ctx *c, double snr_db, int punctured_blocks, long long frames) {
    if (int rc = mt_codes_ctx(c, "ldpc_hip_mt_advance_codes")) return rc;
    if (frames < 0) return fail(LDPC_HIP_EINVAL, "ldpc_hip_mt_advance_codes: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    return mt_llr_rows(c, snr_db, 0, punctured_blocks, frames, 0, 0, nullptr, nullptr);
}

int ldpc_hip_mt_simulate_codes(ldpc_hip_ctx *c, double snr_db, int punctured_blocks, int maxiter, double alpha, long long B,
                               unsigned long long *counters, int32_t *frame_info, int32_t *iters) {
    if (int rc = mt_codes_ctx(c, "ldpc_hip_mt_simulate_codes")) return rc;
    if (!counters || B < 0) return fail(LDPC_HIP_EINVAL, "ldpc_hip_mt_simulate_codes: bad argument");
    if (maxiter < 1) return fail(LDPC_HIP_EINVAL, "ldpc_hip_mt_simulate_codes: maxiter must be >= 1 (got %d)", maxiter);
    if (int rc = mt_codes_channel_check(c, snr_db, punctured_blocks)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    ldpc_codeset_state *s = c->codes;
    const long long piece = codeset_piece(c, B);
    if (int rc = codeset_reserve(c, piece)) return rc;
    const size_t C = (size_t)s->C;
    return codeset_simulate_loop(*s, piece, B, counters, frame_info, [&](long long first, long long nb) -> int {
        if (int rc = mt_codes_piece_launch(c, snr_db, punctured_blocks, maxiter, alpha, nb, frame_info != nullptr, nullptr, 0)) return rc;
        if (iters)   // [C][nb] on the device -> columns [first, first + nb) of the caller's [C][B]
            HIP_TRY(hipMemcpy2D(iters + first, sizeof(int32_t) * (size_t)B, s->w_iters, sizeof(int32_t) * (size_t)nb, sizeof(int32_t) * (size_t)nb, C,
                                hipMemcpyDeviceToHost));
        return 0;
    });
}

int ldpc_hip_frames_codes_host(ldpc_hip_ctx *c, const double *llr, long long B, int maxiter, double alpha, unsigned long long *counters,
                               int32_t *frame_info, int32_t *iters) {
    if (int rc = mt_codes_ctx(c, "ldpc_hip_frames_codes_host")) return rc;
    if (!counters || B < 0 || (B > 0 && !llr)) return fail(LDPC_HIP_EINVAL, "ldpc_hip_frames_codes_host: bad argument");
    if (maxiter < 1) return fail(LDPC_HIP_EINVAL, "ldpc_hip_frames_codes_host: maxiter must be >= 1 (got %d)", maxiter);
    HIP_TRY(hipSetDevice(c->device));
    ldpc_codeset_state *s = c->codes;
    const long long piece = codeset_piece(c, B);
    if (int rc = codeset_reserve(c, piece)) return rc;
    const size_t C = (size_t)s->C;
    return codeset_simulate_loop(*s, piece, B, counters, frame_info, [&](long long first, long long nb) -> int {
        HIP_TRY(hipMemcpy(s->w_llr, llr + (size_t)first * (size_t)c->N, sizeof(double) * (size_t)nb * (size_t)c->N, hipMemcpyHostToDevice));
        if (int rc = codeset_decode_launch(c, s->w_llr, 1, nb, maxiter, alpha, s->w_hard, s->w_iters, nullptr, nullptr, nullptr, 0)) return rc;
        if (int rc = codeset_count_launch(c, s->w_hard, s->w_iters, nb, frame_info ? s->w_info : nullptr, s->w_cnt, nullptr)) return rc;
        if (iters)
            HIP_TRY(hipMemcpy2D(iters + first, sizeof(int32_t) * (size_t)B, s->w_iters, sizeof(int32_t) * (size_t)nb, sizeof(int32_t) * (size_t)nb, C,
                                hipMemcpyDeviceToHost));
        return 0;
    });
}

int ldpc_hip_mt_simulate_codes_stop(ldpc_hip_ctx *c, double snr_db, int punctured_blocks, int maxiter, double alpha, int n_frame_errors,
                                    long long n_experiments, double reference_frame_error, long long first_batch, long long max_batch,
                                    unsigned long long *state) {
    using namespace ldpc_mt;
    if (int rc = mt_codes_ctx(c, "ldpc_hip_mt_simulate_codes_stop")) return rc;
    if (int rc = codeset_stop_args("ldpc_hip_mt_simulate_codes_stop", state, 0, first_batch, max_batch, maxiter)) return rc;
    if (int rc = mt_codes_channel_check(c, snr_db, punctured_blocks)) return rc;
    std::memset(state, 0, sizeof(unsigned long long) * 6 * (size_t)c->codes->C);
    if (n_frame_errors <= 0 || n_experiments < 0) return 0;   // :591 fails before the first frame
    HIP_TRY(hipSetDevice(c->device));
    const long long piece = codeset_piece(c, max_batch < n_experiments + 1 ? max_batch : n_experiments + 1);
    if (int rc = codeset_reserve(c, piece)) return rc;
    // the codes stop at different frames: the generator goes back to where it was, ldpc_hip_mt_advance_codes takes it to one code's end
    DeviceState &m = c->mt;
    std::vector<uint32_t> entry(MTN);
    const long long entry_pos = m.pos, entry_frames = m.frames_taken;
    HIP_TRY(hipMemcpy(entry.data(), m.d_state, sizeof(uint32_t) * MTN, hipMemcpyDeviceToHost));
    const int rc = codeset_stop_loop(*c->codes, piece, n_frame_errors, n_experiments, reference_frame_error, first_batch, max_batch, state,
                                     [&](long long, long long nb, const int32_t *list, int n_active) -> int {   // pieces come in frame order
                                         return mt_codes_piece_launch(c, snr_db, punctured_blocks, maxiter, alpha, nb, true, list, n_active);
                                     }, true);
    if (hipMemcpy(m.d_state, entry.data(), sizeof(uint32_t) * MTN, hipMemcpyHostToDevice) != hipSuccess && rc == 0)
        return fail(LDPC_HIP_EHIP, "ldpc_hip_mt_simulate_codes_stop: the generator's state could not be put back");
    m.pos = entry_pos; m.frames_taken = entry_frames;
    return rc;
}

}  // extern "C"
