// Host side of the GF(q) code-set kernels (ldpc_gfq_codeset.hpp): the concatenated record table, the field tables of the set, the
// ldpc_hip_*codes_gfq* entry points and the shared-noise Monte-Carlo pass.  Included at the end of ldpc_hip.hip, after ldpc_gfq_api.hpp
// (the graph of a code, the tables, the choice and the launch of the kernel instance), ldpc_gfq_chain_api.hpp (the channel launch) and
// ldpc_codeset_api.hpp (codeset_common: tables, workspace and the two simulate loops of a code set).
#pragma once

struct ldpc_codeset_gfq_state : codeset_common {
    int q_bits = 0, q = 0;
    GfqKernel kern;
    int num_cu = 0;
    int16_t *d_i16 = nullptr;          // mul | div, q - 1 rows each
    char *d_ws = nullptr;              // message state, one slot per workgroup
    int ws_slots = 0;
    double *w_soft = nullptr;          // [w_frames][q][N], shared by the codes; [C][w_frames][q][N] while the codes carry words
    int16_t *w_qh = nullptr;           // [C][w_frames][N]
    // exact replay (ldpc_hip_*_codes_gfq with mt_ / noise_host in the name)
    int16_t *d_words = nullptr;        // [C][N] the word each code sends (ldpc_hip_codes_gfq_set_codewords); null = all-zero, shared soft values
    double *x_noise = nullptr;         // [x_frames][N * q_bits] Gaussians of a piece
    long long x_frames = 0;
};

void ldpc_codeset_gfq_release(ldpc_codeset_gfq_state *s) {
    if (!s) return;
    void *dev[] = {s->d_i16, s->d_ws, s->w_soft, s->w_qh, s->d_words, s->x_noise};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    codeset_common_release(*s);
    delete s;
}

namespace {

// Checks a GF(q) code set and builds its table: per code the record of ldpc_gfq_codeset.hpp; off[c] = index of code c's record.
// The per-code rules are those of ldpc_hip_open_gfq; every refusal names the code.
int codeset_gfq_build(const char *who, int q_bits, int rh, int nh, int M, const int16_t *hb, const int16_t *hc, int C, std::vector<int32_t> &off,
                      std::vector<int32_t> &tab, int *ne_max_out = nullptr) {
    if (!hb || !hc || rh <= 0 || nh <= 0 || M <= 0) return fail(LDPC_HIP_EINVAL, "%s: null matrix or non-positive size", who);
    if (C < 1) return fail(LDPC_HIP_EINVAL, "%s: C = %d, a code set holds at least one code", who, C);
    if (q_bits < 2) return fail(LDPC_HIP_EUNSUPPORTED, "%s: q_bits = %d, GF(q) needs q_bits >= 2 (binary sets: ldpc_hip_open_codes)", who, q_bits);
    if (q_bits > 10) return fail(LDPC_HIP_EUNSUPPORTED, "%s: q = 2^%d, at most q = 1024 is supported (upstream's QMAX, decoders.cpp:74)", who, q_bits);
    if (M >= 65536 || nh >= 65536 || rh >= 65536) return fail(LDPC_HIP_EUNSUPPORTED, "%s: M, rh and nh must be < 65536", who);
    if ((long long)nh * M >= (1LL << 28)) return fail(LDPC_HIP_EUNSUPPORTED, "%s: code length nh * M = %lld: at most 2^28 - 1 is supported", who, (long long)nh * M);
    const int q = 1 << q_bits;
    off.clear(); tab.clear();
    GfqGraph g;
    std::vector<int32_t> e_rl;
    int ne_max = 0;
    for (int c = 0; c < C; ++c) {
        char pre[96];
        snprintf(pre, sizeof pre, "%s: code %d, ", who, c);
        if (int rc = gfq_graph(pre, true, rh, nh, M, q, hb + (size_t)c * rh * nh, hc + (size_t)c * rh * nh, g)) return rc;
        if (tab.size() + ldpc_gfq::record_length(rh, nh, g.E) >= ((size_t)1 << 31))
            return fail(LDPC_HIP_EINVAL, "%s: the table of %d codes exceeds 2^31 entries", who, C);
        e_rl.assign(g.e_coef.begin(), g.e_coef.end());   // the set's tables hold every coefficient: row v - 1 is v's
        for (int32_t &v : e_rl) --v;
        off.push_back((int32_t)tab.size());
        tab.push_back(g.E); tab.push_back(g.cw2);
        for (const std::vector<int32_t> *part : {&g.row_start, &g.col_start, &g.e_col, &g.e_circ, &e_rl, &g.ce_edge}) tab.insert(tab.end(), part->begin(), part->end());
        ne_max = g.E > ne_max ? g.E : ne_max;
    }
    if (ne_max_out) *ne_max_out = ne_max;
    return 0;
}

int codeset_gfq_ctx(const ldpc_hip_ctx *c, const char *who) {
    if (!c || !c->codes_gfq) return fail(LDPC_HIP_EINVAL, "%s: not a GF(q) code-set context (ldpc_hip_open_codes_gfq)", who);
    return 0;
}

// The decode launch over n_slots codes: code_list [n_slots] (DEVICE) names them, null = all C codes in order.  Outputs [n_slots][B]...
int codeset_gfq_decode_launch(ldpc_hip_ctx *c, const double *d_soft, int shared_soft, long long B, int maxiter, int16_t *d_qhard, int32_t *d_iters,
                              double *d_post, hipStream_t stream, const int32_t *code_list, int n_slots) {
    if (B < 0) return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_codes_gfq_dev: bad argument");
    if (maxiter < 1) return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_codes_gfq_dev: maxiter must be >= 1 (got %d)", maxiter);
    if (B == 0) return 0;
    if (!d_soft) return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_codes_gfq_dev: null input");
    ldpc_codeset_gfq_state *g = c->codes_gfq;
    if (!code_list) n_slots = g->C;
    if (n_slots < 1) return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_codes_gfq_dev: a launch covers at least one code");   // never a grid of 0 blocks
    const long long items = B * n_slots;
    if (B > 0x7fffffffLL || items > 0x7fffffffLL)
        return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_codes_gfq_dev: %d codes x %lld frames is more than one launch takes", n_slots, B);
    HIP_TRY(hipSetDevice(c->device));

    const size_t stride = ldpc_gfq::slot_bytes(g->ne_max, c->M, c->N, g->q);
    int threads = 0, slots = 0;   // one slot per (code, frame) in flight
    if (int rc = gfq_slots(g->num_cu, c->R, c->N, g->kern.lpc, stride, items, g->d_ws, g->ws_slots, threads, slots)) return rc;
    ldpc_gfq::CodesArgs a{};
    a.soft = d_soft; a.qhard = d_qhard; a.iters = d_iters; a.post = d_post;
    a.ws = g->d_ws; a.ws_stride = stride;
    a.tab = g->d_tab; a.code_off = g->d_off; a.code_list = code_list;
    a.soft_code_stride = shared_soft ? 0 : B * (long long)g->q * c->N;
    a.B = (unsigned)B; a.items = (unsigned)items; a.maxiter = maxiter;
    a.rh = c->rh; a.nh = c->nh; a.M = c->M; a.N = c->N; a.R = c->R; a.q = g->q; a.lpc = g->kern.lpc;
    a.mul = g->d_i16; a.div = g->d_i16 + (size_t)(g->q - 1) * g->q;

    ProfTimer timer;
    if (int rc = timer.begin(c, stream)) return rc;
    c->last_launch = c->kernel_name.c_str();
    gfq_dispatch(g->kern, [&](auto ql, auto lpc) {
        hipLaunchKernelGGL((ldpc_gfq::gfq_codes_kernel<decltype(ql)::value, decltype(lpc)::value>), dim3((unsigned)slots), dim3((unsigned)threads), 0, stream, a);
    });
    HIP_TRY(hipGetLastError());
    return timer.end();
}

int codeset_gfq_count_launch(const ldpc_hip_ctx *c, const int16_t *d_qhard, const int32_t *d_iters, long long B, int32_t *d_frame_info,
                             unsigned long long *d_counters, hipStream_t stream, const int32_t *code_list = nullptr, int n_slots = 0,
                             const int16_t *d_words = nullptr) {
    const int C = code_list ? n_slots : c->codes_gfq->C;
    const int bpc = codeset_count_blocks(B, C);
    ldpc_gfq::CodesCountArgs a{d_qhard, d_iters, d_frame_info, d_counters, code_list, B, bpc, c->N, c->R, d_words};
    hipLaunchKernelGGL(ldpc_gfq::gfq_count_codes_kernel, dim3((unsigned)((long long)bpc * C)), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Frames per piece of the simulate entry points: the [piece][q][N] input -- one copy shared by the codes, or C copies while the codes
// carry words of their own (C * q * N * 8 bytes per frame) -- and the [C][piece] outputs within 1 GiB together, at most 65536,
// LDPC_HIP_GFQ_PIECE=n caps it (as in ldpc_hip_simulate_gfq).
long long codeset_gfq_piece(const ldpc_hip_ctx *c, long long B) {
    const ldpc_codeset_gfq_state *g = c->codes_gfq;
    const size_t copies = g->d_words ? (size_t)g->C : 1;
    const size_t per_frame = copies * sizeof(double) * (size_t)g->q * c->N + (size_t)g->C * (sizeof(int16_t) * (size_t)c->N + 2 * sizeof(int32_t));
    return codeset_piece(per_frame, "LDPC_HIP_GFQ_PIECE", B);
}

// ldpc_hip_codes_gfq_set_codewords drops the workspace when the set changes between shared and per-code soft values, so w_frames
// always speaks of buffers of the current kind
int codeset_gfq_reserve(ldpc_hip_ctx *c, long long piece) {
    ldpc_codeset_gfq_state *g = c->codes_gfq;
    const size_t copies = g->d_words ? (size_t)g->C : 1;
    return codeset_reserve(*g, piece, (void **)&g->w_soft, copies * sizeof(double) * (size_t)g->q * c->N, (void **)&g->w_qh, sizeof(int16_t) * (size_t)c->N);
}

// channel (the all-zero word, Philox stream tag 3) -> set decode on the shared soft values -> set count, for frames
// [first_frame, first_frame + nb) and the n_active codes of `list` (null: all)
int codeset_gfq_piece_launch(ldpc_hip_ctx *c, double sigma, int maxiter, uint64_t seed, long long first_frame, long long nb, bool want_info,
                             const int32_t *list, int n_active) {
    ldpc_codeset_gfq_state *g = c->codes_gfq;
    if (int rc = gfq_channel_launch(g->num_cu, c->N, g->q_bits, nullptr, nullptr, nullptr, sigma, seed, first_frame, nb, g->w_soft, nullptr)) return rc;
    if (int rc = codeset_gfq_decode_launch(c, g->w_soft, 1, nb, maxiter, g->w_qh, g->w_iters, nullptr, nullptr, list, n_active)) return rc;
    return codeset_gfq_count_launch(c, g->w_qh, g->w_iters, nb, want_info ? g->w_info : nullptr, g->w_cnt, nullptr, list, n_active);
}

}  // namespace

extern "C" {

int ldpc_hip_codes_gfq_table_host(int q_bits, int rh, int nh, int M, const int16_t *hb, const int16_t *hc, int C, int32_t *offsets, int32_t *table,
                                  long long capacity, long long *length) {
    std::vector<int32_t> off, tab;
    if (int rc = codeset_gfq_build("ldpc_hip_codes_gfq_table_host", q_bits, rh, nh, M, hb, hc, C, off, tab)) return rc;
    return codeset_table_out("ldpc_hip_codes_gfq_table_host", off, tab, offsets, table, capacity, length);
}

int ldpc_hip_open_codes_gfq(int q_bits, int rh, int nh, int M, const int16_t *hb, const int16_t *hc, int C, int device, ldpc_hip_ctx **out) {
    const char *who = "ldpc_hip_open_codes_gfq";
    if (out) *out = nullptr;
    if (!out) return fail(LDPC_HIP_EINVAL, "%s: bad argument", who);
    std::vector<int32_t> off, tab;
    int ne_max = 0;
    if (int rc = codeset_gfq_build(who, q_bits, rh, nh, M, hb, hc, C, off, tab, &ne_max)) return rc;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(LDPC_HIP_EINVAL, "%s: device %d of %d", who, device, ndev);
    const int q = 1 << q_bits;
    std::vector<int> coefs((size_t)q - 1);   // the tables of all q - 1 coefficients: mul[v - 1][s] = s * v, div[v - 1][s] = s / v
    for (int v = 1; v < q; ++v) coefs[(size_t)v - 1] = v;
    const std::vector<int16_t> ftab = gfq_tables(q_bits, coefs);

    std::unique_ptr<ldpc_hip_ctx, void (*)(ldpc_hip_ctx *)> c(new ldpc_hip_ctx(), ldpc_hip_close);
    ldpc_codeset_gfq_state *g = c->codes_gfq = new ldpc_codeset_gfq_state();
    g->q_bits = q_bits; g->q = q;
    c->decoder_id = LDPC_HIP_FHT_DEC; c->device = device;
    c->rh = rh; c->nh = nh; c->M = M; c->N = nh * M; c->R = rh * M; c->ne = ne_max;
    c->hard_words = (c->N + 31) / 32;
    g->kern = gfq_choose(q);
    c->kernel_name = gfq_kernel_name("gfq_codes_kernel", q, g->kern);
    c->last_launch = "";

    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    g->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;
    if (int rc = codeset_upload(*g, C, ne_max, off, tab)) return rc;
    HIP_TRY(hipMalloc(&g->d_i16, sizeof(int16_t) * ftab.size()));
    HIP_TRY(hipMemcpy(g->d_i16, ftab.data(), sizeof(int16_t) * ftab.size(), hipMemcpyHostToDevice));
    *out = c.release();
    return 0;
}

int ldpc_hip_codes(const ldpc_hip_ctx *c) { return !c ? 0 : c->codes ? c->codes->C : c->codes_gfq ? c->codes_gfq->C : 0; }
int ldpc_hip_gfq_q(const ldpc_hip_ctx *c) { return !c ? 0 : c->gfq ? c->gfq->q : c->codes_gfq ? c->codes_gfq->q : 0; }

int ldpc_hip_decode_codes_gfq_dev(ldpc_hip_ctx *c, const double *d_soft, int shared_soft, long long B, int maxiter, int16_t *d_qhard,
                                  int32_t *d_iters, double *d_post, void *stream_) {
    if (int rc = codeset_gfq_ctx(c, "ldpc_hip_decode_codes_gfq_dev")) return rc;
    return codeset_gfq_decode_launch(c, d_soft, shared_soft, B, maxiter, d_qhard, d_iters, d_post, (hipStream_t)stream_, nullptr, 0);
}

int ldpc_hip_count_errors_codes_gfq_dev(ldpc_hip_ctx *c, const int16_t *d_qhard, const int32_t *d_iters, long long B, int32_t *d_frame_info,
                                        unsigned long long *d_counters, void *stream_) {
    if (int rc = codeset_gfq_ctx(c, "ldpc_hip_count_errors_codes_gfq_dev")) return rc;
    if (!d_qhard || !d_iters || !d_counters || B < 0) return fail(LDPC_HIP_EINVAL, "ldpc_hip_count_errors_codes_gfq_dev: bad argument");
    if (B == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    return codeset_gfq_count_launch(c, d_qhard, d_iters, B, d_frame_info, d_counters, (hipStream_t)stream_);
}

int ldpc_hip_simulate_codes_gfq(ldpc_hip_ctx *c, double snr_db, int maxiter, uint64_t seed, long long first_frame, long long B,
                                unsigned long long *counters, int32_t *frame_info) {
    if (int rc = codeset_gfq_ctx(c, "ldpc_hip_simulate_codes_gfq")) return rc;
    if (!counters || B < 0 || first_frame < 0) return fail(LDPC_HIP_EINVAL, "ldpc_hip_simulate_codes_gfq: bad argument");
    if (maxiter < 1) return fail(LDPC_HIP_EINVAL, "ldpc_hip_simulate_codes_gfq: maxiter must be >= 1 (got %d)", maxiter);
    const double sigma = ldpc_hip_gfq_sigma(c, snr_db);   // rh and nh only: common to the set
    HIP_TRY(hipSetDevice(c->device));
    const long long piece = codeset_gfq_piece(c, B);
    if (int rc = codeset_gfq_reserve(c, piece)) return rc;
    return codeset_simulate_loop(*c->codes_gfq, piece, B, counters, frame_info, [&](long long first, long long nb) -> int {
        return codeset_gfq_piece_launch(c, sigma, maxiter, seed, first_frame + first, nb, frame_info != nullptr, nullptr, 0);
    });
}

int ldpc_hip_simulate_codes_gfq_stop(ldpc_hip_ctx *c, double snr_db, int maxiter, uint64_t seed, long long first_frame, int n_frame_errors,
                                     long long n_experiments, double reference_frame_error, long long first_batch, long long max_batch,
                                     unsigned long long *state) {
    if (int rc = codeset_gfq_ctx(c, "ldpc_hip_simulate_codes_gfq_stop")) return rc;
    if (int rc = codeset_stop_args("ldpc_hip_simulate_codes_gfq_stop", state, first_frame, first_batch, max_batch, maxiter)) return rc;
    const double sigma = ldpc_hip_gfq_sigma(c, snr_db);
    std::memset(state, 0, sizeof(unsigned long long) * 4 * (size_t)c->codes_gfq->C);
    if (n_frame_errors <= 0 || n_experiments < 0) return 0;   // bp_simulation.cpp:591 fails before the first frame
    HIP_TRY(hipSetDevice(c->device));
    const long long piece = codeset_gfq_piece(c, max_batch < n_experiments + 1 ? max_batch : n_experiments + 1);
    if (int rc = codeset_gfq_reserve(c, piece)) return rc;
    return codeset_stop_loop(*c->codes_gfq, piece, n_frame_errors, n_experiments, reference_frame_error, first_batch, max_batch, state,
                             [&](long long first, long long nb, const int32_t *list, int n_active) -> int {
                                 return codeset_gfq_piece_launch(c, sigma, maxiter, seed, first_frame + first, nb, true, list, n_active);
                             });
}

}  // extern "C"

// ---- exact replay on a GF(q) code set: what a search that calls reset_random() and bp_simulation(q_mod, HM, HC, ...) per candidate
// computes (search_ggp/scenario_based_code_generation.cpp:754, :852, :883).  The generator of ldpc_mt_api.hpp in sample mode draws the
// [piece][N * q_bits] Gaussians of upstream's stream once; without words the all-zero word's soft values are shared by the codes, with
// words (upstream encodes a message per candidate) gfq_channel_codes_kernel forms them per code.
namespace {

int gfq_exact_codes_workspace(ldpc_hip_ctx *c, long long piece) {
    ldpc_codeset_gfq_state *g = c->codes_gfq;
    if (int rc = codeset_gfq_reserve(c, piece)) return rc;
    if (piece <= g->x_frames) return 0;
    if (g->x_noise) (void)hipFree(g->x_noise);
    g->x_noise = nullptr; g->x_frames = 0;
    HIP_TRY(hipMalloc(&g->x_noise, sizeof(double) * (size_t)c->N * g->q_bits * (size_t)piece));
    g->x_frames = piece;
    return 0;
}

// x_noise [nb][N * q_bits] -> channel -> set decode -> set count, for the n_active codes of `list` (null: all)
int gfq_exact_codes_piece_launch(ldpc_hip_ctx *c, double sigma, int maxiter, long long nb, bool want_info, const int32_t *list, int n_active) {
    ldpc_codeset_gfq_state *g = c->codes_gfq;
    if (!g->d_words) {
        if (int rc = gfq_channel_launch(g->num_cu, c->N, g->q_bits, nullptr, nullptr, g->x_noise, sigma, 0, 0, nb, g->w_soft, nullptr)) return rc;
    } else {
        ldpc_gfq::CodesChanArgs a{g->d_words, g->x_noise, g->w_soft, list, nb, list ? n_active : g->C, c->N, sigma};
        const dim3 grid((unsigned)gfq_grid(g->num_cu, nb * (long long)c->N, 256)), block(256);
        switch (g->q_bits) {
        case 2: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_codes_kernel<2>, grid, block, 0, nullptr, a); break;
        case 3: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_codes_kernel<3>, grid, block, 0, nullptr, a); break;
        case 4: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_codes_kernel<4>, grid, block, 0, nullptr, a); break;
        case 5: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_codes_kernel<5>, grid, block, 0, nullptr, a); break;
        case 6: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_codes_kernel<6>, grid, block, 0, nullptr, a); break;
        case 7: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_codes_kernel<7>, grid, block, 0, nullptr, a); break;
        case 8: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_codes_kernel<8>, grid, block, 0, nullptr, a); break;
        case 9: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_codes_kernel<9>, grid, block, 0, nullptr, a); break;
        default: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_codes_kernel<10>, grid, block, 0, nullptr, a); break;
        }
        HIP_TRY(hipGetLastError());
    }
    if (int rc = codeset_gfq_decode_launch(c, g->w_soft, g->d_words ? 0 : 1, nb, maxiter, g->w_qh, g->w_iters, nullptr, nullptr, list, n_active)) return rc;
    return codeset_gfq_count_launch(c, g->w_qh, g->w_iters, nb, want_info ? g->w_info : nullptr, g->w_cnt, nullptr, list, n_active, g->d_words);
}

int gfq_exact_codes_draw(ldpc_hip_ctx *c, long long nb) {
    if (int rc = mt_samples(c, nb * (long long)c->N * c->codes_gfq->q_bits, c->codes_gfq->x_noise, nullptr)) return rc;
    c->mt.frames_taken += nb;
    return 0;
}

// what the entry points that draw refuse before anything is drawn or reserved
int gfq_exact_codes_check(ldpc_hip_ctx *c, const char *who, double snr_db, int punctured_blocks, int maxiter, double *sigma) {
    if (maxiter < 1) return fail(LDPC_HIP_EINVAL, "%s: maxiter must be >= 1 (got %d)", who, maxiter);
    if (int rc = gfq_exact_sigma(c, who, snr_db, punctured_blocks, sigma)) return rc;
    if (!c->mt.set) return fail(LDPC_HIP_EINVAL, "the generator has no state: call ldpc_hip_mt_set_state_codes_gfq first");
    const long long per_frame = (long long)c->N * c->codes_gfq->q_bits;
    if ((unsigned long long)per_frame > ldpc_mt::kRoundItems)
        return fail(LDPC_HIP_EUNSUPPORTED, "%s: a frame of %lld samples is beyond one generation round", who, per_frame);
    return 0;
}

}  // namespace

extern "C" {

int ldpc_hip_codes_gfq_set_codewords(ldpc_hip_ctx *c, const int16_t *words) {
    if (int rc = codeset_gfq_ctx(c, "ldpc_hip_codes_gfq_set_codewords")) return rc;
    ldpc_codeset_gfq_state *g = c->codes_gfq;
    const size_t n = (size_t)g->C * c->N;
    if (words)
        for (size_t i = 0; i < n; ++i)
            if (words[i] < 0 || words[i] >= g->q)
                return fail(LDPC_HIP_EINVAL, "ldpc_hip_codes_gfq_set_codewords: symbol %d at position %zu of code %zu is not an element of GF(%d)", words[i],
                            i % (size_t)c->N, i / (size_t)c->N, g->q);
    HIP_TRY(hipSetDevice(c->device));
    if ((words != nullptr) != (g->d_words != nullptr)) {   // shared <-> per-code soft values: the workspace is sized for one kind
        void *old[] = {g->w_soft, g->w_qh, g->w_iters, g->w_info};
        for (void *p : old)
            if (p) (void)hipFree(p);
        g->w_soft = nullptr; g->w_qh = nullptr; g->w_iters = nullptr; g->w_info = nullptr; g->w_frames = 0;
    }
    if (!words) {
        if (g->d_words) (void)hipFree(g->d_words);
        g->d_words = nullptr;
        return 0;
    }
    if (!g->d_words) HIP_TRY(hipMalloc(&g->d_words, sizeof(int16_t) * n));
    HIP_TRY(hipMemcpy(g->d_words, words, sizeof(int16_t) * n, hipMemcpyHostToDevice));
    return 0;
}

int ldpc_hip_mt_set_state_codes_gfq(ldpc_hip_ctx *c, const uint32_t state[624], int pos) {
    if (int rc = codeset_gfq_ctx(c, "ldpc_hip_mt_set_state_codes_gfq")) return rc;
    if (!state || pos < 0 || pos > 624) return fail(LDPC_HIP_EINVAL, "ldpc_hip_mt_set_state_codes_gfq: bad argument");
    return mt_state_store(c, state, pos);
}

int ldpc_hip_mt_get_state_codes_gfq(ldpc_hip_ctx *c, uint32_t state[624], int *pos) {
    if (int rc = codeset_gfq_ctx(c, "ldpc_hip_mt_get_state_codes_gfq")) return rc;
    if (!state || !pos) return fail(LDPC_HIP_EINVAL, "ldpc_hip_mt_get_state_codes_gfq: bad argument");
    return mt_state_load(c, "ldpc_hip_mt_set_state_codes_gfq", state, pos);
}

int ldpc_hip_mt_advance_codes_gfq(ldpc_hip_ctx *c, long long frames) {
    if (int rc = codeset_gfq_ctx(c, "ldpc_hip_mt_advance_codes_gfq")) return rc;
    if (frames < 0) return fail(LDPC_HIP_EINVAL, "ldpc_hip_mt_advance_codes_gfq: bad argument");
    return mt_drop_frames(c, "ldpc_hip_mt_set_state_codes_gfq", frames, (long long)c->N * c->codes_gfq->q_bits);
}

int ldpc_hip_mt_simulate_codes_gfq(ldpc_hip_ctx *c, double snr_db, int punctured_blocks, int maxiter, long long B, unsigned long long *counters,
                                   int32_t *frame_info, int32_t *iters) {
    const char *who = "ldpc_hip_mt_simulate_codes_gfq";
    if (int rc = codeset_gfq_ctx(c, who)) return rc;
    if (!counters || B < 0) return fail(LDPC_HIP_EINVAL, "%s: bad argument", who);
    double sigma = 0;
    if (int rc = gfq_exact_codes_check(c, who, snr_db, punctured_blocks, maxiter, &sigma)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    ldpc_codeset_gfq_state *g = c->codes_gfq;
    const long long piece = codeset_gfq_piece(c, B);
    if (int rc = gfq_exact_codes_workspace(c, piece)) return rc;
    const size_t C = (size_t)g->C;
    return codeset_simulate_loop(*g, piece, B, counters, frame_info, [&](long long first, long long nb) -> int {
        if (int rc = gfq_exact_codes_draw(c, nb)) return rc;
        if (int rc = gfq_exact_codes_piece_launch(c, sigma, maxiter, nb, frame_info != nullptr, nullptr, 0)) return rc;
        if (iters)   // [C][nb] on the device -> columns [first, first + nb) of the caller's [C][B]
            HIP_TRY(hipMemcpy2D(iters + first, sizeof(int32_t) * (size_t)B, g->w_iters, sizeof(int32_t) * (size_t)nb, sizeof(int32_t) * (size_t)nb, C,
                                hipMemcpyDeviceToHost));
        return 0;
    });
}

int ldpc_hip_frames_codes_gfq_noise_host(ldpc_hip_ctx *c, const double *noise, double snr_db, int punctured_blocks, int maxiter, long long B,
                                         unsigned long long *counters, int32_t *frame_info, int32_t *iters) {
    const char *who = "ldpc_hip_frames_codes_gfq_noise_host";
    if (int rc = codeset_gfq_ctx(c, who)) return rc;
    if (!counters || B < 0 || (B > 0 && !noise)) return fail(LDPC_HIP_EINVAL, "%s: bad argument", who);
    if (maxiter < 1) return fail(LDPC_HIP_EINVAL, "%s: maxiter must be >= 1 (got %d)", who, maxiter);
    double sigma = 0;
    if (int rc = gfq_exact_sigma(c, who, snr_db, punctured_blocks, &sigma)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    ldpc_codeset_gfq_state *g = c->codes_gfq;
    const long long piece = codeset_gfq_piece(c, B);
    if (int rc = gfq_exact_codes_workspace(c, piece)) return rc;
    const size_t C = (size_t)g->C, per_frame = (size_t)c->N * g->q_bits;
    return codeset_simulate_loop(*g, piece, B, counters, frame_info, [&](long long first, long long nb) -> int {
        HIP_TRY(hipMemcpy(g->x_noise, noise + per_frame * (size_t)first, sizeof(double) * per_frame * (size_t)nb, hipMemcpyHostToDevice));
        if (int rc = gfq_exact_codes_piece_launch(c, sigma, maxiter, nb, frame_info != nullptr, nullptr, 0)) return rc;
        if (iters)
            HIP_TRY(hipMemcpy2D(iters + first, sizeof(int32_t) * (size_t)B, g->w_iters, sizeof(int32_t) * (size_t)nb, sizeof(int32_t) * (size_t)nb, C,
                                hipMemcpyDeviceToHost));
        return 0;
    });
}

int ldpc_hip_mt_simulate_codes_gfq_stop(ldpc_hip_ctx *c, double snr_db, int punctured_blocks, int maxiter, int n_frame_errors, long long n_experiments,
                                        double reference_frame_error, long long first_batch, long long max_batch, unsigned long long *state) {
    using namespace ldpc_mt;
    const char *who = "ldpc_hip_mt_simulate_codes_gfq_stop";
    if (int rc = codeset_gfq_ctx(c, who)) return rc;
    if (int rc = codeset_stop_args(who, state, 0, first_batch, max_batch, maxiter)) return rc;
    double sigma = 0;
    if (int rc = gfq_exact_codes_check(c, who, snr_db, punctured_blocks, maxiter, &sigma)) return rc;
    std::memset(state, 0, sizeof(unsigned long long) * 6 * (size_t)c->codes_gfq->C);
    if (n_frame_errors <= 0 || n_experiments < 0) return 0;   // :591 fails before the first frame
    HIP_TRY(hipSetDevice(c->device));
    const long long piece = codeset_gfq_piece(c, max_batch < n_experiments + 1 ? max_batch : n_experiments + 1);
    if (int rc = gfq_exact_codes_workspace(c, piece)) return rc;
    // the codes stop at different frames: the generator goes back to where it was, ldpc_hip_mt_advance_codes_gfq takes it to one code's end
    DeviceState &m = c->mt;
    std::vector<uint32_t> entry(MTN);
    const long long entry_pos = m.pos, entry_frames = m.frames_taken;
    HIP_TRY(hipMemcpy(entry.data(), m.d_state, sizeof(uint32_t) * MTN, hipMemcpyDeviceToHost));
    const int rc = codeset_stop_loop(*c->codes_gfq, piece, n_frame_errors, n_experiments, reference_frame_error, first_batch, max_batch, state,
                                     [&](long long, long long nb, const int32_t *list, int n_active) -> int {   // pieces come in frame order
                                         if (int r = gfq_exact_codes_draw(c, nb)) return r;
                                         return gfq_exact_codes_piece_launch(c, sigma, maxiter, nb, true, list, n_active);
                                     }, true);
    if (hipMemcpy(m.d_state, entry.data(), sizeof(uint32_t) * MTN, hipMemcpyHostToDevice) != hipSuccess && rc == 0)
        return fail(LDPC_HIP_EHIP, "%s: the generator's state could not be put back", who);
    m.pos = entry_pos; m.frames_taken = entry_frames;
    return rc;
}

}  // extern "C"
