// Host side of the GF(q) code-set kernels (ldpc_gfq_codeset.hpp): the concatenated record table, the field tables of the set, the
// ldpc_hip_*codes_gfq* entry points and the shared-noise Monte-Carlo pass.  Included at the end of ldpc_hip.hip, after
// ldpc_gfq_chain_api.hpp (the channel launch) and ldpc_codeset_api.hpp (the host loop of the stopping rule).
#pragma once

struct ldpc_codeset_gfq_state {
    int C = 0, q_bits = 0, q = 0;
    int ql = 0, lpc = 0;               // check-node mapping of the kernel this context launches, as in ldpc_gfq_state
    bool spec = false;                 // q = 16 / q = 64 instance
    int ne_max = 0;                    // the largest edge count of a code of the set
    int num_cu = 0;
    std::vector<int32_t> off, tab;     // host copies of the device tables
    int32_t *d_off = nullptr, *d_tab = nullptr;
    int16_t *d_i16 = nullptr;          // mul | div, q - 1 rows each
    char *d_ws = nullptr;              // message state, one slot per workgroup
    int ws_slots = 0;
    // workspace of ldpc_hip_simulate_codes_gfq for w_frames frames per code
    double *w_soft = nullptr;          // [w_frames][q][N], shared by the codes
    int16_t *w_qh = nullptr;           // [C][w_frames][N]
    int32_t *w_it = nullptr, *w_info = nullptr;   // [C][w_frames]
    unsigned long long *w_cnt = nullptr;          // [C][5]
    long long w_frames = 0;
    codeset_rule_ws stop;              // ldpc_hip_simulate_codes_gfq_stop
};

void ldpc_codeset_gfq_release(ldpc_codeset_gfq_state *s) {
    if (!s) return;
    void *dev[] = {s->d_off, s->d_tab, s->d_i16, s->d_ws, s->w_soft, s->w_qh, s->w_it, s->w_info, s->w_cnt, s->stop.rule, s->stop.running, s->stop.list, s->stop.nactive};
    for (void *p : dev)
        if (p) (void)hipFree(p);
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
    std::vector<int32_t> row_start((size_t)rh + 1), col_start((size_t)nh + 1), e_col, e_circ, e_rl, ce_edge;
    int ne_max = 0;
    for (int c = 0; c < C; ++c) {
        const int16_t *b = hb + (size_t)c * rh * nh, *v = hc + (size_t)c * rh * nh;
        e_col.clear(); e_circ.clear(); e_rl.clear(); ce_edge.clear();
        row_start[0] = 0;
        for (int j = 0; j < rh; ++j) {   // rows: edges in ascending column order
            for (int k = 0; k < nh; ++k) {
                const int s = b[(size_t)j * nh + k], x = v[(size_t)j * nh + k];
                if (s < -1) return fail(LDPC_HIP_EINVAL, "%s: code %d, shift %d at (%d, %d) is below -1", who, c, s, j, k);
                if (s < 0) continue;     // the coefficient of an empty circulant is not read
                if (x < 0 || x >= q) return fail(LDPC_HIP_EINVAL, "%s: code %d, coefficient %d at (%d, %d) is not an element of GF(%d)", who, c, x, j, k, q);
                if (x == 0)              // upstream's tables are undefined for it (decoders.cpp:884, :6692)
                    return fail(LDPC_HIP_EUNSUPPORTED, "%s: code %d, coefficient 0 at (%d, %d): upstream's tables are undefined for it", who, c, j, k);
                e_col.push_back(k); e_circ.push_back(s % M); e_rl.push_back(x - 1);
            }
            row_start[(size_t)j + 1] = (int32_t)e_col.size();
            const int rw = row_start[(size_t)j + 1] - row_start[(size_t)j];
            if (rw < 2)                  // map_graph reads products it never set (decoders.cpp:6355-6360)
                return fail(LDPC_HIP_EUNSUPPORTED, "%s: code %d, block row %d has weight %d; upstream's check node needs at least 2", who, c, j, rw);
            if (rw > 1024)
                return fail(LDPC_HIP_EUNSUPPORTED, "%s: code %d, block row %d has weight %d; at most 1024 is supported (upstream's RWMAX, decoders.cpp:73)", who, c, j, rw);
        }
        const int E = (int)e_col.size();
        if ((long long)E * M >= (1LL << 28)) return fail(LDPC_HIP_EUNSUPPORTED, "%s: code %d has %lld edges, at most 2^28 - 1 are supported", who, c, (long long)E * M);
        int cw2 = 1;                     // columns: edges in ascending row order (find_column_weight, decoders.cpp:837-865)
        col_start[0] = 0;
        for (int k = 0; k < nh; ++k) {
            for (int e = 0; e < E; ++e)
                if (e_col[(size_t)e] == k) ce_edge.push_back(e);
            col_start[(size_t)k + 1] = (int32_t)ce_edge.size();
            if (col_start[(size_t)k + 1] - col_start[(size_t)k] != 2) cw2 = 0;
        }
        if (tab.size() + ldpc_gfq::record_length(rh, nh, E) >= ((size_t)1 << 31))
            return fail(LDPC_HIP_EINVAL, "%s: the table of %d codes exceeds 2^31 entries", who, C);
        off.push_back((int32_t)tab.size());
        tab.push_back(E); tab.push_back(cw2);
        for (const std::vector<int32_t> *part : {&row_start, &col_start, &e_col, &e_circ, &e_rl, &ce_edge}) tab.insert(tab.end(), part->begin(), part->end());
        ne_max = E > ne_max ? E : ne_max;
    }
    if (ne_max_out) *ne_max_out = ne_max;
    return 0;
}

int codeset_gfq_ctx(const ldpc_hip_ctx *c, const char *who) {
    if (!c || !c->codes_gfq) return fail(LDPC_HIP_EINVAL, "%s: not a GF(q) code-set context (ldpc_hip_open_codes_gfq)", who);
    return 0;
}

template <int QL, int LPC>
void codeset_gfq_launch(const ldpc_gfq::CodesArgs &a, int grid, int threads, hipStream_t stream) {
    hipLaunchKernelGGL((ldpc_gfq::gfq_codes_kernel<QL, LPC>), dim3((unsigned)grid), dim3((unsigned)threads), 0, stream, a);
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

    // one workgroup per slot of the workspace, as ldpc_hip_decode_gfq_dev; the items beyond the slots are worked off inside the launch
    const long long lanes = std::max((long long)c->R * g->lpc, (long long)c->N);
    const int threads = (int)std::min(256LL, std::max(64LL, (lanes + 63) / 64 * 64));
    const size_t stride = ldpc_gfq::slot_bytes(g->ne_max, c->M, c->N, g->q);
    long long slots = (long long)g->num_cu * 1024 / threads;
    if (const char *e = getenv("LDPC_HIP_GFQ_SLOTS")) { if (atoll(e) > 0) slots = atoll(e); }
    while (slots > 1 && (size_t)slots * stride > ((size_t)4 << 30)) slots /= 2;
    if (slots > items) slots = items;
    if (slots > g->ws_slots) {
        if (g->d_ws) (void)hipFree(g->d_ws);
        g->d_ws = nullptr; g->ws_slots = 0;
        HIP_TRY(hipMalloc(&g->d_ws, (size_t)slots * stride));
        g->ws_slots = (int)slots;
    }
    ldpc_gfq::CodesArgs a{};
    a.soft = d_soft; a.qhard = d_qhard; a.iters = d_iters; a.post = d_post;
    a.ws = g->d_ws; a.ws_stride = stride;
    a.tab = g->d_tab; a.code_off = g->d_off; a.code_list = code_list;
    a.soft_code_stride = shared_soft ? 0 : B * (long long)g->q * c->N;
    a.B = (unsigned)B; a.items = (unsigned)items; a.maxiter = maxiter;
    a.rh = c->rh; a.nh = c->nh; a.M = c->M; a.N = c->N; a.R = c->R; a.q = g->q; a.lpc = g->lpc;
    a.mul = g->d_i16; a.div = g->d_i16 + (size_t)(g->q - 1) * g->q;

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (c->prof) {
        HIP_TRY(hipEventCreate(&ev0));
        HIP_TRY(hipEventCreate(&ev1));
        HIP_TRY(hipEventRecord(ev0, stream));
    }
    c->last_launch = c->kernel_name.c_str();
    if (g->spec && g->lpc == 1) codeset_gfq_launch<16, 1>(a, (int)slots, threads, stream);
    else if (g->spec) codeset_gfq_launch<16, 4>(a, (int)slots, threads, stream);
    else if (g->ql == 4) codeset_gfq_launch<4, 0>(a, (int)slots, threads, stream);
    else if (g->ql == 8) codeset_gfq_launch<8, 0>(a, (int)slots, threads, stream);
    else codeset_gfq_launch<16, 0>(a, (int)slots, threads, stream);
    HIP_TRY(hipGetLastError());
    if (c->prof) {
        HIP_TRY(hipEventRecord(ev1, stream));
        c->events.emplace_back(ev0, ev1);
    }
    return 0;
}

int codeset_gfq_count_launch(const ldpc_hip_ctx *c, const int16_t *d_qhard, const int32_t *d_iters, long long B, int32_t *d_frame_info,
                             unsigned long long *d_counters, hipStream_t stream, const int32_t *code_list = nullptr, int n_slots = 0) {
    const int C = code_list ? n_slots : c->codes_gfq->C;
    long long bpc = (B + 3) / 4;            // workgroups per code: four frames (waves) each, fewer when there are many codes
    const long long cap = 2048 / C > 1 ? 2048 / C : 1;
    if (bpc > cap) bpc = cap;
    ldpc_gfq::CodesCountArgs a{d_qhard, d_iters, d_frame_info, d_counters, code_list, B, (int)bpc, c->N, c->R};
    hipLaunchKernelGGL(ldpc_gfq::gfq_count_codes_kernel, dim3((unsigned)(bpc * C)), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Frames per piece of the simulate entry points: the shared [piece][q][N] input and the [C][piece] outputs within 1 GiB together, at
// most 65536, LDPC_HIP_GFQ_PIECE=n caps it (read per call, as in ldpc_hip_simulate_gfq).
long long codeset_gfq_piece(const ldpc_hip_ctx *c, long long B) {
    const ldpc_codeset_gfq_state *g = c->codes_gfq;
    const size_t per_frame = sizeof(double) * (size_t)g->q * c->N + (size_t)g->C * (sizeof(int16_t) * (size_t)c->N + 2 * sizeof(int32_t));
    long long piece = (long long)(((size_t)1 << 30) / per_frame);
    piece = piece > (1 << 16) ? (1 << 16) : (piece < 1 ? 1 : piece);
    if (const char *e = getenv("LDPC_HIP_GFQ_PIECE")) { if (atoll(e) > 0 && atoll(e) < piece) piece = atoll(e); }
    return piece > B ? B : piece;
}

// The context's workspace for `piece` frames per code (grown, never shrunk).
int codeset_gfq_reserve(ldpc_hip_ctx *c, long long piece) {
    ldpc_codeset_gfq_state *g = c->codes_gfq;
    const size_t C = (size_t)g->C;
    if (piece > g->w_frames) {
        void *old[] = {g->w_soft, g->w_qh, g->w_it, g->w_info};
        for (void *p : old)
            if (p) (void)hipFree(p);
        g->w_soft = nullptr; g->w_qh = nullptr; g->w_it = nullptr; g->w_info = nullptr; g->w_frames = 0;
        HIP_TRY(hipMalloc(&g->w_soft, sizeof(double) * (size_t)piece * g->q * c->N));
        HIP_TRY(hipMalloc(&g->w_qh, sizeof(int16_t) * C * (size_t)piece * c->N));
        HIP_TRY(hipMalloc(&g->w_it, sizeof(int32_t) * C * (size_t)piece));
        HIP_TRY(hipMalloc(&g->w_info, sizeof(int32_t) * C * (size_t)piece));
        g->w_frames = piece;
    }
    return 0;
}

// channel (the all-zero word, Philox stream tag 3) -> set decode on the shared soft values -> set count, for frames
// [first_frame, first_frame + nb) and the n_active codes of `list` (null: all)
int codeset_gfq_piece_launch(ldpc_hip_ctx *c, double sigma, int maxiter, uint64_t seed, long long first_frame, long long nb, bool want_info,
                             const int32_t *list, int n_active) {
    ldpc_codeset_gfq_state *g = c->codes_gfq;
    if (int rc = gfq_channel_launch(g->num_cu, c->N, g->q_bits, nullptr, nullptr, nullptr, sigma, seed, first_frame, nb, g->w_soft, nullptr)) return rc;
    if (int rc = codeset_gfq_decode_launch(c, g->w_soft, 1, nb, maxiter, g->w_qh, g->w_it, nullptr, nullptr, list, n_active)) return rc;
    return codeset_gfq_count_launch(c, g->w_qh, g->w_it, nb, want_info ? g->w_info : nullptr, g->w_cnt, nullptr, list, n_active);
}

}  // namespace

extern "C" {

int ldpc_hip_codes_gfq_table_host(int q_bits, int rh, int nh, int M, const int16_t *hb, const int16_t *hc, int C, int32_t *offsets, int32_t *table,
                                  long long capacity, long long *length) {
    std::vector<int32_t> off, tab;
    if (int rc = codeset_gfq_build("ldpc_hip_codes_gfq_table_host", q_bits, rh, nh, M, hb, hc, C, off, tab)) return rc;
    if (length) *length = (long long)tab.size();
    if (offsets) std::memcpy(offsets, off.data(), sizeof(int32_t) * off.size());
    if (table) {
        if (capacity < (long long)tab.size())
            return fail(LDPC_HIP_EINVAL, "ldpc_hip_codes_gfq_table_host: the table has %lld entries, room for %lld", (long long)tab.size(), capacity);
        std::memcpy(table, tab.data(), sizeof(int32_t) * tab.size());
    }
    return 0;
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

    // the field's tables for all q - 1 coefficients (p2table, decoders.cpp:6673-6750): mul[c - 1][s] = s * c, div[c - 1][s] = s / c
    std::vector<int> lg, alog;
    gfq_field(q_bits, lg, alog);
    const int ncoef = q - 1, mod = q - 1;
    std::vector<int16_t> ftab((size_t)2 * ncoef * q, 0);
    for (int v = 1; v < q; ++v)
        for (int s = 1; s < q; ++s) {
            const int x = lg[s], y = lg[v];
            int r = x + y;
            if (r >= mod) r -= mod;
            ftab[(size_t)(v - 1) * q + s] = (int16_t)alog[r];
            r = x - y;
            if (r < 0) r += mod;
            ftab[(size_t)(ncoef + v - 1) * q + s] = (int16_t)alog[r];
        }

    std::unique_ptr<ldpc_hip_ctx, void (*)(ldpc_hip_ctx *)> c(new ldpc_hip_ctx(), ldpc_hip_close);
    ldpc_codeset_gfq_state *g = c->codes_gfq = new ldpc_codeset_gfq_state();
    g->off.swap(off); g->tab.swap(tab);
    g->C = C; g->q_bits = q_bits; g->q = q; g->ne_max = ne_max;
    c->decoder_id = LDPC_HIP_FHT_DEC; c->device = device;
    c->rh = rh; c->nh = nh; c->M = M; c->N = nh * M; c->R = rh * M; c->ne = ne_max;
    c->hard_words = (c->N + 31) / 32;
    const char *genv = getenv("LDPC_HIP_GFQ_GENERIC");   // the choice of ldpc_hip_open_gfq
    const bool force_generic = genv && atoi(genv) != 0;
    if (!force_generic && q == 16) { g->spec = true; g->ql = 16; g->lpc = 1; }
    else if (!force_generic && q == 64) { g->spec = true; g->ql = 16; g->lpc = 4; }
    else { g->ql = q <= 256 ? 4 : q / 64; g->lpc = q / g->ql; }
    char name[64];
    snprintf(name, sizeof name, "gfq_codes_kernel<%sq=%d,%dx%d>", g->spec ? "" : "generic,", q, g->ql, g->lpc);
    c->kernel_name = name;
    c->last_launch = "";

    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    g->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;
    HIP_TRY(hipMalloc(&g->d_off, sizeof(int32_t) * g->off.size()));
    HIP_TRY(hipMemcpy(g->d_off, g->off.data(), sizeof(int32_t) * g->off.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&g->d_tab, sizeof(int32_t) * g->tab.size()));
    HIP_TRY(hipMemcpy(g->d_tab, g->tab.data(), sizeof(int32_t) * g->tab.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&g->d_i16, sizeof(int16_t) * ftab.size()));
    HIP_TRY(hipMemcpy(g->d_i16, ftab.data(), sizeof(int16_t) * ftab.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&g->w_cnt, sizeof(unsigned long long) * 5 * (size_t)C));
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
    ldpc_codeset_gfq_state *g = c->codes_gfq;
    const size_t C = (size_t)g->C;
    const double sigma = ldpc_hip_gfq_sigma(c, snr_db);   // rh and nh only: common to the set
    HIP_TRY(hipSetDevice(c->device));
    const long long piece = codeset_gfq_piece(c, B);
    if (int rc = codeset_gfq_reserve(c, piece)) return rc;
    HIP_TRY(hipMemsetAsync(g->w_cnt, 0, sizeof(unsigned long long) * 5 * C, nullptr));
    for (long long done = 0; done < B; done += piece) {
        const long long nb = (B - done) < piece ? (B - done) : piece;
        if (int rc = codeset_gfq_piece_launch(c, sigma, maxiter, seed, first_frame + done, nb, frame_info != nullptr, nullptr, 0)) return rc;
        if (frame_info)   // [C][nb] on the device -> columns [done, done + nb) of the caller's [C][B]
            HIP_TRY(hipMemcpy2D(frame_info + done, sizeof(int32_t) * (size_t)B, g->w_info, sizeof(int32_t) * (size_t)nb, sizeof(int32_t) * (size_t)nb, C,
                                hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipMemcpy(counters, g->w_cnt, sizeof(unsigned long long) * 5 * C, hipMemcpyDeviceToHost));
    return 0;
}

int ldpc_hip_simulate_codes_gfq_stop(ldpc_hip_ctx *c, double snr_db, int maxiter, uint64_t seed, long long first_frame, int n_frame_errors,
                                     long long n_experiments, double reference_frame_error, long long first_batch, long long max_batch,
                                     unsigned long long *state) {
    if (int rc = codeset_gfq_ctx(c, "ldpc_hip_simulate_codes_gfq_stop")) return rc;
    if (!state || first_frame < 0) return fail(LDPC_HIP_EINVAL, "ldpc_hip_simulate_codes_gfq_stop: bad argument");
    if (first_batch < 1 || max_batch < first_batch)
        return fail(LDPC_HIP_EINVAL, "ldpc_hip_simulate_codes_gfq_stop: batches of %lld .. %lld frames; 1 <= first_batch <= max_batch", first_batch, max_batch);
    if (maxiter < 1) return fail(LDPC_HIP_EINVAL, "ldpc_hip_simulate_codes_gfq_stop: maxiter must be >= 1 (got %d)", maxiter);
    ldpc_codeset_gfq_state *g = c->codes_gfq;
    const size_t C = (size_t)g->C;
    const double sigma = ldpc_hip_gfq_sigma(c, snr_db);
    std::memset(state, 0, sizeof(unsigned long long) * 4 * C);
    if (n_frame_errors <= 0 || n_experiments < 0) return 0;   // bp_simulation.cpp:591 fails before the first frame
    HIP_TRY(hipSetDevice(c->device));
    const long long piece = codeset_gfq_piece(c, max_batch < n_experiments + 1 ? max_batch : n_experiments + 1);
    if (int rc = codeset_gfq_reserve(c, piece)) return rc;
    return codeset_stop_loop(C, piece, n_frame_errors, n_experiments, reference_frame_error, first_batch, max_batch, g->stop, g->w_info, g->w_cnt, state,
                             [&](long long first, long long nb, const int32_t *list, int n_active) -> int {
                                 return codeset_gfq_piece_launch(c, sigma, maxiter, seed, first_frame + first, nb, true, list, n_active);
                             });
}

}  // extern "C"
