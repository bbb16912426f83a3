// Host side of FHT_DEC (decoder id 6, ldpc_gfq.hpp): what decod_open(FHT_DEC, q_bits, ...) + decod_init build once per context
// (decoders.cpp:1104-1161) and the ldpc_hip_*gfq* entry points.  What a GF(q) code-set context (ldpc_gfq_codeset_api.hpp) builds and
// launches the same way lives here once: the graph of one code (gfq_graph), the mul | div tables (gfq_tables), the choice of the
// kernel instance (gfq_choose, gfq_dispatch) and the sizing of the workspace slots (gfq_slots).  Included at the end of ldpc_hip.hip.
#pragma once

struct GfqKernel {                // the gfq_kernel / gfq_codes_kernel instance a context launches
    bool spec = false;            // q = 16 / q = 64 instance
    int ql = 0, lpc = 0;          // its check-node mapping
};

struct ldpc_gfq_state {
    int q_bits = 0, q = 0, ncoef = 0, cw2 = 0, max_rw = 0;
    GfqKernel kern;
    std::vector<int16_t> hc_after;   // hc as decod_init leaves it (ncols2convert applied)
    int32_t *d_i32 = nullptr;     // row_start | e_col | e_circ | e_rl | col_start | ce_edge
    int16_t *d_i16 = nullptr;     // mul | div
    size_t off_e_col = 0, off_e_circ = 0, off_e_rl = 0, off_col_start = 0, off_ce_edge = 0, off_div = 0;
    char *d_ws = nullptr;
    int ws_slots = 0;
    int num_cu = 0;
    // transmit chain (ldpc_gfq_chain_api.hpp)
    std::vector<int16_t> hb;      // the shifts as given: the encoder reads hb and hc_after, as upstream's reads st->hb and st->hc
    int enc_state = 0;            // 0 = not decided yet, 1 = encodable, -1 = refused for enc_why (decided on the first encode call)
    std::string enc_why;
    ldpc_gfq::EncArgs enc{};
    size_t enc_lds = 0;
    int16_t *d_enc = nullptr;     // shift | log of coefficient | log | alog
    double *w_soft = nullptr;     // workspace of ldpc_hip_simulate_gfq for w_frames frames
    int16_t *w_msg = nullptr, *w_cw = nullptr, *w_qh = nullptr;
    int32_t *w_ok = nullptr, *w_it = nullptr;
    unsigned long long *w_cnt = nullptr;
    long long w_frames = 0;
    // exact replay (ldpc_gfq_exact_api.hpp)
    int16_t *d_word = nullptr;    // [N] the word every frame carries (ldpc_hip_gfq_set_codeword); null = the all-zero word
    double *x_noise = nullptr;    // [x_frames][N * q_bits] Gaussians of a piece
    int32_t *x_info = nullptr;    // [x_frames] frame records of a piece
    long long x_frames = 0;
};

void ldpc_gfq_release(ldpc_gfq_state *g) {
    if (!g) return;
    if (g->d_i32) (void)hipFree(g->d_i32);
    if (g->d_i16) (void)hipFree(g->d_i16);
    if (g->d_ws) (void)hipFree(g->d_ws);
    void *chain[] = {g->d_enc, g->w_soft, g->w_msg, g->w_cw, g->w_qh, g->w_ok, g->w_it, g->w_cnt, g->d_word, g->x_noise, g->x_info};
    for (void *p : chain)
        if (p) (void)hipFree(p);
    delete g;
}

namespace {

// first primitive polynomial of each degree in upstream's bank (decoders.cpp:6594, asked for with {q_bits, 1})
constexpr int kGfqPoly[11] = {0, 3, 7, 13, 19, 37, 67, 131, 285, 529, 1033};

// logarithm / antilogarithm tables as decoders.cpp:6636 leaves them in zeroed arrays: alog[q - 1] = 0, log[0] = -1
void gfq_field(int q_bits, std::vector<int> &lg, std::vector<int> &alog) {
    const int q = 1 << q_bits;
    lg.assign(q, 0);
    alog.assign(q, 0);
    lg[0] = -1;
    int e = 1;
    for (int i = 0; i < q - 1; ++i) {
        alog[i] = e;
        lg[e] = i;
        e <<= 1;
        if (e >= q) e ^= kGfqPoly[q_bits];
    }
}

// mul | div for the listed coefficients (p2table, decoders.cpp:6673-6750): mul[c][s] = s * coefs[c], div[c][s] = s / coefs[c], both
// [coefs.size()][q]; the entries of s = 0 stay 0
std::vector<int16_t> gfq_tables(int q_bits, const std::vector<int> &coefs) {
    std::vector<int> lg, alog;
    gfq_field(q_bits, lg, alog);
    const int q = 1 << q_bits, ncoef = (int)coefs.size(), mod = q - 1;
    std::vector<int16_t> tab((size_t)2 * ncoef * q, 0);
    for (int c = 0; c < ncoef; ++c)
        for (int s = 1; s < q; ++s) {
            const int x = lg[s], y = lg[coefs[c]];
            int r = x + y;
            if (r >= mod) r -= mod;
            tab[(size_t)c * q + s] = (int16_t)alog[r];
            r = x - y;
            if (r < 0) r += mod;
            tab[(size_t)(ncoef + c) * q + s] = (int16_t)alog[r];
        }
    return tab;
}

// One code's graph as decod_init maps it: rows hold their edges in ascending column order (find_list_of_symbols, decoders.cpp:867-901),
// columns theirs in ascending row order, cw2 = "every block column has weight 2" (find_column_weight, :837-865).
struct GfqGraph {
    std::vector<int32_t> row_start, col_start, e_col, e_circ, e_coef, ce_edge;   // e_coef: the coefficient of the edge, 1 .. q - 1
    int cw2 = 0, max_rw = 0, E = 0;
};

// Builds g from the (hb, hc) of one code, with upstream's limits; every refusal starts with `pre`.  in_a_set: the rules a code set
// reads differently -- it refuses a shift below -1 (a single code takes it as an empty circulant), and it does not read the coefficient
// under an empty circulant (a single code refuses one >= q there, and names a negative one on a circulant "no coefficient").
int gfq_graph(const char *pre, bool in_a_set, int rh, int nh, int M, int q, const int16_t *hb, const int16_t *hc, GfqGraph &g) {
    g.row_start.assign((size_t)rh + 1, 0); g.col_start.assign((size_t)nh + 1, 0);
    g.e_col.clear(); g.e_circ.clear(); g.e_coef.clear(); g.ce_edge.clear();
    g.max_rw = 0;
    for (int j = 0; j < rh; ++j) {
        for (int k = 0; k < nh; ++k) {
            const int s = hb[(size_t)j * nh + k], v = hc[(size_t)j * nh + k];
            if (!in_a_set && v >= q) return fail(LDPC_HIP_EINVAL, "%scoefficient %d at (%d, %d) is not an element of GF(%d)", pre, v, j, k, q);
            if (in_a_set && s < -1) return fail(LDPC_HIP_EINVAL, "%sshift %d at (%d, %d) is below -1", pre, s, j, k);
            if (s < 0) continue;
            if (!in_a_set && v < 0) return fail(LDPC_HIP_EINVAL, "%scirculant (%d, %d) has no coefficient", pre, j, k);
            if (v < 0 || v >= q) return fail(LDPC_HIP_EINVAL, "%scoefficient %d at (%d, %d) is not an element of GF(%d)", pre, v, j, k, q);
            if (v == 0)   // upstream files it under index q and then reads its logarithm table one entry past the end (decoders.cpp:884, :6692)
                return fail(LDPC_HIP_EUNSUPPORTED, "%scoefficient 0 at (%d, %d): upstream's tables are undefined for it", pre, j, k);
            g.e_col.push_back(k); g.e_circ.push_back(s % M); g.e_coef.push_back(v);
        }
        g.row_start[(size_t)j + 1] = (int32_t)g.e_col.size();
        const int rw = g.row_start[(size_t)j + 1] - g.row_start[(size_t)j];
        if (rw < 2)   // map_graph reads Sigma_backH[1] / Sigma_forwardH[rw-2] it never set (decoders.cpp:6355-6360)
            return fail(LDPC_HIP_EUNSUPPORTED, "%sblock row %d has weight %d; upstream's check node needs at least 2", pre, j, rw);
        if (rw > 1024)
            return fail(LDPC_HIP_EUNSUPPORTED, "%sblock row %d has weight %d; at most 1024 is supported (upstream's RWMAX, decoders.cpp:73)", pre, j, rw);
        if (rw > g.max_rw) g.max_rw = rw;
    }
    g.E = (int)g.e_col.size();
    if ((long long)g.E * M >= (1LL << 28)) return fail(LDPC_HIP_EUNSUPPORTED, "%s%lld edges, at most 2^28 - 1 are supported", pre, (long long)g.E * M);
    g.cw2 = 1;
    for (int k = 0; k < nh; ++k) {
        for (int e = 0; e < g.E; ++e)
            if (g.e_col[(size_t)e] == k) g.ce_edge.push_back(e);
        g.col_start[(size_t)k + 1] = (int32_t)g.ce_edge.size();
        if (g.col_start[(size_t)k + 1] - g.col_start[(size_t)k] != 2) g.cw2 = 0;
    }
    return 0;
}

// q = 16 and q = 64 have their own instances (LDPC_HIP_GFQ_GENERIC=1: the generic ones for them too)
GfqKernel gfq_choose(int q) {
    const char *genv = getenv("LDPC_HIP_GFQ_GENERIC");
    const bool force_generic = genv && atoi(genv) != 0;
    GfqKernel k;
    if (!force_generic && q == 16) { k.spec = true; k.ql = 16; k.lpc = 1; }
    else if (!force_generic && q == 64) { k.spec = true; k.ql = 16; k.lpc = 4; }
    else { k.ql = q <= 256 ? 4 : q / 64; k.lpc = q / k.ql; }
    return k;
}

std::string gfq_kernel_name(const char *kernel, int q, const GfqKernel &k) {
    char name[64];
    snprintf(name, sizeof name, "%s<%sq=%d,%dx%d>", kernel, k.spec ? "" : "generic,", q, k.ql, k.lpc);
    return name;
}

// launch(QL, LPC) with the template arguments of the chosen instance as std::integral_constants
template <class Launch>
void gfq_dispatch(const GfqKernel &k, Launch launch) {
    using std::integral_constant;
    if (k.spec && k.lpc == 1) launch(integral_constant<int, 16>(), integral_constant<int, 1>());
    else if (k.spec) launch(integral_constant<int, 16>(), integral_constant<int, 4>());
    else if (k.ql == 4) launch(integral_constant<int, 4>(), integral_constant<int, 0>());
    else if (k.ql == 8) launch(integral_constant<int, 8>(), integral_constant<int, 0>());
    else launch(integral_constant<int, 16>(), integral_constant<int, 0>());
}

// One workgroup per slot of the workspace; the work items beyond the slots are worked off inside the launch, slot by slot.  Gives the
// workgroup size and the slots of a launch over `items` work items, and grows d_ws [ws_slots][stride] to hold them.
int gfq_slots(int num_cu, int R, int N, int lpc, size_t stride, long long items, char *&d_ws, int &ws_slots, int &threads, int &slots_out) {
    const long long lanes = std::max((long long)R * lpc, (long long)N);
    threads = (int)std::min(256LL, std::max(64LL, (lanes + 63) / 64 * 64));
    long long slots = (long long)num_cu * 1024 / threads;
    if (const char *e = getenv("LDPC_HIP_GFQ_SLOTS")) { if (atoll(e) > 0) slots = atoll(e); }
    while (slots > 1 && (size_t)slots * stride > ((size_t)4 << 30)) slots /= 2;
    if (slots > items) slots = items;
    if (slots > ws_slots) {
        if (d_ws) (void)hipFree(d_ws);
        d_ws = nullptr; ws_slots = 0;
        HIP_TRY(hipMalloc(&d_ws, (size_t)slots * stride));
        ws_slots = (int)slots;
    }
    slots_out = (int)slots;
    return 0;
}

}  // namespace

extern "C" {

int ldpc_hip_open_gfq(int q_bits, int rh, int nh, int M, const int16_t *hb, const int16_t *hc, int ncols2convert, int device,
                      ldpc_hip_ctx **out) {
    if (out) *out = nullptr;
    if (!out || !hb || !hc || rh <= 0 || nh <= 0 || M <= 0 || ncols2convert < 0 || ncols2convert > nh)
        return fail(LDPC_HIP_EINVAL, "ldpc_hip_open_gfq: bad argument");
    if (q_bits < 2) return fail(LDPC_HIP_EUNSUPPORTED, "FHT_DEC: q_bits = %d, GF(q) needs q_bits >= 2 (binary codes: ldpc_hip_open)", q_bits);
    if (q_bits > 10) return fail(LDPC_HIP_EUNSUPPORTED, "FHT_DEC: q = 2^%d, at most q = 1024 is supported (upstream's QMAX, decoders.cpp:74)", q_bits);
    if (M >= 65536 || nh >= 65536 || rh >= 65536) return fail(LDPC_HIP_EUNSUPPORTED, "M, rh and nh must be < 65536");
    if ((long long)nh * M >= (1LL << 28)) return fail(LDPC_HIP_EUNSUPPORTED, "code length nh * M = %lld: at most 2^28 - 1 is supported", (long long)nh * M);
    const int q = 1 << q_bits;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(LDPC_HIP_EINVAL, "ldpc_hip_open_gfq: device %d of %d", device, ndev);

    GfqGraph gr;
    if (int rc = gfq_graph("FHT_DEC: ", false, rh, nh, M, q, hb, hc, gr)) return rc;
    // the tables hold the coefficients in use, ascending (find_list_of_symbols, decoders.cpp:867-901)
    std::vector<char> used(q, 0);
    for (int v : gr.e_coef) used[v] = 1;
    std::vector<int> coef_index(q, -1), coefs;
    for (int v = 1; v < q; ++v)
        if (used[v]) { coef_index[v] = (int)coefs.size(); coefs.push_back(v); }
    std::vector<int32_t> e_rl(gr.E);
    for (int e = 0; e < gr.E; ++e) e_rl[e] = coef_index[gr.e_coef[e]];
    const int ncoef = (int)coefs.size();
    const std::vector<int16_t> tab = gfq_tables(q_bits, coefs);

    std::unique_ptr<ldpc_hip_ctx, void (*)(ldpc_hip_ctx *)> c(new ldpc_hip_ctx(), ldpc_hip_close);
    c->decoder_id = LDPC_HIP_FHT_DEC; c->device = device;
    c->rh = rh; c->nh = nh; c->M = M; c->N = nh * M; c->R = rh * M; c->ne = gr.E;
    c->hard_words = (c->N + 31) / 32;
    ldpc_gfq_state *g = c->gfq = new ldpc_gfq_state();
    g->q_bits = q_bits; g->q = q; g->ncoef = ncoef; g->cw2 = gr.cw2; g->max_rw = gr.max_rw;
    // the matrix decod_init leaves in hc: the first ncols2convert columns go from power to natural representation AFTER the
    // tables were made from the values as given (:1151-1159)
    g->hc_after.assign(hc, hc + (size_t)rh * nh);
    g->hb.assign(hb, hb + (size_t)rh * nh);
    std::vector<int> lg, alog;
    gfq_field(q_bits, lg, alog);
    for (int j = 0; j < rh; ++j)
        for (int k = 0; k < ncols2convert; ++k)
            if (g->hc_after[(size_t)j * nh + k] > -1) g->hc_after[(size_t)j * nh + k] = (int16_t)alog[g->hc_after[(size_t)j * nh + k]];

    g->kern = gfq_choose(q);
    c->kernel_name = gfq_kernel_name("gfq_kernel", q, g->kern);
    c->last_launch = "";

    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    g->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;
    std::vector<int32_t> i32;
    auto put = [&](const std::vector<int32_t> &v) { const size_t at = i32.size(); i32.insert(i32.end(), v.begin(), v.end()); return at; };
    put(gr.row_start);
    g->off_e_col = put(gr.e_col); g->off_e_circ = put(gr.e_circ); g->off_e_rl = put(e_rl);
    g->off_col_start = put(gr.col_start); g->off_ce_edge = put(gr.ce_edge);
    g->off_div = (size_t)ncoef * q;
    HIP_TRY(hipMalloc(&g->d_i32, sizeof(int32_t) * i32.size()));
    HIP_TRY(hipMemcpy(g->d_i32, i32.data(), sizeof(int32_t) * i32.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&g->d_i16, sizeof(int16_t) * (tab.size() + 1)));
    if (!tab.empty()) HIP_TRY(hipMemcpy(g->d_i16, tab.data(), sizeof(int16_t) * tab.size(), hipMemcpyHostToDevice));
    *out = c.release();
    return 0;
}

int ldpc_hip_gfq_coefficients(const ldpc_hip_ctx *c, int16_t *hc_out) {
    if (!c || !c->gfq || !hc_out) return fail(LDPC_HIP_EINVAL, "ldpc_hip_gfq_coefficients: not a GF(q) context, or null output");
    std::memcpy(hc_out, c->gfq->hc_after.data(), sizeof(int16_t) * c->gfq->hc_after.size());
    return 0;
}

int ldpc_hip_decode_gfq_dev(ldpc_hip_ctx *c, const double *d_soft, long long B, int maxiter, double p_thr, int16_t *d_qhard,
                            int32_t *d_iters, double *d_post, void *stream_) {
    if (!c || !c->gfq || B < 0) return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_gfq_dev: not a GF(q) context (ldpc_hip_open_gfq), or bad argument");
    if (p_thr != 0) return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_gfq_dev: p_thr = %g; only 0 is supported (the only value upstream's harness passes)", p_thr);
    if (maxiter < 1) return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_gfq_dev: maxiter must be >= 1 (got %d)", maxiter);
    if (B == 0) return 0;
    if (!d_soft) return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_gfq_dev: null input");
    if (B > 0x7fffffffLL) return fail(LDPC_HIP_EINVAL, "batch too large");
    ldpc_gfq_state *g = c->gfq;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = (hipStream_t)stream_;

    const size_t stride = ldpc_gfq::slot_bytes(c->ne, c->M, c->N, g->q);
    int threads = 0, slots = 0;   // one slot per frame in flight
    if (int rc = gfq_slots(g->num_cu, c->R, c->N, g->kern.lpc, stride, B, g->d_ws, g->ws_slots, threads, slots)) return rc;
    ldpc_gfq::Args a{};
    a.soft = d_soft; a.qhard = d_qhard; a.iters = d_iters; a.post = d_post;
    a.ws = g->d_ws; a.ws_stride = stride; a.B = B; a.maxiter = maxiter;
    a.rh = c->rh; a.nh = c->nh; a.M = c->M; a.N = c->N; a.R = c->R; a.E = c->ne; a.q = g->q; a.lpc = g->kern.lpc; a.cw2 = g->cw2;
    a.row_start = g->d_i32; a.e_col = g->d_i32 + g->off_e_col; a.e_circ = g->d_i32 + g->off_e_circ; a.e_rl = g->d_i32 + g->off_e_rl;
    a.col_start = g->d_i32 + g->off_col_start; a.ce_edge = g->d_i32 + g->off_ce_edge;
    a.mul = g->d_i16; a.div = g->d_i16 + g->off_div;

    ProfTimer timer;
    if (int rc = timer.begin(c, stream)) return rc;
    c->last_launch = c->kernel_name.c_str();
    gfq_dispatch(g->kern, [&](auto ql, auto lpc) {
        hipLaunchKernelGGL((ldpc_gfq::gfq_kernel<decltype(ql)::value, decltype(lpc)::value>), dim3((unsigned)slots), dim3((unsigned)threads), 0, stream, a);
    });
    HIP_TRY(hipGetLastError());
    return timer.end();
}

int ldpc_hip_decode_gfq_host(ldpc_hip_ctx *c, const double *soft, long long B, int maxiter, double p_thr, int16_t *qhard, int32_t *iters,
                             double *post) {
    if (!c || !c->gfq || B < 0) return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_gfq_host: not a GF(q) context (ldpc_hip_open_gfq), or bad argument");
    if (B == 0) return 0;
    if (!soft) return fail(LDPC_HIP_EINVAL, "ldpc_hip_decode_gfq_host: null input");
    HIP_TRY(hipSetDevice(c->device));
    const size_t per = (size_t)c->gfq->q * c->N;   // doubles per frame
    long long chunk = (long long)(((size_t)1 << 30) / (sizeof(double) * per));   // staging: at most 1 GiB in, 1 GiB out
    if (chunk < 1) chunk = 1;
    if (chunk > B) chunk = B;
    double *d_in = nullptr, *d_post = nullptr;
    int16_t *d_qh = nullptr;
    int32_t *d_it = nullptr;
    int rc = 0;
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc(&d_in, sizeof(double) * per * chunk));
        if (post) HIP_TRY(hipMalloc(&d_post, sizeof(double) * per * chunk));
        HIP_TRY(hipMalloc(&d_qh, sizeof(int16_t) * (size_t)c->N * chunk));
        HIP_TRY(hipMalloc(&d_it, sizeof(int32_t) * (size_t)chunk));
        for (long long b0 = 0; b0 < B; b0 += chunk) {
            const long long nb = std::min(chunk, B - b0);
            HIP_TRY(hipMemcpy(d_in, soft + per * b0, sizeof(double) * per * nb, hipMemcpyHostToDevice));
            if (int r = ldpc_hip_decode_gfq_dev(c, d_in, nb, maxiter, p_thr, d_qh, d_it, d_post, nullptr)) return r;
            HIP_TRY(hipDeviceSynchronize());
            if (qhard) HIP_TRY(hipMemcpy(qhard + (size_t)c->N * b0, d_qh, sizeof(int16_t) * (size_t)c->N * nb, hipMemcpyDeviceToHost));
            if (iters) HIP_TRY(hipMemcpy(iters + b0, d_it, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost));
            if (post) HIP_TRY(hipMemcpy(post + per * b0, d_post, sizeof(double) * per * nb, hipMemcpyDeviceToHost));
        }
        return 0;
    };
    rc = body();
    if (d_in) (void)hipFree(d_in);
    if (d_post) (void)hipFree(d_post);
    if (d_qh) (void)hipFree(d_qh);
    if (d_it) (void)hipFree(d_it);
    return rc;
}

}  // extern "C"
