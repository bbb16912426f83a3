// Host side of the GF(q) transmit chain (ldpc_gfq_chain.hpp): left2right, the encoder's plan (what encode_NBQCLDPC decides before it
// touches a symbol, decoders.cpp:1415-1496), and the ldpc_hip_*gfq* entry points for encode, channel, count and simulate.
// Included from ldpc_hip.hip after ldpc_gfq_api.hpp.
#pragma once

namespace {

// Decided on the first encode call and cached in the state; a refusal leaves the decoder of the context untouched.
int gfq_encoder_plan(ldpc_hip_ctx *c) {
    ldpc_gfq_state *g = c->gfq;
    if (g->enc_state > 0) return 0;
    if (g->enc_state < 0) return fail(LDPC_HIP_EUNSUPPORTED, "%s", g->enc_why.c_str());
    auto refuse = [&](const char *fmt, ...) -> int {
        char buf[400];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        g->enc_state = -1;
        g->enc_why = std::string("encode_NBQCLDPC: ") + buf;
        return fail(LDPC_HIP_EUNSUPPORTED, "%s", g->enc_why.c_str());
    };
    const int rh = c->rh, nh = c->nh, M = c->M, q = g->q;
    if (rh < 2) return refuse("rh = %d: the recursion needs at least 2 block rows (upstream would read row -1 of the matrix)", rh);
    if (nh <= rh) return refuse("nh = %d <= rh = %d: there is no information column, the special column nh - rh falls outside the matrix", nh, rh);
    auto HB = [&](int i, int j) -> int { return g->hb[(size_t)i * nh + j]; };
    auto HC = [&](int i, int j) -> int { return g->hc_after[(size_t)i * nh + j]; };
    for (int i = 0; i < rh; ++i)
        for (int j = 0; j < nh; ++j) {
            if (HB(i, j) < -1)
                return refuse("shift %d at (%d, %d): the decoder reads a shift below -1 as empty, upstream's encoder as a rotation", HB(i, j), i, j);
            if (HB(i, j) != -1 && (HC(i, j) <= 0 || HC(i, j) >= q))
                return refuse("coefficient %d at (%d, %d) after ncols2convert: elements of HC are to be nonzero elements of GF (decoders.cpp:1421-1425)",
                              HC(i, j), i, j);
        }
    const int cb = nh - rh;
    int weight = 0, pos_beta = 0;
    for (int i = 0; i < rh; ++i)
        if (HB(i, cb) != -1 && ++weight == 2) pos_beta = i;
    if (weight != 2 && weight != 3)
        return refuse("special column %d has weight %d: wrong weight special column of H (decoders.cpp:1493-1495)", cb, weight);
    if (HB(0, cb) == -1) return refuse("empty circulant at (0, nh-rh) = (0, %d): upstream would multiply by a coefficient that is not there", cb);
    if (HB(rh - 1, cb) == -1)
        return refuse("empty circulant at (rh-1, nh-rh) = (%d, %d): upstream would multiply by a coefficient that is not there", rh - 1, cb);
    for (int j = 0; j + 1 < rh; ++j)
        if (HB(j, cb + 1 + j) == -1)
            return refuse("empty circulant at (j, nh-rh+1+j) = (%d, %d): the dual diagonal is broken, upstream would invert a coefficient that is not there",
                          j, cb + 1 + j);
    const int alpha = HC(0, cb), gamma = HC(rh - 1, cb);
    int beta, rot_cw = 0, rot_synd = 0;
    if (weight == 2) {
        if (alpha == gamma)
            return refuse("special column of weight 2 with equal coefficients %d: correct column of HC is (x -1...-1, y), x~=y (decoders.cpp:1461-1465)", alpha);
        if (HB(0, cb) != 0 || HB(rh - 1, cb) != 0)
            return refuse("special column of weight 2 with shifts (%d, %d): both have to be 0 (decoders.cpp:1467-1471)", HB(0, cb), HB(rh - 1, cb));
        beta = alpha ^ gamma;
    } else {
        if (alpha != gamma)
            return refuse("special column of weight 3 with end coefficients %d != %d: correct column of HC is (x -1...y...-1, x) (decoders.cpp:1477-1481)",
                          alpha, gamma);
        beta = HC(pos_beta, cb);
        // the shape complaint of :1486-1490 only prints; the scheme follows d1 alone (:1491) and the final check decides
        const int d1 = HB(0, cb), d2 = HB(pos_beta, cb);
        if (d1 == 0) rot_cw = rot_synd = (M - d2 % M) % M;   // OXO (:1584-1590)
        else rot_synd = d1 % M;                              // XOX (:1612)
    }
    const int F = M >= ldpc_gfq::kEncThreads ? 1 : ldpc_gfq::kEncThreads / M;
    const size_t lds = ldpc_gfq::enc_lds_bytes(F, c->N, c->R, M, q);
    if (lds > 64 * 1024)
        return refuse("the frame state needs %zu bytes of LDS, at most 65536 are available to the encoder (nh + rh too large for this build)", lds);

    std::vector<int> lg, alog;
    gfq_field(g->q_bits, lg, alog);
    std::vector<int16_t> tab((size_t)2 * rh * nh + 2 * q);
    for (int i = 0; i < rh * nh; ++i) {
        const bool there = g->hb[i] != -1;
        tab[i] = (int16_t)(there ? g->hb[i] % M : -1);
        tab[(size_t)rh * nh + i] = (int16_t)(there ? lg[g->hc_after[i]] : 0);
    }
    for (int s = 0; s < q; ++s) { tab[(size_t)2 * rh * nh + s] = (int16_t)lg[s]; tab[(size_t)2 * rh * nh + q + s] = (int16_t)alog[s]; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMalloc(&g->d_enc, sizeof(int16_t) * tab.size()));
    HIP_TRY(hipMemcpy(g->d_enc, tab.data(), sizeof(int16_t) * tab.size(), hipMemcpyHostToDevice));
    ldpc_gfq::EncArgs &a = g->enc;
    a = ldpc_gfq::EncArgs{};
    a.rh = rh; a.nh = nh; a.M = M; a.N = c->N; a.R = c->R; a.K = cb * M; a.q = q; a.F = F;
    a.shift = g->d_enc; a.lgc = g->d_enc + (size_t)rh * nh; a.field = g->d_enc + (size_t)2 * rh * nh;
    a.weight3 = weight == 3; a.pos_beta = pos_beta;
    a.lg_alpha = lg[alpha]; a.lg_gamma = lg[gamma]; a.lg_beta = lg[beta];
    a.rot_cw = rot_cw; a.rot_synd = rot_synd;
    g->enc_lds = lds;
    g->enc_state = 1;
    return 0;
}

int gfq_grid(int num_cu, long long items, int per_block) {
    long long blocks = (items + per_block - 1) / per_block;
    const long long cap = (long long)num_cu * 32;
    if (blocks > cap) blocks = cap;
    return (int)(blocks < 1 ? 1 : blocks);
}
int gfq_grid(const ldpc_gfq_state *g, long long items, int per_block) { return gfq_grid(g->num_cu, items, per_block); }

// the channel of a code of length N over GF(2^q_bits); a code-set context (ldpc_gfq_codeset_api.hpp) launches it too.  one_word: d_codeword
// is a single [N] word that every frame carries (the exact-replay entry points), not [B][N]
int gfq_channel_launch(int num_cu, int N, int q_bits, const int16_t *d_codeword, const int32_t *d_ok, const double *d_noise, double sigma, uint64_t seed,
                       long long first_frame, long long B, double *d_soft, hipStream_t stream, bool one_word = false) {
    ldpc_gfq::QChanArgs a{};
    a.codeword = d_codeword; a.cw_stride = one_word ? 0 : N; a.ok = d_ok; a.noise = d_noise; a.soft = d_soft;
    a.B = B; a.first_frame = first_frame; a.N = N; a.q_bits = q_bits; a.sigma = sigma; a.seed = seed;
    const dim3 grid((unsigned)gfq_grid(num_cu, B * (long long)N, 256)), block(256);
    switch (q_bits) {
    case 2: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_kernel<2>, grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_kernel<3>, grid, block, 0, stream, a); break;
    case 4: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_kernel<4>, grid, block, 0, stream, a); break;
    case 5: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_kernel<5>, grid, block, 0, stream, a); break;
    case 6: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_kernel<6>, grid, block, 0, stream, a); break;
    case 7: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_kernel<7>, grid, block, 0, stream, a); break;
    case 8: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_kernel<8>, grid, block, 0, stream, a); break;
    case 9: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_kernel<9>, grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL(ldpc_gfq::gfq_channel_kernel<10>, grid, block, 0, stream, a); break;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
int gfq_channel_launch(ldpc_hip_ctx *c, const int16_t *d_codeword, const int32_t *d_ok, const double *d_noise, double sigma, uint64_t seed,
                       long long first_frame, long long B, double *d_soft, hipStream_t stream, bool one_word = false) {
    return gfq_channel_launch(c->gfq->num_cu, c->N, c->gfq->q_bits, d_codeword, d_ok, d_noise, sigma, seed, first_frame, B, d_soft, stream, one_word);
}

int gfq_count_launch(ldpc_hip_ctx *c, const int16_t *d_qhard, const int16_t *d_codeword, const int32_t *d_ok, const int32_t *d_iters, long long B,
                     unsigned long long *d_counters, int32_t *d_frame_info, hipStream_t stream, bool one_word = false) {
    ldpc_gfq::QCountArgs a{};
    a.qhard = d_qhard; a.codeword = d_codeword; a.cw_stride = one_word ? 0 : c->N; a.ok = d_ok; a.iters = d_iters; a.frame_info = d_frame_info; a.counters = d_counters;
    a.B = B; a.N = c->N; a.R = c->R;
    hipLaunchKernelGGL(ldpc_gfq::gfq_count_kernel, dim3((unsigned)gfq_grid(c->gfq, B, 4)), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// workspace of the chain for `frames` frames; grows on demand, freed in ldpc_gfq_release
int gfq_chain_workspace(ldpc_hip_ctx *c, long long frames) {
    ldpc_gfq_state *g = c->gfq;
    if (!g->w_cnt) HIP_TRY(hipMalloc(&g->w_cnt, sizeof(unsigned long long) * 5));
    if (frames <= g->w_frames) return 0;
    void *old[] = {g->w_soft, g->w_msg, g->w_cw, g->w_qh, g->w_ok, g->w_it};
    for (void *p : old)
        if (p) (void)hipFree(p);
    g->w_soft = nullptr; g->w_msg = g->w_cw = g->w_qh = nullptr; g->w_ok = g->w_it = nullptr; g->w_frames = 0;
    const size_t K = (size_t)std::max(1, (c->nh - c->rh) * c->M);
    HIP_TRY(hipMalloc(&g->w_soft, sizeof(double) * (size_t)g->q * c->N * frames));
    HIP_TRY(hipMalloc(&g->w_msg, sizeof(int16_t) * K * frames));
    HIP_TRY(hipMalloc(&g->w_cw, sizeof(int16_t) * (size_t)c->N * frames));
    HIP_TRY(hipMalloc(&g->w_qh, sizeof(int16_t) * (size_t)c->N * frames));
    HIP_TRY(hipMalloc(&g->w_ok, sizeof(int32_t) * (size_t)frames));
    HIP_TRY(hipMalloc(&g->w_it, sizeof(int32_t) * (size_t)frames));
    g->w_frames = frames;
    return 0;
}

}  // namespace

extern "C" {

int ldpc_hip_gfq_left2right(int16_t *matr, int rh, int nh) {
    if (!matr || rh <= 0 || nh <= 0 || nh < rh) return fail(LDPC_HIP_EINVAL, "ldpc_hip_gfq_left2right: null matrix, non-positive size or nh < rh");
    std::vector<int16_t> buf((size_t)nh);
    for (int i = 0; i < rh; ++i) {
        int16_t *row = matr + (size_t)i * nh;
        int k = 0;
        for (int j = rh; j < nh; ++j) buf[k++] = row[j];
        buf[k++] = row[rh - 1];
        for (int j = 0; j < rh - 1; ++j) buf[k++] = row[j];
        std::memcpy(row, buf.data(), sizeof(int16_t) * (size_t)nh);
    }
    return 0;
}

int ldpc_hip_gfq_k(const ldpc_hip_ctx *c) { return c && c->gfq && c->nh > c->rh ? (c->nh - c->rh) * c->M : 0; }

double ldpc_hip_gfq_sigma(const ldpc_hip_ctx *c, double snr_db) {
    if (!c || (!c->gfq && !c->codes_gfq)) return 0.0;
    const double bitrate = (double)(c->nh - c->rh) / c->nh;   // bp_simulation.cpp:444 with punctured_blocks = 0
    return sqrt(pow(10, -snr_db / 10) / 2 / bitrate);          // :445
}

int ldpc_hip_encode_gfq_dev(ldpc_hip_ctx *c, const int16_t *d_msg, long long B, int16_t *d_codeword, int32_t *d_ok, void *stream_) {
    if (!c || !c->gfq || B < 0) return fail(LDPC_HIP_EINVAL, "ldpc_hip_encode_gfq_dev: not a GF(q) context (ldpc_hip_open_gfq), or bad argument");
    if (int rc = gfq_encoder_plan(c)) return rc;
    if (B == 0) return 0;
    if (!d_msg || !d_codeword) return fail(LDPC_HIP_EINVAL, "ldpc_hip_encode_gfq_dev: null message or codeword");
    ldpc_gfq_state *g = c->gfq;
    const long long blocks = (B + g->enc.F - 1) / g->enc.F;
    if (blocks > 0x7fffffffLL) return fail(LDPC_HIP_EINVAL, "batch too large");
    HIP_TRY(hipSetDevice(c->device));
    ldpc_gfq::EncArgs a = g->enc;
    a.msg = d_msg; a.codeword = d_codeword; a.ok = d_ok; a.B = B;
    hipLaunchKernelGGL(ldpc_gfq::gfq_encode_kernel, dim3((unsigned)blocks), dim3(ldpc_gfq::kEncThreads), g->enc_lds, (hipStream_t)stream_, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ldpc_hip_encode_gfq_host(ldpc_hip_ctx *c, const int16_t *msg, long long B, int16_t *codeword, int32_t *ok) {
    if (!c || !c->gfq || B < 0) return fail(LDPC_HIP_EINVAL, "ldpc_hip_encode_gfq_host: not a GF(q) context (ldpc_hip_open_gfq), or bad argument");
    if (int rc = gfq_encoder_plan(c)) return rc;
    if (B == 0) return 0;
    if (!msg || !codeword) return fail(LDPC_HIP_EINVAL, "ldpc_hip_encode_gfq_host: null message or codeword");
    const size_t K = (size_t)c->gfq->enc.K, N = (size_t)c->N;
    int16_t *d_msg = nullptr, *d_cw = nullptr;
    int32_t *d_ok = nullptr;
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc(&d_msg, sizeof(int16_t) * K * B));
        HIP_TRY(hipMalloc(&d_cw, sizeof(int16_t) * N * B));
        HIP_TRY(hipMalloc(&d_ok, sizeof(int32_t) * (size_t)B));
        HIP_TRY(hipMemcpy(d_msg, msg, sizeof(int16_t) * K * B, hipMemcpyHostToDevice));
        if (int r = ldpc_hip_encode_gfq_dev(c, d_msg, B, d_cw, d_ok, nullptr)) return r;
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(codeword, d_cw, sizeof(int16_t) * N * B, hipMemcpyDeviceToHost));
        if (ok) HIP_TRY(hipMemcpy(ok, d_ok, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost));
        return 0;
    };
    const int rc = body();
    if (d_msg) (void)hipFree(d_msg);
    if (d_cw) (void)hipFree(d_cw);
    if (d_ok) (void)hipFree(d_ok);
    return rc;
}

int ldpc_hip_gfq_channel_dev(ldpc_hip_ctx *c, const int16_t *d_codeword, const double *d_noise, double sigma, uint64_t seed, long long first_frame,
                             long long B, double *d_soft, void *stream_) {
    if (!c || !c->gfq || B < 0 || first_frame < 0)
        return fail(LDPC_HIP_EINVAL, "ldpc_hip_gfq_channel_dev: not a GF(q) context (ldpc_hip_open_gfq), or bad argument");
    if (B == 0) return 0;
    if (!d_soft) return fail(LDPC_HIP_EINVAL, "ldpc_hip_gfq_channel_dev: null output");
    if (B > 0x7fffffffLL) return fail(LDPC_HIP_EINVAL, "batch too large");
    HIP_TRY(hipSetDevice(c->device));
    return gfq_channel_launch(c, d_codeword, nullptr, d_noise, sigma, seed, first_frame, B, d_soft, (hipStream_t)stream_);
}

int ldpc_hip_count_errors_gfq_dev(ldpc_hip_ctx *c, const int16_t *d_qhard, const int16_t *d_codeword, const int32_t *d_iters, long long B,
                                  unsigned long long *d_counters, int32_t *d_frame_info, void *stream_) {
    if (!c || !c->gfq || B < 0) return fail(LDPC_HIP_EINVAL, "ldpc_hip_count_errors_gfq_dev: not a GF(q) context (ldpc_hip_open_gfq), or bad argument");
    if (B == 0) return 0;
    if (!d_qhard || !d_iters || !d_counters) return fail(LDPC_HIP_EINVAL, "ldpc_hip_count_errors_gfq_dev: null qhard, iters or counters");
    HIP_TRY(hipSetDevice(c->device));
    return gfq_count_launch(c, d_qhard, d_codeword, nullptr, d_iters, B, d_counters, d_frame_info, (hipStream_t)stream_);
}

int ldpc_hip_simulate_gfq(ldpc_hip_ctx *c, double snr_db, int maxiter, uint64_t seed, long long first_frame, long long B, int random_messages,
                          unsigned long long counters[5]) {
    if (!c || !c->gfq || !counters || B < 0 || first_frame < 0)
        return fail(LDPC_HIP_EINVAL, "ldpc_hip_simulate_gfq: not a GF(q) context (ldpc_hip_open_gfq), or bad argument");
    if (maxiter < 1) return fail(LDPC_HIP_EINVAL, "ldpc_hip_simulate_gfq: maxiter must be >= 1 (got %d)", maxiter);
    if (random_messages) { if (int rc = gfq_encoder_plan(c)) return rc; }
    if (B == 0) return 0;
    ldpc_gfq_state *g = c->gfq;
    HIP_TRY(hipSetDevice(c->device));
    // pieces whose [q][N] float64 workspace stays under 1 GiB (as ldpc_hip_decode_gfq_host stages); LDPC_HIP_GFQ_PIECE=n caps them further
    long long piece = (long long)(((size_t)1 << 30) / (sizeof(double) * (size_t)g->q * c->N));
    if (const char *e = getenv("LDPC_HIP_GFQ_PIECE")) { if (atoll(e) > 0 && atoll(e) < piece) piece = atoll(e); }
    if (piece < 1) piece = 1;
    if (piece > B) piece = B;
    if (int rc = gfq_chain_workspace(c, piece)) return rc;
    hipStream_t stream = nullptr;
    const double sigma = ldpc_hip_gfq_sigma(c, snr_db);
    HIP_TRY(hipMemsetAsync(g->w_cnt, 0, sizeof(unsigned long long) * 5, stream));
    for (long long done = 0; done < B; done += piece) {
        const long long nb = std::min(piece, B - done);
        const int16_t *cw = nullptr;
        const int32_t *ok = nullptr;
        if (random_messages) {
            ldpc_gfq::MsgArgs m{};
            m.msg = g->w_msg; m.B = nb; m.first_frame = first_frame + done; m.K = g->enc.K; m.q = g->q; m.seed = seed;
            hipLaunchKernelGGL(ldpc_gfq::gfq_message_kernel, dim3((unsigned)gfq_grid(g, nb * (long long)((m.K + 3) / 4), 256)), dim3(256), 0, stream, m);
            HIP_TRY(hipGetLastError());
            if (int rc = ldpc_hip_encode_gfq_dev(c, g->w_msg, nb, g->w_cw, g->w_ok, stream)) return rc;
            cw = g->w_cw; ok = g->w_ok;
        }
        if (int rc = gfq_channel_launch(c, cw, ok, nullptr, sigma, seed, first_frame + done, nb, g->w_soft, stream)) return rc;
        if (int rc = ldpc_hip_decode_gfq_dev(c, g->w_soft, nb, maxiter, 0.0, g->w_qh, g->w_it, nullptr, stream)) return rc;
        if (int rc = gfq_count_launch(c, g->w_qh, cw, ok, g->w_it, nb, g->w_cnt, nullptr, stream)) return rc;
    }
    unsigned long long h[5];
    HIP_TRY(hipMemcpy(h, g->w_cnt, sizeof h, hipMemcpyDeviceToHost));
    for (int i = 0; i < 5; ++i) counters[i] += h[i];
    return 0;
}

}  // extern "C"
