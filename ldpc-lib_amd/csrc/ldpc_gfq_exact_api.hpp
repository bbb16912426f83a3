// Exact replay of upstream's q-ary frame loop (bp_simulation.cpp with q_mod > 2) on a GF(q) context: the generator of ldpc_mt_api.hpp
// in sample mode draws the [frames][N * q_bits] Gaussians of upstream's own stream (:638-642: n * q_bits draws per frame in index order,
// nothing before the frame loop), gfq_channel_kernel turns them into symbol probabilities around the one word every frame carries
// (:581-582, :644-676), ldpc_hip_decode_gfq_dev decodes and gfq_count_kernel writes the frame records (:746-755).
// Included from ldpc_hip.hip after ldpc_gfq_chain_api.hpp.
#pragma once

namespace {

constexpr int16_t kGfqUpstreamMessage[8] = {6, 11, 0, 4, 2, 1, 2, 5};   // bp_simulation.cpp:544

int gfq_exact_ctx(const ldpc_hip_ctx *c, const char *who) {
    if (!c || !c->gfq) return fail(LDPC_HIP_EINVAL, "%s: not a GF(q) context (ldpc_hip_open_gfq)", who);
    return 0;
}

// bp_simulation.cpp:444-445: punctured_blocks enters the bitrate and nothing else (no position is punctured for q_mod > 2, :711-714)
int gfq_exact_sigma(const ldpc_hip_ctx *c, const char *who, double snr_db, int punctured_blocks, double *sigma) {
    if (punctured_blocks < 0 || punctured_blocks >= c->nh)
        return fail(LDPC_HIP_EINVAL, "%s: punctured_blocks = %d, must lie in 0 .. nh - 1 = %d", who, punctured_blocks, c->nh - 1);
    if (c->nh <= c->rh) return fail(LDPC_HIP_EINVAL, "%s: nh = %d <= rh = %d, the code has no rate", who, c->nh, c->rh);
    const double bitrate = (double)(c->nh - c->rh) / (c->nh - punctured_blocks);
    *sigma = sqrt(pow(10, -snr_db / 10) / 2 / bitrate);
    return 0;
}

// frames per piece: the [q][N] float64 soft values of a piece stay under 1 GiB; LDPC_HIP_GFQ_PIECE=n caps them further
long long gfq_exact_piece(const ldpc_hip_ctx *c, long long B) {
    long long piece = (long long)(((size_t)1 << 30) / (sizeof(double) * (size_t)c->gfq->q * c->N));
    if (const char *e = getenv("LDPC_HIP_GFQ_PIECE")) { if (atoll(e) > 0 && atoll(e) < piece) piece = atoll(e); }
    if (piece < 1) piece = 1;
    return piece > B ? B : piece;
}

int gfq_exact_workspace(ldpc_hip_ctx *c, long long frames) {
    ldpc_gfq_state *g = c->gfq;
    if (int rc = gfq_chain_workspace(c, frames)) return rc;
    if (frames <= g->x_frames) return 0;
    if (g->x_noise) (void)hipFree(g->x_noise);
    if (g->x_info) (void)hipFree(g->x_info);
    g->x_noise = nullptr; g->x_info = nullptr; g->x_frames = 0;
    HIP_TRY(hipMalloc(&g->x_noise, sizeof(double) * (size_t)c->N * g->q_bits * frames));
    HIP_TRY(hipMalloc(&g->x_info, sizeof(int32_t) * (size_t)frames));
    g->x_frames = frames;
    return 0;
}

// B frames in pieces: fill(first, nb) leaves the piece's Gaussians in x_noise; channel -> decode -> count; records to the HOST arrays
template <class Fill>
int gfq_exact_frames(ldpc_hip_ctx *c, double sigma, int maxiter, long long B, int32_t *frame_info, int32_t *iters, Fill fill) {
    ldpc_gfq_state *g = c->gfq;
    const long long piece = gfq_exact_piece(c, B);
    if (int rc = gfq_exact_workspace(c, piece)) return rc;
    hipStream_t stream = nullptr;
    HIP_TRY(hipMemsetAsync(g->w_cnt, 0, sizeof(unsigned long long) * 5, stream));   // the count kernel accumulates; nobody reads the sum here
    for (long long done = 0; done < B; done += piece) {
        const long long nb = std::min(piece, B - done);
        if (int rc = fill(done, nb)) return rc;
        if (int rc = gfq_channel_launch(c, g->d_word, nullptr, g->x_noise, sigma, 0, 0, nb, g->w_soft, stream, true)) return rc;
        if (int rc = ldpc_hip_decode_gfq_dev(c, g->w_soft, nb, maxiter, 0.0, g->w_qh, g->w_it, nullptr, stream)) return rc;
        if (int rc = gfq_count_launch(c, g->w_qh, g->d_word, nullptr, g->w_it, nb, g->w_cnt, g->x_info, stream, true)) return rc;
        HIP_TRY(hipMemcpyAsync(frame_info + done, g->x_info, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(iters + done, g->w_it, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    return 0;
}

}  // namespace

extern "C" {

int ldpc_hip_gfq_upstream_message(int q_bits, int K, int16_t *msg) {
    if (q_bits < 2 || q_bits > 10 || K < 0 || (K > 0 && !msg))
        return fail(LDPC_HIP_EINVAL, "ldpc_hip_gfq_upstream_message: q_bits must lie in 2 .. 10, K must be >= 0, msg must not be null");
    for (int i = 0; i < K; ++i) msg[i] = (int16_t)(i < 8 ? kGfqUpstreamMessage[i] & ((1 << q_bits) - 1) : 0);
    return 0;
}

int ldpc_hip_gfq_set_codeword(ldpc_hip_ctx *c, const int16_t *codeword) {
    if (int rc = gfq_exact_ctx(c, "ldpc_hip_gfq_set_codeword")) return rc;
    ldpc_gfq_state *g = c->gfq;
    if (codeword)
        for (int i = 0; i < c->N; ++i)
            if (codeword[i] < 0 || codeword[i] >= g->q)
                return fail(LDPC_HIP_EINVAL, "ldpc_hip_gfq_set_codeword: symbol %d at position %d is not an element of GF(%d)", codeword[i], i, g->q);
    HIP_TRY(hipSetDevice(c->device));
    if (!codeword) {
        if (g->d_word) (void)hipFree(g->d_word);
        g->d_word = nullptr;
        return 0;
    }
    if (!g->d_word) HIP_TRY(hipMalloc(&g->d_word, sizeof(int16_t) * (size_t)c->N));
    HIP_TRY(hipMemcpy(g->d_word, codeword, sizeof(int16_t) * (size_t)c->N, hipMemcpyHostToDevice));
    return 0;
}

int ldpc_hip_mt_set_state_gfq(ldpc_hip_ctx *c, const uint32_t state[624], int pos) {
    if (int rc = gfq_exact_ctx(c, "ldpc_hip_mt_set_state_gfq")) return rc;
    if (!state || pos < 0 || pos > 624) return fail(LDPC_HIP_EINVAL, "ldpc_hip_mt_set_state_gfq: bad argument");
    return mt_state_store(c, state, pos);
}

int ldpc_hip_mt_get_state_gfq(ldpc_hip_ctx *c, uint32_t state[624], int *pos) {
    if (int rc = gfq_exact_ctx(c, "ldpc_hip_mt_get_state_gfq")) return rc;
    if (!state || !pos) return fail(LDPC_HIP_EINVAL, "ldpc_hip_mt_get_state_gfq: bad argument");
    return mt_state_load(c, "ldpc_hip_mt_set_state_gfq", state, pos);
}

int ldpc_hip_mt_advance_gfq(ldpc_hip_ctx *c, long long frames) {
    if (int rc = gfq_exact_ctx(c, "ldpc_hip_mt_advance_gfq")) return rc;
    if (frames < 0) return fail(LDPC_HIP_EINVAL, "ldpc_hip_mt_advance_gfq: bad argument");
    return mt_drop_frames(c, "ldpc_hip_mt_set_state_gfq", frames, (long long)c->N * c->gfq->q_bits);
}

int ldpc_hip_mt_frames_gfq(ldpc_hip_ctx *c, double snr_db, int punctured_blocks, int maxiter, long long B, int32_t *frame_info, int32_t *iters) {
    if (int rc = gfq_exact_ctx(c, "ldpc_hip_mt_frames_gfq")) return rc;
    if (B < 0 || (B > 0 && (!frame_info || !iters))) return fail(LDPC_HIP_EINVAL, "ldpc_hip_mt_frames_gfq: bad argument");
    if (maxiter < 1) return fail(LDPC_HIP_EINVAL, "ldpc_hip_mt_frames_gfq: maxiter must be >= 1 (got %d)", maxiter);
    double sigma = 0;
    if (int rc = gfq_exact_sigma(c, "ldpc_hip_mt_frames_gfq", snr_db, punctured_blocks, &sigma)) return rc;
    if (!c->mt.set) return fail(LDPC_HIP_EINVAL, "the generator has no state: call ldpc_hip_mt_set_state_gfq first");
    const long long per_frame = (long long)c->N * c->gfq->q_bits;
    if ((unsigned long long)per_frame > ldpc_mt::kRoundItems)
        return fail(LDPC_HIP_EUNSUPPORTED, "ldpc_hip_mt_frames_gfq: a frame of %lld samples is beyond one generation round", per_frame);
    if (B == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    return gfq_exact_frames(c, sigma, maxiter, B, frame_info, iters, [&](long long, long long nb) -> int {
        if (int rc = mt_samples(c, nb * per_frame, c->gfq->x_noise, nullptr)) return rc;
        c->mt.frames_taken += nb;
        return 0;
    });
}

int ldpc_hip_frames_gfq_noise_host(ldpc_hip_ctx *c, const double *noise, double snr_db, int punctured_blocks, int maxiter, long long B,
                                   int32_t *frame_info, int32_t *iters) {
    if (int rc = gfq_exact_ctx(c, "ldpc_hip_frames_gfq_noise_host")) return rc;
    if (B < 0 || (B > 0 && (!noise || !frame_info || !iters))) return fail(LDPC_HIP_EINVAL, "ldpc_hip_frames_gfq_noise_host: bad argument");
    if (maxiter < 1) return fail(LDPC_HIP_EINVAL, "ldpc_hip_frames_gfq_noise_host: maxiter must be >= 1 (got %d)", maxiter);
    double sigma = 0;
    if (int rc = gfq_exact_sigma(c, "ldpc_hip_frames_gfq_noise_host", snr_db, punctured_blocks, &sigma)) return rc;
    if (B == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    const size_t per_frame = (size_t)c->N * c->gfq->q_bits;
    return gfq_exact_frames(c, sigma, maxiter, B, frame_info, iters, [&](long long first, long long nb) -> int {
        HIP_TRY(hipMemcpyAsync(c->gfq->x_noise, noise + per_frame * (size_t)first, sizeof(double) * per_frame * (size_t)nb, hipMemcpyHostToDevice, nullptr));
        return 0;
    });
}

}  // extern "C"
