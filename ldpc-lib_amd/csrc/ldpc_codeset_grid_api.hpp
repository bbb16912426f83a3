// An SNR grid on a binary code set: P points x C codes = P * C work items over ONE noise draw per piece.  Upstream's
// `simulation` command resets its generator before every (code, SNR) pair (main_simulation.cpp:477-518), so every point of every curve
// sees the same unit-variance samples and only sigma differs; the channel kernels here (channel_llr_grid_kernel, mt_polar_kernel<2>)
// write the LLRs of all points from one sample, the set kernels decode items i = p * C + c (codeset_view splits them), and the
// counting, the stopping rule and the list of running items work on P * C rows.  Every (point, code) result is what the single-SNR
// entry point of ldpc_codeset_api.hpp returns for that SNR from the same seed or generator state.
// Included after ldpc_codeset_api.hpp at the end of ldpc_hip.hip.
#pragma once

namespace {

// What the four grid entry points refuse before anything is drawn, reserved or launched; sigma [P] as awgn_sigma gives it per point
// for the common rate (nh - rh) / (nh - punctured_blocks).
int codes_grid_args(const char *who, const ldpc_hip_ctx *c, const double *snr_db, int P, int punctured_blocks, int maxiter, double alpha,
                    double *sigma) {
    if (P < 1 || P > ldpc::kGridPoints) return fail(LDPC_HIP_EINVAL, "%s: P = %d; an SNR grid holds 1 .. %d points", who, P, ldpc::kGridPoints);
    if (!snr_db) return fail(LDPC_HIP_EINVAL, "%s: null snr_db", who);
    if (!c || !c->codes) return fail(LDPC_HIP_EINVAL, "%s: not a binary code-set context (ldpc_hip_open_codes and its kin)", who);
    if (maxiter < 1) return fail(LDPC_HIP_EINVAL, "%s: maxiter must be >= 1 (got %d)", who, maxiter);
    if (int rc = alpha_refusal(who, c->decoder_id, alpha)) return rc;
    if (ms_alpha_not_positive(c->decoder_id, alpha) && !(codeset_kind_of(c).is & CS_GLOBAL))   // the rule of codeset_decode_launch
        return fail(LDPC_HIP_EINVAL, "%s: alpha = %g is not above zero; %s gives upstream's bits for alpha > 0 only, "
                    "a set opened with ldpc_hip_open_codes_global takes any alpha", who, alpha, c->kernel_name.c_str());
    for (int p = 0; p < P; ++p) {
        if (!std::isfinite(snr_db[p])) return fail(LDPC_HIP_EINVAL, "%s: point %d, snr_db = %g", who, p, snr_db[p]);
        if (int rc = awgn_sigma(c, snr_db[p], 0, punctured_blocks, &sigma[p])) return rc;
    }
    return 0;
}

// A piece of the grid, or the first refusal of its decode launch: ceil(piece / F) * P * C workgroups
int codes_grid_piece(const char *who, const ldpc_hip_ctx *c, int P, long long B, long long *piece) {
    *piece = codeset_piece(c, B, P);
    const long long bpc = (*piece + c->F - 1) / c->F;
    if (bpc * P * c->codes->C > 0x7fffffffLL)
        return fail(LDPC_HIP_EINVAL, "%s: %d codes x %lld frames is more than one launch takes", who, P * c->codes->C, *piece);
    return 0;
}

// Philox: frames [first_frame, first_frame + nb) for every point -> w_llr [P][nb][N] -> the n_active items of `list` (null: all)
int codes_grid_piece_launch(ldpc_hip_ctx *c, ldpc::ChannelGridArgs &g, int maxiter, double alpha, long long first_frame, long long nb, bool want_info,
                            const int32_t *list, int n_active) {
    ldpc_codeset_state *s = c->codes;
    g.c.B = nb; g.c.first_frame = first_frame; g.point_stride = nb * (long long)c->N;
    long long blocks = (nb * (long long)((c->N + 1) / 2) + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(ldpc::channel_llr_grid_kernel, dim3((unsigned)blocks), dim3(256), 0, nullptr, g);
    HIP_TRY(hipGetLastError());
    if (int rc = codeset_decode_launch(c, s->w_llr, 1, nb, maxiter, alpha, s->w_hard, s->w_iters, nullptr, nullptr, list, n_active, g.P)) return rc;
    return codeset_count_launch(c, s->w_hard, s->w_iters, nb, want_info ? s->w_info : nullptr, s->w_cnt, nullptr, list, n_active, g.P);
}

// exact replay: the next nb frames of the stream, once, for every point -> w_llr [P][nb][N] -> the n_active items of `list` (null: all)
int mt_codes_grid_piece_launch(ldpc_hip_ctx *c, const double *snr_db, int P, const double *sigma, int punctured_blocks, int maxiter, double alpha,
                               long long nb, bool want_info, const int32_t *list, int n_active) {
    ldpc_codeset_state *s = c->codes;
    const MtGrid grid{P, nb * (long long)c->N, sigma};
    if (int rc = mt_llr_rows(c, snr_db[0], 0, punctured_blocks, nb, 0, nb, s->w_llr, nullptr, &grid)) return rc;
    if (int rc = codeset_decode_launch(c, s->w_llr, 1, nb, maxiter, alpha, s->w_hard, s->w_iters, nullptr, nullptr, list, n_active, P)) return rc;
    return codeset_count_launch(c, s->w_hard, s->w_iters, nb, want_info ? s->w_info : nullptr, s->w_cnt, nullptr, list, n_active, P);
}

void codes_grid_channel_args(const ldpc_hip_ctx *c, int P, const double *sigma, int punctured_blocks, uint64_t seed, ldpc::ChannelGridArgs &g) {
    codeset_channel_args(c, punctured_blocks, seed, g.c);
    g.P = P;
    for (int p = 0; p < P; ++p) g.sigma[p] = sigma[p];
}

}  // namespace

extern "C" {

int ldpc_hip_simulate_codes_grid(ldpc_hip_ctx *c, const double *snr_db, int P, int punctured_blocks, int maxiter, double alpha, uint64_t seed,
                                 long long first_frame, long long B, unsigned long long *counters, int32_t *frame_info) {
    const char *const who = "ldpc_hip_simulate_codes_grid";
    double sigma[ldpc::kGridPoints];
    if (int rc = codes_grid_args(who, c, snr_db, P, punctured_blocks, maxiter, alpha, sigma)) return rc;
    if (!counters || B < 0 || first_frame < 0) return fail(LDPC_HIP_EINVAL, "%s: bad argument", who);
    long long piece = 0;
    if (int rc = codes_grid_piece(who, c, P, B, &piece)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = codeset_reserve(c, piece, P)) return rc;
    ldpc::ChannelGridArgs g{};
    codes_grid_channel_args(c, P, sigma, punctured_blocks, seed, g);
    return codeset_simulate_loop(*c->codes, piece, B, counters, frame_info, [&](long long first, long long nb) -> int {
        return codes_grid_piece_launch(c, g, maxiter, alpha, first_frame + first, nb, frame_info != nullptr, nullptr, 0);
    }, P);
}

int ldpc_hip_simulate_codes_grid_stop(ldpc_hip_ctx *c, const double *snr_db, int P, int punctured_blocks, int maxiter, double alpha, uint64_t seed,
                                      long long first_frame, int n_frame_errors, long long n_experiments, const double *reference_frame_error,
                                      long long first_batch, long long max_batch, unsigned long long *state) {
    const char *const who = "ldpc_hip_simulate_codes_grid_stop";
    double sigma[ldpc::kGridPoints];
    if (int rc = codes_grid_args(who, c, snr_db, P, punctured_blocks, maxiter, alpha, sigma)) return rc;
    if (!reference_frame_error) return fail(LDPC_HIP_EINVAL, "%s: null reference_frame_error", who);
    if (int rc = codeset_stop_args(who, state, first_frame, first_batch, max_batch, maxiter)) return rc;
    long long piece = 0;
    if (int rc = codes_grid_piece(who, c, P, max_batch < n_experiments + 1 ? max_batch : n_experiments + 1, &piece)) return rc;
    std::memset(state, 0, sizeof(unsigned long long) * 4 * (size_t)P * (size_t)c->codes->C);
    if (n_frame_errors <= 0 || n_experiments < 0) return 0;   // :591 fails before the first frame
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = codeset_reserve(c, piece, P)) return rc;
    ldpc::ChannelGridArgs g{};
    codes_grid_channel_args(c, P, sigma, punctured_blocks, seed, g);
    return codeset_stop_loop(*c->codes, piece, n_frame_errors, n_experiments, 0.0, first_batch, max_batch, state,
                             [&](long long first, long long nb, const int32_t *list, int n_active) -> int {
                                 return codes_grid_piece_launch(c, g, maxiter, alpha, first_frame + first, nb, true, list, n_active);
                             }, false, reference_frame_error, P);
}

int ldpc_hip_mt_simulate_codes_grid(ldpc_hip_ctx *c, const double *snr_db, int P, int punctured_blocks, int maxiter, double alpha, long long B,
                                    unsigned long long *counters, int32_t *frame_info, int32_t *iters) {
    const char *const who = "ldpc_hip_mt_simulate_codes_grid";
    double sigma[ldpc::kGridPoints];
    if (int rc = codes_grid_args(who, c, snr_db, P, punctured_blocks, maxiter, alpha, sigma)) return rc;
    if (!counters || B < 0) return fail(LDPC_HIP_EINVAL, "%s: bad argument", who);
    if (int rc = mt_codes_channel_check(c, snr_db[0], punctured_blocks)) return rc;
    long long piece = 0;
    if (int rc = codes_grid_piece(who, c, P, B, &piece)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    ldpc_codeset_state *s = c->codes;
    if (int rc = codeset_reserve(c, piece, P)) return rc;
    const size_t rows = (size_t)P * (size_t)s->C;
    return codeset_simulate_loop(*s, piece, B, counters, frame_info, [&](long long first, long long nb) -> int {
        if (int rc = mt_codes_grid_piece_launch(c, snr_db, P, sigma, punctured_blocks, maxiter, alpha, nb, frame_info != nullptr, nullptr, 0)) return rc;
        if (iters)   // [P * C][nb] on the device -> columns [first, first + nb) of the caller's [P][C][B]
            HIP_TRY(hipMemcpy2D(iters + first, sizeof(int32_t) * (size_t)B, s->w_iters, sizeof(int32_t) * (size_t)nb, sizeof(int32_t) * (size_t)nb, rows,
                                hipMemcpyDeviceToHost));
        return 0;
    }, P);
}

int ldpc_hip_mt_simulate_codes_grid_stop(ldpc_hip_ctx *c, const double *snr_db, int P, int punctured_blocks, int maxiter, double alpha,
                                         int n_frame_errors, long long n_experiments, const double *reference_frame_error, long long first_batch,
                                         long long max_batch, unsigned long long *state) {
    using namespace ldpc_mt;
    const char *const who = "ldpc_hip_mt_simulate_codes_grid_stop";
    double sigma[ldpc::kGridPoints];
    if (int rc = codes_grid_args(who, c, snr_db, P, punctured_blocks, maxiter, alpha, sigma)) return rc;
    if (!reference_frame_error) return fail(LDPC_HIP_EINVAL, "%s: null reference_frame_error", who);
    if (int rc = codeset_stop_args(who, state, 0, first_batch, max_batch, maxiter)) return rc;
    if (int rc = mt_codes_channel_check(c, snr_db[0], punctured_blocks)) return rc;
    long long piece = 0;
    if (int rc = codes_grid_piece(who, c, P, max_batch < n_experiments + 1 ? max_batch : n_experiments + 1, &piece)) return rc;
    std::memset(state, 0, sizeof(unsigned long long) * 6 * (size_t)P * (size_t)c->codes->C);
    if (n_frame_errors <= 0 || n_experiments < 0) return 0;   // :591 fails before the first frame
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = codeset_reserve(c, piece, P)) return rc;
    // the items stop at different frames: the generator goes back to where it was, ldpc_hip_mt_advance_codes takes it to one item's end
    DeviceState &m = c->mt;
    std::vector<uint32_t> entry(MTN);
    const long long entry_pos = m.pos, entry_frames = m.frames_taken;
    HIP_TRY(hipMemcpy(entry.data(), m.d_state, sizeof(uint32_t) * MTN, hipMemcpyDeviceToHost));
    const int rc = codeset_stop_loop(*c->codes, piece, n_frame_errors, n_experiments, 0.0, first_batch, max_batch, state,
                                     [&](long long, long long nb, const int32_t *list, int n_active) -> int {   // pieces come in frame order
                                         return mt_codes_grid_piece_launch(c, snr_db, P, sigma, punctured_blocks, maxiter, alpha, nb, true, list, n_active);
                                     }, true, reference_frame_error, P);
    if (hipMemcpy(m.d_state, entry.data(), sizeof(uint32_t) * MTN, hipMemcpyHostToDevice) != hipSuccess && rc == 0)
        return fail(LDPC_HIP_EHIP, "%s: the generator's state could not be put back", who);
    m.pos = entry_pos; m.frames_taken = entry_frames;
    return rc;
}

}  // extern "C"
