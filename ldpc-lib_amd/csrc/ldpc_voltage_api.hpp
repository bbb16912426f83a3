// Host side of the voltage check (kernels: ldpc_voltage.hpp): the argument checks, the equation table with every edge counted as
// random, and the batch worked off in pieces.  Included from ldpc_hip.hip after ldpc_label_api.hpp, whose checks and table it uses.
#pragma once

namespace {

constexpr long long kVoltagePieceBytes = 256ll << 20;   // device memory of one piece's labellings and results
constexpr long long kVoltagePieceMax = 1ll << 20;       // labellings of one launch

}  // namespace

extern "C" int ldpc_hip_check_voltages(int rh, int nh, const int16_t *proto, int target_girth, int max_modulo, const int32_t *voltages,
                                       const int32_t *coefs, long long K, int device, int32_t *status, int32_t *min_ok, int32_t *max_nonok,
                                       int32_t *max_abs_sum, uint64_t *failed, int *tree_girth, int *n_equations) {
    using namespace ldpc_voltage;
    const char *who = "ldpc_hip_check_voltages";
    if (int rc = label_check(who, rh, nh, proto, target_girth)) return rc;
    if (max_modulo < 1) return fail(LDPC_HIP_EINVAL, "%s: max_modulo = %d, must be >= 1", who, max_modulo);
    if (max_modulo > kMaxModulo) return fail(LDPC_HIP_EUNSUPPORTED, "%s: max_modulo = %d, at most %d (the bitmap of a labelling is kept in LDS)", who, max_modulo, kMaxModulo);
    if (K < 1) return fail(LDPC_HIP_EINVAL, "%s: K = %lld, at least one labelling must be given", who, K);
    if (!voltages || !status || !min_ok || !max_nonok || !max_abs_sum)
        return fail(LDPC_HIP_EINVAL, "%s: voltages, status, min_ok, max_nonok and max_abs_sum must not be NULL", who);
    std::vector<int16_t> all_random((size_t)rh * nh);
    for (size_t i = 0; i < all_random.size(); ++i) all_random[i] = proto[i] > 0 ? 1 : 0;
    const long long E = std::count(all_random.begin(), all_random.end(), (int16_t)1);
    if (E > kMaxEdges) return fail(LDPC_HIP_EUNSUPPORTED, "%s: %lld edges, at most %d (a wave keeps its labelling in LDS)", who, E, kMaxEdges);
    long long bad = first_bad_value(voltages, K * E);
    if (bad >= 0) return fail(LDPC_HIP_EINVAL, "%s: labelling %lld, edge %lld: voltage %d outside 0 .. %d", who, bad / E, bad % E, (int)voltages[bad], kMaxValue);
    bad = coefs ? first_bad_value(coefs, K * E) : -1;
    if (bad >= 0) return fail(LDPC_HIP_EINVAL, "%s: labelling %lld, edge %lld: coefficient %d outside 0 .. %d", who, bad / E, bad % E, (int)coefs[bad], kMaxValue);
    ldpc_label::Table t;
    if (int rc = label_table(who, rh, nh, all_random.data(), target_girth, t)) return rc;

    const int W = bitmap_words(max_modulo);
    long long forced = 0;
    if (const char *e = getenv("LDPC_HIP_VOLTAGE_PIECE")) forced = atoll(e);
    const long long piece = piece_size(K, E, coefs != nullptr, failed != nullptr, W, kVoltagePieceBytes, kVoltagePieceMax, forced);
    bool moduli = false;
    if (const char *e = getenv("LDPC_HIP_VOLTAGE_LAYOUT")) moduli = strcmp(e, "moduli") == 0;

    HIP_TRY(hipSetDevice(device));
    GirthBuffers buf;
    Args a{};
    int32_t *d_eq_begin = nullptr, *d_terms = nullptr, *d_v = nullptr, *d_c = nullptr;
    std::vector<int32_t> terms(t.term_edge.size());
    for (size_t i = 0; i < terms.size(); ++i) terms[i] = (t.term_edge[i] << 8) | (t.term_mult[i] & 0xff);
    HIP_TRY(buf.get(&d_eq_begin, sizeof(int32_t) * t.eq_begin.size()));
    HIP_TRY(buf.get(&d_terms, sizeof(int32_t) * terms.size()));
    HIP_TRY(buf.get(&d_v, sizeof(int32_t) * (size_t)(piece * E)));
    if (coefs) HIP_TRY(buf.get(&d_c, sizeof(int32_t) * (size_t)(piece * E)));
    HIP_TRY(buf.get(&a.status, sizeof(int32_t) * (size_t)piece));
    HIP_TRY(buf.get(&a.min_ok, sizeof(int32_t) * (size_t)piece));
    HIP_TRY(buf.get(&a.max_nonok, sizeof(int32_t) * (size_t)piece));
    HIP_TRY(buf.get(&a.max_abs_sum, sizeof(int32_t) * (size_t)piece));
    if (failed) HIP_TRY(buf.get(&a.failed, sizeof(uint64_t) * (size_t)(piece * W)));
    HIP_TRY(hipMemcpy(d_eq_begin, t.eq_begin.data(), sizeof(int32_t) * t.eq_begin.size(), hipMemcpyHostToDevice));
    if (!terms.empty()) HIP_TRY(hipMemcpy(d_terms, terms.data(), sizeof(int32_t) * terms.size(), hipMemcpyHostToDevice));
    a.q = Equations{t.n_equations, d_eq_begin, d_terms};
    a.E = (int)E; a.max_modulo = max_modulo; a.W = W;
    a.voltages = d_v; a.coefs = d_c;
    const size_t lds = lds_bytes((int)E, coefs != nullptr, W);
    for (long long k0 = 0; k0 < K; k0 += piece) {
        const long long n = std::min(piece, K - k0);
        HIP_TRY(hipMemcpy(d_v, voltages + k0 * E, sizeof(int32_t) * (size_t)(n * E), hipMemcpyHostToDevice));
        if (coefs) HIP_TRY(hipMemcpy(d_c, coefs + k0 * E, sizeof(int32_t) * (size_t)(n * E), hipMemcpyHostToDevice));
        if (moduli) hipLaunchKernelGGL(check_kernel<true>, dim3((unsigned)n), dim3(64), lds, nullptr, a);
        else hipLaunchKernelGGL(check_kernel<false>, dim3((unsigned)n), dim3(64), lds, nullptr, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(status + k0, a.status, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(min_ok + k0, a.min_ok, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(max_nonok + k0, a.max_nonok, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(max_abs_sum + k0, a.max_abs_sum, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
        if (failed) HIP_TRY(hipMemcpy(failed + k0 * W, a.failed, sizeof(uint64_t) * (size_t)(n * W), hipMemcpyDeviceToHost));
    }
    if (tree_girth) *tree_girth = t.tree_girth;
    if (n_equations) *n_equations = t.n_equations;
    return 0;
}

extern "C" int ldpc_hip_label_bank(int rh, int nh, const int16_t *proto, int target_girth, int T, int exact_modulo, long long max_attempts, int want,
                                   const uint32_t state_in[624], int pos_in, int device, int16_t *hd_out, int32_t *min_ok_out,
                                   long long *attempt_index, int *found, long long *attempts_tested, int *tree_girth, uint32_t state_out[624],
                                   int *pos_out) {
    using namespace ldpc_voltage;
    const char *who = "ldpc_hip_label_bank";
    if (exact_modulo != 0 && (exact_modulo < T || exact_modulo > kMaxModulo))
        return fail(LDPC_HIP_EINVAL, "%s: exact_modulo = %d, must be 0 or T = %d .. %d", who, exact_modulo, T, kMaxModulo);
    if (!min_ok_out) return fail(LDPC_HIP_EINVAL, "%s: min_ok_out must not be NULL", who);
    BankArgs b{};
    b.T = T; b.exact_modulo = exact_modulo;
    b.max_modulo = std::max(T, exact_modulo);   // decides as upstream's unbounded check does
    b.W = bitmap_words(b.max_modulo);
    SecondPass bank;
    bank.m_name = "T";
    bank.min_ok_out = min_ok_out;
    bank.prepare = [&b](GirthBuffers &buf, long long n_max, int32_t **min_ok_att) {
        const hipError_t e = buf.get(&b.min_ok_att, sizeof(int32_t) * (size_t)n_max);
        *min_ok_att = b.min_ok_att;
        return e;
    };
    bank.launch = [&b](const ldpc_label::Args &a, unsigned nwaves, hipStream_t st) {
        b.l = a;
        hipLaunchKernelGGL(bank_kernel, dim3(nwaves), dim3(64), lds_bytes(a.Er, false, b.W), st, b);
    };
    return label_search(who, rh, nh, proto, target_girth, T, &bank, max_attempts, want, state_in, pos_in, device, hd_out, attempt_index,
                        found, attempts_tested, tree_girth, state_out, pos_out);
}
