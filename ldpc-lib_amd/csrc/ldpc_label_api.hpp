// Host side of the labelling search (enumeration and kernels: ldpc_label.hpp): the argument checks, the equation table, the rounds of
// attempts over the mt19937 word tape of ldpc_mt_api.hpp, and the generator handed back where upstream's loop leaves it.  The search
// serves generate_code here and, through a second pass it knows nothing about, the bank search of ldpc_voltage_api.hpp.
// Included from ldpc_hip.hip after ldpc_mt_api.hpp.
#pragma once

#include <functional>

namespace {

constexpr long long kLabelFirstRound = 4096;        // attempts of the first round; every later round is eight times the one before
constexpr long long kLabelRoundWords = 1ll << 26;   // ... up to this many draws (256 MiB of tape)

thread_local long long t_label_stats[4] = {0, 0, 0, 0};   // ldpc_hip_label_last_stats

int label_check(const char *who, int rh, int nh, const int16_t *proto, int target_girth) {
    if (rh < 1 || nh < 1) return fail(LDPC_HIP_EINVAL, "%s: rh = %d, nh = %d must be positive", who, rh, nh);
    if (!proto) return fail(LDPC_HIP_EINVAL, "%s: proto is NULL", who);
    if (target_girth < 4) return fail(LDPC_HIP_EINVAL, "%s: target_girth = %d, must be >= 4", who, target_girth);
    long long edges = 0;
    for (long long i = 0; i < (long long)rh * nh; ++i) {
        if (proto[i] < 0) return fail(LDPC_HIP_EINVAL, "%s: row %lld, column %lld: entry %d is negative", who, i / nh, i % nh, (int)proto[i]);
        edges += proto[i] > 0;
    }
    if (edges == 0) return fail(LDPC_HIP_EINVAL, "%s: the protograph has no edge", who);
    return 0;
}

int label_table(const char *who, int rh, int nh, const int16_t *proto, int target_girth, ldpc_label::Table &t) {
    if (target_girth > ldpc_label::kMaxGirth)
        return fail(LDPC_HIP_EUNSUPPORTED, "%s: target_girth = %d, at most %d (multiplicities are kept in 8 bits)", who, target_girth, ldpc_label::kMaxGirth);
    if (!ldpc_label::equations(rh, nh, proto, target_girth, t))
        return fail(LDPC_HIP_EUNSUPPORTED, "%s: target_girth = %d needs more than %lld %s (limits: %lld equations, %lld paths per layer)", who, target_girth,
                    t.refused_count - 1, t.refused_what, ldpc_label::kMaxEquations, ldpc_label::kMaxLayerNodes);
    return 0;
}

struct LabelCtx {   // the generator machinery of a context, without a decoder
    ldpc_hip_ctx c;
    ~LabelCtx() { ldpc_mt::release(c.mt); }
};

}  // namespace

extern "C" int ldpc_hip_label_equations_host(int rh, int nh, const int16_t *proto, int target_girth, int *tree_girth, int *n_equations, int *n_random,
                                             long long *n_terms, int *never_accepts, int32_t *eq_begin, int32_t *term_edge, int32_t *term_mult) {
    const char *who = "ldpc_hip_label_equations_host";
    if (int rc = label_check(who, rh, nh, proto, target_girth)) return rc;
    ldpc_label::Table t;
    if (int rc = label_table(who, rh, nh, proto, target_girth, t)) return rc;
    if (tree_girth) *tree_girth = t.tree_girth;
    if (n_equations) *n_equations = t.n_equations;
    if (n_random) *n_random = t.n_random;
    if (n_terms) *n_terms = (long long)t.term_edge.size();
    if (never_accepts) *never_accepts = t.never_accepts ? 1 : 0;
    if (eq_begin) std::copy(t.eq_begin.begin(), t.eq_begin.end(), eq_begin);
    if (term_edge) std::copy(t.term_edge.begin(), t.term_edge.end(), term_edge);
    if (term_mult) std::copy(t.term_mult.begin(), t.term_mult.end(), term_mult);
    return 0;
}

extern "C" void ldpc_hip_label_last_stats(long long stats[4]) {
    if (stats) std::copy(t_label_stats, t_label_stats + 4, stats);
}

namespace {

// The search: attempts drawn from the tape in rounds, tested, selected in attempt order, the generator handed back.  Without a
// second pass it is generate_code (ldpc_hip_label_codes): an attempt passes when no sum is divisible by M and no two columns are
// equal.  A caller with another test (ldpc_hip_label_bank, ldpc_voltage_api.hpp) hands in a SecondPass: check_kernel then drops only
// the attempts with a zero sum, the caller's kernel narrows the round's bitmap to what it accepts and notes a min_ok per attempt,
// there is no equal-columns test and no early return for a tree girth below the target.
struct SecondPass {
    const char *m_name;                                                                            // what M is called in messages
    int32_t *min_ok_out;                                                                           // HOST [want]
    std::function<hipError_t(GirthBuffers &buf, long long n_max, int32_t **min_ok_att)> prepare;   // device [n_max], once per call
    std::function<void(const ldpc_label::Args &a, unsigned nwaves, hipStream_t st)> launch;        // once per round
};

int label_search(const char *who, int rh, int nh, const int16_t *proto, int target_girth, int M, const SecondPass *second, long long max_attempts, int want,
                 const uint32_t state_in[624], int pos_in, int device, int16_t *hd_out, long long *attempt_index, int *found,
                 long long *attempts_tested, int *tree_girth, uint32_t state_out[624], int *pos_out) {
    using namespace ldpc_label;
    if (int rc = label_check(who, rh, nh, proto, target_girth)) return rc;
    if (M < 2 || M > 32767) return fail(LDPC_HIP_EINVAL, "%s: %s = %d outside 2 .. 32767", who, second ? second->m_name : "M", M);
    if (max_attempts < 1) return fail(LDPC_HIP_EINVAL, "%s: max_attempts = %lld, must be >= 1", who, max_attempts);
    if (want < 1) return fail(LDPC_HIP_EINVAL, "%s: want = %d, at least one labelling must be asked for", who, want);
    if (!state_in || pos_in < 0 || pos_in > 624) return fail(LDPC_HIP_EINVAL, "%s: state_in is NULL or pos_in = %d outside 0 .. 624", who, pos_in);
    if (!hd_out || !attempt_index || !found || !attempts_tested || !tree_girth || !state_out || !pos_out)
        return fail(LDPC_HIP_EINVAL, "%s: hd_out, attempt_index, found, attempts_tested, tree_girth, state_out and pos_out must not be NULL", who);
    Table t;
    if (int rc = label_table(who, rh, nh, proto, target_girth, t)) return rc;
    if (t.n_random > kMaxRandomEdges)
        return fail(LDPC_HIP_EUNSUPPORTED, "%s: %d edges with a random shift, at most %d (a wave keeps 64 labellings in LDS)", who, t.n_random, kMaxRandomEdges);

    std::fill(t_label_stats, t_label_stats + 4, 0ll);
    *tree_girth = t.tree_girth;
    *found = 0;
    *attempts_tested = 0;
    std::copy(state_in, state_in + 624, state_out);
    *pos_out = pos_in;
    if (!second && t.tree_girth < target_girth) return 0;   // upstream returns before any draw
    const int Er = t.n_random;
    if (Er == 0) {   // nothing is drawn: every attempt is the all-zero labelling
        std::vector<int> by_col((size_t)nh * rh);
        for (size_t i = 0; i < by_col.size(); ++i) by_col[i] = t.cell[i] == -1 ? -1 : 0;
        const bool ok = t.n_equations == 0 && (second || !same_columns(rh, nh, by_col));   // every sum would be 0
        const long long k = ok ? std::min<long long>(want, max_attempts) : 0;
        for (long long c = 0; c < k; ++c) {
            attempt_index[c] = c;
            if (second) second->min_ok_out[c] = 2;   // no equation: the failed set is empty
            for (int i = 0; i < rh; ++i)
                for (int j = 0; j < nh; ++j) hd_out[((size_t)c * rh + i) * nh + j] = (int16_t)by_col[(size_t)j * rh + i];
        }
        *found = (int)k;
        *attempts_tested = k == want ? k : max_attempts;
        return 0;
    }

    long long forced = 0;
    if (const char *e = getenv("LDPC_HIP_LABEL_ROUND")) { if (atoll(e) > 0) forced = atoll(e); }
    const long long round_cap = std::max<long long>(1, kLabelRoundWords / Er);

    HIP_TRY(hipSetDevice(device));
    LabelCtx lc;
    ldpc_hip_ctx *c = &lc.c;
    c->device = device;
    if (int rc = mt_state_store(c, state_in, pos_in)) return rc;
    hipStream_t st = nullptr;
    GirthBuffers buf;
    Args a{};
    int32_t *d_eq_begin = nullptr, *d_terms = nullptr, *d_cell = nullptr, *d_pairs = nullptr;
    const std::vector<int32_t> pairs = second ? std::vector<int32_t>() : column_pairs(rh, nh, t.cell);
    std::vector<int32_t> terms(t.term_edge.size());
    for (size_t i = 0; i < terms.size(); ++i) terms[i] = (t.term_edge[i] << 8) | (t.term_mult[i] & 0xff);
    HIP_TRY(buf.get(&d_eq_begin, sizeof(int32_t) * t.eq_begin.size()));
    HIP_TRY(buf.get(&d_terms, sizeof(int32_t) * terms.size()));
    HIP_TRY(buf.get(&d_cell, sizeof(int32_t) * t.cell.size()));
    HIP_TRY(buf.get(&d_pairs, sizeof(int32_t) * pairs.size()));
    if (!pairs.empty()) HIP_TRY(hipMemcpyAsync(d_pairs, pairs.data(), sizeof(int32_t) * pairs.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(buf.get(&a.ctr, sizeof(unsigned long long) * kCounters));
    HIP_TRY(buf.get(&a.hd_out, sizeof(int16_t) * (size_t)want * rh * nh));
    HIP_TRY(buf.get(&a.attempt_index, sizeof(long long) * (size_t)want));
    HIP_TRY(hipMemcpyAsync(d_eq_begin, t.eq_begin.data(), sizeof(int32_t) * t.eq_begin.size(), hipMemcpyHostToDevice, st));
    if (!terms.empty()) HIP_TRY(hipMemcpyAsync(d_terms, terms.data(), sizeof(int32_t) * terms.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_cell, t.cell.data(), sizeof(int32_t) * t.cell.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(a.ctr, 0, sizeof(unsigned long long) * kCounters, st));
    a.Er = Er; a.M = M;
    a.thresh = (uint32_t)((1ull << 32) % (unsigned long long)M);
    a.er_magic = Er >= 2 ? (uint32_t)((1ull << 32) / (unsigned long long)Er + 1ull) : 0u;
    a.div_M = second ? 1u << 22 : (uint32_t)M;
    a.m_magic = (1ull << 40) / (unsigned long long)a.div_M + 1ull;
    a.n_eq = t.n_equations; a.eq_begin = d_eq_begin; a.terms = d_terms;
    a.rh = rh; a.nh = nh; a.want = want; a.cell = d_cell;
    a.pairs = d_pairs; a.n_pairs = (int)(pairs.size() / 2);
    a.state_next = c->mt.d_state_next;
    const size_t lds = sizeof(int16_t) * (size_t)kRowStride * (size_t)Er;
    if (second) HIP_TRY(buf.get(&a.min_ok_out, sizeof(int32_t) * (size_t)want));

    // the largest round of this call sizes the redraw lists and the survivor bitmap
    const long long n_max = std::min(std::min(forced ? forced : round_cap, round_cap), max_attempts);
    HIP_TRY(buf.get(&a.rej_raw, sizeof(uint32_t) * (size_t)(64 + n_max * Er / 8192 + 1)));
    HIP_TRY(buf.get(&a.rej, sizeof(uint32_t) * (size_t)(64 + n_max * Er / 8192 + 1)));
    HIP_TRY(buf.get(&a.bitmap, sizeof(unsigned long long) * (size_t)((n_max + 63) / 64)));
    int32_t *min_ok_att = nullptr;
    if (second) HIP_TRY(second->prepare(buf, n_max, &min_ok_att));
    a.min_ok_att = min_ok_att;

    long long tested = 0, accepted = 0;
    long long n_next = forced ? forced : kLabelFirstRound;
    unsigned long long ctr[kCounters];
    while (accepted < want && tested < max_attempts) {
        const long long n = std::min(std::min(n_next, round_cap), max_attempts - tested);
        const long long draws = n * Er;
        const long long rej_cap = 64 + draws / 8192;   // sixteen times the expected number of redraws at M = 32767, and 64
        const long long words = draws + rej_cap;
        // the tape: words [pos, pos + words) are scanned, the 624 behind any of them can become the next state
        MtPlan pl;
        pl.pos = c->mt.pos;
        pl.tape_words = 1ll << 40;
        const MtWindow w = mt_window(pl, 0, pl.pos + words + ldpc_mt::MTN);
        if (int rc = mt_ensure(c, w)) return rc;
        if (int rc = mt_generate(c, w, st)) return rc;
        const long long nwaves = (n + 63) / 64;
        a.xw = c->mt.d_xraw + pl.pos;
        a.p = pl.pos;
        a.words = (uint32_t)words; a.n = (uint32_t)n; a.att_base = tested;
        a.rej_cap = (uint32_t)rej_cap;
        HIP_TRY(hipMemsetAsync(a.ctr, 0, sizeof(unsigned long long) * 2, st));   // kRejected, kSurvivors
        const unsigned mark_blocks = (unsigned)std::min<long long>((words + 2047) / 2048, 4096);
        hipLaunchKernelGGL(mark_kernel, dim3(mark_blocks), dim3(256), 0, st, a);
        hipLaunchKernelGGL(sort_kernel, dim3(1), dim3(256), 0, st, a);
        hipLaunchKernelGGL(check_kernel, dim3((unsigned)nwaves), dim3(64), lds, st, a);
        if (second) second->launch(a, (unsigned)nwaves, st);
        hipLaunchKernelGGL(select_kernel, dim3(1), dim3(kSelectThreads), lds, st, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c->mt.d_state, c->mt.d_state_next, sizeof(uint32_t) * ldpc_mt::MTN, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctr, a.ctr, sizeof ctr, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (ctr[kRejected] > (unsigned long long)rej_cap)
            return fail(LDPC_HIP_EHIP, "%s: %llu redraws among %lld words, more than the %lld a round provides for", who, ctr[kRejected], words, rej_cap);
        c->mt.pos = 0;
        accepted = (long long)ctr[kAccepted];
        t_label_stats[0] += 1;
        if (accepted >= want) {
            long long last = 0;
            HIP_TRY(hipMemcpy(&last, a.attempt_index + (want - 1), sizeof last, hipMemcpyDeviceToHost));
            tested = last + 1;
        } else {
            tested += n;
        }
        if (!forced) n_next = n * 8;
    }
    t_label_stats[1] = (long long)ctr[kRedraws];
    t_label_stats[2] = (long long)ctr[kEvaluated];
    t_label_stats[3] = (long long)ctr[kChecked];
    if (accepted > 0) {
        HIP_TRY(hipMemcpy(hd_out, a.hd_out, sizeof(int16_t) * (size_t)accepted * rh * nh, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(attempt_index, a.attempt_index, sizeof(long long) * (size_t)accepted, hipMemcpyDeviceToHost));
        if (second) HIP_TRY(hipMemcpy(second->min_ok_out, a.min_ok_out, sizeof(int32_t) * (size_t)accepted, hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipMemcpy(state_out, c->mt.d_state, sizeof(uint32_t) * ldpc_mt::MTN, hipMemcpyDeviceToHost));
    *pos_out = 0;
    *found = (int)accepted;
    *attempts_tested = tested;
    return 0;
}

}  // namespace

extern "C" int ldpc_hip_label_codes(int rh, int nh, const int16_t *proto, int target_girth, int M, long long max_attempts, int want,
                                    const uint32_t state_in[624], int pos_in, int device, int16_t *hd_out, long long *attempt_index, int *found,
                                    long long *attempts_tested, int *tree_girth, uint32_t state_out[624], int *pos_out) {
    return label_search("ldpc_hip_label_codes", rh, nh, proto, target_girth, M, nullptr, max_attempts, want, state_in, pos_in, device, hd_out, attempt_index,
                        found, attempts_tested, tree_girth, state_out, pos_out);
}
