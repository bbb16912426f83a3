// Host side of the girth / ACE trace (kernels: ldpc_girth.hpp): the graph as predecessor lists, the argument checks, the workspace
// and its pieces, the launches of one piece, and upstream's reduction of S / SA to girth, ACE and spectrum.
// Included from ldpc_hip.hip after the other *_api.hpp.
#pragma once

namespace {

constexpr int kGirthGmax = 20;      // trace_pm.h:8 GMAX
constexpr int kGirthGtarget = 4;    // trace_pm.h:9 GTARGET

struct GirthGraph {
    int E = 0;
    std::vector<int32_t> pred_begin;   // [E + 1]
    std::vector<int32_t> pred;         // [3 * n]: j, a, as -- j ascending per J
};

// tanner_mon + hp2a_mon_pm as one pass over the base matrix.  Returns the number of predecessor entries, -1 beyond 2^31 - 1.
long long girth_graph(int rh, int nh, int M, const int16_t *hd, GirthGraph &g) {
    std::vector<int> cw(nh, 0), er, ek;
    for (int k = 0; k < nh; ++k)
        for (int j = 0; j < rh; ++j)
            if (hd[j * nh + k] >= 0) { ++cw[k]; er.push_back(j); ek.push_back(k); }
    g.E = (int)er.size();
    g.pred_begin.assign((size_t)g.E + 1, 0);
    g.pred.clear();
    long long n = 0;
    for (int J = 0; J < g.E; ++J) {
        const int j2 = er[J], k2 = ek[J];
        if ((long long)(int32_t)n != n) return -1;
        g.pred_begin[J] = (int32_t)n;
        for (int j = 0; j < g.E; ++j) {
            const int j1 = er[j], k1 = ek[j];
            if (j1 == j2 || k1 == k2 || hd[j1 * nh + k2] < 0) continue;
            g.pred.push_back(j);
            g.pred.push_back(((M - hd[j1 * nh + k2]) % M + hd[j2 * nh + k2]) % M);
            g.pred.push_back(2 * cw[k2]);
            ++n;
        }
    }
    if ((long long)(int32_t)n != n) return -1;
    g.pred_begin[g.E] = (int32_t)n;
    return n;
}

int girth_check_codes(const char *who, int rh, int nh, int M, const int16_t *hd, int C) {
    if (C < 1) return fail(LDPC_HIP_EINVAL, "%s: C = %d, at least one code is needed", who, C);
    if (rh < 1 || nh < 1 || M < 1) return fail(LDPC_HIP_EINVAL, "%s: rh = %d, nh = %d, M = %d must be positive", who, rh, nh, M);
    if (nh > 1000) return fail(LDPC_HIP_EINVAL, "%s: nh = %d, at most 1000 block columns (upstream's cw[1000], trace_pm.cpp:303)", who, nh);
    if (!hd) return fail(LDPC_HIP_EINVAL, "%s: hd is NULL", who);
    for (long long i = 0; i < (long long)C * rh * nh; ++i)
        if (hd[i] < -1 || hd[i] >= M)
            return fail(LDPC_HIP_EINVAL, "%s: code %lld, block row %lld, block column %lld: shift %d outside [-1, %d)", who, i / ((long long)rh * nh),
                        i / nh % rh, i % nh, (int)hd[i], M);
    return 0;
}

struct GirthBuffers {
    void *p[12] = {};
    int n = 0;
    ~GirthBuffers() { for (int i = 0; i < n; ++i) (void)hipFree(p[i]); }
    template <class T>
    hipError_t get(T **out, size_t bytes) {
        hipError_t e = hipMalloc(reinterpret_cast<void **>(out), bytes ? bytes : 1);
        if (e == hipSuccess) p[n++] = *out;
        return e;
    }
};

}  // namespace

extern "C" int ldpc_hip_girth_graph_host(int rh, int nh, int M, const int16_t *hd, int *E, int32_t *pred_begin, int32_t *pred, long long *n) {
    if (int rc = girth_check_codes("ldpc_hip_girth_graph_host", rh, nh, M, hd, 1)) return rc;
    GirthGraph g;
    const long long len = girth_graph(rh, nh, M, hd, g);
    if (len < 0) return fail(LDPC_HIP_EUNSUPPORTED, "ldpc_hip_girth_graph_host: more than 2^31 - 1 predecessor entries");
    if (E) *E = g.E;
    if (n) *n = len;
    if (pred_begin) std::copy(g.pred_begin.begin(), g.pred_begin.end(), pred_begin);
    if (pred) std::copy(g.pred.begin(), g.pred.end(), pred);
    return 0;
}

extern "C" int ldpc_hip_trace_matrix_host(const int32_t *S, const int32_t *SA, int gmax, int *girth, int32_t ACE[4], int32_t spectrum[4]) {
    if (!S || !SA || !girth || !ACE || !spectrum) return fail(LDPC_HIP_EINVAL, "ldpc_hip_trace_matrix_host: NULL argument");
    if (gmax < 4 || gmax > kGirthGmax) return fail(LDPC_HIP_EINVAL, "ldpc_hip_trace_matrix_host: gmax = %d outside 4 .. %d", gmax, kGirthGmax);
    int g = 1;
    while (g < gmax + 1 && !S[g - 1]) ++g;                                  // main_simulation.cpp:177-181
    if (g == gmax + 1) g = kGirthGmax + 1;
    for (int j = 0; j < kGirthGtarget; ++j) ACE[j] = spectrum[j] = 0;
    for (int j = 0, i = g - 1; i < gmax && j < kGirthGtarget; ++i) if (SA[i]) ACE[j++] = SA[i];       // :185-192
    for (int j = 0, i = g - 1; i < gmax && j < kGirthGtarget; ++i) if (S[i]) spectrum[j++] = S[i];    // :194-201
    *girth = g;
    return 0;
}

extern "C" int ldpc_hip_girth_codes(int rh, int nh, int M, const int16_t *hd, int C, int gmax, int gtarget, const int32_t *min_ace,
                                    const int32_t *max_spec, int device, int32_t *S, int32_t *SA, int32_t *status) {
    const char *who = "ldpc_hip_girth_codes";
    if (int rc = girth_check_codes(who, rh, nh, M, hd, C)) return rc;
    if (gmax < 4 || gmax > kGirthGmax) return fail(LDPC_HIP_EINVAL, "%s: gmax = %d outside 4 .. %d (GMAX)", who, gmax, kGirthGmax);
    if (gtarget < 1) return fail(LDPC_HIP_EINVAL, "%s: gtarget = %d, must be >= 1", who, gtarget);
    if (!S || !SA || !status) return fail(LDPC_HIP_EINVAL, "%s: S, SA and status must not be NULL", who);
    if (20LL * rh > 65535) return fail(LDPC_HIP_EUNSUPPORTED, "%s: rh = %d: an ace of up to 20 * rh does not fit the 16 bits it is kept in", who, rh);

    // the graphs, padded to the largest E and the longest predecessor list of the set
    std::vector<GirthGraph> graphs((size_t)C);
    int Emax = 1;
    long long pred_stride = 1;
    for (int c = 0; c < C; ++c) {
        const long long len = girth_graph(rh, nh, M, hd + (size_t)c * rh * nh, graphs[(size_t)c]);
        if (len < 0 || 3 * len > 0x7fffffffLL) return fail(LDPC_HIP_EUNSUPPORTED, "%s: code %d has more than (2^31 - 1) / 3 predecessor entries", who, c);
        Emax = std::max(Emax, graphs[(size_t)c].E);
        pred_stride = std::max(pred_stride, len);
    }
    const unsigned long long per_code = 2ULL * ldpc_girth::code_elems(Emax, M) * (sizeof(int32_t) + sizeof(uint16_t));
    if (per_code > (4ULL << 30))
        return fail(LDPC_HIP_EUNSUPPORTED, "%s: the workspace of one code (E = %d, M = %d) is %llu bytes, more than 4 GiB", who, Emax, M, per_code);
    long long piece = std::max<long long>(1, (long long)((1ULL << 30) / per_code));
    if (const char *e = getenv("LDPC_HIP_GIRTH_PIECE")) { if (atoll(e) > 0) piece = atoll(e); }
    piece = std::min<long long>(std::min<long long>(piece, C), 65535);   // codes are the grid's y dimension

    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = nullptr;
    GirthBuffers buf;
    ldpc_girth::Args a{};
    int32_t *d_E = nullptr, *d_pb = nullptr, *d_pred = nullptr, *d_bounds = nullptr;
    const size_t elems = ldpc_girth::code_elems(Emax, M) * (size_t)piece;
    for (int b = 0; b < 2; ++b) {
        HIP_TRY(buf.get(&a.coef[b], elems * sizeof(int32_t)));
        HIP_TRY(buf.get(&a.ace[b], elems * sizeof(uint16_t)));
    }
    HIP_TRY(buf.get(&d_E, sizeof(int32_t) * (size_t)piece));
    HIP_TRY(buf.get(&d_pb, sizeof(int32_t) * (size_t)piece * (Emax + 1)));
    HIP_TRY(buf.get(&d_pred, sizeof(int32_t) * (size_t)piece * pred_stride * 3));
    HIP_TRY(buf.get(&a.state, sizeof(int32_t) * (size_t)piece * ldpc_girth::kState));
    HIP_TRY(buf.get(&a.S, sizeof(int32_t) * (size_t)piece * gmax));
    HIP_TRY(buf.get(&a.SA, sizeof(int32_t) * (size_t)piece * gmax));
    HIP_TRY(buf.get(&d_bounds, sizeof(int32_t) * 2 * (size_t)gmax));
    if (min_ace) HIP_TRY(hipMemcpy(d_bounds, min_ace, sizeof(int32_t) * (size_t)gmax, hipMemcpyHostToDevice));
    if (max_spec) HIP_TRY(hipMemcpy(d_bounds + gmax, max_spec, sizeof(int32_t) * (size_t)gmax, hipMemcpyHostToDevice));
    a.E = d_E; a.pred_begin = d_pb; a.pred = d_pred;
    a.min_ace = min_ace ? d_bounds : nullptr;
    a.max_spec = max_spec ? d_bounds + gmax : nullptr;
    a.pred_stride = pred_stride;
    a.Emax = Emax; a.M = M; a.gmax = gmax; a.gtarget = gtarget;
    a.lanes = std::min((M + 63) / 64 * 64, ldpc_girth::kMaxLanes);   // M rounded up to a wave
    const int groups = std::max(1, std::min(512 / a.lanes, Emax));   // several J in flight where a row of lanes is short
    const size_t lds = ldpc_girth::row_bytes(Emax, M);
    const bool use_lds = lds <= ldpc_girth::kLdsLimit;

    std::vector<int32_t> h_E, h_pb, h_pred, h_state;
    for (long long first = 0; first < C; first += piece) {
        const int nc = (int)std::min<long long>(piece, C - first);
        h_E.assign((size_t)nc, 0);
        h_pb.assign((size_t)nc * (Emax + 1), 0);
        h_pred.assign((size_t)nc * pred_stride * 3, 0);
        for (int c = 0; c < nc; ++c) {
            const GirthGraph &g = graphs[(size_t)(first + c)];
            h_E[(size_t)c] = g.E;
            std::copy(g.pred_begin.begin(), g.pred_begin.end(), h_pb.begin() + (size_t)c * (Emax + 1));
            std::copy(g.pred.begin(), g.pred.end(), h_pred.begin() + (size_t)c * pred_stride * 3);
        }
        HIP_TRY(hipMemcpyAsync(d_E, h_E.data(), sizeof(int32_t) * h_E.size(), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(d_pb, h_pb.data(), sizeof(int32_t) * h_pb.size(), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(d_pred, h_pred.data(), sizeof(int32_t) * h_pred.size(), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(a.coef[0], 0, ldpc_girth::code_elems(Emax, M) * (size_t)nc * sizeof(int32_t), stream));
        HIP_TRY(hipMemsetAsync(a.ace[0], 0, ldpc_girth::code_elems(Emax, M) * (size_t)nc * sizeof(uint16_t), stream));
        HIP_TRY(hipMemsetAsync(a.state, 0, sizeof(int32_t) * (size_t)nc * ldpc_girth::kState, stream));
        HIP_TRY(hipMemsetAsync(a.S, 0, sizeof(int32_t) * (size_t)nc * gmax, stream));
        HIP_TRY(hipMemsetAsync(a.SA, 0, sizeof(int32_t) * (size_t)nc * gmax, stream));
        const dim3 rows((unsigned)Emax, (unsigned)nc);
        hipLaunchKernelGGL(ldpc_girth::init_kernel, rows, dim3(64), 0, stream, a);
        int src = 0;
        for (int d = 3; d < gmax; d += 2, src ^= 1) {
            if (use_lds) hipLaunchKernelGGL(ldpc_girth::step_kernel<true>, rows, dim3((unsigned)(a.lanes * groups)), lds, stream, a, src);
            else hipLaunchKernelGGL(ldpc_girth::step_kernel<false>, rows, dim3((unsigned)(a.lanes * groups)), 0, stream, a, src);
            hipLaunchKernelGGL(ldpc_girth::trace_kernel, dim3((unsigned)nc), dim3(256), 0, stream, a, src ^ 1, d);
        }
        HIP_TRY(hipGetLastError());
        h_state.resize((size_t)nc * ldpc_girth::kState);
        int32_t *So = S + (size_t)first * gmax, *SAo = SA + (size_t)first * gmax;
        HIP_TRY(hipMemcpyAsync(So, a.S, sizeof(int32_t) * (size_t)nc * gmax, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(SAo, a.SA, sizeof(int32_t) * (size_t)nc * gmax, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(h_state.data(), a.state, sizeof(int32_t) * h_state.size(), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        for (int c = 0; c < nc; ++c) {
            for (int i = 3; i < gmax; i += 2) {   // trace_pm.cpp:276-280
                So[(size_t)c * gmax + i] /= i + 1;
                SAo[(size_t)c * gmax + i] /= 2;
            }
            const int32_t *st = &h_state[(size_t)c * ldpc_girth::kState];
            status[first + c] = (st[ldpc_girth::kOk] ? 1 : 0) | (st[ldpc_girth::kOverflow] ? 2 : 0);
        }
    }
    return 0;
}
