// gfq_codes_exact_driver.cpp -- ldpc::bp_simulation_codes_gfq_exact on one set of GF(q) candidates through both of its routes
// (show_process = 0: the rule on the device; 1: records per batch, the rule on the host, a line per error frame), next to what the loop
// it replaces computes: reset_random(); bp_simulation_gfq_t per candidate.
// usage: gfq_codes_exact_driver <in.bin> ; in.bin: int32 {q_mod, C, rh, nh, M, ncols2convert, maxiter, n_frame_errors, n_experiments,
//        punctured_blocks, seed, leave_at, first_batch, max_batch}, float64 {snr, reference_frame_error}, int32 H[C][rh][nh],
//        int32 coef[C][rh][nh]
// prints per route "set <show> <c> <BER> <FER> nse nde nue experiment sum_abs_iters" (hex floats), "coef <show> <c> ..." (the
// coefficients as the call left them) and "next <show> g0 g1 g2 g3" (the generator afterwards); per candidate "one <c> ..." with the
// same fields from bp_simulation_gfq_t, "onecoef <c> ..." and "onenext <c> g0 g1 g2 g3".
// LDPC_HIP_EXACT_NOISE=host in the environment takes the host noise route.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ldpc/bp_simulation.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t p[14];
    double d[2];
    if (fread(p, sizeof p, 1, f) != 1 || fread(d, sizeof d, 1, f) != 1) return 2;
    const int q_mod = p[0], C = p[1], rh = p[2], nh = p[3], M = p[4], n2c = p[5], maxiter = p[6], nfe = p[7], nexp = p[8], punct = p[9], seed = p[10];
    const int leave_at = p[11], first_batch = p[12], max_batch = p[13];
    std::vector<int32_t> h((size_t)C * rh * nh), g((size_t)C * rh * nh);
    if (fread(h.data(), sizeof(int32_t), h.size(), f) != h.size() || fread(g.data(), sizeof(int32_t), g.size(), f) != g.size()) return 2;
    fclose(f);
    std::vector<ldpc::Matrix> codes, coefs;
    for (int c = 0; c < C; ++c) {
        ldpc::Matrix H(rh, nh), G(rh, nh);
        for (int i = 0; i < rh * nh; ++i) { H.v[(size_t)i] = h[(size_t)c * rh * nh + i]; G.v[(size_t)i] = g[(size_t)c * rh * nh + i]; }
        codes.push_back(H);
        coefs.push_back(G);
    }
    const auto row = [](const char *tag, int a, int c, std::pair<double, double> res, const ldpc::SimCounters &k) {
        if (a >= 0) printf("%s %d %d", tag, a, c); else printf("%s %d", tag, c);
        printf(" %a %a %lld %lld %lld %lld %lld\n", res.first, res.second, k.nse, k.nde, k.nue, k.experiment, k.sum_abs_iters);
    };
    ldpc::initial_random_seed = seed;
    for (int show = 0; show < 2; ++show) {
        ldpc::reset_random();
        std::vector<ldpc::Matrix> back = coefs;
        std::vector<ldpc::SimCounters> cnt;
        const auto res = ldpc::bp_simulation_codes_gfq_exact(q_mod, codes, back, n2c, M, maxiter, nfe, nexp, d[0], d[1], punct, show, 0, &cnt, first_batch,
                                                             max_batch, leave_at);
        for (int c = 0; c < C; ++c) {
            row("set", show, c, res[(size_t)c], cnt[(size_t)c]);
            printf("coef %d %d", show, c);
            for (int v : back[(size_t)c].v) printf(" %d", v);
            printf("\n");
        }
        printf("next %d", show);
        for (int i = 0; i < 4; ++i) printf(" %a", ldpc::next_random_gaussian());
        printf("\n");
    }
    for (int c = 0; c < C; ++c) {
        ldpc::reset_random();
        ldpc::Matrix back = coefs[(size_t)c];
        ldpc::SimCounters k;
        const auto res = ldpc::bp_simulation_gfq_t<ldpc::Matrix, ldpc::OwnRngEnv>(q_mod, codes[(size_t)c], back, n2c, M, maxiter, nfe, nexp, d[0], d[1], LDPC_HIP_FHT_DEC,
                                                                                  0, 0, punct, 0, &k);
        row("one", -1, c, res, k);
        printf("onecoef %d", c);
        for (int v : back.v) printf(" %d", v);
        printf("\nonenext %d", c);
        for (int i = 0; i < 4; ++i) printf(" %a", ldpc::next_random_gaussian());
        printf("\n");
    }
    return 0;
}
