// codes_gfq_driver.cpp -- ldpc::bp_simulation_codes_gfq on one set of GF(q) codes through both of its routes: show_process = 0 (the
// stopping rule on the device, ldpc_hip_simulate_codes_gfq_stop) and show_process = 1 (the records replayed on the host, a line per
// error frame).
// usage: codes_gfq_driver <in.bin> ; in.bin: int32 {C, rh, nh, M, q_mod, maxiter, n_frame_errors, n_experiments, batch, seed},
//        float64 {snr, reference_frame_error}, int16 hb[C][rh][nh], int16 hc[C][rh][nh]
// prints per code one line "device" and one line "host": SER and FER as hex floats, nse, nde, experiment
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ldpc/bp_simulation.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t p[10];
    double d[2];
    if (fread(p, sizeof p, 1, f) != 1 || fread(d, sizeof d, 1, f) != 1) return 2;
    const int C = p[0], rh = p[1], nh = p[2], M = p[3], q_mod = p[4], maxiter = p[5], nfe = p[6], nexp = p[7], batch = p[8];
    const unsigned long long seed = (unsigned long long)p[9];
    std::vector<int16_t> hb((size_t)C * rh * nh), hc((size_t)C * rh * nh);
    if (fread(hb.data(), sizeof(int16_t), hb.size(), f) != hb.size() || fread(hc.data(), sizeof(int16_t), hc.size(), f) != hc.size()) return 2;
    fclose(f);
    std::vector<ldpc::Matrix> codes, coefs;
    for (int c = 0; c < C; ++c) {
        ldpc::Matrix H(rh, nh), G(rh, nh);
        for (int i = 0; i < rh; ++i)
            for (int j = 0; j < nh; ++j) {
                H(i, j) = hb[((size_t)c * rh + i) * nh + j];
                G(i, j) = hc[((size_t)c * rh + i) * nh + j];
            }
        codes.push_back(H);
        coefs.push_back(G);
    }
    const char *route[2] = {"device", "host"};
    for (int show = 0; show < 2; ++show) {
        std::vector<ldpc::SimCounters> cnt;
        const auto res = ldpc::bp_simulation_codes_gfq(q_mod, codes, coefs, M, maxiter, nfe, nexp, d[0], d[1], show, seed, 0, &cnt, batch, batch);
        for (int c = 0; c < C; ++c)
            printf("%s %d %a %a %lld %lld %lld\n", route[show], c, res[(size_t)c].first, res[(size_t)c].second, cnt[(size_t)c].nse, cnt[(size_t)c].nde,
                   cnt[(size_t)c].experiment);
    }
    return 0;
}
