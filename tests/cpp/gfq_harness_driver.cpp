// gfq_harness_driver.cpp -- ldpc::bp_simulation(q_mod > 2, ...) of include/ldpc/bp_simulation.h on one GF(q) code, as a caller of
// upstream's harness would use it: seed, reset_random(), bp_simulation(), then more draws from the same generator.
// usage: gfq_harness_driver <in.bin> ; in.bin: int32 {q_mod, rh, nh, M, ncols2convert, maxiter, n_frame_errors, n_experiments,
//        punctured_blocks, seed, show_process, decoder_type, modulation_type, permutation_type}, float64 {snr, reference_frame_error}, int32 H[rh][nh], int32 coef[rh][nh]
// prints: "pair <BER> <FER>" (hex floats) and "next <g0> <g1> <g2> <g3>" (the next next_random_gaussian() values) after
// ldpc::bp_simulation(); "coef ..." the coefficient matrix as the call left it; "counters nse nde nue experiment sum_abs_iters" and
// "pair2 ..." of a second run from the same seed through bp_simulation_gfq_t, which hands the SimCounters out.
// A wrong decoder_type, modulation_type or permutation_type ends the program with the reason on stderr and exit status 1.
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
    const int q_mod = p[0], rh = p[1], nh = p[2], M = p[3], n2c = p[4], maxiter = p[5], nfe = p[6], nexp = p[7], punct = p[8], seed = p[9], show = p[10];
    const int dec = p[11], mod = p[12], perm = p[13];
    std::vector<int32_t> h((size_t)rh * nh), g((size_t)rh * nh);
    if (fread(h.data(), sizeof(int32_t), h.size(), f) != h.size() || fread(g.data(), sizeof(int32_t), g.size(), f) != g.size()) return 2;
    fclose(f);
    ldpc::Matrix H(rh, nh), coef(rh, nh);
    for (int i = 0; i < rh * nh; ++i) { H.v[(size_t)i] = h[(size_t)i]; coef.v[(size_t)i] = g[(size_t)i]; }

    ldpc::initial_random_seed = seed;
    ldpc::reset_random();
    ldpc::Matrix back = coef;
    const std::pair<double, double> res = ldpc::bp_simulation(q_mod, H, back, n2c, M, maxiter, nfe, nexp, d[0], d[1], dec, mod, perm, 128, 1, punct, show);
    printf("pair %a %a\n", res.first, res.second);
    printf("next");
    for (int i = 0; i < 4; ++i) printf(" %a", ldpc::next_random_gaussian());
    printf("\ncoef");
    for (int v : back.v) printf(" %d", v);
    printf("\n");

    ldpc::reset_random();
    ldpc::Matrix again = coef;
    ldpc::SimCounters k;
    const std::pair<double, double> res2 = ldpc::bp_simulation_gfq_t<ldpc::Matrix, ldpc::OwnRngEnv>(q_mod, H, again, n2c, M, maxiter, nfe, nexp, d[0], d[1], dec, mod, perm,
                                                                                                    punct, 0, &k, 0, 64);
    printf("counters %lld %lld %lld %lld %lld\n", k.nse, k.nde, k.nue, k.experiment, k.sum_abs_iters);
    printf("pair2 %a %a\n", res2.first, res2.second);
    return again.v == back.v ? 0 : 3;
}
