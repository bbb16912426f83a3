/* simulate_codes_exact.c -- score a set of candidate codes over upstream's OWN noise: what a search computes that calls
 * reset_random() before every candidate (std::mt19937(seed), the codeword draws, then one polar-method sample per code bit), with
 * the noise drawn once and all candidates decoded in one launch per batch.  Plain C, one MI355X.
 *
 *   gcc -O2 -Iinclude examples/simulate_codes_exact.c -o simulate_codes_exact -Lldpc-lib_amd -lldpc_hip -Wl,-rpath,$PWD/ldpc-lib_amd
 *   ./simulate_codes_exact 16 2.5 50 25 100000 1e-3 1
 *                          codes snr max-iterations error-frames experiments reference-FER seed
 *
 * The candidates are those of examples/simulate_codes_stop.c.  Every row is upstream's SimCounters for that matrix after
 * reset_random(): experiment, nse, nde, nue and the sum of the iteration counts, bit for bit what bp_simulation() returns for it.
 * The call leaves the generator where it found it; ldpc_hip_mt_advance_codes then moves it to the end of one candidate's run: the
 * last line shows the state a caller's generator holds after the last candidate.
 */
#include <stdio.h>
#include <stdlib.h>

#include "ldpc_hip.h"

enum { RH = 4, NH = 8, M = 64 };

/* std::mt19937(seed) after `skip` raw draws: init_genrand, then the public recurrence */
static void mt_seed(uint32_t w[624], int *pos, uint32_t seed, long long skip) {
    w[0] = seed;
    for (int i = 1; i < 624; ++i) w[i] = 1812433253u * (w[i - 1] ^ (w[i - 1] >> 30)) + (uint32_t)i;
    *pos = 624;
    while (skip > 0) {
        if (*pos == 624) {
            for (int i = 0; i < 624; ++i) {
                const uint32_t y = (w[i] & 0x80000000u) | (w[(i + 1) % 624] & 0x7fffffffu);
                w[i] = w[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            *pos = 0;
        }
        const long long take = skip < 624 - *pos ? skip : 624 - *pos;
        *pos += (int)take;
        skip -= take;
    }
}

int main(int argc, char **argv) {
    if (argc < 8) {
        fprintf(stderr, "usage: %s <codes> <snr-db> <max-iterations> <error-frames> <experiments> <reference-FER> <seed>\n", argv[0]);
        return 2;
    }
    const int C = atoi(argv[1]), maxit = atoi(argv[3]), nfe = atoi(argv[4]);
    const double snr = atof(argv[2]), ref_fer = atof(argv[6]);
    const long long nexp = atoll(argv[5]);
    const uint32_t seed = (uint32_t)strtoul(argv[7], NULL, 10);
    if (C < 1) { fprintf(stderr, "codes must be positive\n"); return 2; }
    static const int mask[RH * NH] = {1, 0, 0, 1,  1, 1, 0, 1,
                                      1, 1, 0, 0,  1, 0, 1, 1,
                                      0, 1, 1, 1,  0, 1, 1, 1,
                                      0, 0, 1, 1,  1, 1, 1, 0};
    int16_t *hd = malloc(sizeof(int16_t) * (size_t)C * RH * NH);
    unsigned long long *st = malloc(sizeof(unsigned long long) * 6 * (size_t)C);
    if (!hd || !st) return 1;
    unsigned lcg = 12345u;
    for (int c = 0; c < C; ++c)
        for (int i = 0; i < RH * NH; ++i) {
            lcg = lcg * 1664525u + 1013904223u;
            const int info_column = i % NH >= RH;
            hd[(size_t)c * RH * NH + i] = (int16_t)(mask[i] ? (info_column ? (int)((lcg >> 16) % M) : 0) : -1);
        }
    ldpc_hip_ctx *ctx = NULL;
    if (ldpc_hip_open_codes(LDPC_HIP_MS_DEC, RH, NH, M, hd, C, 0, &ctx) != 0) { fprintf(stderr, "ldpc_hip_open_codes: %s\n", ldpc_hip_last_error()); return 1; }
    uint32_t words[624];
    int pos = 0;
    mt_seed(words, &pos, seed, (long long)(NH - RH) * M);   /* random_codeword() draws one word per information bit first */
    if (ldpc_hip_mt_set_state_codes(ctx, words, pos) != 0 ||
        ldpc_hip_mt_simulate_codes_stop(ctx, snr, 0, maxit, 0.8, nfe, nexp, ref_fer, /*first_batch*/ 1024, /*max_batch*/ 65536, st) != 0) {
        fprintf(stderr, "%s\n", ldpc_hip_last_error());
        return 1;
    }
    const int K = ldpc_hip_n(ctx) - ldpc_hip_r(ctx);
    printf("# code  experiments  error-frames  undetected          FER          BER  mean-iterations  frames-decoded\n");
    for (int c = 0; c < C; ++c) {
        const unsigned long long *k = st + 6 * (size_t)c;   /* experiment, nse, nde, nue, sum |iters|, frames_decoded */
        const double n = k[0] ? (double)k[0] : 1.0;
        printf("%6d %12llu %13llu %11llu %12.5e %12.5e %16.3f %15llu\n", c, k[0], k[2], k[3], (double)k[2] / n, (double)k[1] / n / K, (double)k[4] / n, k[5]);
    }
    /* where `for (candidate) { reset_random(); bp_simulation(); }` leaves the generator: after the last candidate's frames */
    if (ldpc_hip_mt_advance_codes(ctx, snr, 0, (long long)st[6 * (size_t)(C - 1)]) != 0 || ldpc_hip_mt_get_state_codes(ctx, words, &pos) != 0) {
        fprintf(stderr, "%s\n", ldpc_hip_last_error());
        return 1;
    }
    printf("# %d codes (%d,%d), M=%d [%s], %.2f dB, seed %u; generator afterwards: word %d of the block that starts with %08x\n", C, ldpc_hip_n(ctx),
           K, M, ldpc_hip_kernel_name(ctx), snr, seed, pos, words[0]);
    ldpc_hip_close(ctx);
    free(hd);
    free(st);
    return 0;
}
