/* simulate_codes.c -- score a set of candidate codes of one shape over the same noise, from plain C, on one MI355X.
 *
 *   gcc -O2 -Iinclude examples/simulate_codes.c -o simulate_codes -Lldpc-lib_amd -lldpc_hip -Wl,-rpath,$PWD/ldpc-lib_amd
 *   ./simulate_codes 16 2.5 50 4096
 *                    codes snr max-iterations frames
 *
 * What a code search does per round: C base matrices with the same rh x nh and lifting M (here: one 4 x 8 protograph with fresh
 * random shifts per candidate), each run over the SAME frames [0, frames) of the Philox channel -- one launch decodes all of them.
 */
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

#include "ldpc_hip.h"

enum { RH = 4, NH = 8, M = 64 };

int main(int argc, char **argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: %s <codes> <snr-db> <max-iterations> <frames>\n", argv[0]);
        return 2;
    }
    const int C = atoi(argv[1]), maxit = atoi(argv[3]);
    const double snr = atof(argv[2]);
    const long long frames = atoll(argv[4]);
    if (C < 1 || frames < 1) { fprintf(stderr, "codes and frames must be positive\n"); return 2; }
    /* 1 = a circulant sits here; parity part dual-diagonal, three circulants in every information column */
    static const int mask[RH * NH] = {1, 0, 0, 1,  1, 1, 0, 1,
                                      1, 1, 0, 0,  1, 0, 1, 1,
                                      0, 1, 1, 1,  0, 1, 1, 1,
                                      0, 0, 1, 1,  1, 1, 1, 0};
    int16_t *hd = malloc(sizeof(int16_t) * (size_t)C * RH * NH);
    unsigned long long *cnt = malloc(sizeof(unsigned long long) * 5 * (size_t)C);
    if (!hd || !cnt) return 1;
    unsigned lcg = 12345u;
    for (int c = 0; c < C; ++c)
        for (int i = 0; i < RH * NH; ++i) {
            lcg = lcg * 1664525u + 1013904223u;
            const int info_column = i % NH >= RH;
            hd[(size_t)c * RH * NH + i] = (int16_t)(mask[i] ? (info_column ? (int)((lcg >> 16) % M) : 0) : -1);
        }
    ldpc_hip_ctx *ctx = NULL;
    if (ldpc_hip_open_codes(LDPC_HIP_MS_DEC, RH, NH, M, hd, C, 0, &ctx) != 0) { fprintf(stderr, "ldpc_hip_open_codes: %s\n", ldpc_hip_last_error()); return 1; }
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    if (ldpc_hip_simulate_codes(ctx, snr, 0, maxit, 0.8, /*seed*/ 1, /*first_frame*/ 0, frames, cnt, NULL) != 0) {
        fprintf(stderr, "ldpc_hip_simulate_codes: %s\n", ldpc_hip_last_error());
        return 1;
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    const double sec = (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
    printf("# %d codes (%d,%d), M=%d [%s], %.2f dB, %d iterations, %lld frames each: %.3f ms, %.0f frames/s\n", ldpc_hip_codes(ctx), ldpc_hip_n(ctx),
           ldpc_hip_n(ctx) - ldpc_hip_r(ctx), M, ldpc_hip_kernel_name(ctx), snr, maxit, frames, 1e3 * sec, (double)C * frames / sec);
    printf("# code          FER          BER   mean-iters\n");
    int best = 0;
    for (int c = 0; c < C; ++c) {
        const unsigned long long *k = cnt + 5 * (size_t)c;
        printf("%6d %12.5e %12.5e %10.2f\n", c, (double)k[1] / k[3], (double)k[0] / k[3] / (ldpc_hip_n(ctx) - ldpc_hip_r(ctx)), (double)k[4] / k[3]);
        if (k[1] < cnt[5 * (size_t)best + 1]) best = c;
    }
    printf("# best candidate: %d\n", best);
    ldpc_hip_close(ctx);
    free(hd);
    free(cnt);
    return 0;
}
