/* simulate_codes_stop.c -- score a set of candidate codes the way a code search does: every candidate runs until upstream's stopping
 * rule ends it, and a candidate that has stopped is not decoded any further.  Plain C, one MI355X.
 *
 *   gcc -O2 -Iinclude examples/simulate_codes_stop.c -o simulate_codes_stop -Lldpc-lib_amd -lldpc_hip -Wl,-rpath,$PWD/ldpc-lib_amd
 *   ./simulate_codes_stop 64 2.5 50 25 100000 1e-3
 *                         codes snr max-iterations error-frames experiments reference-FER
 *
 * The candidates are one 4 x 8 protograph with fresh random shifts each (examples/simulate_codes.c), all over the SAME noise.  The
 * rule (bp_simulation.cpp:591, :805-823): stop at `error-frames` error frames, after experiments + 1 frames, or as soon as
 * nde >= 10 and nde / experiment > 2.5 * reference-FER -- a candidate that is clearly worse than the reference ends early.  The rule
 * runs on the device after every batch; the last column shows how many frames each candidate was decoded for.
 */
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

#include "ldpc_hip.h"

enum { RH = 4, NH = 8, M = 64 };

int main(int argc, char **argv) {
    if (argc < 7) {
        fprintf(stderr, "usage: %s <codes> <snr-db> <max-iterations> <error-frames> <experiments> <reference-FER>\n", argv[0]);
        return 2;
    }
    const int C = atoi(argv[1]), maxit = atoi(argv[3]), nfe = atoi(argv[4]);
    const double snr = atof(argv[2]), ref_fer = atof(argv[6]);
    const long long nexp = atoll(argv[5]);
    if (C < 1) { fprintf(stderr, "codes must be positive\n"); return 2; }
    static const int mask[RH * NH] = {1, 0, 0, 1,  1, 1, 0, 1,
                                      1, 1, 0, 0,  1, 0, 1, 1,
                                      0, 1, 1, 1,  0, 1, 1, 1,
                                      0, 0, 1, 1,  1, 1, 1, 0};
    int16_t *hd = malloc(sizeof(int16_t) * (size_t)C * RH * NH);
    unsigned long long *st = malloc(sizeof(unsigned long long) * 4 * (size_t)C);
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
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    if (ldpc_hip_simulate_codes_stop(ctx, snr, 0, maxit, 0.8, /*seed*/ 1, /*first_frame*/ 0, nfe, nexp, ref_fer, /*first_batch*/ 1024,
                                     /*max_batch*/ 65536, st) != 0) {
        fprintf(stderr, "ldpc_hip_simulate_codes_stop: %s\n", ldpc_hip_last_error());
        return 1;
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    const double sec = (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
    const int K = ldpc_hip_n(ctx) - ldpc_hip_r(ctx);
    unsigned long long decoded = 0, longest = 0;
    printf("# code  experiments  error-frames          FER          BER  frames-decoded\n");
    int best = -1;
    for (int c = 0; c < C; ++c) {
        const unsigned long long *k = st + 4 * (size_t)c;   /* experiment, nse, nde, frames_decoded */
        const double n = k[0] ? (double)k[0] : 1.0;
        printf("%6d %12llu %13llu %12.5e %12.5e %15llu\n", c, k[0], k[2], (double)k[2] / n, (double)k[1] / n / K, k[3]);
        decoded += k[3];
        if (k[3] > longest) longest = k[3];
        if (k[0] && (best < 0 || (double)k[2] / (double)k[0] < (double)st[4 * (size_t)best + 2] / (double)st[4 * (size_t)best])) best = c;
    }
    printf("# %d codes (%d,%d), M=%d [%s], %.2f dB: %.3f ms; %llu frames decoded, %llu had every code run as long as the longest\n", C, ldpc_hip_n(ctx), K,
           M, ldpc_hip_kernel_name(ctx), snr, 1e3 * sec, decoded, (unsigned long long)C * longest);
    printf("# best candidate: %d\n", best);
    ldpc_hip_close(ctx);
    free(hd);
    free(st);
    return 0;
}
