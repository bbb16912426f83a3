/* simulate_gfq.c -- the GF(q) chain from plain C: symbol / frame error rates of a small QC-LDPC code over GF(16) on one MI355X.
 *
 *   gcc -O2 -Iinclude examples/simulate_gfq.c -o simulate_gfq -Lldpc-lib_amd -lldpc_hip -Wl,-rpath,$PWD/ldpc-lib_amd
 *   ./simulate_gfq 15 3.0 5.0 0.5 100000
 *                  max-iterations  snr-from snr-to step  frames
 *
 * The code is written "parity part first", as upstream's q-ary files are: rh dual-diagonal / special columns, then the information
 * columns.  ldpc_hip_gfq_left2right moves the information part to the front (bp_simulation.cpp:391-394) before the context is
 * opened; random messages are drawn, encoded, sent, decoded and counted on the device.
 */
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

#include "ldpc_hip.h"

enum { RH = 3, NH = 6, M = 8, Q_BITS = 4 };

int main(int argc, char **argv) {
    if (argc < 6) {
        fprintf(stderr, "usage: %s <max-iterations> <snr-from> <snr-to> <snr-step> <frames>\n", argv[0]);
        return 2;
    }
    const int maxit = atoi(argv[1]);
    const double s0 = atof(argv[2]), s1 = atof(argv[3]), ds = atof(argv[4]);
    const long long frames = atoll(argv[5]);
    /* columns: two dual-diagonal ones, the special one (weight 3: shifts 0, d2, 0), three information columns */
    int16_t hb[RH * NH] = { 0, -1,  0,   0,  3,  7,
                            0,  0,  5,   2, -1,  1,
                           -1,  0,  0,  -1,  6,  4};
    int16_t hc[RH * NH] = { 5, -1,  9,   1,  7, 12,
                            5,  3,  2,  14, -1,  6,
                           -1,  3,  9,  -1, 11,  8};
    if (ldpc_hip_gfq_left2right(hb, RH, NH) != 0 || ldpc_hip_gfq_left2right(hc, RH, NH) != 0) {
        fprintf(stderr, "ldpc_hip_gfq_left2right: %s\n", ldpc_hip_last_error());
        return 1;
    }
    ldpc_hip_ctx *ctx = NULL;
    if (ldpc_hip_open_gfq(Q_BITS, RH, NH, M, hb, hc, 0, 0, &ctx) != 0) { fprintf(stderr, "ldpc_hip_open_gfq: %s\n", ldpc_hip_last_error()); return 1; }
    const int n = ldpc_hip_n(ctx), k = ldpc_hip_gfq_k(ctx);
    printf("# GF(%d) (%d,%d) code, M=%d [%s], %d iterations, %lld frames per point\n", ldpc_hip_gfq_q(ctx), n, k, M, ldpc_hip_kernel_name(ctx), maxit,
           frames);
    printf("# Eb/N0[dB]      sigma          FER          SER   mean-iters   frames/s\n");
    for (double snr = s0; snr <= s1 + 1e-9; snr += ds) {
        unsigned long long cnt[5] = {0, 0, 0, 0, 0};   /* accumulated into: start from zero */
        struct timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        if (ldpc_hip_simulate_gfq(ctx, snr, maxit, /*seed*/ 1, /*first_frame*/ 0, frames, /*random_messages*/ 1, cnt) != 0) {
            fprintf(stderr, "ldpc_hip_simulate_gfq: %s\n", ldpc_hip_last_error());
            return 1;
        }
        clock_gettime(CLOCK_MONOTONIC, &t1);
        const double sec = (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
        printf("%9.3f %10.5f %12.5e %12.5e %10.2f %12.0f\n", snr, ldpc_hip_gfq_sigma(ctx, snr), (double)cnt[1] / cnt[3], (double)cnt[0] / cnt[3] / k,
               (double)cnt[4] / cnt[3], cnt[3] / sec);
    }
    ldpc_hip_close(ctx);
    return 0;
}
