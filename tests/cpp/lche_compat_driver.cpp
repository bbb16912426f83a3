// lche_compat_driver.cpp -- the decoders.h call surface for the low-complexity high-efficiency decoder (LCHE_DEC), the way
// bp_simulation.cpp drives a decoder: decod_open -> fill hd -> decod_init -> per frame: copy the LLRs into st->y and call
// lche_decod(st, st->y, st->decword, maxiter, decision).
// usage: lche_compat_driver <in.bin> <out.bin>
//   in : int32 rh, nh, M, B, maxiter, decision ; int16 hd[rh*nh] ; double llr[B*N]
//   out: int32 iters[B] ; double decword[B*N] ; double y_after[B*N]
#include <cstdio>
#include <cstring>
#include <vector>

#include "ldpc/decoders.h"

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int hdr[6];
    if (fread(hdr, sizeof(int), 6, f) != 6) return 4;
    const int rh = hdr[0], nh = hdr[1], M = hdr[2], B = hdr[3], maxiter = hdr[4], decision = hdr[5];
    const int N = nh * M;
    std::vector<short> hd((size_t)rh * nh);
    std::vector<double> llr((size_t)B * N), dec((size_t)B * N), after((size_t)B * N);
    std::vector<int> iters(B);
    if (fread(hd.data(), sizeof(short), hd.size(), f) != hd.size()) return 5;
    if (fread(llr.data(), sizeof(double), llr.size(), f) != llr.size()) return 6;
    fclose(f);

    DEC_STATE *st = decod_open(LCHE_DEC, 1, rh, nh, M);
    if (!st) return 12;
    for (int i = 0; i < rh; i++) for (int j = 0; j < nh; j++) st->hd[i][j] = hd[(size_t)i * nh + j];
    if (!decod_init(st)) return 13;
    for (int b = 0; b < B; b++) {
        memcpy(st->y, &llr[(size_t)b * N], sizeof(double) * N);
        iters[b] = lche_decod(st, st->y, st->decword, maxiter, decision);   // bp_simulation.cpp:716-729
        memcpy(&dec[(size_t)b * N], st->decword, sizeof(double) * N);
        memcpy(&after[(size_t)b * N], st->y, sizeof(double) * N);
    }
    decod_close(st);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 20;
    fwrite(iters.data(), sizeof(int), B, o);
    fwrite(dec.data(), sizeof(double), dec.size(), o);
    fwrite(after.data(), sizeof(double), after.size(), o);
    fclose(o);
    return 0;
}
