// Test driver of include/ldpc/code_generation.h: upstream's loop on the library's own generator.  Reads rh, nh, target_girth, M,
// max_attempts, seed, calls, then rh * nh protograph entries, all int32, from the file named on the command line; does
//   initial_random_seed = seed; reset_random(); generate_code x calls; eight next_random_int(0, 1 << 30)
// and prints per call   call <ok> <rh * nh result entries when ok>   and at the end   fingerprint <eight values>.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ldpc/bp_simulation.h"
#include "ldpc/code_generation.h"

int main(int argc, char **argv) {
    FILE *f = argc == 2 ? fopen(argv[1], "rb") : nullptr;
    int32_t head[7];
    if (!f || fread(head, sizeof(int32_t), 7, f) != 7) return 2;
    const int rh = head[0], nh = head[1], g = head[2], M = head[3], A = head[4], seed = head[5], calls = head[6];
    std::vector<int32_t> cells((size_t)rh * nh);
    if (fread(cells.data(), sizeof(int32_t), cells.size(), f) != cells.size()) return 2;
    fclose(f);
    ldpc::Matrix proto(rh, nh), result;
    for (int i = 0; i < rh * nh; ++i) proto.v[(size_t)i] = cells[(size_t)i];
    ldpc::initial_random_seed = seed;
    ldpc::reset_random();
    try {
        for (int k = 0; k < calls; ++k) {
            const bool ok = ldpc::generate_code(proto, g, M, A, result);
            printf("call %d", ok ? 1 : 0);
            if (ok) for (int v : result.v) printf(" %d", v);
            printf("\n");
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    printf("fingerprint");
    for (int i = 0; i < 8; ++i) printf(" %d", ldpc::next_random_int(0, 1 << 30));
    printf("\n");
    return 0;
}
