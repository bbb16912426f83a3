// The host code of the voltage check that needs no device, as a program of its own for a sanitizer build
// (-fsanitize=address,undefined): piece_size() and first_bad_value() of csrc/ldpc_voltage.hpp, which ldpc_voltage_api.hpp runs on
// every call, and failed_set() of include/ldpc/equations.h.  The rest of ldpc_voltage_api.hpp (allocation, copies, launches) needs
// HIP and is not covered here.  Reads from standard input
//   K E has_coef has_failed max_modulo forced piece_bytes piece_max     then K * E values     then max_modulo / 64 + 1 bitmap words (hex)
// walks the batch in pieces exactly as the API's loop does, reading every value of every piece, and prints
//   bad <index of the first value outside 0 .. 32767, or -1>
//   pieces <first labelling of each piece ...> <K>
//   set <members of the bitmap ...>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ldpc/equations.h"
#include "ldpc_voltage.hpp"

int main() {
    long long K, E, forced, piece_bytes, piece_max;
    int has_coef, has_failed, max_modulo;
    if (scanf("%lld %lld %d %d %d %lld %lld %lld", &K, &E, &has_coef, &has_failed, &max_modulo, &forced, &piece_bytes, &piece_max) != 8) return 2;
    if (K < 1 || E < 1 || max_modulo < 1) return 2;
    std::vector<int32_t> values((size_t)(K * E));
    for (int32_t &v : values) if (scanf("%d", &v) != 1) return 2;
    const int W = ldpc_voltage::bitmap_words(max_modulo);
    std::vector<uint64_t> row((size_t)W);
    for (uint64_t &w : row) {
        unsigned long long x;
        if (scanf("%llx", &x) != 1) return 2;
        w = x;
    }
    printf("bad %lld\n", ldpc_voltage::first_bad_value(values.data(), K * E));
    const long long piece = ldpc_voltage::piece_size(K, E, has_coef != 0, has_failed != 0, W, piece_bytes, piece_max, forced);
    printf("pieces");
    for (long long k0 = 0; k0 < K; k0 += piece) {
        const long long n = piece < K - k0 ? piece : K - k0;
        if (ldpc_voltage::first_bad_value(values.data() + k0 * E, n * E) >= 0 && ldpc_voltage::first_bad_value(values.data(), K * E) < 0) return 4;
        printf(" %lld", k0);
    }
    printf(" %lld\nset", K);
    for (int m : ldpc::failed_set(row.data(), max_modulo)) printf(" %d", m);
    printf("\n");
    return 0;
}
