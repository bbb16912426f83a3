// Test driver of include/ldpc/equations.h.  Reads rh, nh, target_girth, max_modulo, K, has_coef, then rh * nh protograph entries, then
// K labellings of E voltages (each followed by E coefficients when has_coef), all int32, from the file named on the command line.
// Checks the batch in one call and labelling 0 through the one-labelling overload, and prints per labelling
//   v <first_failed_equation> <min_ok_modulo> <max_nonok_modulo> <check_modulo(max_modulo)> <failed moduli ...>
// and at the end   single <the same fields of labelling 0>.  With coefficients every labelling goes through the one-labelling overload
// (the batch throws as a whole where upstream exits) and a throw prints   die <message>.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ldpc/bp_simulation.h"
#include "ldpc/equations.h"

static void print(const char *tag, ldpc::voltage_check_result const &r, int max_modulo) {
    printf("%s %d %d %d %d", tag, r.first_failed_equation, r.min_ok_modulo, r.max_nonok_modulo, r.check_modulo(max_modulo) ? 1 : 0);
    for (int m : r.failed_modulos) printf(" %d", m);
    printf("\n");
}

int main(int argc, char **argv) {
    FILE *f = argc == 2 ? fopen(argv[1], "rb") : nullptr;
    int32_t head[6];
    if (!f || fread(head, sizeof(int32_t), 6, f) != 6) return 2;
    const int rh = head[0], nh = head[1], g = head[2], max_modulo = head[3], K = head[4], has_coef = head[5];
    std::vector<int32_t> cells((size_t)rh * nh);
    if (fread(cells.data(), sizeof(int32_t), cells.size(), f) != cells.size()) return 2;
    ldpc::Matrix proto(rh, nh);
    size_t E = 0;
    for (int i = 0; i < rh * nh; ++i) E += (proto.v[(size_t)i] = cells[(size_t)i]) > 0;
    std::vector<std::vector<int>> V((size_t)K, std::vector<int>(E)), Cf((size_t)K, std::vector<int>(E));
    for (int k = 0; k < K; ++k) {
        std::vector<int32_t> row(E);
        if (fread(row.data(), sizeof(int32_t), E, f) != E) return 2;
        V[(size_t)k].assign(row.begin(), row.end());
        if (has_coef) {
            if (fread(row.data(), sizeof(int32_t), E, f) != E) return 2;
            Cf[(size_t)k].assign(row.begin(), row.end());
        }
    }
    fclose(f);
    try {
        if (!has_coef) {
            const std::vector<ldpc::voltage_check_result> all = ldpc::check_voltages(proto, g, V, max_modulo);
            for (ldpc::voltage_check_result const &r : all) print("v", r, max_modulo);
            print("single", ldpc::check_voltages(proto, g, V[0], max_modulo), max_modulo);
            return 0;
        }
        for (int k = 0; k < K; ++k) {
            try {
                print("v", ldpc::check_voltages_and_coefs(proto, g, V[(size_t)k], max_modulo, Cf[(size_t)k], 16), max_modulo);
            } catch (const std::runtime_error &e) {
                printf("die %s\n", e.what());
            }
        }
        bool threw = false;
        try {
            ldpc::check_voltages_and_coefs(proto, g, V, max_modulo, Cf, 16);
        } catch (const std::runtime_error &) {
            threw = true;
        }
        printf("batch %d\n", threw ? 1 : 0);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
