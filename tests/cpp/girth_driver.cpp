// Test driver of include/ldpc/girth.h: reads C, rh, nh, M, then 20 + 20 bounds (a first entry of -1: that bound is not applied),
// then C * rh * nh shifts, all int32, from the file named on the command line; prints per code
//   one <c> girth ACE[4] spectrum[4]       ldpc::trace_matrix on the code alone
//   set <c> girth ACE[4] spectrum[4]       ldpc::trace_matrices on the whole vector, no bounds
//   bounded <c> girth ACE[4] spectrum[4]   ldpc::trace_matrices with the bounds: the ggp variant's signed girth
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ldpc/bp_simulation.h"
#include "ldpc/girth.h"

static void show(const char *tag, int c, int girth, const std::vector<int> &ace, const std::vector<int> &spectrum) {
    printf("%s %d %d", tag, c, girth);
    for (int v : ace) printf(" %d", v);
    for (int v : spectrum) printf(" %d", v);
    printf("\n");
}

int main(int argc, char **argv) {
    FILE *f = argc == 2 ? fopen(argv[1], "rb") : nullptr;
    int32_t head[4];
    if (!f || fread(head, sizeof(int32_t), 4, f) != 4) return 2;
    const int C = head[0], rh = head[1], nh = head[2], M = head[3];
    std::vector<int32_t> bounds(40), cells((size_t)C * rh * nh);
    if (fread(bounds.data(), sizeof(int32_t), 40, f) != 40 || fread(cells.data(), sizeof(int32_t), cells.size(), f) != cells.size()) return 2;
    fclose(f);
    std::vector<ldpc::Matrix> codes;
    for (int c = 0; c < C; ++c) {
        ldpc::Matrix H(rh, nh);
        for (int i = 0; i < rh * nh; ++i) H.v[(size_t)i] = cells[(size_t)c * rh * nh + i];
        codes.push_back(H);
    }
    try {
        for (int c = 0; c < C; ++c) {
            std::vector<int> ace, spectrum;
            const int girth = ldpc::trace_matrix(codes[(size_t)c], M, ldpc::kGirthGTARGET, ace, spectrum);
            show("one", c, girth, ace, spectrum);
        }
        std::vector<std::vector<int>> ace, spectrum;
        std::vector<int> girth = ldpc::trace_matrices(codes, M, ldpc::kGirthGTARGET, ace, spectrum);
        for (int c = 0; c < C; ++c) show("set", c, girth[(size_t)c], ace[(size_t)c], spectrum[(size_t)c]);
        const std::vector<int> mn(bounds.begin(), bounds.begin() + 20), mx(bounds.begin() + 20, bounds.end());
        girth = ldpc::trace_matrices(codes, M, ldpc::kGirthGTARGET, ace, spectrum, &mn, &mx);
        for (int c = 0; c < C; ++c) show("bounded", c, girth[(size_t)c], ace[(size_t)c], spectrum[(size_t)c]);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
