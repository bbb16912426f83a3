// The host half of csrc/ldpc_label.hpp as a program of its own, for a sanitizer build (-fsanitize=address,undefined): reads rh, nh,
// target_girth and rh * nh protograph entries from standard input, builds the equation table and prints
//   <equations> <tree girth> <random edges> <terms> <never accepts>
// after walking the whole table once (every index it holds is used to address the arrays it refers to).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ldpc_label.hpp"

int main() {
    int rh, nh, g;
    if (scanf("%d %d %d", &rh, &nh, &g) != 3 || rh < 1 || nh < 1) return 2;
    std::vector<int16_t> proto((size_t)rh * nh);
    for (int16_t &v : proto) {
        int x;
        if (scanf("%d", &x) != 1) return 2;
        v = (int16_t)x;
    }
    ldpc_label::Table t;
    if (!ldpc_label::equations(rh, nh, proto.data(), g, t)) {
        printf("refused %lld %s\n", t.refused_count, t.refused_what);
        return 3;
    }
    std::vector<long long> weight((size_t)t.n_random + 1, 0);
    for (int e = 0; e < t.n_equations; ++e)
        for (int32_t k = t.eq_begin[(size_t)e]; k < t.eq_begin[(size_t)e + 1]; ++k) weight[(size_t)t.term_edge[(size_t)k]] += t.term_mult[(size_t)k];
    std::vector<int> by_col((size_t)nh * rh);
    for (size_t i = 0; i < by_col.size(); ++i) by_col[i] = t.cell[i] == -1 ? -1 : t.cell[i] == -2 ? 0 : (int)(weight[(size_t)t.cell[i]] & 7);
    const bool same = ldpc_label::same_columns(rh, nh, by_col);
    printf("%d %d %d %zu %d %d\n", t.n_equations, t.tree_girth, t.n_random, t.term_edge.size(), t.never_accepts ? 1 : 0, same ? 1 : 0);
    return 0;
}
