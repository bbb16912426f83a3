/*
 * ldpc/equations.h -- upstream's voltage check (equations.h / equations.cpp:150-267: equation_builder::check_voltages and
 * check_voltages_and_coefs, what its `ggp` command turns on) on the MI355X (ldpc_hip_check_voltages, csrc/ldpc_voltage.hpp):
 *
 *   ldpc::voltage_check_result        upstream's four fields and check_modulo
 *   ldpc::check_voltages(code_matrix, target_girth, voltages, max_modulo)
 *   ldpc::check_voltages_and_coefs(code_matrix, target_girth, voltages, max_modulo, coefs, q_mod)
 *
 * code_matrix is the protograph: any positive entry is an edge; a labelling holds one voltage per edge, column by column with the rows
 * ascending, in 0 .. 32767.  Each function takes one labelling (std::vector<int>) or a batch (std::vector<std::vector<int>>), which is
 * one device call.  Upstream builds the equations once (equation_builder(graph, target_girth)) and calls the check on the object; here
 * the protograph and the girth are arguments of the check.  max_modulo (1 .. 65535) has no default: upstream's unbounded call
 * check_voltages(v) is the bounded one wherever no |sum| exceeds max_modulo.  With a first_failed_equation other than -1 upstream leaves
 * the other fields uninitialised; here they are 0 and the set is empty.  Where upstream exits -- a zero voltage sum whose coefficient
 * sum is not zero reaches divisors(0) -- the functions throw std::runtime_error with upstream's message.  A batch throws as a whole
 * when any of its labellings is such a one, and the other results are lost: a caller who wants every labelling's outcome uses the
 * one-labelling overload, or the status array of ldpc_hip_check_voltages.  q_mod is not read, as upstream does not read it.  Generic over the matrix type (n_rows(), n_cols(), operator()(i, j)).  Errors of the library are thrown as
 * std::runtime_error with its message.
 */
#ifndef LDPC_COMPAT_EQUATIONS_H_
#define LDPC_COMPAT_EQUATIONS_H_

#include <cstdint>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "ldpc_hip.h"

namespace ldpc {

struct voltage_check_result {
    int first_failed_equation = 0;
    std::set<int> failed_modulos;
    int min_ok_modulo = 0;
    int max_nonok_modulo = 0;

    bool check_modulo(int modulo) const {
        return first_failed_equation == -1 && modulo >= min_ok_modulo && (modulo > max_nonok_modulo || failed_modulos.count(modulo) == 0);
    }
};

// the members <= max_modulo of a bitmap row of ldpc_hip_check_voltages, as upstream's set
inline std::set<int> failed_set(const uint64_t *row, int max_modulo) {
    std::set<int> out;
    for (int m = 1; m <= max_modulo; ++m)
        if ((row[m >> 6] >> (m & 63)) & 1u) out.insert(out.end(), m);
    return out;
}

// one device call for the batch; coefs == nullptr: the binary check
template <class Mat>
std::vector<voltage_check_result> voltage_check_batch(Mat const &code_matrix, int target_girth, std::vector<std::vector<int>> const &voltages,
                                                      int max_modulo, std::vector<std::vector<int>> const *coefs, int device) {
    const int rh = code_matrix.n_rows(), nh = code_matrix.n_cols();
    std::vector<int16_t> proto((size_t)rh * nh);
    size_t E = 0;
    for (int i = 0; i < rh; ++i)
        for (int j = 0; j < nh; ++j) E += (proto[(size_t)i * nh + j] = (int16_t)(code_matrix(i, j) > 0 ? 1 : 0));
    const size_t K = voltages.size();
    if (coefs && coefs->size() != K) throw std::runtime_error("ldpc::check_voltages_and_coefs: as many coefficient vectors as labellings are needed");
    std::vector<int32_t> v(K * E), c(coefs ? K * E : 0);
    for (size_t k = 0; k < K; ++k) {
        if (voltages[k].size() != E || (coefs && (*coefs)[k].size() != E))
            throw std::runtime_error("ldpc::check_voltages: labelling " + std::to_string(k) + " does not hold one value per edge (" + std::to_string(E) + ")");
        for (size_t e = 0; e < E; ++e) {
            v[k * E + e] = voltages[k][e];
            if (coefs) c[k * E + e] = (*coefs)[k][e];
        }
    }
    const size_t W = max_modulo >= 1 && max_modulo <= 65535 ? (size_t)max_modulo / 64 + 1 : 1;
    std::vector<int32_t> status(K), min_ok(K), max_nonok(K), max_abs(K);
    std::vector<uint64_t> failed(K * W);
    if (ldpc_hip_check_voltages(rh, nh, proto.data(), target_girth, max_modulo, v.data(), coefs ? c.data() : nullptr, (long long)K, device, status.data(),
                                min_ok.data(), max_nonok.data(), max_abs.data(), failed.data(), nullptr, nullptr) != 0)
        throw std::runtime_error(std::string("ldpc::check_voltages: ") + ldpc_hip_last_error());
    std::vector<voltage_check_result> out(K);
    for (size_t k = 0; k < K; ++k) {
        if (status[k] == 2) throw std::runtime_error("global_divisor_table is called with the argument 0");
        out[k].first_failed_equation = status[k] == 0 ? -1 : 0;
        out[k].min_ok_modulo = min_ok[k];
        out[k].max_nonok_modulo = max_nonok[k];
        out[k].failed_modulos = failed_set(&failed[k * W], max_modulo);
    }
    return out;
}

template <class Mat>
std::vector<voltage_check_result> check_voltages(Mat const &code_matrix, int target_girth, std::vector<std::vector<int>> const &voltages, int max_modulo,
                                                 int device = 0) {
    return voltage_check_batch(code_matrix, target_girth, voltages, max_modulo, nullptr, device);
}

template <class Mat>
voltage_check_result check_voltages(Mat const &code_matrix, int target_girth, std::vector<int> const &voltages, int max_modulo, int device = 0) {
    return voltage_check_batch(code_matrix, target_girth, std::vector<std::vector<int>>(1, voltages), max_modulo, nullptr, device)[0];
}

template <class Mat>
std::vector<voltage_check_result> check_voltages_and_coefs(Mat const &code_matrix, int target_girth, std::vector<std::vector<int>> const &voltages,
                                                           int max_modulo, std::vector<std::vector<int>> const &coefs, int /*q_mod*/, int device = 0) {
    return voltage_check_batch(code_matrix, target_girth, voltages, max_modulo, &coefs, device);
}

template <class Mat>
voltage_check_result check_voltages_and_coefs(Mat const &code_matrix, int target_girth, std::vector<int> const &voltages, int max_modulo,
                                              std::vector<int> const &coefs, int /*q_mod*/, int device = 0) {
    const std::vector<std::vector<int>> c(1, coefs);
    return voltage_check_batch(code_matrix, target_girth, std::vector<std::vector<int>>(1, voltages), max_modulo, &c, device)[0];
}

}  // namespace ldpc
#endif  // LDPC_COMPAT_EQUATIONS_H_
