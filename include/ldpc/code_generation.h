/*
 * ldpc/code_generation.h -- upstream's generate_code (code_generation.h / code_generation.cpp:35-115) on the MI355X
 * (ldpc_hip_label_codes, csrc/ldpc_label.hpp):
 *
 *   ldpc::generate_code(code_matrix, target_girth, max_module, max_codes_to_test, result_matrix)
 *       labels the protograph code_matrix (0 = empty, 1 = edge with a random shift, any other positive value = edge with shift 0)
 *       with shifts below max_module so that no closed walk shorter than target_girth closes in the lifted graph and no two columns
 *       of the result are equal; tests at most max_codes_to_test random labellings; true and the labelling in result_matrix (-1 =
 *       empty) on success, false otherwise -- also, before any draw, when the protograph itself does not allow the girth.
 *
 * The draws come from the process-wide generator of ldpc/bp_simulation.h (ldpc::next_random_int, ldpc::reset_random,
 * ldpc::initial_random_seed), which is left exactly where upstream's loop leaves its own: upstream's search loop (generate_code;
 * reset_random; bp_simulation; ...) can be written unchanged.  Upstream's progress printfs and console hooks are not reproduced.
 * Generic over the matrix type (n_rows(), n_cols(), operator()(i, j), copy assignment).  Errors of the library are thrown as
 * std::runtime_error with its message.
 */
#ifndef LDPC_COMPAT_CODE_GENERATION_H_
#define LDPC_COMPAT_CODE_GENERATION_H_

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "ldpc_hip.h"
#include "ldpc/bp_simulation.h"

namespace ldpc {

template <class Mat>
bool generate_code(Mat const &code_matrix, int target_girth, int max_module, int max_codes_to_test, Mat &result_matrix, int device = 0) {
    const int rh = code_matrix.n_rows(), nh = code_matrix.n_cols();
    std::vector<int16_t> proto((size_t)rh * nh), hd((size_t)rh * nh);
    for (int i = 0; i < rh; ++i)
        for (int j = 0; j < nh; ++j) {
            const int v = code_matrix(i, j);
            proto[(size_t)i * nh + j] = (int16_t)(v <= 0 ? 0 : v == 1 ? 1 : 2);   // upstream reads `> 0` and `!= 1` only
        }
    if (max_codes_to_test < 1) {   // upstream's loop does not run; the equations alone decide nothing then
        return false;
    }
    // the protograph's own girth first: upstream returns before it touches the generator
    int tree_girth = 0;
    if (ldpc_hip_label_equations_host(rh, nh, proto.data(), target_girth, &tree_girth, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0)
        throw std::runtime_error(std::string("ldpc::generate_code: ") + ldpc_hip_last_error());
    if (tree_girth < target_girth) return false;
    uint32_t words[624], next[624];
    int pos = 0, next_pos = 0, found = 0;
    long long index = 0, tested = 0;
    if (!mt_export(random_generator(), words, pos)) throw std::runtime_error("ldpc::generate_code: the state of std::mt19937 could not be read");
    if (ldpc_hip_label_codes(rh, nh, proto.data(), target_girth, max_module, max_codes_to_test, 1, words, pos, device, hd.data(), &index, &found, &tested,
                             &tree_girth, next, &next_pos) != 0)
        throw std::runtime_error(std::string("ldpc::generate_code: ") + ldpc_hip_last_error());
    if (!mt_import(random_generator(), next, next_pos)) throw std::runtime_error("ldpc::generate_code: the generator state could not be handed back to std::mt19937");
    if (!found) return false;
    result_matrix = code_matrix;
    for (int i = 0; i < rh; ++i)
        for (int j = 0; j < nh; ++j) result_matrix(i, j) = hd[(size_t)i * nh + j];
    return true;
}

}  // namespace ldpc
#endif  // LDPC_COMPAT_CODE_GENERATION_H_
