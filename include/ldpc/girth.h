/*
 * ldpc/girth.h -- upstream's girth / ACE trace of a base matrix on the MI355X (ldpc_hip_girth_codes, csrc/ldpc_girth.hpp):
 *
 *   ldpc::trace_matrix(H, M, gtarget, ACE, girth_spectrum)
 *       the static helper of main_simulation.cpp:148-205: trace_bound_pol_mon_pm with GMAX = 20, bounds every matrix passes
 *       (minACE = 0, maxACEspec = 10^8); returns the girth (21 when no cycle up to length 20 was found) and leaves the first
 *       GTARGET = 4 non-zero ACE / spectrum entries from the girth on in ACE / girth_spectrum, zeros behind them.
 *   ldpc::trace_matrices(codes, M, gtarget, ACE, girth_spectrum[, min_ACE, max_ACE_spec])
 *       the same for a vector of matrices of one shape in ONE call -- what a search does per candidate, for all candidates at
 *       once.  With the two bounds it is the variant of search_ggp/scenario_based_code_generation.cpp:1406-1480: their first
 *       entries override the defaults, a bound whose first entry is negative is not applied, and the girth of a matrix that
 *       failed the bounds is returned negated.
 * Generic over the matrix type (n_rows(), n_cols(), operator()(i, j)).  Errors are thrown as std::runtime_error with the library's
 * message.  The arithmetic is 32-bit like upstream's; a matrix on which it overflows (status bit 1 of the C-ABI) is an error here.
 */
#ifndef LDPC_COMPAT_GIRTH_H_
#define LDPC_COMPAT_GIRTH_H_

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "ldpc_hip.h"

namespace ldpc {

constexpr int kGirthGMAX = 20;     // trace_pm.h:8
constexpr int kGirthGTARGET = 4;   // trace_pm.h:9

template <class Mat>
std::vector<int> trace_matrices(std::vector<Mat> const &codes, int M, int gtarget, std::vector<std::vector<int>> &ACE,
                                std::vector<std::vector<int>> &girth_spectrum, const std::vector<int> *min_ACE = nullptr,
                                const std::vector<int> *max_ACE_spec = nullptr, int device = 0) {
    const int C = (int)codes.size();
    if (C == 0) return {};
    const int rh = codes[0].n_rows(), nh = codes[0].n_cols();
    std::vector<int16_t> hd((size_t)C * rh * nh);
    for (int c = 0; c < C; ++c) {
        if (codes[(size_t)c].n_rows() != rh || codes[(size_t)c].n_cols() != nh) throw std::runtime_error("ldpc::trace_matrices: the matrices differ in shape");
        for (int i = 0; i < rh; ++i)
            for (int j = 0; j < nh; ++j) {
                const int v = codes[(size_t)c](i, j);
                hd[((size_t)c * rh + i) * nh + j] = (int16_t)(v < -1 || v > 32767 ? -2 : v);   // -2: refused by the library as it is
            }
    }
    int32_t mn[kGirthGMAX], mx[kGirthGMAX];
    for (int i = 0; i < kGirthGMAX; ++i) { mn[i] = 0; mx[i] = 100000000; }
    if (min_ACE) for (size_t i = 0; i < min_ACE->size() && i < (size_t)kGirthGMAX; ++i) mn[i] = (*min_ACE)[i];
    if (max_ACE_spec) for (size_t i = 0; i < max_ACE_spec->size() && i < (size_t)kGirthGMAX; ++i) mx[i] = (*max_ACE_spec)[i];
    const bool signed_girth = min_ACE || max_ACE_spec;
    std::vector<int32_t> S((size_t)C * kGirthGMAX), SA((size_t)C * kGirthGMAX), status((size_t)C);
    if (ldpc_hip_girth_codes(rh, nh, M, hd.data(), C, kGirthGMAX, gtarget, mn[0] < 0 ? nullptr : mn, mx[0] < 0 ? nullptr : mx, device, S.data(),
                             SA.data(), status.data()) != 0)
        throw std::runtime_error(std::string("ldpc::trace_matrices: ") + ldpc_hip_last_error());
    std::vector<int> girth((size_t)C);
    ACE.assign((size_t)C, std::vector<int>());
    girth_spectrum.assign((size_t)C, std::vector<int>());
    for (int c = 0; c < C; ++c) {
        if (status[(size_t)c] & 2) throw std::runtime_error("ldpc::trace_matrices: a 32-bit sum overflowed on matrix " + std::to_string(c));
        int g = 0;
        int32_t a[kGirthGTARGET], s[kGirthGTARGET];
        if (ldpc_hip_trace_matrix_host(&S[(size_t)c * kGirthGMAX], &SA[(size_t)c * kGirthGMAX], kGirthGMAX, &g, a, s) != 0)
            throw std::runtime_error(std::string("ldpc::trace_matrices: ") + ldpc_hip_last_error());
        ACE[(size_t)c].assign(a, a + kGirthGTARGET);
        girth_spectrum[(size_t)c].assign(s, s + kGirthGTARGET);
        girth[(size_t)c] = signed_girth && !(status[(size_t)c] & 1) ? -g : g;
    }
    return girth;
}

template <class Mat>
int trace_matrix(Mat const &H, int M, int gtarget, std::vector<int> &ACE, std::vector<int> &girth_spectrum, int device = 0) {
    std::vector<std::vector<int>> a, s;
    const int girth = trace_matrices(std::vector<Mat>(1, H), M, gtarget, a, s, nullptr, nullptr, device)[0];
    ACE = a[0];
    girth_spectrum = s[0];
    return girth;
}

}  // namespace ldpc
#endif  // LDPC_COMPAT_GIRTH_H_
