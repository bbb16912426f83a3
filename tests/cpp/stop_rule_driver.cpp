// ldpc::replay_stop_rule (include/ldpc/bp_simulation.h) on records from a text file, fed in batches (tests/test_stop_rule_cpp_cpu.py).
// Input: n_frame_errors n_experiments reference_frame_error batch count, then `count` pairs "record iters".  Batches go in until the
// rule stops or the records run out.  Output: experiment nse nde nue sum_abs_iters, then the frames consumed from the last batch.
#include <cstdio>
#include <vector>

#include "ldpc/bp_simulation.h"

int main(int argc, char **argv) {
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    int n_frame_errors = 0;
    long long n_experiments = 0, batch = 0, count = 0;
    double reference_frame_error = 0;
    if (!f || fscanf(f, "%d %lld %lf %lld %lld", &n_frame_errors, &n_experiments, &reference_frame_error, &batch, &count) != 5 || batch < 1 || count < 0)
        return 2;
    std::vector<int> record((size_t)count), iters((size_t)count);
    for (long long i = 0; i < count; ++i)
        if (fscanf(f, "%d %d", &record[(size_t)i], &iters[(size_t)i]) != 2) return 2;
    fclose(f);
    ldpc::SimCounters k;
    ldpc::StopReplay r{0, false};
    long long errors_seen = 0;
    for (long long lo = 0; lo < count && !r.stop; lo += batch) {
        const long long B = batch < count - lo ? batch : count - lo;
        r = ldpc::replay_stop_rule(k, n_frame_errors, n_experiments, reference_frame_error, B,
                                   [&](long long i) { return std::make_pair((int32_t)record[(size_t)(lo + i)], iters[(size_t)(lo + i)]); },
                                   [&] { ++errors_seen; });
    }
    if (errors_seen != k.nde) return 3;   // on_error runs once per error frame
    printf("%lld %lld %lld %lld %lld %lld\n", k.experiment, k.nse, k.nde, k.nue, k.sum_abs_iters, r.used);
    return 0;
}
