// ldpc_sim.cpp -- `ldpc_sim simulation <scenario.jsonx> <result.jsonx>`: upstream's `simulation` driver
// (main_simulation.cpp:222-679) on top of this repository's bp_simulation (GPU decoders, upstream's noise order), for binary codes
// and for codes over GF(q) (`_q_mod` > 2: decoder 6 whatever `_decoder_type` says, :348-349; `coef` read, :359-360, and reduced,
// :416-434; ncols2convert = 0; `_q_mod` and `coef` in the result record, :608-614).
//
// What it keeps from upstream: the scenario fields (:260-283), the per-code fields (:343-364), the reduction of the shifts
// modulo the lifting with the special last parity column (:400-414), one generator reset per (code, SNR) so that all codes
// see the same noise (:483), the call into bp_simulation with reference_frame_error = error_minimization/threshold (:492-510),
// the result record written per code (:574-606).  What it does not do: marking files (`_marking` must be "skip"), GF(q) codes with
// --throughput (reported and skipped).  `girth` is copied through; upstream's own trace is behind --girth.
//
//   --throughput   device-side noise (counter-based Philox, not upstream's mt19937 stream): 10^6-10^7 frames/s per GPU; every
//                  modulation_type 0..4 and permutation_type 0..4; upstream's stopping rule frame by frame over the ordered records
//   --code-sets    exact mode only: codes that agree in shape, _decoder_type, _lifting, _punctured_blocks, _iterations and _SNRs are
//                  scored as ONE set per SNR (ldpc::bp_simulation_codes_exact: the noise of the reset generator drawn once, all codes
//                  of the group in one launch); the result file is the one without the flag except for `time`.  Codes over GF(q) of
//                  one q are grouped the same way into ldpc::bp_simulation_codes_gfq_exact
//   --snr-grid     implies the grouping of --code-sets; every binary group -- a group of ONE code too -- goes
//                  through one ldpc::bp_simulation_codes_grid_exact call for all its SNRs instead of one call per SNR: the (SNR, code)
//                  pairs are one set of work items over one draw of the reset generator's noise.  Up to 64 SNRs per code; a group with
//                  more, and a group over GF(q), runs per SNR as with --code-sets.  A line says whether the group ran as one call or, with
//                  host-drawn noise, as the per-SNR loop inside that function.  The result file differs from the one without the
//                  flag in `time` only; --code-sets alone behaves as it always did
//   --girth        upstream's trace_matrix per code (:148-205, :496) on the device (ldpc::trace_matrix, include/ldpc/girth.h): every
//                  record gains girth_, girth_ACE and girth_spectrum behind `girth` (:600-603).  The trace depends on the code alone,
//                  so it runs once per code and not once per SNR; with --code-sets once per group (ldpc::trace_matrices).  A code
//                  over GF(q) gets girth_ = 0 and zeros, as upstream traces none (:494-498).  Without the flag the output is
//                  byte for byte what it always was (and so is the usage text, which does not list the flag)
//   --device N     GPU ordinal;  --devices 0,1,2,3 | all   shard the frames over several GPUs (RCCL all-reduce of the counters)
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ldpc/bp_simulation.h"
#include "ldpc/decoders.h"
#include "ldpc/girth.h"
#include "ldpc/jsonx.h"
#include "ldpc_hip.h"

namespace {

[[noreturn]] void die(const std::string &msg) {
    fprintf(stderr, "%s\n", msg.c_str());
    exit(1);
}

// main_simulation.cpp:400-414: positive shifts are reduced modulo the lifting; a zero in the last column of the bidiagonal
// part (column index rows-1) becomes 1
void reduce_shifts(ldpc::Matrix &H, int M) {
    const int rows = H.n_rows(), cols = H.n_cols();
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < cols; ++j)
            if (H(i, j) > 0) {
                int t = H(i, j) % M;
                if (j == rows - 1) t = t == 0 ? 1 : t;
                H(i, j) = t;
            }
}

// main_simulation.cpp:416-434: where the code has a circulant, a coefficient > -1 is reduced modulo q, and 0 becomes q - 1
void reduce_coefs(ldpc::Matrix &HC, const ldpc::Matrix &H, int q_mod) {
    for (int i = 0; i < H.n_rows(); ++i)
        for (int j = 0; j < H.n_cols(); ++j)
            if (H(i, j) > -1 && HC(i, j) > -1) {
                HC(i, j) = HC(i, j) % q_mod;
                if (HC(i, j) == 0) HC(i, j) = q_mod - 1;
            }
}

// the `coef` matrix of a q-ary code record, in the shape of its `code`
ldpc::Matrix read_coefs(const jsonx::Value &code, size_t code_idx, int rows, int columns) {
    int r = 0, c = 0;
    const std::vector<int> cells = code.select("coef").as_int_matrix(r, c);
    if (r != rows || c != columns) die("code #" + std::to_string(code_idx) + ": 'coef' must have the shape of 'code'");
    ldpc::Matrix HC(r, c);
    HC.v = cells;
    return HC;
}

struct Pair { double ber, fer; };

// --code-sets: what decides whether two codes of the scenario can share a set
struct SetKey {
    int decoder_type, lifting, punctured_blocks, iterations;
    std::vector<double> snrs;
    int q_mod = 2;
    bool operator==(const SetKey &o) const {
        return decoder_type == o.decoder_type && lifting == o.lifting && punctured_blocks == o.punctured_blocks && iterations == o.iterations &&
               snrs == o.snrs && q_mod == o.q_mod;
    }
};
struct SetGroup {
    SetKey key;
    std::vector<size_t> members;        // indices into the scenario's `results`
    std::vector<ldpc::Matrix> codes;    // shifts already reduced
    std::vector<ldpc::Matrix> coefs;    // q_mod > 2: coefficients already reduced
};
struct SetResult { std::vector<Pair> per_snr; double secs = 0; };
struct GirthRecord {   // --girth: what main_simulation.cpp:496 leaves for :601-603
    bool traced = false;
    int girth = 0;
    std::vector<int> ace = std::vector<int>(ldpc::kGirthGTARGET, 0), spectrum = std::vector<int>(ldpc::kGirthGTARGET, 0);
};

// does a set context take these codes?  The host-side table builders apply the checks of the open entry points without a GPU.
bool set_takes(const SetGroup &g, int rows, int columns) {
    const int C = (int)g.codes.size(), dec = g.key.decoder_type, M = g.key.lifting;
    std::vector<int16_t> hd((size_t)C * rows * columns);
    for (int q = 0; q < C; ++q)
        for (int i = 0; i < rows * columns; ++i) hd[(size_t)q * rows * columns + i] = (int16_t)g.codes[(size_t)q].v[(size_t)i];
    long long len = 0;
    if (g.key.q_mod > 2) {   // the per-code rules of a GF(q) set do not depend on the column order left2right changes
        int q_bits = 0;
        while ((1 << q_bits) < g.key.q_mod) ++q_bits;
        if ((1 << q_bits) != g.key.q_mod) return false;
        std::vector<int16_t> hc(hd.size());
        for (int q = 0; q < C; ++q)
            for (int i = 0; i < rows * columns; ++i) hc[(size_t)q * rows * columns + i] = (int16_t)g.coefs[(size_t)q].v[(size_t)i];
        return ldpc_hip_codes_gfq_table_host(q_bits, rows, columns, M, hd.data(), hc.data(), C, nullptr, nullptr, 0, &len) == 0;
    }
    // the rule of open_code_set: a lifting above 512, or a set that the decoder's own entry point refuses for the size of its image
    // (LDPC_HIP_EUNSUPPORTED), goes to the global-memory tier of a set; a structural refusal stays one
    int rc = LDPC_HIP_EUNSUPPORTED;
    if (M <= 512) switch (dec) {
    case LDPC_HIP_MS_DEC: case LDPC_HIP_LMS_DEC: case LDPC_HIP_TASP_DEC:
        if (rows > 16 || (dec == LDPC_HIP_MS_DEC && columns > 32))   // the route open_code_set takes for these shapes
            rc = ldpc_hip_codes_table_wide_host(dec, rows, columns, M, hd.data(), C, nullptr, nullptr, 0, &len);
        else rc = ldpc_hip_codes_table_host(dec, rows, columns, M, hd.data(), C, nullptr, nullptr, 0, &len);
        break;
    case LDPC_HIP_IASP_DEC: rc = ldpc_hip_codes_table_host(dec, rows, columns, M, hd.data(), C, nullptr, nullptr, 0, &len); break;
    case LDPC_HIP_LCHE_DEC: rc = ldpc_hip_codes_table_lche_host(rows, columns, M, hd.data(), C, nullptr, nullptr, 0, &len); break;
    case LDPC_HIP_IMS_DEC: rc = ldpc_hip_codes_table_ims_host(rows, columns, M, hd.data(), C, nullptr, nullptr, 0, &len); break;
    case LDPC_HIP_SP_DEC: case LDPC_HIP_ASP_DEC:
        rc = ldpc_hip_codes_table_sp_host(dec, rows, columns, M, hd.data(), C, nullptr, nullptr, 0, &len);
        break;
    default: return false;   // BP_DEC and anything else: one code at a time
    }
    if (rc == LDPC_HIP_EUNSUPPORTED) rc = ldpc_hip_codes_table_global_host(dec, rows, columns, M, hd.data(), C, nullptr, nullptr, 0, &len);
    return rc == 0;
}

}  // namespace

int main(int argc, char **argv) {
    bool throughput = false, code_sets = false, girth = false, snr_grid = false;
    int random_codewords = 0;   // --throughput only: transmit this many random codewords encoded on the device instead of the all-zero word
    int device = 0;
    std::string devices_arg;
    std::vector<std::string> pos;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--throughput")) throughput = true;
        else if (!strcmp(argv[i], "--code-sets")) code_sets = true;
        else if (!strcmp(argv[i], "--snr-grid")) snr_grid = code_sets = true;
        else if (!strcmp(argv[i], "--girth")) girth = true;
        else if (!strcmp(argv[i], "--random-codewords") && i + 1 < argc) random_codewords = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--device") && i + 1 < argc) device = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--devices") && i + 1 < argc) devices_arg = argv[++i];
        else pos.push_back(argv[i]);
    }
    // jsonx utilities (no GPU needed): re-emit a file in canonical form / print one value addressed like upstream's select()
    if (pos.size() == 3 && pos[0] == "jsonx") {
        try {
            const std::string text = jsonx::parse_file(pos[1]).dump();
            FILE *f = fopen(pos[2].c_str(), "wt");
            if (!f) die("cannot write '" + pos[2] + "'");
            fwrite(text.data(), 1, text.size(), f);
            fclose(f);
        } catch (const jsonx::Error &e) { die(e.what()); }
        return 0;
    }
    if (pos.size() == 3 && pos[0] == "jsonx-get") {
        try {
            const jsonx::Value root = jsonx::parse_file(pos[1]);
            const jsonx::Value &v = root.select(pos[2]);
            if (v.type == jsonx::Value::STRING) printf("%s\n", v.str.c_str());
            else fputs(v.dump().c_str(), stdout);
        } catch (const jsonx::Error &e) { die(e.what()); }
        return 0;
    }
    if (pos.size() != 3 || pos[0] != "simulation")
        die("usage: ldpc_sim simulation <scenario file name> <result file name> [--throughput [--random-codewords N]] [--code-sets] [--device N | --devices 0,1,.. | --devices all]\n"
            "       ldpc_sim jsonx <in.jsonx> <out.jsonx>        re-emit in canonical form\n"
            "       ldpc_sim jsonx-get <in.jsonx> <path/to/field>  print one value (falls back to 'defaults' records)");

    if (!devices_arg.empty()) setenv("LDPC_HIP_DEVICES", devices_arg.c_str(), 1);
    const std::vector<int> devices = ldpc::devices_from_env(device);

    try {
        const jsonx::Value scenario = jsonx::parse_file(pos[1]);
        // 1. scenario (main_simulation.cpp:260-283)
        const int seed = (int)scenario.select("settings/random_seed").as_int();
        const long long num_experiments = scenario.select("settings/num_codewords").as_int();
        const int num_frame_errors = (int)scenario.select("settings/error_blocks").as_int();
        const std::string error_name = scenario.select("settings/error_minimization/name").as_string();
        const double error_rate_threshold = scenario.select("settings/error_minimization/threshold").as_double();
        if (error_name != "BER" && error_name != "FER") die("Unknown error name: '" + error_name + "'");
        const int modulation_type = (int)scenario.select("settings/modulation_type").as_int();
        const int permutation_type = (int)scenario.select("settings/permutation_type").as_int();
        const int permutation_block = (int)scenario.select("settings/permutation_block").as_int();
        const int permutation_inter = (int)scenario.select("settings/permutation_inter").as_int();
        printf("scenario OK\n");

        const jsonx::Value &codes = scenario.select("results");
        if (codes.type != jsonx::Value::ARRAY) die("'results' must be an array of code records");

        jsonx::Value out;
        out.set("settings", scenario.select("settings"));
        jsonx::Value &results = out.set("results", jsonx::Value::array());

        // --code-sets: the groups are scored first, each SNR of a group in one bp_simulation_codes_exact call after reset_random(); the
        // loop below then takes a grouped code's numbers from here and runs every other code as it always did
        std::vector<SetResult> from_set(codes.items.size());
        std::vector<GirthRecord> traced(codes.items.size());
        if (code_sets && !throughput && modulation_type == 0 && permutation_type == 0) {
            std::vector<SetGroup> groups;
            int rows0 = -1, columns0 = -1;
            for (size_t code_idx = 0; code_idx < codes.items.size(); ++code_idx) {
                const jsonx::Value &code = codes.items[code_idx];
                const int q_mod = code.has("_q_mod") ? (int)code.select("_q_mod").as_int() : 2;
                if (code.select("_marking").as_string() != "skip") break;   // the loop below dies there: nothing behind it is simulated
                int r = 0, c = 0;
                const std::vector<int> cells = code.select("code").as_int_matrix(r, c);
                if (rows0 == -1) { rows0 = r; columns0 = c; }
                else if (rows0 != r || columns0 != c) continue;
                SetKey key{q_mod > 2 ? LDPC_HIP_FHT_DEC : (int)code.select("_decoder_type").as_int(), (int)code.select("_lifting").as_int(),
                           (int)code.select("_punctured_blocks").as_int(), (int)code.select("_iterations").as_int(), code.select("_SNRs").as_doubles(),
                           q_mod};
                ldpc::Matrix H(r, c);
                H.v = cells;
                reduce_shifts(H, key.lifting);
                ldpc::Matrix HC;
                if (q_mod > 2) { HC = read_coefs(code, code_idx, r, c); reduce_coefs(HC, H, q_mod); }
                size_t g = 0;
                while (g < groups.size() && !(groups[g].key == key)) ++g;
                if (g == groups.size()) { groups.emplace_back(); groups[g].key = key; }
                groups[g].members.push_back(code_idx);
                groups[g].codes.push_back(H);
                if (q_mod > 2) groups[g].coefs.push_back(HC);
            }
            for (const SetGroup &g : groups) {
                const bool grid = snr_grid && g.key.q_mod <= 2 && !g.key.snrs.empty() && g.key.snrs.size() <= 64;
                if ((g.members.size() < 2 && !grid) || g.key.punctured_blocks < 0 || g.key.punctured_blocks >= columns0 || !set_takes(g, rows0, columns0)) continue;
                const auto t0 = std::chrono::steady_clock::now();
                for (size_t m : g.members) from_set[m].per_snr.resize(g.key.snrs.size());
                if (grid) {
                    printf("set of %zu codes from code #%zu on, grid of %zu SNRs\n", g.members.size(), g.members[0], g.key.snrs.size());
                    ldpc::initial_random_seed = seed;
                    ldpc::reset_random();                                                                                     // :483, the state every (code, SNR) pair starts from
                    const long long runs_before = ldpc::codes_grid_device_runs().load();
                    const std::vector<std::vector<std::pair<double, double>>> p = ldpc::bp_simulation_codes_grid_exact(
                        g.codes, g.key.lifting, g.key.iterations, num_frame_errors, (int)num_experiments, g.key.snrs,
                        std::vector<double>(g.key.snrs.size(), error_rate_threshold), g.key.decoder_type, modulation_type, permutation_type,
                        g.key.punctured_blocks, 0, devices[0]);
                    for (size_t s = 0; s < g.key.snrs.size(); ++s)
                        for (size_t q = 0; q < g.members.size(); ++q) from_set[g.members[q]].per_snr[s] = {p[s][q].first, p[s][q].second};
                    printf("  %s\n", ldpc::codes_grid_device_runs().load() > runs_before ? "one grid call" : "per-SNR calls (host-drawn noise)");
                } else for (size_t s = 0; s < g.key.snrs.size(); ++s) {
                    printf("set of %zu codes from code #%zu on, SNR = %6.3f\n", g.members.size(), g.members[0], g.key.snrs[s]);
                    ldpc::initial_random_seed = seed;
                    ldpc::reset_random();                                                                                     // :483 all codes are tested with same noise
                    std::vector<ldpc::Matrix> coefs = g.coefs;   // the call rewrites them (ncols2convert = 0: with the same values)
                    const std::vector<std::pair<double, double>> p =
                        g.key.q_mod > 2 ? ldpc::bp_simulation_codes_gfq_exact(g.key.q_mod, g.codes, coefs, 0, g.key.lifting, g.key.iterations, num_frame_errors,
                                                                              (int)num_experiments, g.key.snrs[s], error_rate_threshold,
                                                                              g.key.punctured_blocks, 0, devices[0])
                                        : ldpc::bp_simulation_codes_exact(
                        g.codes, g.key.lifting, g.key.iterations, num_frame_errors, (int)num_experiments, g.key.snrs[s], error_rate_threshold,
                        g.key.decoder_type, modulation_type, permutation_type, permutation_block, permutation_inter, g.key.punctured_blocks, 0, devices[0]);
                    for (size_t q = 0; q < g.members.size(); ++q) from_set[g.members[q]].per_snr[s] = {p[q].first, p[q].second};
                }
                const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                for (size_t m : g.members) from_set[m].secs = secs / (double)g.members.size();
                if (girth && g.key.q_mod <= 2) {   // the whole group in one ldpc_hip_girth_codes call
                    std::vector<std::vector<int>> ace, spectrum;
                    const std::vector<int> girths = ldpc::trace_matrices(g.codes, g.key.lifting, ldpc::kGirthGTARGET, ace, spectrum, nullptr, nullptr, devices[0]);
                    for (size_t q = 0; q < g.members.size(); ++q) traced[g.members[q]] = {true, girths[q], ace[q], spectrum[q]};
                }
            }
        }

        int rows = -1, columns = -1;
        for (size_t code_idx = 0; code_idx < codes.items.size(); ++code_idx) {
            const jsonx::Value &code = codes.items[code_idx];
            const std::vector<double> snrs = code.select("_SNRs").as_doubles();
            const int q_mod = code.has("_q_mod") ? (int)code.select("_q_mod").as_int() : 2;
            const int decoder_type = q_mod > 2 ? LDPC_HIP_FHT_DEC : (int)code.select("_decoder_type").as_int();   // :348-349
            const int lifting = (int)code.select("_lifting").as_int();
            const int punctured_blocks = (int)code.select("_punctured_blocks").as_int();
            const int iterations = (int)code.select("_iterations").as_int();
            const std::string marking = code.select("_marking").as_string();
            if (q_mod > 2 && throughput) { printf("code #%zu: GF(%d) codes (FHT decoder) are not built in ldpc-lib_amd, skipped\n", code_idx, q_mod); continue; }
            if (marking != "skip") die("code #" + std::to_string(code_idx) + ": marking files are not built (\"_marking\" must be \"skip\")");
            int r = 0, c = 0;
            const std::vector<int> cells = code.select("code").as_int_matrix(r, c);
            if (rows == -1) { rows = r; columns = c; }
            else if (rows != r || columns != c) { printf("Warning: unequal matrices in the input!\n"); continue; }   // :366-370
            ldpc::Matrix H(r, c);
            H.v = cells;
            reduce_shifts(H, lifting);
            ldpc::Matrix HC;
            if (q_mod > 2) { HC = read_coefs(code, code_idx, r, c); reduce_coefs(HC, H, q_mod); }                                // :359-360, :416-434
            const double bitrate = (double)(columns - rows) / (columns - punctured_blocks);                                  // :372
            GirthRecord &trace = traced[code_idx];
            if (girth && q_mod <= 2 && !trace.traced) {                                                                      // :494-498
                trace.girth = ldpc::trace_matrix(H, lifting, ldpc::kGirthGTARGET, trace.ace, trace.spectrum, devices[0]);
                trace.traced = true;
            }

            std::vector<double> ber(snrs.size()), fer(snrs.size()), esn0(snrs.size());
            const auto t0 = std::chrono::steady_clock::now();
            for (size_t s = 0; s < snrs.size(); ++s) {
                if (s == 0) printf("====================================================\n");
                printf("code #%zu, original matrix is being processed, SNR = %6.3f\n", code_idx, snrs[s]);
                esn0[s] = snrs[s] + 10.0 * std::log10(2.0 * bitrate);                                                        // :481
                Pair res;
                if (!from_set[code_idx].per_snr.empty()) {
                    res = from_set[code_idx].per_snr[s];
                } else if (throughput) {
                    const std::pair<double, double> p = ldpc::bp_simulation_throughput_t<ldpc::Matrix, ldpc::OwnRngEnv>(
                        2, H, lifting, iterations, num_frame_errors, num_experiments, snrs[s], error_rate_threshold, decoder_type, modulation_type,
                        permutation_type, permutation_block, permutation_inter, punctured_blocks, 0, (unsigned long long)seed, devices, nullptr, 65536, nullptr,
                        random_codewords);
                    res = {p.first, p.second};
                } else if (q_mod > 2) {
                    ldpc::initial_random_seed = seed;
                    ldpc::reset_random();                                                                                     // :483
                    const std::pair<double, double> p = ldpc::bp_simulation_gfq_t<ldpc::Matrix, ldpc::OwnRngEnv>(
                        q_mod, H, HC, 0, lifting, iterations, num_frame_errors, (int)num_experiments, snrs[s], error_rate_threshold, decoder_type,
                        modulation_type, permutation_type, punctured_blocks, 0, nullptr, devices[0]);
                    res = {p.first, p.second};
                } else {
                    ldpc::initial_random_seed = seed;
                    ldpc::reset_random();                                                                                     // :483 all codes are tested with same noise
                    ldpc::Matrix coef;
                    const std::pair<double, double> p = ldpc::bp_simulation_t<ldpc::Matrix, ldpc::OwnRngEnv>(
                        2, H, lifting, iterations, num_frame_errors, (int)num_experiments, snrs[s], error_rate_threshold, decoder_type,
                        modulation_type, permutation_type, punctured_blocks, 0, nullptr, devices, 4096, permutation_block, permutation_inter);
                    (void)coef;
                    res = {p.first, p.second};
                }
                if (res.ber < 0 || res.fer < 0) res = {1.0, 1.0};                                                            // :527-531
                ber[s] = res.ber; fer[s] = res.fer;
            }
            const double secs = from_set[code_idx].per_snr.empty() ? std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()
                                                                   : from_set[code_idx].secs;

            printf("        |     FER     |     BER\n");
            for (size_t s = 0; s < snrs.size(); ++s) printf("%7.3f | %10.8f  | %10.8f\n", snrs[s], fer[s], ber[s]);
            printf("--------\n");

            // :574-606 the record upstream appends per code
            jsonx::Value log;
            log.set("SNR_per_bit___", jsonx::Value::numbers(snrs));
            log.set("SNR_per_symbol", jsonx::Value::numbers(esn0));
            log.set("BER", jsonx::Value::numbers(ber));
            log.set("FER", jsonx::Value::numbers(fer));
            jsonx::Value d;
            d.set("_decoder_name", jsonx::Value::string(decoder_type >= 0 && decoder_type < 10 ? DEC_FULL_NAME[decoder_type] : "?"));
            d.set("_decoder_type", jsonx::Value::number((long long)decoder_type));
            d.set("_lifting", jsonx::Value::number((long long)lifting));
            d.set("_SNRs", jsonx::Value::numbers(snrs));
            d.set("_punctured_blocks", jsonx::Value::number((long long)punctured_blocks));
            d.set("_iterations", jsonx::Value::number((long long)iterations));
            d.set("_marking", jsonx::Value::string("skip"));
            d.set("code_bitrate", jsonx::Value::number(bitrate));
            d.set("code", jsonx::Value::matrix(r, c, H.v));
            for (const char *key : {"column_weights", "row_weights", "girth"})
                if (const jsonx::Value *v = code.find(key)) d.set(key, *v);
            if (girth) {                                                                                                     // :601-603
                d.set("girth_", jsonx::Value::number((long long)trace.girth));
                d.set("girth_ACE", jsonx::Value::numbers(std::vector<long long>(trace.ace.begin(), trace.ace.end())));
                d.set("girth_spectrum", jsonx::Value::numbers(std::vector<long long>(trace.spectrum.begin(), trace.spectrum.end())));
            }
            for (const char *key : {"config_index", "matrix_index", "code_index"})
                if (const jsonx::Value *v = code.find(key)) d.set(key, *v);
            d.set("simulation_logs", jsonx::Value::array({log}));
            if (q_mod > 2) {                                                                                                 // :608-614
                d.set("_q_mod", jsonx::Value::number((long long)q_mod));
                d.set("coef", jsonx::Value::matrix(r, c, HC.v));
            }
            d.set("time", jsonx::Value::number(std::round(secs * 1000.0) / 1000.0));
            results.items.push_back(std::move(d));
        }
        FILE *f = fopen(pos[2].c_str(), "wt");
        if (!f) die("cannot write '" + pos[2] + "'");
        const std::string text = out.dump();
        fwrite(text.data(), 1, text.size(), f);
        fclose(f);
    } catch (const jsonx::Error &e) {
        die(e.what());
    } catch (const std::runtime_error &e) {   // ldpc::trace_matrix
        die(e.what());
    }
    return 0;
}
