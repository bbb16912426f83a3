/*
 * ldpc/bp_simulation.h -- the Monte-Carlo harness of upstream's bp_simulation.h:9-27 / bp_simulation.cpp:305-841
 * on the MI355X batch decoder, in EXACT-REPLAY mode: the channel noise is the stream of the same std::mt19937 in the same
 * draw order as upstream (commons_portable.cpp:138-178, bp_simulation.cpp:512,600-611) -- continued ON THE GPU by default
 * (ldpc_hip_mt_*: the generator's words, libstdc++'s polar method and glibc's log reproduced bit for bit, so only the 8-byte frame
 * records cross PCIe; LDPC_HIP_EXACT_NOISE=host draws on the host instead) -- frames are decoded in GPU batches, and upstream's
 * sequential stopping rule (bp_simulation.cpp:591,820) is replayed over the ordered per-frame results (ldpc::replay_stop_rule, the one
 * replay behind every harness of this header).  On an early stop the
 * generator is rolled back and re-advanced so that it is left exactly where upstream's frame-by-frame loop leaves it (later
 * callers draw from it: main_good_code_search.cpp:316).
 * Result, counters and generator state are identical to upstream's for q_mod == 2, modulation SKIP/QAM4,
 * permutation_type 0 (the only mode the shipped configurations use, files/default_constants.jsonx:6), and for q_mod > 2
 * (FHT_DEC, MODULATION_SKIP, permutation_type 0: bp_simulation_gfq_t below) up to the one spot upstream leaves undefined, the
 * message beyond its first eight symbols, which include/ldpc_hip.h defines.
 *
 *   ldpc::bp_simulation_throughput_t() the same harness in THROUGHPUT mode: channel noise drawn on the GPUs (counter-based Philox
 *                                      keyed by the global frame index), frames sharded over `devices` behind the C-ABI
 *                                      (ldpc_hip_open_multi: one host thread + stream per GPU, RCCL all-reduce of the counters),
 *                                      upstream's sequential stopping rule replayed over the ordered per-frame records;
 *   LDPC_HIP_DEVICES="0,1,2,3" | "all" selects the GPUs for every entry point below that takes no explicit list.
 *   ldpc::bp_simulation_t<Mat, Env>()  generic over the matrix type (needs n_rows(), n_cols(), operator()(i,j))
 *                                      and over the environment that owns the generator (see RngEnv below);
 *   ldpc::bp_simulation()              standalone: ldpc::Matrix + the library's own generator (ldpc::reset_random); q_mod > 2 goes
 *                                      to ldpc::bp_simulation_gfq_t<Mat, Env>(), upstream's q-ary harness on the GF(q) decoder.
 *   ldpc::bp_simulation_codes_exact()  a set of candidate codes of one shape in exact-replay mode: the stream of the reset generator
 *                                      drawn once and decoded by every candidate in one launch per batch (_t: generic as above).
 *   ldpc::bp_simulation_codes_grid() / _grid_exact()  a set of candidate codes at every point of an SNR grid over one noise draw.
 *   ldpc::bp_simulation_codes_gfq_exact()  the same for candidates over GF(q): upstream's q-ary set-up and an own word per candidate.
 * The drop-in definition of upstream's exact `bp_simulation(int, matrix<int> const&, matrix<int>&, ...)` symbol is
 * csrc/compat/bp_simulation_dropin.cpp (compiled inside the upstream tree).
 */
#ifndef LDPC_COMPAT_BP_SIMULATION_H_
#define LDPC_COMPAT_BP_SIMULATION_H_

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "ldpc_hip.h"
#include "ldpc/interleaver.h"

namespace ldpc {

enum { MODULATION_SKIP_ = 0, MODULATION_QAM4_ = 1 };  // modulation.h:4-11
enum { DEC_DECISION_HARD = 0 };                        // decoders.h:7 DEC_DECISION

struct Matrix {  // minimal stand-in for upstream's matrix<int> (data_structures.h:11-57)
    std::vector<int> v;
    int rows = 0, cols = 0;
    Matrix() {}
    Matrix(int r, int c, int init = 0) : v((size_t)r * c, init), rows(r), cols(c) {}
    int n_rows() const { return rows; }
    int n_cols() const { return cols; }
    int &operator()(int r, int c) { return v[(size_t)r * cols + c]; }
    int const &operator()(int r, int c) const { return v[(size_t)r * cols + c]; }
};

// The library's own generator with upstream's contract (commons_portable.cpp:138-178): one global mt19937, seeded
// from initial_random_seed at the first draw after reset_random(); a FRESH distribution object per call.
extern int initial_random_seed;
void reset_random();
std::mt19937 &random_generator();  // seeded on demand
int next_random_int(int min_inclusive, int max_exclusive);
double next_random_gaussian();

// GPUs to shard over: LDPC_HIP_DEVICES = "all" or a comma separated list of HIP ordinals; otherwise {fallback}.
inline std::vector<int> devices_from_env(int fallback = 0) {
    std::vector<int> d;
    if (const char *e = getenv("LDPC_HIP_DEVICES")) {
        const std::string v(e);
        if (v == "all") {
            for (int i = 0, n = ldpc_hip_device_count(); i < n; ++i) d.push_back(i);
        } else {
            size_t pos = 0;
            while (pos < v.size()) {
                size_t end = v.find(',', pos);
                if (end == std::string::npos) end = v.size();
                if (end > pos) d.push_back(atoi(v.substr(pos, end - pos).c_str()));
                pos = end + 1;
            }
        }
    }
    if (d.empty()) d.push_back(fallback);
    return d;
}

struct OwnRngEnv {
    static std::mt19937 &generator() { return random_generator(); }
    static double gaussian() { return next_random_gaussian(); }
    // bp_simulation.cpp:512 -> random_codeword() :142-191 draws (nh-rh)*M values of next_random_int(0,2) (:160-162);
    // the codeword itself is overwritten with zeros afterwards (:568), so only the draws matter here.
    template <class Mat>
    static void burn_codeword_draws(Mat const &H, int M) {
        for (long long i = 0, n = (long long)(H.n_cols() - H.n_rows()) * M; i < n; ++i) (void)next_random_int(0, 2);
    }
    [[noreturn]] static void fail(const char *msg) { fprintf(stderr, "%s\n", msg); exit(1); }  // die()
};

// std::mt19937 <-> (624 state words, index of the next word): libstdc++ streams exactly that (bits/random.tcc operator<<).  The
// export is checked against the generator's own next output; any other standard library fails the check and the harness then
// keeps the noise on the host.
inline unsigned mt_word_after(const uint32_t *w, int pos) {
    unsigned y;
    if (pos < 624) y = w[pos];
    else {   // the block is used up: the next word is x[624] of the sequence that starts with these 624 words
        const unsigned t = (w[0] & 0x80000000u) | (w[1] & 0x7fffffffu);
        y = w[397] ^ (t >> 1) ^ ((t & 1u) ? 0x9908b0dfu : 0u);
    }
    y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
    return y;
}
inline bool mt_export(const std::mt19937 &g, uint32_t w[624], int &pos) {
    std::ostringstream os;
    os << g;
    std::istringstream is(os.str());
    for (int i = 0; i < 624; ++i) { unsigned long v = 0; is >> v; w[i] = (uint32_t)v; }
    long p = -1;
    is >> p;
    if (is.fail() || p < 0 || p > 624) return false;
    pos = (int)p;
    std::mt19937 probe = g;
    return (unsigned)probe() == mt_word_after(w, pos);
}
inline bool mt_import(std::mt19937 &g, const uint32_t w[624], int pos) {
    std::ostringstream os;
    for (int i = 0; i < 624; ++i) os << w[i] << ' ';
    os << pos;
    std::istringstream is(os.str());
    std::mt19937 t;
    is >> t;
    if (is.fail()) return false;
    std::mt19937 probe = t;
    if ((unsigned)probe() != mt_word_after(w, pos)) return false;
    g = t;
    return true;
}

// Once per process: does the device-side stream reproduce THIS host's std::mt19937 + std::normal_distribution (libstdc++'s polar
// method, this libm's log / sqrt)?  4096 samples from a scratch generator, compared bit for bit.  If not -- another standard
// library, a libm whose log differs in the last place -- the harness keeps drawing on the host, so exact replay stays exact.
inline std::atomic<int> &device_stream_verdict() {   // -1: not checked yet in this process
    static std::atomic<int> verdict(-1);   // concurrent first calls both run the check and store the same answer
    return verdict;
}
inline bool device_stream_matches_host(ldpc_hip_ctx *ctx) {
    std::atomic<int> &verdict = device_stream_verdict();
    if (verdict.load() >= 0) return verdict.load() == 1;
    std::mt19937 probe(20240611u);
    uint32_t w[624];
    int pos = 0;
    bool same = mt_export(probe, w, pos) && ldpc_hip_mt_set_state(ctx, w, pos) == 0;
    std::vector<double> dev(4096);
    same = same && ldpc_hip_mt_normal_host(ctx, (long long)dev.size(), dev.data()) == 0;
    for (size_t i = 0; same && i < dev.size(); ++i) {
        std::normal_distribution<double> dist;   // a fresh one per sample, as upstream (commons_portable.cpp:174-178)
        const double h = dist(probe);
        same = std::memcmp(&h, &dev[i], sizeof h) == 0;
    }
    verdict.store(same ? 1 : 0);
    return same;
}

struct SimCounters { long long nse = 0, nde = 0, nue = 0, experiment = 0, sum_abs_iters = 0; };

// Upstream's sequential stopping rule (bp_simulation.cpp:591, :805-823) replayed over the ordered results of a batch of B frames, the
// one place where the harnesses below apply it.  frame(f) gives the record of frame f -- the low 30 bits hold the wrong information
// bits, bit 30 is set when any bit is wrong -- and its iteration count; on_error() runs at each error frame once it is counted (the
// show_process line).  used: the frames of the batch the rule consumed; stop: the run ends with the last of them.
struct StopReplay { long long used; bool stop; };
template <class Frame, class OnError>
inline StopReplay replay_stop_rule(SimCounters &k, int n_frame_errors, long long n_experiments, double reference_frame_error, long long B,
                                   Frame frame, OnError on_error) {
    const auto running = [&] { return k.nde < n_frame_errors && k.experiment <= n_experiments; };   // :591
    StopReplay r{0, false};
    while (!r.stop && r.used < B && running()) {
        const std::pair<int32_t, int> rec = frame(r.used);
        ++k.experiment; ++r.used;
        k.sum_abs_iters += rec.second < 0 ? -rec.second : rec.second;
        if (rec.first != 0) {                                                                        // :805
            k.nse += rec.first & ((1 << 30) - 1); ++k.nde;
            if (rec.second >= 0) ++k.nue;
            on_error();
            r.stop = k.nde >= 10 && (double)k.nde / k.experiment > 2.5 * reference_frame_error;      // :820
        }
    }
    r.stop = r.stop || !running();
    return r;
}

template <class Mat, class Env>
std::pair<double, double> bp_simulation_t(int q_mod, Mat const &H, int tailbite_length, int max_iterations,
                                          int n_frame_errors, int n_experiments, double snr,
                                          double reference_frame_error, int decoder_type, int modulation_type,
                                          int permutation_type, int punctured_blocks, int show_process,
                                          SimCounters *counters_out, const std::vector<int> &devices, long long max_batch = 4096,
                                          int permutation_block = 128, int permutation_inter = 1) {
    if (q_mod != 2) Env::fail("bp_simulation_t: binary codes (q_mod == 2) only; q_mod > 2 runs through bp_simulation() / bp_simulation_gfq_t");
    if (modulation_type != MODULATION_SKIP_ && modulation_type != MODULATION_QAM4_)
        Env::fail("bp_simulation: exact-replay mode supports MODULATION_SKIP and MODULATION_QAM4 (upstream's QAM16+ wiring "
                  "is broken, SURVEY Appendix B Q5/Q6; use the device-side chain ldpc_hip_awgn_qam16_llr_dev)");
    const int b = H.n_rows(), c = H.n_cols(), M = tailbite_length;
    const int r = b * M, n = c * M;

    std::vector<int16_t> hd((size_t)b * c);
    for (int i = 0; i < b; ++i) for (int j = 0; j < c; ++j) hd[(size_t)i * c + j] = (int16_t)H(i, j);  // :359-361
    ldpc_hip_multi *ctx = nullptr;   // one DEC_STATE per GPU; the batch of a round is cut into contiguous slices
    if (devices.empty()) Env::fail("bp_simulation: empty device list");
    // a code search calls this once per candidate matrix (main_good_code_search.cpp:320): never wait for hiprtc here, start on the
    // table-driven / shape-unlimited kernel and move to the code-specialised instance when the background compile delivers it
    const int jit_before = ldpc_hip_set_jit_mode_thread(2);   // this thread's opens only: concurrent callers keep their own mode
    const int open_rc = ldpc_hip_open_multi(decoder_type, b, c, M, hd.data(), devices.data(), (int)devices.size(), &ctx);  // :353-355
    (void)ldpc_hip_set_jit_mode_thread(jit_before);
    if (open_rc != 0) Env::fail(ldpc_hip_last_error());
    max_batch *= (long long)devices.size();

    int out_type;  // :451-466
    switch (decoder_type) {
    case LDPC_HIP_SP_DEC: case LDPC_HIP_ASP_DEC: case LDPC_HIP_IASP_DEC: case LDPC_HIP_TASP_DEC: case LDPC_HIP_LCHE_DEC: out_type = 1; break;
    case LDPC_HIP_BP_DEC: case LDPC_HIP_MS_DEC: case LDPC_HIP_LMS_DEC: case LDPC_HIP_IMS_DEC: out_type = 0; break;
    default: out_type = 0; Env::fail("Unknown decoder type");
    }
    const int QAM = modulation_type == MODULATION_SKIP_ ? 1 : 4, halfmlog = 1;                  // :405-406
    const double bitrate = (double)(c - b) / (c - punctured_blocks);                             // :444
    const double sigma = std::sqrt(std::pow(10, -snr / 10) / 2 / bitrate);                       // :445
    const double norm_factor = 2.0 * (QAM - 1.0) / 3.0;                                          // :447
    const double sigmaQAM = std::sqrt(std::pow(10., -snr / 10.) / (2 * bitrate * halfmlog * 2) * norm_factor);  // :449
    const double sg = modulation_type == MODULATION_SKIP_ ? sigma : sigmaQAM;

    // :413-427 interleaver between demapper and decoder (identity for permutation_type 0); same maps as upstream's
    Interleaver il;
    {
        std::vector<int> hflat((size_t)b * c);
        for (int i = 0; i < b; ++i) for (int j = 0; j < c; ++j) hflat[(size_t)i * c + j] = H(i, j);
        std::string err;
        if (!build_interleaver(b, c, M, halfmlog, permutation_type, permutation_block, permutation_inter, hflat.data(), il, err))
            Env::fail(err.c_str());
    }
    std::vector<double> chan((size_t)n);

    Env::burn_codeword_draws(H, M);  // :512

    SimCounters k;
    std::vector<double> llr, decword;
    std::vector<int32_t> iters;
    long long batch = 64;
    bool stop = n_frame_errors <= 0 || n_experiments < 0;                                        // :591 fails before the first frame
    const auto show = [&] {
        if (show_process)
            printf("SNR=%5.3lf,step=%4d,s_ers=%d,f_ers=%d,u_ers=%d,BER=%5.3le,FER=%5.3le\n", snr, (int)k.experiment, (int)k.nse, (int)k.nde,
                   (int)k.nue, (double)k.nse / k.experiment / (n - r), (double)k.nde / k.experiment);
    };

    // Noise on the device (default): the GPUs continue the generator's own stream -- same words, same polar-method attempts, same
    // libm log -- so nothing but the 8-byte frame records crosses PCIe.  LDPC_HIP_EXACT_NOISE=host keeps the draws on the host.
    uint32_t mt_words[624];
    int mt_pos = 0;
    const char *noise_env = getenv("LDPC_HIP_EXACT_NOISE");
    bool device_noise = !(noise_env && std::string(noise_env) == "host") && device_stream_matches_host(ldpc_hip_multi_ctx(ctx, 0)) &&
                        mt_export(Env::generator(), mt_words, mt_pos);
    if (device_noise) {
        if (ldpc_hip_multi_set_interleaver(ctx, permutation_type, permutation_block, permutation_inter) != 0) Env::fail(ldpc_hip_last_error());
        if (ldpc_hip_mt_set_state_multi(ctx, mt_words, mt_pos) != 0) Env::fail(ldpc_hip_last_error());
        const long long cap = (max_batch > 65536 * (long long)devices.size()) ? max_batch : 65536 * (long long)devices.size();
        std::vector<int32_t> info;
        batch = 256;
        while (!stop) {
            const long long room = (long long)n_experiments + 1 - k.experiment;
            const long long B = batch < room ? batch : room;
            info.resize((size_t)B); iters.resize((size_t)B);
            if (ldpc_hip_mt_get_state_multi(ctx, mt_words, &mt_pos) != 0) Env::fail(ldpc_hip_last_error());   // snapshot (+ the frame count: experiment)
            if (ldpc_hip_mt_frames_multi(ctx, snr, modulation_type, punctured_blocks, max_iterations, 0.8 /*MS_ALPHA*/, B, info.data(),
                                         iters.data()) != 0)
                Env::fail(ldpc_hip_last_error());
            const StopReplay rp = replay_stop_rule(k, n_frame_errors, n_experiments, reference_frame_error, B,
                                                   [&](long long f) { return std::make_pair(info[(size_t)f], (int)iters[(size_t)f]); }, show);
            stop = rp.stop;
            const long long used = rp.used, experiment = k.experiment;
            if (used < B) {  // stopped inside the batch: put the generator where the frame-by-frame loop leaves it
                if (ldpc_hip_mt_set_state_multi(ctx, mt_words, mt_pos) != 0) Env::fail(ldpc_hip_last_error());
                if (ldpc_hip_mt_set_frame_index_multi(ctx, experiment - used) != 0) Env::fail(ldpc_hip_last_error());   // set_state restarts the count
                if (ldpc_hip_mt_advance_multi(ctx, snr, modulation_type, punctured_blocks, used) != 0) Env::fail(ldpc_hip_last_error());
            }
            if (batch < cap) batch = batch * 4 < cap ? batch * 4 : cap;
        }
        if (ldpc_hip_mt_get_state_multi(ctx, mt_words, &mt_pos) != 0) Env::fail(ldpc_hip_last_error());
        if (!mt_import(Env::generator(), mt_words, mt_pos)) Env::fail("bp_simulation: could not hand the generator state back to std::mt19937");
        stop = true;   // the host-noise loop below is skipped
    }
    while (!stop) {
        const long long room = (long long)n_experiments + 1 - k.experiment;
        const long long B = batch < room ? batch : room;
        llr.resize((size_t)B * n); decword.resize((size_t)B * n); iters.resize((size_t)B);
        const std::mt19937 snapshot = Env::generator();
        for (long long f = 0; f < B; ++f) {
            double *y = llr.data() + (size_t)f * n;
            for (int i = 0; i < n; ++i) {                                                       // :601-611
                const double noise = Env::gaussian();
                chan[(size_t)i] = -2.0 * (sg * noise + 2.0 * 0.0 - 1.0) / (sg * sg);              // codeword == 0 (:568)
            }
            for (int i = 0; i < n; ++i) y[i] = chan[(size_t)il.inverse[(size_t)i]];              // :684 inverse permutation
            const double init_val = out_type == 1 ? 0 : 0.5;                                     // :700 (sic)
            const int plen = M * punctured_blocks, pstart = n - plen;
            for (int i = pstart; i < pstart + plen; ++i) y[i] = init_val;                        // :702-709
        }
        if (ldpc_hip_decode_host_multi(ctx, llr.data(), B, max_iterations, DEC_DECISION_HARD, 0.8 /*MS_ALPHA*/, decword.data(),
                                       iters.data(), 0) != 0)
            Env::fail(ldpc_hip_last_error());
        const StopReplay rp = replay_stop_rule(k, n_frame_errors, n_experiments, reference_frame_error, B, [&](long long f) {
            const double *d = decword.data() + (size_t)f * n;
            int curr_nse = 0, curr_nse_info = 0;                                                 // :735-742
            for (int i = 0; i < n; ++i)
                if (d[i] != 0.0) { ++curr_nse; if (i >= r) ++curr_nse_info; }
            return std::make_pair((int32_t)(curr_nse_info | (curr_nse > 0 ? 1 << 30 : 0)), (int)iters[(size_t)f]);   // the device's record
        }, show);
        stop = rp.stop;
        const long long used = rp.used;
        if (used < B) {  // stopped inside the batch: leave the generator where the frame-by-frame loop would
            Env::generator() = snapshot;
            for (long long i = 0, cnt = used * n; i < cnt; ++i) (void)Env::gaussian();
        }
        if (batch < max_batch) batch *= 4;
    }
    ldpc_hip_close_multi(ctx);                                                                   // :831
    if (counters_out) *counters_out = k;
    return std::make_pair((double)k.nse / k.experiment / (n - r), (double)k.nde / k.experiment); // :840
}

// the single-device form (device ordinal; LDPC_HIP_DEVICES overrides it)
template <class Mat, class Env>
std::pair<double, double> bp_simulation_t(int q_mod, Mat const &H, int tailbite_length, int max_iterations,
                                          int n_frame_errors, int n_experiments, double snr,
                                          double reference_frame_error, int decoder_type, int modulation_type,
                                          int permutation_type, int punctured_blocks, int show_process,
                                          SimCounters *counters_out = nullptr, int device = 0, long long max_batch = 4096,
                                          int permutation_block = 128, int permutation_inter = 1) {
    return bp_simulation_t<Mat, Env>(q_mod, H, tailbite_length, max_iterations, n_frame_errors, n_experiments, snr, reference_frame_error,
                                     decoder_type, modulation_type, permutation_type, punctured_blocks, show_process, counters_out,
                                     devices_from_env(device), max_batch, permutation_block, permutation_inter);
}

// Throughput mode.  Same arguments and return value as bp_simulation(); differences from exact-replay mode: the noise is the
// device-side Philox stream (seed), every modulation_type 0..4 is available (QAM16+ as the evidently intended chain), and
// `codewords` (optional, [ncw][n] 0/1 bytes) are really transmitted; ncw > 0 with codewords == nullptr transmits ncw random codewords
// encoded on the device (ldpc_hip_set_random_codewords).  The stopping rule is upstream's, frame by frame in global
// frame order (:591, :805-823), so the result equals a sequential loop over the same noise whatever the batch size or GPU count.
template <class Mat, class Env>
std::pair<double, double> bp_simulation_throughput_t(int q_mod, Mat const &H, int tailbite_length, int max_iterations, int n_frame_errors,
                                                     long long n_experiments, double snr, double reference_frame_error, int decoder_type,
                                                     int modulation_type, int permutation_type, int permutation_block, int permutation_inter,
                                                     int punctured_blocks, int show_process, unsigned long long seed,
                                                     const std::vector<int> &devices, SimCounters *counters_out = nullptr,
                                                     long long batch_per_gpu = 65536, const unsigned char *codewords = nullptr, int ncw = 0) {
    if (q_mod != 2) Env::fail("bp_simulation: only binary codes (q_mod == 2) are built in ldpc-lib_amd");
    if (devices.empty()) Env::fail("bp_simulation: empty device list");
    const int b = H.n_rows(), c = H.n_cols(), M = tailbite_length;
    const long long r = (long long)b * M, n = (long long)c * M;
    std::vector<int16_t> hd((size_t)b * c);
    for (int i = 0; i < b; ++i) for (int j = 0; j < c; ++j) hd[(size_t)i * c + j] = (int16_t)H(i, j);
    ldpc_hip_multi *m = nullptr;
    const int jit_before = ldpc_hip_set_jit_mode_thread(2);   // as in exact-replay mode: no waiting for hiprtc
    const int open_rc = ldpc_hip_open_multi(decoder_type, b, c, M, hd.data(), devices.data(), (int)devices.size(), &m);
    (void)ldpc_hip_set_jit_mode_thread(jit_before);
    if (open_rc != 0) Env::fail(ldpc_hip_last_error());
    if (ldpc_hip_multi_set_interleaver(m, permutation_type, permutation_block, permutation_inter) != 0) Env::fail(ldpc_hip_last_error());
    if (ncw > 0 && codewords && ldpc_hip_multi_set_codewords(m, codewords, ncw) != 0) Env::fail(ldpc_hip_last_error());
    if (ncw > 0 && !codewords && ldpc_hip_multi_set_random_codewords(m, seed, ncw) != 0) Env::fail(ldpc_hip_last_error());   // made on the device
    const int nsh = (int)devices.size();
    SimCounters k;
    long long first = 0;
    std::vector<int32_t> info, iters;
    bool stop = n_frame_errors <= 0 || n_experiments < 0;                                        // :591 fails before the first frame
    long long batch = 1024;   // ramp up like the exact harness: short runs stop after few frames
    while (!stop) {
        const long long room = n_experiments + 1 - k.experiment;
        long long B = batch * nsh;
        if (B > room) B = room;
        info.resize((size_t)B); iters.resize((size_t)B);
        if (ldpc_hip_frames_multi(m, snr, modulation_type, punctured_blocks, max_iterations, 0.8 /*MS_ALPHA*/, seed, first, B, batch,
                                  info.data(), iters.data(), nullptr, nullptr) != 0)
            Env::fail(ldpc_hip_last_error());
        stop = replay_stop_rule(k, n_frame_errors, n_experiments, reference_frame_error, B,
                                [&](long long f) { return std::make_pair(info[(size_t)f], (int)iters[(size_t)f]); }, [&] {
                                    if (show_process)
                                        printf("SNR=%5.3lf,step=%4d,s_ers=%d,f_ers=%d,u_ers=%d,BER=%5.3le,FER=%5.3le\n", snr, (int)k.experiment, (int)k.nse,
                                               (int)k.nde, (int)k.nue, (double)k.nse / k.experiment / (double)(n - r), (double)k.nde / k.experiment);
                                }).stop;
        first += B;
        if (batch < batch_per_gpu) batch = batch * 4 < batch_per_gpu ? batch * 4 : batch_per_gpu;
    }
    ldpc_hip_close_multi(m);
    if (counters_out) *counters_out = k;
    return std::make_pair((double)k.nse / k.experiment / (double)(n - r), (double)k.nde / k.experiment);
}

// The run of an opened code-set context, binary or GF(q): stop(state [C][4]) is the context's *_stop call (the rule on the device),
// simulate(first, B, totals [C][5], info [C][B]) its simulate call over frames [first, first + B).  show_process == 0 takes the first
// route, anything else the per-batch loop with the rule replayed on the host and a line per error frame.  info_len: the divisor of
// the error rate, information bits (or symbols) per frame.
template <class Env, class Stop, class Simulate>
std::vector<std::pair<double, double>> run_code_set(int C, long long info_len, int n_frame_errors, long long n_experiments, double snr,
                                                    double reference_frame_error, int show_process, long long first_batch, long long max_batch,
                                                    Stop stop_route, Simulate simulate, std::vector<SimCounters> *counters_out) {
    std::vector<SimCounters> cnt((size_t)C);
    if (!show_process) {   // nothing to print per error frame: the rule runs on the device
        std::vector<unsigned long long> state((size_t)C * 4);
        if (stop_route(state.data()) != 0) Env::fail(ldpc_hip_last_error());
        for (int q = 0; q < C; ++q) {
            cnt[(size_t)q].experiment = (long long)state[(size_t)q * 4];
            cnt[(size_t)q].nse = (long long)state[(size_t)q * 4 + 1];
            cnt[(size_t)q].nde = (long long)state[(size_t)q * 4 + 2];
        }
    }
    std::vector<char> running((size_t)C, 1);
    std::vector<unsigned long long> totals((size_t)C * 5);
    std::vector<int32_t> info;
    int n_running = show_process ? C : 0;
    long long first = 0, batch = first_batch;
    while (n_running > 0) {
        // every running code has replayed the same number of frames so far: `first`
        const long long room = n_experiments + 1 - first;
        const long long B = batch < room ? batch : room;
        if (B <= 0) break;
        info.resize((size_t)C * (size_t)B);
        if (simulate(first, B, totals.data(), info.data()) != 0) Env::fail(ldpc_hip_last_error());
        for (int q = 0; q < C; ++q) {
            if (!running[(size_t)q]) continue;
            SimCounters &k = cnt[(size_t)q];
            const int32_t *rec = info.data() + (size_t)q * (size_t)B;
            const bool stop = replay_stop_rule(k, n_frame_errors, n_experiments, reference_frame_error, B,
                                               [&](long long f) { return std::make_pair(rec[f], 0); }, [&] {
                                                   printf("code=%d,SNR=%5.3lf,step=%4d,s_ers=%d,f_ers=%d,BER=%5.3le,FER=%5.3le\n", q, snr, (int)k.experiment, (int)k.nse,
                                                          (int)k.nde, (double)k.nse / k.experiment / (double)info_len, (double)k.nde / k.experiment);
                                               }).stop;
            k.nue = 0;   // the records carry no iteration counts: nue and sum_abs_iters stay 0
            if (stop) { running[(size_t)q] = 0; --n_running; }
        }
        first += B;
        if (batch < max_batch) batch = batch * 4 < max_batch ? batch * 4 : max_batch;
    }
    std::vector<std::pair<double, double>> out((size_t)C);
    for (int q = 0; q < C; ++q)
        out[(size_t)q] = std::make_pair((double)cnt[(size_t)q].nse / cnt[(size_t)q].experiment / (double)info_len,
                                        (double)cnt[(size_t)q].nde / cnt[(size_t)q].experiment);
    if (counters_out) *counters_out = cnt;
    return out;
}


// What the code-set harnesses below ask of their arguments, and the set's context: one shape, MODULATION_SKIP, permutation_type 0,
// opened through the entry point of its decoder.
template <class Mat, class Env>
ldpc_hip_ctx *open_code_set(std::vector<Mat> const &codes, int M, int decoder_type, int modulation_type, int permutation_type, long long first_batch,
                            long long max_batch, int device) {
    if (codes.empty()) Env::fail("bp_simulation_codes: empty code set");
    if (modulation_type != MODULATION_SKIP_) Env::fail("bp_simulation_codes: only MODULATION_SKIP (BPSK) is built for code sets");
    if (permutation_type != 0) Env::fail("bp_simulation_codes: only permutation_type 0 is built for code sets");
    if (first_batch < 1 || max_batch < first_batch) Env::fail("bp_simulation_codes: bad batch sizes");
    const int C = (int)codes.size(), b = codes[0].n_rows(), c = codes[0].n_cols();
    std::vector<int16_t> hd((size_t)C * b * c);
    for (int q = 0; q < C; ++q) {
        if (codes[(size_t)q].n_rows() != b || codes[(size_t)q].n_cols() != c) Env::fail("bp_simulation_codes: the codes of a set share one shape");
        for (int i = 0; i < b; ++i) for (int j = 0; j < c; ++j) hd[((size_t)q * b + i) * c + j] = (int16_t)codes[(size_t)q](i, j);
    }
    ldpc_hip_ctx *ctx = nullptr;
    // MS_DEC, TASP_DEC and LMS_DEC beyond the 16 block rows (MS_DEC: or 32 block columns) of their register-resident set kernels:
    // ldpc_hip_open_codes_wide, the records in LDS
    const bool wide = (decoder_type == LDPC_HIP_MS_DEC || decoder_type == LDPC_HIP_TASP_DEC || decoder_type == LDPC_HIP_LMS_DEC) &&
                      (b > 16 || (decoder_type == LDPC_HIP_MS_DEC && c > 32));
    // Any lifting above 512, and any set whose image the entry point below refuses for its size (LDPC_HIP_EUNSUPPORTED): the
    // global-memory tier of a set, ldpc_hip_open_codes_global.  A structural refusal (LDPC_HIP_EINVAL) stays the first entry point's
    int rc = LDPC_HIP_EUNSUPPORTED;
    if (M <= 512) {
        rc = (wide                                ? ldpc_hip_open_codes_wide(decoder_type, b, c, M, hd.data(), C, device, &ctx)
             : decoder_type == LDPC_HIP_TASP_DEC ? ldpc_hip_open_codes_tdmp(b, c, M, hd.data(), C, device, &ctx)
             : decoder_type == LDPC_HIP_IASP_DEC ? ldpc_hip_open_codes_iasp(b, c, M, hd.data(), C, device, &ctx)
             : decoder_type == LDPC_HIP_LCHE_DEC ? ldpc_hip_open_codes_lche(b, c, M, hd.data(), C, device, &ctx)
             : decoder_type == LDPC_HIP_IMS_DEC  ? ldpc_hip_open_codes_ims(b, c, M, hd.data(), C, device, &ctx)
             : decoder_type == LDPC_HIP_SP_DEC || decoder_type == LDPC_HIP_ASP_DEC
                 ? ldpc_hip_open_codes_sp(decoder_type, b, c, M, hd.data(), C, device, &ctx)
                                                 : ldpc_hip_open_codes(decoder_type, b, c, M, hd.data(), C, device, &ctx));
    }
    if (rc == LDPC_HIP_EUNSUPPORTED) rc = ldpc_hip_open_codes_global(decoder_type, b, c, M, hd.data(), C, device, &ctx);
    if (rc != 0) Env::fail(ldpc_hip_last_error());
    return ctx;
}

// A set of candidate codes of one shape over the SAME noise, in throughput mode: what a code search does when it calls
// reset_random() before every candidate.  One pair <BER, FER> per code, each equal to what bp_simulation_throughput_t returns for
// that matrix alone with the same seed on one GPU (modulation SKIP, permutation_type 0, the all-zero codeword).  Every batch is
// one ldpc_hip_simulate_codes call for the whole set (C codes x B frames in one launch, the LLRs drawn once); upstream's
// sequential stopping rule (:591, :805-823) is replayed per code over its ordered records, and a code that has stopped ignores the
// records of later batches.  With show_process == 0 the whole run is one ldpc_hip_simulate_codes_stop call instead: the same rule on
// the device, every launch over the codes still running, no records on the host; the results are the same integers.  decoder_type: MS_DEC, LMS_DEC, TASP_DEC (7, ldpc_hip_open_codes_tdmp),
// IASP_DEC (5, ldpc_hip_open_codes_iasp), LCHE_DEC (9, ldpc_hip_open_codes_lche), IMS_DEC (4, ldpc_hip_open_codes_ims), SP_DEC or ASP_DEC (1, 2, ldpc_hip_open_codes_sp); MS_DEC, TASP_DEC and LMS_DEC beyond 16 block rows (MS_DEC: or 32 block columns)
// through ldpc_hip_open_codes_wide, and a lifting above 512 or an image beyond the LDS through ldpc_hip_open_codes_global, so no shape is refused.  counters_out: nse, nde and experiment per code (the [C][B] records carry
// no iteration counts, so nue and sum_abs_iters stay 0).
template <class Mat, class Env>
std::vector<std::pair<double, double>> bp_simulation_codes_t(std::vector<Mat> const &codes, int tailbite_length, int max_iterations,
                                                             int n_frame_errors, long long n_experiments, double snr,
                                                             double reference_frame_error, int decoder_type, int modulation_type,
                                                             int permutation_type, int punctured_blocks, int show_process,
                                                             unsigned long long seed, int device = 0,
                                                             std::vector<SimCounters> *counters_out = nullptr, long long first_batch = 1024,
                                                             long long max_batch = 65536) {
    ldpc_hip_ctx *ctx = open_code_set<Mat, Env>(codes, tailbite_length, decoder_type, modulation_type, permutation_type, first_batch, max_batch, device);
    const int C = (int)codes.size(), b = codes[0].n_rows(), c = codes[0].n_cols(), M = tailbite_length;
    const long long r = (long long)b * M, n = (long long)c * M;
    const auto out = run_code_set<Env>(
        C, n - r, n_frame_errors, n_experiments, snr, reference_frame_error, show_process, first_batch, max_batch,
        [&](unsigned long long *state) {
            return ldpc_hip_simulate_codes_stop(ctx, snr, punctured_blocks, max_iterations, 0.8 /*MS_ALPHA*/, seed, 0, n_frame_errors, n_experiments,
                                                reference_frame_error, first_batch, max_batch, state);
        },
        [&](long long first, long long B, unsigned long long *totals, int32_t *info) {
            return ldpc_hip_simulate_codes(ctx, snr, punctured_blocks, max_iterations, 0.8 /*MS_ALPHA*/, seed, first, B, totals, info);
        },
        counters_out);
    ldpc_hip_close(ctx);
    return out;
}

// Does the device draw the noise of an exact replay on a code set?  Not with LDPC_HIP_EXACT_NOISE=host, not when std::mt19937 does not
// export its state, and not on a host whose stream the device does not reproduce: that is probed once per process, on a single-code
// context opened with `code` (the probe draws plain samples).
template <class Mat, class Env>
bool code_set_device_noise(Mat const &code, int M, int decoder_type, int device, bool exported) {
    const char *noise_env = getenv("LDPC_HIP_EXACT_NOISE");
    bool device_noise = exported && !(noise_env && std::string(noise_env) == "host");
    if (device_noise && device_stream_verdict().load() < 0) {
        const int b = code.n_rows(), c = code.n_cols();
        std::vector<int16_t> hd((size_t)b * c);
        for (int i = 0; i < b; ++i) for (int j = 0; j < c; ++j) hd[(size_t)i * c + j] = (int16_t)code(i, j);
        ldpc_hip_ctx *probe = nullptr;
        const int jit_before = ldpc_hip_set_jit_mode_thread(0);   // the probe decodes nothing
        const int open_rc = ldpc_hip_open(decoder_type, b, c, M, hd.data(), device, &probe);
        (void)ldpc_hip_set_jit_mode_thread(jit_before);
        if (open_rc != 0) Env::fail(ldpc_hip_last_error());
        (void)device_stream_matches_host(probe);
        ldpc_hip_close(probe);
    }
    return device_noise && device_stream_verdict().load() == 1;
}

// A set of candidate codes of one shape in EXACT-REPLAY mode: what `for (candidate) { reset_random(); bp_simulation(...); }` computes
// (search_ggp/scenario_based_code_generation.cpp:851, main_simulation.cpp:483/492, ldpc_sim.cpp:148), with the noise of upstream's
// own stream drawn once per batch and decoded by all codes in one launch.  Call it where the loop would call reset_random() for its
// first candidate: Env::generator() is the generator every candidate starts from.  One pair <BER, FER> per code, and in counters_out
// the whole SimCounters; each equals what bp_simulation_t returns for that matrix from the same generator state (modulation SKIP,
// permutation_type 0).  show_process == 0: one ldpc_hip_mt_simulate_codes_stop call, the rule on the device.  Otherwise
// ldpc_hip_mt_simulate_codes per batch with the records of all codes, the rule replayed per code on the host and a line per error
// frame.  LDPC_HIP_EXACT_NOISE=host, or a host whose stream the device does not reproduce (device_stream_matches_host), draws the
// LLRs on the host as bp_simulation_t does and decodes them with ldpc_hip_frames_codes_host.
// Afterwards Env::generator() holds the state after the last frame code `leave_at` consumed (-1: the last code, what the loop
// above leaves behind).
// NOT covered: a caller that goes on with the stream from one SNR to the next per candidate WITHOUT a reset
// (main_good_code_search.cpp:316-338).  There the candidates' streams part after the first SNR, because each code stops at a
// frame of its own, and there is no shared noise left to draw once; such a caller stays with bp_simulation_t per candidate.  The SNR
// grid below (bp_simulation_codes_grid_exact_t) does not change that: it shares noise between SNRs only where every SNR starts from
// the reset generator.
template <class Mat, class Env>
std::vector<std::pair<double, double>> bp_simulation_codes_exact_t(std::vector<Mat> const &codes, int tailbite_length, int max_iterations,
                                                                   int n_frame_errors, long long n_experiments, double snr,
                                                                   double reference_frame_error, int decoder_type, int modulation_type,
                                                                   int permutation_type, int punctured_blocks, int show_process, int device = 0,
                                                                   std::vector<SimCounters> *counters_out = nullptr, long long first_batch = 1024,
                                                                   long long max_batch = 65536, int leave_at = -1) {
    ldpc_hip_ctx *ctx = open_code_set<Mat, Env>(codes, tailbite_length, decoder_type, modulation_type, permutation_type, first_batch, max_batch, device);
    const int C = (int)codes.size(), b = codes[0].n_rows(), c = codes[0].n_cols(), M = tailbite_length;
    const long long r = (long long)b * M, n = (long long)c * M;
    if (leave_at < -1 || leave_at >= C) Env::fail("bp_simulation_codes_exact: leave_at names no code of the set");
    const int leave = leave_at < 0 ? C - 1 : leave_at;
    if (punctured_blocks < 0 || punctured_blocks >= c) Env::fail("bp_simulation_codes_exact: punctured_blocks outside [0, nh)");

    Env::burn_codeword_draws(codes[0], M);   // :512, the count depends on the shape only
    uint32_t words[624];
    int pos = 0;
    const bool exported = mt_export(Env::generator(), words, pos);
    const bool device_noise = code_set_device_noise<Mat, Env>(codes[0], M, decoder_type, device, exported);

    std::vector<SimCounters> cnt((size_t)C);
    const bool nothing = n_frame_errors <= 0 || n_experiments < 0;   // :591 fails before the first frame
    const auto line = [&](int q) {
        const SimCounters &k = cnt[(size_t)q];
        printf("code=%d,SNR=%5.3lf,step=%4d,s_ers=%d,f_ers=%d,u_ers=%d,BER=%5.3le,FER=%5.3le\n", q, snr, (int)k.experiment, (int)k.nse, (int)k.nde,
               (int)k.nue, (double)k.nse / k.experiment / (double)(n - r), (double)k.nde / k.experiment);
    };
    // The per-batch run of both noise sources: frames(B, totals, info, iters) gives the records of the next B frames for all codes
    const auto batches = [&](auto frames) {
        std::vector<char> running((size_t)C, 1);
        std::vector<unsigned long long> totals((size_t)C * 5);
        std::vector<int32_t> info, iters;
        int n_running = nothing ? 0 : C;
        long long first = 0, batch = first_batch;
        while (n_running > 0) {   // every running code has replayed the same number of frames so far: `first`
            const long long room = n_experiments + 1 - first;
            const long long B = batch < room ? batch : room;
            if (B <= 0) break;
            info.resize((size_t)C * (size_t)B); iters.resize((size_t)C * (size_t)B);
            frames(B, totals.data(), info.data(), iters.data());
            for (int q = 0; q < C; ++q) {
                if (!running[(size_t)q]) continue;
                const int32_t *rec = info.data() + (size_t)q * (size_t)B, *it = iters.data() + (size_t)q * (size_t)B;
                if (replay_stop_rule(cnt[(size_t)q], n_frame_errors, n_experiments, reference_frame_error, B,
                                     [&](long long f) { return std::make_pair(rec[f], (int)it[f]); }, [&] { if (show_process) line(q); }).stop) {
                    running[(size_t)q] = 0; --n_running;
                }
            }
            first += B;
            if (batch < max_batch) batch = batch * 4 < max_batch ? batch * 4 : max_batch;
        }
    };

    if (device_noise) {
        if (ldpc_hip_mt_set_state_codes(ctx, words, pos) != 0) Env::fail(ldpc_hip_last_error());
        if (!show_process) {   // nothing to print per error frame: the rule runs on the device
            std::vector<unsigned long long> state((size_t)C * 6);
            if (ldpc_hip_mt_simulate_codes_stop(ctx, snr, punctured_blocks, max_iterations, 0.8 /*MS_ALPHA*/, n_frame_errors, n_experiments,
                                                reference_frame_error, first_batch, max_batch, state.data()) != 0)
                Env::fail(ldpc_hip_last_error());
            for (int q = 0; q < C; ++q) {
                const unsigned long long *s = state.data() + (size_t)q * 6;
                SimCounters &k = cnt[(size_t)q];
                k.experiment = (long long)s[0]; k.nse = (long long)s[1]; k.nde = (long long)s[2]; k.nue = (long long)s[3];
                k.sum_abs_iters = (long long)s[4];
            }
        } else {
            batches([&](long long B, unsigned long long *totals, int32_t *info, int32_t *iters) {
                if (ldpc_hip_mt_simulate_codes(ctx, snr, punctured_blocks, max_iterations, 0.8 /*MS_ALPHA*/, B, totals, info, iters) != 0)
                    Env::fail(ldpc_hip_last_error());
            });
            if (ldpc_hip_mt_set_state_codes(ctx, words, pos) != 0) Env::fail(ldpc_hip_last_error());   // back to the state at entry
        }
        // the generator where upstream's loop leaves it for code `leave`
        if (ldpc_hip_mt_advance_codes(ctx, snr, punctured_blocks, cnt[(size_t)leave].experiment) != 0) Env::fail(ldpc_hip_last_error());
        if (ldpc_hip_mt_get_state_codes(ctx, words, &pos) != 0) Env::fail(ldpc_hip_last_error());
        if (!mt_import(Env::generator(), words, pos)) Env::fail("bp_simulation_codes_exact: could not hand the generator state back to std::mt19937");
    } else {
        const std::mt19937 entry = Env::generator();
        const int out_type = decoder_type == LDPC_HIP_SP_DEC || decoder_type == LDPC_HIP_ASP_DEC || decoder_type == LDPC_HIP_IASP_DEC ||
                             decoder_type == LDPC_HIP_TASP_DEC || decoder_type == LDPC_HIP_LCHE_DEC;                    // :451-466
        const double bitrate = (double)(c - b) / (c - punctured_blocks);                                               // :444
        const double sg = std::sqrt(std::pow(10, -snr / 10) / 2 / bitrate);                                            // :445
        std::vector<double> llr;
        batches([&](long long B, unsigned long long *totals, int32_t *info, int32_t *iters) {
            llr.resize((size_t)B * (size_t)n);
            for (long long f = 0; f < B; ++f) {
                double *y = llr.data() + (size_t)f * (size_t)n;
                for (long long i = 0; i < n; ++i) y[i] = -2.0 * (sg * Env::gaussian() + 2.0 * 0.0 - 1.0) / (sg * sg);   // :601-611, codeword == 0
                for (long long i = n - (long long)M * punctured_blocks; i < n; ++i) y[i] = out_type == 1 ? 0 : 0.5;     // :700-709
            }
            if (ldpc_hip_frames_codes_host(ctx, llr.data(), B, max_iterations, 0.8 /*MS_ALPHA*/, totals, info, iters) != 0)
                Env::fail(ldpc_hip_last_error());
        });
        Env::generator() = entry;
        for (long long i = 0, draws = cnt[(size_t)leave].experiment * n; i < draws; ++i) (void)Env::gaussian();
    }
    ldpc_hip_close(ctx);
    std::vector<std::pair<double, double>> out((size_t)C);
    for (int q = 0; q < C; ++q)
        out[(size_t)q] = std::make_pair((double)cnt[(size_t)q].nse / cnt[(size_t)q].experiment / (double)(n - r),   // :840
                                        (double)cnt[(size_t)q].nde / cnt[(size_t)q].experiment);
    if (counters_out) *counters_out = cnt;
    return out;
}

// the standalone form: ldpc::Matrix and the library's own generator
inline std::vector<std::pair<double, double>> bp_simulation_codes_exact(std::vector<Matrix> const &codes, int tailbite_length, int max_iterations,
                                                                        int n_frame_errors, int n_experiments, double snr,
                                                                        double reference_frame_error, int decoder_type, int modulation_type,
                                                                        int permutation_type, int permutation_block, int permutation_inter,
                                                                        int punctured_blocks, int show_process, int device = 0,
                                                                        std::vector<SimCounters> *counters_out = nullptr, long long first_batch = 1024,
                                                                        long long max_batch = 65536, int leave_at = -1) {
    (void)permutation_block; (void)permutation_inter;   // permutation_type 0 only
    return bp_simulation_codes_exact_t<Matrix, OwnRngEnv>(codes, tailbite_length, max_iterations, n_frame_errors, n_experiments, snr,
                                                          reference_frame_error, decoder_type, modulation_type, permutation_type, punctured_blocks,
                                                          show_process, device, counters_out, first_batch, max_batch, leave_at);
}

// AN SNR GRID on a set of candidate codes, throughput mode: bp_simulation_codes_t at every entry of `snrs` with the reference frame
// error of that entry, the P x C (point, code) pairs as ONE set of work items over one noise draw (ldpc_hip_simulate_codes_grid_stop;
// 1 <= P <= 64).  out[p][q] is what bp_simulation_codes_t returns for code q at snrs[p] with reference_frame_errors[p] and the same
// seed; counters_out likewise [P][C].  With show_process != 0 the function calls bp_simulation_codes_t once per point, which keeps the
// printed lines and their order.
template <class Mat, class Env>
std::vector<std::vector<std::pair<double, double>>> bp_simulation_codes_grid_t(
    std::vector<Mat> const &codes, int tailbite_length, int max_iterations, int n_frame_errors, long long n_experiments, std::vector<double> const &snrs,
    std::vector<double> const &reference_frame_errors, int decoder_type, int modulation_type, int permutation_type, int punctured_blocks, int show_process,
    unsigned long long seed, int device = 0, std::vector<std::vector<SimCounters>> *counters_out = nullptr, long long first_batch = 1024,
    long long max_batch = 65536) {
    const int P = (int)snrs.size();
    if (P < 1 || P > 64 || reference_frame_errors.size() != snrs.size())
        Env::fail("bp_simulation_codes_grid: 1 .. 64 SNRs and one reference frame error per SNR");
    std::vector<std::vector<std::pair<double, double>>> out((size_t)P);
    std::vector<std::vector<SimCounters>> cnt((size_t)P);
    if (show_process) {
        for (int p = 0; p < P; ++p)
            out[(size_t)p] = bp_simulation_codes_t<Mat, Env>(codes, tailbite_length, max_iterations, n_frame_errors, n_experiments, snrs[(size_t)p],
                                                             reference_frame_errors[(size_t)p], decoder_type, modulation_type, permutation_type,
                                                             punctured_blocks, show_process, seed, device, &cnt[(size_t)p], first_batch, max_batch);
    } else {
        ldpc_hip_ctx *ctx = open_code_set<Mat, Env>(codes, tailbite_length, decoder_type, modulation_type, permutation_type, first_batch, max_batch, device);
        const int C = (int)codes.size(), b = codes[0].n_rows(), c = codes[0].n_cols();
        const long long info_len = (long long)(c - b) * tailbite_length;
        std::vector<unsigned long long> state((size_t)P * C * 4);
        if (ldpc_hip_simulate_codes_grid_stop(ctx, snrs.data(), P, punctured_blocks, max_iterations, 0.8 /*MS_ALPHA*/, seed, 0, n_frame_errors, n_experiments,
                                              reference_frame_errors.data(), first_batch, max_batch, state.data()) != 0)
            Env::fail(ldpc_hip_last_error());
        ldpc_hip_close(ctx);
        for (int p = 0; p < P; ++p) {
            cnt[(size_t)p].resize((size_t)C);
            for (int q = 0; q < C; ++q) {
                const unsigned long long *s = state.data() + ((size_t)p * C + q) * 4;
                SimCounters &k = cnt[(size_t)p][(size_t)q];
                k.experiment = (long long)s[0]; k.nse = (long long)s[1]; k.nde = (long long)s[2];
                out[(size_t)p].push_back(std::make_pair((double)k.nse / k.experiment / (double)info_len, (double)k.nde / k.experiment));
            }
        }
    }
    if (counters_out) *counters_out = cnt;
    return out;
}

// How often bp_simulation_codes_grid_exact_t has taken its one-call route in this process (and not the per-SNR loop it falls back to):
// both give the same numbers, so a caller or a test that wants to know which one ran reads this.
inline std::atomic<long long> &codes_grid_device_runs() {
    static std::atomic<long long> n{0};
    return n;
}

// AN SNR GRID on a set of candidate codes in EXACT-REPLAY mode: what
//     for (candidate) for (snr) { reset_random(); bp_simulation(candidate, snr, reference[snr]); }
// computes (upstream's `simulation` command, main_simulation.cpp:477-518): every (code, SNR) pair starts from the reset generator, so
// all of them see the same unit-variance samples and only sigma differs.  Call it where the loop would call reset_random() first:
// Env::generator() is the generator every pair starts from.  The P x C pairs are ONE set of work items over one noise draw
// (ldpc_hip_mt_simulate_codes_grid_stop; 1 <= P <= 64); the codeword draws are burnt once.  out[p][q] and (*counters_out)[p][q] are
// what bp_simulation_codes_exact_t gives for code q at snrs[p] with reference_frame_errors[p] from that generator state.
// Afterwards Env::generator() holds the state after the last frame that pair (leave_point, leave_at) consumed; -1 names the last
// point and the last code, where the loop above over the last code leaves it.
// With show_process != 0, and with host-drawn noise (LDPC_HIP_EXACT_NOISE=host, or a host whose stream the device does not reproduce),
// the function calls bp_simulation_codes_exact_t once per point, each from the generator at entry: that keeps upstream's printed lines
// in their order, and the host draws stay one stream per SNR.  Binary sets, BPSK, permutation_type 0, the all-zero word.
template <class Mat, class Env>
std::vector<std::vector<std::pair<double, double>>> bp_simulation_codes_grid_exact_t(
    std::vector<Mat> const &codes, int tailbite_length, int max_iterations, int n_frame_errors, long long n_experiments, std::vector<double> const &snrs,
    std::vector<double> const &reference_frame_errors, int decoder_type, int modulation_type, int permutation_type, int punctured_blocks, int show_process,
    int device = 0, std::vector<std::vector<SimCounters>> *counters_out = nullptr, long long first_batch = 1024, long long max_batch = 65536,
    int leave_at = -1, int leave_point = -1) {
    const int P = (int)snrs.size(), C = (int)codes.size(), M = tailbite_length;
    if (P < 1 || P > 64 || reference_frame_errors.size() != snrs.size())
        Env::fail("bp_simulation_codes_grid_exact: 1 .. 64 SNRs and one reference frame error per SNR");
    if (codes.empty()) Env::fail("bp_simulation_codes: empty code set");
    if (leave_at < -1 || leave_at >= C) Env::fail("bp_simulation_codes_grid_exact: leave_at names no code of the set");
    if (leave_point < -1 || leave_point >= P) Env::fail("bp_simulation_codes_grid_exact: leave_point names no point of the grid");
    const int leave = leave_at < 0 ? C - 1 : leave_at, leave_p = leave_point < 0 ? P - 1 : leave_point;
    std::vector<std::vector<std::pair<double, double>>> out((size_t)P);
    std::vector<std::vector<SimCounters>> cnt((size_t)P);
    const std::mt19937 entry = Env::generator();
    uint32_t words[624];
    int pos = 0;
    const bool device_noise = !show_process && code_set_device_noise<Mat, Env>(codes[0], M, decoder_type, device, mt_export(entry, words, pos));
    if (!device_noise) {   // one call per point, each from the reset generator, as the loop itself runs
        std::mt19937 left = entry;
        for (int p = 0; p < P; ++p) {
            Env::generator() = entry;
            out[(size_t)p] = bp_simulation_codes_exact_t<Mat, Env>(codes, M, max_iterations, n_frame_errors, n_experiments, snrs[(size_t)p],
                                                                   reference_frame_errors[(size_t)p], decoder_type, modulation_type, permutation_type,
                                                                   punctured_blocks, show_process, device, &cnt[(size_t)p], first_batch, max_batch, leave);
            if (p == leave_p) left = Env::generator();
        }
        Env::generator() = left;
    } else {
        ldpc_hip_ctx *ctx = open_code_set<Mat, Env>(codes, M, decoder_type, modulation_type, permutation_type, first_batch, max_batch, device);
        const int b = codes[0].n_rows(), c = codes[0].n_cols();
        const long long info_len = (long long)(c - b) * M;
        if (punctured_blocks < 0 || punctured_blocks >= c) Env::fail("bp_simulation_codes_exact: punctured_blocks outside [0, nh)");
        Env::burn_codeword_draws(codes[0], M);   // :512, once: the count depends on the shape only
        if (!mt_export(Env::generator(), words, pos)) Env::fail("bp_simulation_codes_grid_exact: std::mt19937 does not export its state");
        if (ldpc_hip_mt_set_state_codes(ctx, words, pos) != 0) Env::fail(ldpc_hip_last_error());
        std::vector<unsigned long long> state((size_t)P * C * 6);
        if (ldpc_hip_mt_simulate_codes_grid_stop(ctx, snrs.data(), P, punctured_blocks, max_iterations, 0.8 /*MS_ALPHA*/, n_frame_errors, n_experiments,
                                                 reference_frame_errors.data(), first_batch, max_batch, state.data()) != 0)
            Env::fail(ldpc_hip_last_error());
        for (int p = 0; p < P; ++p) {
            cnt[(size_t)p].resize((size_t)C);
            for (int q = 0; q < C; ++q) {
                const unsigned long long *s = state.data() + ((size_t)p * C + q) * 6;
                SimCounters &k = cnt[(size_t)p][(size_t)q];
                k.experiment = (long long)s[0]; k.nse = (long long)s[1]; k.nde = (long long)s[2]; k.nue = (long long)s[3];
                k.sum_abs_iters = (long long)s[4];
                out[(size_t)p].push_back(std::make_pair((double)k.nse / k.experiment / (double)info_len, (double)k.nde / k.experiment));   // :840
            }
        }
        // the generator where upstream's loop leaves it for the pair (leave_p, leave)
        if (ldpc_hip_mt_advance_codes(ctx, snrs[(size_t)leave_p], punctured_blocks, cnt[(size_t)leave_p][(size_t)leave].experiment) != 0)
            Env::fail(ldpc_hip_last_error());
        if (ldpc_hip_mt_get_state_codes(ctx, words, &pos) != 0) Env::fail(ldpc_hip_last_error());
        if (!mt_import(Env::generator(), words, pos)) Env::fail("bp_simulation_codes_grid_exact: could not hand the generator state back to std::mt19937");
        ldpc_hip_close(ctx);
        ++codes_grid_device_runs();
    }
    if (counters_out) *counters_out = cnt;
    return out;
}

// the standalone forms: ldpc::Matrix and the library's own generator
inline std::vector<std::vector<std::pair<double, double>>> bp_simulation_codes_grid(
    std::vector<Matrix> const &codes, int tailbite_length, int max_iterations, int n_frame_errors, long long n_experiments, std::vector<double> const &snrs,
    std::vector<double> const &reference_frame_errors, int decoder_type, int modulation_type, int permutation_type, int punctured_blocks, int show_process,
    unsigned long long seed, int device = 0, std::vector<std::vector<SimCounters>> *counters_out = nullptr, long long first_batch = 1024,
    long long max_batch = 65536) {
    return bp_simulation_codes_grid_t<Matrix, OwnRngEnv>(codes, tailbite_length, max_iterations, n_frame_errors, n_experiments, snrs, reference_frame_errors,
                                                         decoder_type, modulation_type, permutation_type, punctured_blocks, show_process, seed, device,
                                                         counters_out, first_batch, max_batch);
}

inline std::vector<std::vector<std::pair<double, double>>> bp_simulation_codes_grid_exact(
    std::vector<Matrix> const &codes, int tailbite_length, int max_iterations, int n_frame_errors, long long n_experiments, std::vector<double> const &snrs,
    std::vector<double> const &reference_frame_errors, int decoder_type, int modulation_type, int permutation_type, int punctured_blocks, int show_process,
    int device = 0, std::vector<std::vector<SimCounters>> *counters_out = nullptr, long long first_batch = 1024, long long max_batch = 65536,
    int leave_at = -1, int leave_point = -1) {
    return bp_simulation_codes_grid_exact_t<Matrix, OwnRngEnv>(codes, tailbite_length, max_iterations, n_frame_errors, n_experiments, snrs,
                                                               reference_frame_errors, decoder_type, modulation_type, permutation_type, punctured_blocks,
                                                               show_process, device, counters_out, first_batch, max_batch, leave_at, leave_point);
}

// The same for a set of candidate codes over GF(q), q = q_mod = 2^p (FHT_DEC): what upstream's ggp search does when it scores every
// candidate of one pattern with bp_simulation(q_mod, HM, HC, ...) after reset_random() (search_ggp/scenario_based_code_generation.cpp:
// 692-940).  codes[c] holds the shifts and coefs[c] the coefficients (natural representation, ncols2convert = 0) of candidate c; the
// matrices are taken as given -- left2right, which upstream's bp_simulation applies to both, is the caller's, as with ldpc_hip_open_gfq.
// One pair <SER, FER> per code: symbol errors at the information positions per frame and information symbol, and frame errors per
// frame, each equal to what a frame-by-frame run of ldpc_hip_simulate_gfq (random_messages = 0) gives for that code alone under the
// same rule.  show_process == 0 is one ldpc_hip_simulate_codes_gfq_stop call; otherwise ldpc_hip_simulate_codes_gfq per batch with the
// rule replayed on the host.  This form runs over Philox noise and the all-zero word; upstream's own stream and message for ONE code:
// bp_simulation(q_mod > 2, ...) / bp_simulation_gfq_t below.
template <class Mat, class Env>
std::vector<std::pair<double, double>> bp_simulation_codes_gfq_t(int q_mod, std::vector<Mat> const &codes, std::vector<Mat> const &coefs,
                                                                 int tailbite_length, int max_iterations, int n_frame_errors,
                                                                 long long n_experiments, double snr, double reference_frame_error,
                                                                 int show_process, unsigned long long seed, int device = 0,
                                                                 std::vector<SimCounters> *counters_out = nullptr, long long first_batch = 1024,
                                                                 long long max_batch = 65536) {
    if (codes.empty() || codes.size() != coefs.size()) Env::fail("bp_simulation_codes_gfq: empty code set, or not one coefficient matrix per code");
    if (first_batch < 1 || max_batch < first_batch) Env::fail("bp_simulation_codes_gfq: bad batch sizes");
    int q_bits = 0;
    while ((1 << q_bits) < q_mod) ++q_bits;
    if (q_mod < 4 || (1 << q_bits) != q_mod) Env::fail("bp_simulation_codes_gfq: q_mod is a power of two, at least 4 (binary sets: bp_simulation_codes)");
    const int C = (int)codes.size(), b = codes[0].n_rows(), c = codes[0].n_cols(), M = tailbite_length;
    const long long r = (long long)b * M, n = (long long)c * M;
    std::vector<int16_t> hb((size_t)C * b * c), hc((size_t)C * b * c);
    for (int q = 0; q < C; ++q) {
        if (codes[(size_t)q].n_rows() != b || codes[(size_t)q].n_cols() != c || coefs[(size_t)q].n_rows() != b || coefs[(size_t)q].n_cols() != c)
            Env::fail("bp_simulation_codes_gfq: the codes of a set share one shape");
        for (int i = 0; i < b; ++i)
            for (int j = 0; j < c; ++j) {
                hb[((size_t)q * b + i) * c + j] = (int16_t)codes[(size_t)q](i, j);
                hc[((size_t)q * b + i) * c + j] = (int16_t)coefs[(size_t)q](i, j);
            }
    }
    ldpc_hip_ctx *ctx = nullptr;
    if (ldpc_hip_open_codes_gfq(q_bits, b, c, M, hb.data(), hc.data(), C, device, &ctx) != 0) Env::fail(ldpc_hip_last_error());
    const auto out = run_code_set<Env>(
        C, n - r, n_frame_errors, n_experiments, snr, reference_frame_error, show_process, first_batch, max_batch,
        [&](unsigned long long *state) {
            return ldpc_hip_simulate_codes_gfq_stop(ctx, snr, max_iterations, seed, 0, n_frame_errors, n_experiments, reference_frame_error, first_batch,
                                                    max_batch, state);
        },
        [&](long long first, long long B, unsigned long long *totals, int32_t *info) {
            return ldpc_hip_simulate_codes_gfq(ctx, snr, max_iterations, seed, first, B, totals, info);
        },
        counters_out);
    ldpc_hip_close(ctx);
    return out;
}

inline std::vector<std::pair<double, double>> bp_simulation_codes_gfq(int q_mod, std::vector<Matrix> const &codes, std::vector<Matrix> const &coefs,
                                                                      int tailbite_length, int max_iterations, int n_frame_errors, int n_experiments,
                                                                      double snr, double reference_frame_error, int show_process,
                                                                      unsigned long long seed = 1, int device = 0,
                                                                      std::vector<SimCounters> *counters_out = nullptr, long long first_batch = 1024,
                                                                      long long max_batch = 65536) {
    return bp_simulation_codes_gfq_t<Matrix, OwnRngEnv>(q_mod, codes, coefs, tailbite_length, max_iterations, n_frame_errors, n_experiments, snr,
                                                        reference_frame_error, show_process, seed, device, counters_out, first_batch, max_batch);
}

// the standalone form: ldpc::Matrix, same tail as bp_simulation() plus the Philox seed
inline std::vector<std::pair<double, double>> bp_simulation_codes(std::vector<Matrix> const &codes, int tailbite_length, int max_iterations,
                                                                  int n_frame_errors, int n_experiments, double snr,
                                                                  double reference_frame_error, int decoder_type, int modulation_type,
                                                                  int permutation_type, int permutation_block, int permutation_inter,
                                                                  int punctured_blocks, int show_process, unsigned long long seed = 1,
                                                                  int device = 0, std::vector<SimCounters> *counters_out = nullptr,
                                                                  long long first_batch = 1024, long long max_batch = 65536) {
    (void)permutation_block; (void)permutation_inter;   // permutation_type 0 only
    return bp_simulation_codes_t<Matrix, OwnRngEnv>(codes, tailbite_length, max_iterations, n_frame_errors, n_experiments, snr,
                                                    reference_frame_error, decoder_type, modulation_type, permutation_type, punctured_blocks,
                                                    show_process, seed, device, counters_out, first_batch, max_batch);
}

// ---- what the two q-ary harnesses below share ------------------------------------------------------------------------------------
// q_bits of q_mod, after the checks of what upstream's q-ary path has at all
template <class Env>
int gfq_harness_check(int q_mod, int decoder_type, int modulation_type, int permutation_type) {
    int q_bits = 0;
    while ((1 << q_bits) < q_mod) ++q_bits;
    if (q_mod < 4 || q_mod > 1024 || (1 << q_bits) != q_mod) Env::fail("bp_simulation: q_mod > 2 must be a power of two in 4 .. 1024");
    if (decoder_type != LDPC_HIP_FHT_DEC) Env::fail("bp_simulation: q_mod > 2 decodes with FHT_DEC (decoder_type 6) only");
    if (modulation_type != MODULATION_SKIP_)
        Env::fail("bp_simulation: q_mod > 2 takes MODULATION_SKIP only (upstream's switch at bp_simulation.cpp:635-678 has no other case)");
    if (permutation_type != 0) Env::fail("bp_simulation: q_mod > 2 takes permutation_type 0 only (upstream never inverts the permutation, :683-686)");
    return q_bits;
}

// Upstream's set-up of one code (:348-399) and its word (:537-557): hb, hc [b][c] as the frame loop uses them (after ncols2convert and
// left2right), the rewritten coefficients written back into coef_matrix (:384-389), word [n] = the encoded message.  Returns whether
// the encoder produced a codeword (false: flag == 0 or a code the encoder refuses -- the all-zero word is sent, word is zero).
// keep != null: the context opened on (hb, hc) is handed out instead of closed.
template <class Mat, class Env>
bool gfq_harness_setup(int q_bits, Mat const &H, Mat &coef_matrix, int ncols2convert, int M, int device, std::vector<int16_t> &hb,
                       std::vector<int16_t> &hc, std::vector<int16_t> &word, ldpc_hip_ctx **keep) {
    const int b = H.n_rows(), c = H.n_cols();
    if (coef_matrix.n_rows() != b || coef_matrix.n_cols() != c) Env::fail("bp_simulation: coef_matrix must have the shape of the code matrix");
    hb.assign((size_t)b * c, 0); hc.assign((size_t)b * c, 0);
    for (int i = 0; i < b; ++i)
        for (int j = 0; j < c; ++j) { hb[(size_t)i * c + j] = (int16_t)H(i, j); hc[(size_t)i * c + j] = (int16_t)coef_matrix(i, j); }   // :359-366
    ldpc_hip_ctx *ctx = nullptr;
    if (ldpc_hip_open_gfq(q_bits, b, c, M, hb.data(), hc.data(), ncols2convert, device, &ctx) != 0) Env::fail(ldpc_hip_last_error());     // :368-382
    if (ldpc_hip_gfq_coefficients(ctx, hc.data()) != 0) Env::fail(ldpc_hip_last_error());
    ldpc_hip_close(ctx);
    ctx = nullptr;
    for (int i = 0; i < b; ++i)
        for (int j = 0; j < c; ++j) coef_matrix(i, j) = hc[(size_t)i * c + j];                                                           // :384-389
    if (ldpc_hip_gfq_left2right(hb.data(), b, c) != 0 || ldpc_hip_gfq_left2right(hc.data(), b, c) != 0) Env::fail(ldpc_hip_last_error());   // :391-394
    if (ldpc_hip_open_gfq(q_bits, b, c, M, hb.data(), hc.data(), 0, device, &ctx) != 0) Env::fail(ldpc_hip_last_error());                 // :396-399
    const int K = ldpc_hip_gfq_k(ctx);                                                                                                   // :537-557
    std::vector<int16_t> msg((size_t)(K > 0 ? K : 1));
    word.assign((size_t)c * M, 0);
    int32_t ok = 0;
    if (ldpc_hip_gfq_upstream_message(q_bits, K, msg.data()) != 0) Env::fail(ldpc_hip_last_error());
    const int rc = ldpc_hip_encode_gfq_host(ctx, msg.data(), 1, word.data(), &ok);
    if (rc != 0 && rc != LDPC_HIP_EUNSUPPORTED) Env::fail(ldpc_hip_last_error());
    const bool encoded = rc == 0 && ok != 0;
    if (!encoded) word.assign((size_t)c * M, 0);
    if (keep) *keep = ctx; else ldpc_hip_close(ctx);
    return encoded;
}

// Once per process, on a binary context of the same shape (the probe draws plain samples, which a GF(q) context does not serve): does
// the device reproduce this host's std::normal_distribution?  A shape the binary opener refuses leaves the verdict open, and the
// draws then stay on the host.
inline void gfq_harness_probe(const std::vector<int16_t> &hb, int b, int c, int M, int device) {
    if (device_stream_verdict().load() >= 0) return;
    std::vector<int16_t> hd(hb.size());
    for (size_t i = 0; i < hd.size(); ++i) hd[i] = (int16_t)(hb[i] < 0 ? -1 : hb[i] % M);
    ldpc_hip_ctx *probe = nullptr;
    const int jit_before = ldpc_hip_set_jit_mode_thread(0);   // the probe decodes nothing
    const int open_rc = ldpc_hip_open(LDPC_HIP_MS_DEC, b, c, M, hd.data(), device, &probe);
    (void)ldpc_hip_set_jit_mode_thread(jit_before);
    if (open_rc == 0) {
        (void)device_stream_matches_host(probe);
        ldpc_hip_close(probe);
    }
}

// frames of a batch whose Gaussians are drawn on the host: at most 256 MiB of doubles at a time, whatever the batch schedule says
inline long long gfq_host_noise_frames(long long per_frame) {
    const long long cap = ((long long)256 << 20) / ((long long)sizeof(double) * (per_frame > 0 ? per_frame : 1));
    return cap < 1 ? 1 : cap;
}

// bp_simulation() for q_mod > 2: upstream's q-ary harness (bp_simulation.cpp with q_mod > 2) in exact-replay mode on FHT_DEC.
//   set-up (:348-399)   decod_init with ncols2convert on the matrices as given; the rewritten coefficients go back into coef_matrix
//                       (:384-389); left2right on both; decod_init again with 0 -- ldpc_hip_open_gfq(ncols2convert),
//                       ldpc_hip_gfq_coefficients, ldpc_hip_gfq_left2right, ldpc_hip_open_gfq(0);
//   message (:537-557)  the message include/ldpc_hip.h defines (ldpc_hip_gfq_upstream_message: upstream's eight symbols reduced
//                       with & (q - 1), then zeros) through the encoder; ok = 0 or a code the encoder refuses sends the all-zero word;
//   frames              no draw before the loop, n * q_bits Gaussians per frame (:638-642), p_thr = 0, the binary accounting and
//                       stopping rule; batches x 4, the snapshot and roll-forward after a stop inside a batch, the show_process line.
// The noise is the generator's own stream continued on the device (ldpc_hip_mt_frames_gfq) when the device reproduces this host's
// std::normal_distribution; otherwise, or with LDPC_HIP_EXACT_NOISE=host, Env::gaussian() through ldpc_hip_frames_gfq_noise_host.
// Only decoder_type 6, MODULATION_SKIP and permutation_type 0 mean anything upstream for q_mod > 2 (the switch at :635-678 has no other
// case, the permutation is never inverted, :683-686); anything else fails with the reason.  punctured_blocks enters sigma only.
template <class Mat, class Env>
std::pair<double, double> bp_simulation_gfq_t(int q_mod, Mat const &H, Mat &coef_matrix, int ncols2convert, int tailbite_length, int max_iterations,
                                              int n_frame_errors, int n_experiments, double snr, double reference_frame_error, int decoder_type,
                                              int modulation_type, int permutation_type, int punctured_blocks, int show_process,
                                              SimCounters *counters_out = nullptr, int device = 0, long long max_batch = 65536) {
    const int q_bits = gfq_harness_check<Env>(q_mod, decoder_type, modulation_type, permutation_type);
    const int b = H.n_rows(), c = H.n_cols(), M = tailbite_length;
    const long long r = (long long)b * M, n = (long long)c * M;
    const std::vector<int> devs = devices_from_env(device);   // the first device of the list is used
    device = devs[0];
    std::vector<int16_t> hb, hc, word;
    ldpc_hip_ctx *ctx = nullptr;
    const bool encoded = gfq_harness_setup<Mat, Env>(q_bits, H, coef_matrix, ncols2convert, M, device, hb, hc, word, &ctx);
    if (ldpc_hip_gfq_set_codeword(ctx, encoded ? word.data() : nullptr) != 0) Env::fail(ldpc_hip_last_error());   // flag == 0: the all-zero word

    SimCounters k;
    std::vector<int32_t> info, iters;
    bool stop = n_frame_errors <= 0 || n_experiments < 0;                                        // :591 fails before the first frame
    const auto show = [&] {
        if (show_process)
            printf("SNR=%5.3lf,step=%4d,s_ers=%d,f_ers=%d,u_ers=%d,BER=%5.3le,FER=%5.3le\n", snr, (int)k.experiment, (int)k.nse, (int)k.nde,
                   (int)k.nue, (double)k.nse / k.experiment / (double)(n - r), (double)k.nde / k.experiment);
    };
    const auto record = [&](long long f) { return std::make_pair(info[(size_t)f], (int)iters[(size_t)f]); };

    uint32_t mt_words[624];
    int mt_pos = 0;
    const char *noise_env = getenv("LDPC_HIP_EXACT_NOISE");
    bool device_noise = !(noise_env && std::string(noise_env) == "host") && mt_export(Env::generator(), mt_words, mt_pos);
    if (device_noise) gfq_harness_probe(hb, b, c, M, device);
    device_noise = device_noise && device_stream_verdict().load() == 1;

    long long batch = max_batch < 256 ? max_batch : 256;
    if (device_noise) {
        if (ldpc_hip_mt_set_state_gfq(ctx, mt_words, mt_pos) != 0) Env::fail(ldpc_hip_last_error());
        while (!stop) {
            const long long room = (long long)n_experiments + 1 - k.experiment;
            const long long B = batch < room ? batch : room;
            info.resize((size_t)B); iters.resize((size_t)B);
            if (ldpc_hip_mt_get_state_gfq(ctx, mt_words, &mt_pos) != 0) Env::fail(ldpc_hip_last_error());   // snapshot
            if (ldpc_hip_mt_frames_gfq(ctx, snr, punctured_blocks, max_iterations, B, info.data(), iters.data()) != 0) Env::fail(ldpc_hip_last_error());
            const StopReplay rp = replay_stop_rule(k, n_frame_errors, n_experiments, reference_frame_error, B, record, show);
            stop = rp.stop;
            if (rp.used < B) {  // stopped inside the batch: put the generator where the frame-by-frame loop leaves it
                if (ldpc_hip_mt_set_state_gfq(ctx, mt_words, mt_pos) != 0) Env::fail(ldpc_hip_last_error());
                if (ldpc_hip_mt_advance_gfq(ctx, rp.used) != 0) Env::fail(ldpc_hip_last_error());
            }
            if (batch < max_batch) batch = batch * 4 < max_batch ? batch * 4 : max_batch;
        }
        if (ldpc_hip_mt_get_state_gfq(ctx, mt_words, &mt_pos) != 0) Env::fail(ldpc_hip_last_error());
        if (!mt_import(Env::generator(), mt_words, mt_pos)) Env::fail("bp_simulation: could not hand the generator state back to std::mt19937");
    } else {
        const long long per_frame = n * q_bits, host_cap = gfq_host_noise_frames(per_frame);
        std::vector<double> noise;
        while (!stop) {
            const long long room = (long long)n_experiments + 1 - k.experiment;
            long long B = batch < room ? batch : room;
            if (B > host_cap) B = host_cap;   // the batch carries B * n * q_bits doubles through host memory
            info.resize((size_t)B); iters.resize((size_t)B); noise.resize((size_t)(B * per_frame));
            const std::mt19937 snapshot = Env::generator();
            for (double &g : noise) g = Env::gaussian();                                         // :638-642, index order
            if (ldpc_hip_frames_gfq_noise_host(ctx, noise.data(), snr, punctured_blocks, max_iterations, B, info.data(), iters.data()) != 0)
                Env::fail(ldpc_hip_last_error());
            const StopReplay rp = replay_stop_rule(k, n_frame_errors, n_experiments, reference_frame_error, B, record, show);
            stop = rp.stop;
            if (rp.used < B) {  // stopped inside the batch: leave the generator where the frame-by-frame loop would
                Env::generator() = snapshot;
                for (long long i = 0, cnt = rp.used * per_frame; i < cnt; ++i) (void)Env::gaussian();
            }
            if (batch < max_batch) batch = batch * 4 < max_batch ? batch * 4 : max_batch;
        }
    }
    ldpc_hip_close(ctx);                                                                         // :831
    if (counters_out) *counters_out = k;
    return std::make_pair((double)k.nse / k.experiment / (double)(n - r), (double)k.nde / k.experiment);   // :840
}

// The same for a set of candidate codes over GF(q) of one shape: what `for (candidate) { reset_random(); bp_simulation(q_mod, HM, HC,
// ...); }` computes (search_ggp/scenario_based_code_generation.cpp:754, :852, :883), with the shape and contract of
// bp_simulation_codes_exact_t.  Call it where the loop would call reset_random() for its first candidate.  Every candidate gets
// upstream's set-up (its coefficients are rewritten in coefs[q], as bp_simulation does) and its own word; the noise of the generator's
// stream is drawn once per batch and all candidates are decoded in one launch (ldpc_hip_mt_simulate_codes_gfq*).  show_process == 0
// runs the rule on the device; otherwise the records come back per batch, the rule is replayed per code on the host and a line is
// printed per error frame.  LDPC_HIP_EXACT_NOISE=host, or a host whose stream the device does not reproduce, draws the Gaussians on the
// host (ldpc_hip_frames_codes_gfq_noise_host).  Afterwards Env::generator() holds the state after the last frame code `leave_at`
// consumed (-1: the last code).  One pair and one SimCounters per code, each equal to bp_simulation_gfq_t on that candidate.
template <class Mat, class Env>
std::vector<std::pair<double, double>> bp_simulation_codes_gfq_exact_t(int q_mod, std::vector<Mat> const &codes, std::vector<Mat> &coefs, int ncols2convert,
                                                                       int tailbite_length, int max_iterations, int n_frame_errors,
                                                                       long long n_experiments, double snr, double reference_frame_error,
                                                                       int decoder_type, int modulation_type, int permutation_type,
                                                                       int punctured_blocks, int show_process, int device = 0,
                                                                       std::vector<SimCounters> *counters_out = nullptr, long long first_batch = 1024,
                                                                       long long max_batch = 65536, int leave_at = -1) {
    if (codes.empty() || codes.size() != coefs.size()) Env::fail("bp_simulation_codes_gfq_exact: empty code set, or not one coefficient matrix per code");
    if (first_batch < 1 || max_batch < first_batch) Env::fail("bp_simulation_codes_gfq_exact: bad batch sizes");
    const int q_bits = gfq_harness_check<Env>(q_mod, decoder_type, modulation_type, permutation_type);
    const int C = (int)codes.size(), b = codes[0].n_rows(), c = codes[0].n_cols(), M = tailbite_length;
    const long long r = (long long)b * M, n = (long long)c * M;
    if (leave_at < -1 || leave_at >= C) Env::fail("bp_simulation_codes_gfq_exact: leave_at names no code of the set");
    const int leave = leave_at < 0 ? C - 1 : leave_at;
    device = devices_from_env(device)[0];

    std::vector<int16_t> hb((size_t)C * b * c), hc((size_t)C * b * c), words((size_t)C * (size_t)n), hb1, hc1, word1;
    bool any_word = false;
    for (int q = 0; q < C; ++q) {
        if (codes[(size_t)q].n_rows() != b || codes[(size_t)q].n_cols() != c) Env::fail("bp_simulation_codes_gfq_exact: the codes of a set share one shape");
        any_word = gfq_harness_setup<Mat, Env>(q_bits, codes[(size_t)q], coefs[(size_t)q], ncols2convert, M, device, hb1, hc1, word1, nullptr) || any_word;
        std::copy(hb1.begin(), hb1.end(), hb.begin() + (size_t)q * b * c);
        std::copy(hc1.begin(), hc1.end(), hc.begin() + (size_t)q * b * c);
        std::copy(word1.begin(), word1.end(), words.begin() + (size_t)q * (size_t)n);
    }
    ldpc_hip_ctx *ctx = nullptr;
    if (ldpc_hip_open_codes_gfq(q_bits, b, c, M, hb.data(), hc.data(), C, device, &ctx) != 0) Env::fail(ldpc_hip_last_error());
    if (ldpc_hip_codes_gfq_set_codewords(ctx, any_word ? words.data() : nullptr) != 0) Env::fail(ldpc_hip_last_error());   // no word: shared soft values

    uint32_t mt_words[624];
    int mt_pos = 0;
    const char *noise_env = getenv("LDPC_HIP_EXACT_NOISE");
    bool device_noise = !(noise_env && std::string(noise_env) == "host") && mt_export(Env::generator(), mt_words, mt_pos);
    if (device_noise) gfq_harness_probe(hb, b, c, M, device);   // the first code's shifts stand at the front
    device_noise = device_noise && device_stream_verdict().load() == 1;

    std::vector<SimCounters> cnt((size_t)C);
    const bool nothing = n_frame_errors <= 0 || n_experiments < 0;   // :591 fails before the first frame
    const auto line = [&](int q) {
        const SimCounters &k = cnt[(size_t)q];
        printf("code=%d,SNR=%5.3lf,step=%4d,s_ers=%d,f_ers=%d,u_ers=%d,BER=%5.3le,FER=%5.3le\n", q, snr, (int)k.experiment, (int)k.nse, (int)k.nde,
               (int)k.nue, (double)k.nse / k.experiment / (double)(n - r), (double)k.nde / k.experiment);
    };
    // The per-batch run of both noise sources: frames(B, totals, info, iters) gives the records of the next B frames for all codes
    const auto batches = [&](long long frame_cap, auto frames) {
        std::vector<char> running((size_t)C, 1);
        std::vector<unsigned long long> totals((size_t)C * 5);
        std::vector<int32_t> info, iters;
        int n_running = nothing ? 0 : C;
        long long first = 0, batch = first_batch;
        while (n_running > 0) {   // every running code has replayed the same number of frames so far: `first`
            const long long room = n_experiments + 1 - first;
            long long B = batch < room ? batch : room;
            if (B > frame_cap) B = frame_cap;
            if (B <= 0) break;
            info.resize((size_t)C * (size_t)B); iters.resize((size_t)C * (size_t)B);
            frames(B, totals.data(), info.data(), iters.data());
            for (int q = 0; q < C; ++q) {
                if (!running[(size_t)q]) continue;
                const int32_t *rec = info.data() + (size_t)q * (size_t)B, *it = iters.data() + (size_t)q * (size_t)B;
                if (replay_stop_rule(cnt[(size_t)q], n_frame_errors, n_experiments, reference_frame_error, B,
                                     [&](long long f) { return std::make_pair(rec[f], (int)it[f]); }, [&] { if (show_process) line(q); }).stop) {
                    running[(size_t)q] = 0; --n_running;
                }
            }
            first += B;
            if (batch < max_batch) batch = batch * 4 < max_batch ? batch * 4 : max_batch;
        }
    };

    if (device_noise) {
        if (ldpc_hip_mt_set_state_codes_gfq(ctx, mt_words, mt_pos) != 0) Env::fail(ldpc_hip_last_error());
        if (!show_process) {   // nothing to print per error frame: the rule runs on the device
            std::vector<unsigned long long> state((size_t)C * 6);
            if (ldpc_hip_mt_simulate_codes_gfq_stop(ctx, snr, punctured_blocks, max_iterations, n_frame_errors, n_experiments, reference_frame_error,
                                                    first_batch, max_batch, state.data()) != 0)
                Env::fail(ldpc_hip_last_error());
            for (int q = 0; q < C; ++q) {
                const unsigned long long *st = state.data() + (size_t)q * 6;
                SimCounters &k = cnt[(size_t)q];
                k.experiment = (long long)st[0]; k.nse = (long long)st[1]; k.nde = (long long)st[2]; k.nue = (long long)st[3];
                k.sum_abs_iters = (long long)st[4];
            }
        } else {
            batches(max_batch, [&](long long B, unsigned long long *totals, int32_t *info, int32_t *iters) {
                if (ldpc_hip_mt_simulate_codes_gfq(ctx, snr, punctured_blocks, max_iterations, B, totals, info, iters) != 0) Env::fail(ldpc_hip_last_error());
            });
            if (ldpc_hip_mt_set_state_codes_gfq(ctx, mt_words, mt_pos) != 0) Env::fail(ldpc_hip_last_error());   // back to the state at entry
        }
        // the generator where upstream's loop leaves it for code `leave`
        if (ldpc_hip_mt_advance_codes_gfq(ctx, cnt[(size_t)leave].experiment) != 0) Env::fail(ldpc_hip_last_error());
        if (ldpc_hip_mt_get_state_codes_gfq(ctx, mt_words, &mt_pos) != 0) Env::fail(ldpc_hip_last_error());
        if (!mt_import(Env::generator(), mt_words, mt_pos)) Env::fail("bp_simulation_codes_gfq_exact: could not hand the generator state back to std::mt19937");
    } else {
        const std::mt19937 entry = Env::generator();
        const long long per_frame = n * q_bits;
        std::vector<double> noise;
        batches(gfq_host_noise_frames(per_frame), [&](long long B, unsigned long long *totals, int32_t *info, int32_t *iters) {
            noise.resize((size_t)(B * per_frame));
            for (double &g : noise) g = Env::gaussian();                                         // :638-642, index order
            if (ldpc_hip_frames_codes_gfq_noise_host(ctx, noise.data(), snr, punctured_blocks, max_iterations, B, totals, info, iters) != 0)
                Env::fail(ldpc_hip_last_error());
        });
        Env::generator() = entry;
        for (long long i = 0, draws = cnt[(size_t)leave].experiment * per_frame; i < draws; ++i) (void)Env::gaussian();
    }
    ldpc_hip_close(ctx);
    std::vector<std::pair<double, double>> out((size_t)C);
    for (int q = 0; q < C; ++q)
        out[(size_t)q] = std::make_pair((double)cnt[(size_t)q].nse / cnt[(size_t)q].experiment / (double)(n - r),   // :840
                                        (double)cnt[(size_t)q].nde / cnt[(size_t)q].experiment);
    if (counters_out) *counters_out = cnt;
    return out;
}

// the standalone form: ldpc::Matrix and the library's own generator
inline std::vector<std::pair<double, double>> bp_simulation_codes_gfq_exact(int q_mod, std::vector<Matrix> const &codes, std::vector<Matrix> &coefs,
                                                                            int ncols2convert, int tailbite_length, int max_iterations,
                                                                            int n_frame_errors, int n_experiments, double snr,
                                                                            double reference_frame_error, int punctured_blocks, int show_process,
                                                                            int device = 0, std::vector<SimCounters> *counters_out = nullptr,
                                                                            long long first_batch = 1024, long long max_batch = 65536, int leave_at = -1) {
    return bp_simulation_codes_gfq_exact_t<Matrix, OwnRngEnv>(q_mod, codes, coefs, ncols2convert, tailbite_length, max_iterations, n_frame_errors,
                                                              n_experiments, snr, reference_frame_error, LDPC_HIP_FHT_DEC, MODULATION_SKIP_, 0,
                                                              punctured_blocks, show_process, device, counters_out, first_batch, max_batch, leave_at);
}

// Standalone entry point with upstream's argument list (bp_simulation.h:9-27); q_mod > 2 goes to bp_simulation_gfq_t, which reads
// and rewrites coef_matrix and takes ncols2convert; a binary run ignores both.
std::pair<double, double> bp_simulation(int q_mod, Matrix const &code_generating_matrix, Matrix &coef_matrix,
                                        int ncols2convert, int tailbite_length, int max_iterations, int n_frame_errors,
                                        int n_experiments, double snr, double reference_frame_error, int decoder_type,
                                        int modulation_type, int permutation_type, int permutation_block,
                                        int permutation_inter, int punctured_blocks, int show_process);

}  // namespace ldpc

#endif
