// The transmit side and the error accounting around FHT_DEC (ldpc_gfq.hpp), all on the device:
//   gfq_encode_kernel    encode_NBQCLDPC (decoders.cpp:1381-1705), batched: one launch encodes and re-checks the whole batch
//   gfq_message_kernel   K uniform message symbols per frame from Philox (stream tag 4)
//   gfq_channel_kernel   word2bin -> BPSK -> AWGN -> symbol probabilities (bp_simulation.cpp:581-582, :638-676)
//   gfq_count_kernel     symbol errors against the transmitted word (bp_simulation.cpp:746-755, :805-810)
//
// Encoder.  A workgroup of 256 lanes holds F = max(1, 256 / M) frames at once (M = 8: 32 frames, so no lane idles; M >= 256: one
// frame, the lanes stride over the positions).  Lane (f, I) owns position I of every block row of frame f.  In LDS: the field's
// log / antilog tables (2 q int16, shared by the workgroup -- products go through them, a q x q table would be 2 MB at q = 1024),
// and per frame the codeword (N int16), the syndrome (R int16) and the un-rotated special block (M int16).  The message is read
// from global memory once, as one contiguous run of F * K symbols, and every rotated read after that is an LDS gather
// cw[col * M + (I + shift) % M]: upstream's rotate() (decoders.cpp:327) puts x[(I + shift) % M] at y[I].  Data crosses lanes at
// three places only, and a barrier stands at each: after the message is staged, after the special block is made (its rotation by
// M - d2 or d1 is a gather again), and before the final re-check gathers the parity part.  Everything else -- the partial
// syndrome, its sum over the block rows, the syndrome update and the rh - 1 steps of the dual-diagonal recursion, which upstream
// writes without any rotation -- touches position I of the frame's rows only, so it is ordered by the lane's own program order.
// Integer arithmetic throughout: equality with upstream is integer equality.
//
// Channel.  Lane = position i of a frame, so that for a fixed symbol s a wave stores 64 consecutive doubles of d_soft[b][s][:].
// q <= 16 keeps the q likelihoods in VGPRs; beyond that the lane re-reads its own stores for the normalisation.  The values are
// upstream's: lh accumulates from 0 in the order k = 0 .. q_bits - 1, no contraction, correctly rounded division, glibc's exp.
// The transmitted word is per frame ([B][N]) or one [N] word for all frames (exact replay of upstream's harness, which encodes one
// message before its frame loop); the count kernel takes it the same way.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ldpc_frontend.hpp"
#include "ldpc_spec.hpp"

namespace ldpc_gfq {

constexpr uint32_t kTagNoise = 3u;     // Philox stream tags 0, 1 (binary channel) and 2 (information bits) are taken
constexpr uint32_t kTagMessage = 4u;
constexpr int kEncThreads = 256;

struct EncArgs {
    const int16_t *msg;    // [B][K]
    int16_t *codeword;     // [B][N]
    int32_t *ok;           // [B] or null
    long long B;
    int rh, nh, M, N, R, K, q, F;
    const int16_t *shift;  // [rh][nh] shift reduced to 0 .. M-1, -1 = empty circulant
    const int16_t *lgc;    // [rh][nh] logarithm of the coefficient
    const int16_t *field;  // log[q] | alog[q]
    int weight3;           // special column of weight 3 (else 2)
    int pos_beta;          // its middle block row (weight 3)
    int lg_alpha, lg_gamma, lg_beta;
    int rot_cw;            // the special block of the codeword is the un-rotated one rotated by this (OXO: M - d2, else 0)
    int rot_synd;          // ... and enters rows 0 and rh-1 of the syndrome rotated by this (OXO: M - d2, XOX weight 3: d1, else 0)
};

__host__ __device__ inline size_t enc_lds_bytes(int F, int N, int R, int M, int q) {
    const size_t i16 = ((size_t)2 * q + (size_t)F * ((size_t)N + R + M) + 1) & ~(size_t)1;   // the int32 flags behind stay aligned
    return sizeof(int16_t) * i16 + sizeof(int32_t) * (size_t)F;
}

#if defined(__HIPCC__)

__global__ __launch_bounds__(kEncThreads) void gfq_encode_kernel(const EncArgs a) {
    extern __shared__ int16_t enc_lds[];
    const int q = a.q, M = a.M, N = a.N, R = a.R, K = a.K, mod = a.q - 1;
    int16_t *lg = enc_lds, *alog = enc_lds + q;
    int16_t *cw_all = enc_lds + 2 * q;
    int16_t *synd_all = cw_all + (size_t)a.F * N;
    int16_t *mb_all = synd_all + (size_t)a.F * R;
    int32_t *ok_all = reinterpret_cast<int32_t *>(enc_lds + (((size_t)2 * q + (size_t)a.F * ((size_t)N + R + M) + 1) & ~(size_t)1));
    const int tid = (int)threadIdx.x;

    // x * c and x / c for a coefficient given by its logarithm (x = 0 stays 0, as MulTable's row 0 does)
    auto mul = [&](int x, int lc) -> int {
        if (x == 0) return 0;
        int e = lg[x] + lc;
        if (e >= mod) e -= mod;
        return alog[e];
    };
    auto dvd = [&](int x, int lc) -> int {
        if (x == 0) return 0;
        int e = lg[x] - lc;
        if (e < 0) e += mod;
        return alog[e];
    };

    const long long f0 = (long long)blockIdx.x * a.F;
    const int nf = (int)(a.B - f0 < a.F ? a.B - f0 : a.F);   // frames of this workgroup
    for (int t = tid; t < 2 * q; t += kEncThreads) enc_lds[t] = a.field[t];
    // the message: one contiguous run of nf * K symbols, read once
    for (long long t = tid; t < (long long)nf * K; t += kEncThreads) {
        const int f = (int)(t / K), i = (int)(t - (long long)f * K);
        cw_all[(size_t)f * N + i] = (int16_t)(a.msg[f0 * K + t] & mod);   // a symbol outside 0 .. q-1 breaks the precondition; it must not leave the tables
    }
    if (tid < a.F) ok_all[tid] = 1;
    __syncthreads();

    // lane -> (frame slot, first position); M >= 256: slot 0 and a stride of 256
    const int f = a.F > 1 ? tid / M : 0;
    const int I0 = a.F > 1 ? tid - f * M : tid;
    const int step = a.F > 1 ? M : kEncThreads;
    const bool live = f < nf;
    int16_t *cw = cw_all + (size_t)f * N, *synd = synd_all + (size_t)f * R, *mb = mb_all + (size_t)f * M;
    const int cb = a.nh - a.rh;   // the special column

    if (live)
        for (int I = I0; I < M; I += step) {
            // partial syndrome over the information columns (:1541-1569), its sum over the block rows (:1572-1578), and the special
            // block before rotation (:1580-1581)
            int sum = 0;
            for (int i = 0; i < a.rh; ++i) {
                int acc = 0;
                for (int j = 0; j < cb; ++j) {
                    const int s = a.shift[i * a.nh + j];
                    if (s < 0) continue;
                    int p = I + s;
                    if (p >= M) p -= M;
                    acc ^= mul(cw[j * M + p], a.lgc[i * a.nh + j]);
                }
                synd[i * M + I] = (int16_t)acc;
                sum ^= acc;
            }
            mb[I] = (int16_t)dvd(sum, a.lg_beta);
        }
    __syncthreads();
    if (live)
        for (int I = I0; I < M; I += step) {
            int p = I + a.rot_cw;
            if (p >= M) p -= M;
            cw[K + I] = mb[p];                                   // :1584-1593
            p = I + a.rot_synd;
            if (p >= M) p -= M;
            const int ms = mb[p];
            int s0 = synd[I] ^ mul(ms, a.lg_alpha);              // :1596-1626
            if (a.weight3) {
                int sum = 0;   // sumsynd[I] again: the rows as the first phase left them
                for (int i = 0; i < a.rh; ++i) sum ^= synd[i * M + I];
                synd[I] = (int16_t)s0;
                synd[a.pos_beta * M + I] ^= (int16_t)sum;
                synd[(a.rh - 1) * M + I] ^= (int16_t)mul(ms, a.lg_gamma);
                s0 = synd[I];
            } else {
                synd[I] = (int16_t)s0;
                synd[(a.rh - 1) * M + I] ^= (int16_t)mul(ms, a.lg_gamma);
            }
            // dual-diagonal recursion (:1629-1644): row j gives column cb + 1 + j, then is added to row j + 1
            int run = s0;
            for (int j = 0; j + 1 < a.rh; ++j) {
                const int col = cb + 1 + j;
                cw[col * M + I] = (int16_t)dvd(run, a.lgc[j * a.nh + col]);
                run ^= synd[(j + 1) * M + I];
                synd[(j + 1) * M + I] = (int16_t)run;
            }
        }
    __syncthreads();
    if (live) {
        // the full re-check (:1646-1692)
        int bad = 0;
        for (int I = I0; I < M; I += step)
            for (int i = 0; i < a.rh; ++i) {
                int acc = 0;
                for (int j = 0; j < a.nh; ++j) {
                    const int s = a.shift[i * a.nh + j];
                    if (s < 0) continue;
                    int p = I + s;
                    if (p >= M) p -= M;
                    acc ^= mul(cw[j * M + p], a.lgc[i * a.nh + j]);
                }
                bad |= acc;
            }
        if (bad) ok_all[f] = 0;   // every writer stores the same value
    }
    __syncthreads();
    for (long long t = tid; t < (long long)nf * N; t += kEncThreads) a.codeword[f0 * N + t] = cw_all[t];
    if (a.ok && tid < nf) a.ok[f0 + tid] = ok_all[tid];
}

struct MsgArgs {
    int16_t *msg;   // [B][K]
    long long B, first_frame;
    int K, q;
    uint64_t seed;
};

// symbol i of global frame g: word i % 4 of the Philox block (g, i / 4, tag 4), reduced mod q (q is a power of two)
__global__ __launch_bounds__(256) void gfq_message_kernel(const MsgArgs a) {
    const int blocks = (a.K + 3) / 4;
    const long long total = a.B * (long long)blocks;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long b = t / blocks;
        const int g = (int)(t - b * blocks);
        const uint64_t fr = (uint64_t)(a.first_frame + b);
        const ldpc::Philox4 p = ldpc::philox4x32_10((uint32_t)fr, (uint32_t)(fr >> 32), (uint32_t)g, kTagMessage, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if (4 * g + w < a.K) a.msg[b * a.K + 4 * g + w] = (int16_t)(p.x[w] & (uint32_t)(a.q - 1));
    }
}

struct QChanArgs {
    const int16_t *codeword;   // [B][N], or one [N] word for all frames (cw_stride = 0), or null = the all-zero word
    long long cw_stride;       // symbols from one frame's word to the next: N or 0
    const int32_t *ok;         // [B] or null; a frame with ok = 0 goes out as the all-zero word (bp_simulation.cpp:552-556)
    const double *noise;       // [B][N * q_bits] or null = Philox
    double *soft;              // [B][q][N]
    long long B, first_frame;
    int N, q_bits;
    double sigma;
    uint64_t seed;
};

// The symbol probabilities of one position (bp_simulation.cpp:641, :644-676) from the q_bits Gaussians g[] of the position and the
// symbol sym that was sent there: out[s * N], s = 0 .. q-1.  The one statement of this arithmetic: the single-code channel and the
// channel of a code set with per-code words (ldpc_gfq_codeset.hpp) both call it.  q <= 16 keeps the q likelihoods in VGPRs; beyond that
// the lane re-reads its own stores for the normalisation.
template <int QB>
__device__ __forceinline__ void gfq_symbol_probabilities(int sym, const double (&g)[QB], double sigma, double s2, double *out, int N) {
    constexpr int qb = QB, q = 1 << QB, QREG = QB <= 4 ? q : 0;
    double x[QB];
#pragma unroll
    for (int k = 0; k < qb; ++k) {
        const double c = (double)((sym >> (qb - 1 - k)) & 1);   // word2bin: most significant bit first
        x[k] = sigma * g[k] + 2.0 * c - 1.0;                   // :641
    }
    auto likelihood = [&](int s) -> double {
        double lh = 0;
#pragma unroll
        for (int k = 0; k < qb; ++k) lh += ((s >> (qb - 1 - k)) & 1) ? x[k] : -x[k];   // V[k] * x[k], V = +-1 (:656-662)
        return ldpc_spec::exp_glibc_wide(lh / s2, ldpc_spec::kExpTab);                // :664, :670
    };
    if constexpr (QREG != 0) {
        double e[QREG ? QREG : 1], sum = 0.0;
#pragma unroll
        for (int s = 0; s < QREG; ++s) { e[s] = likelihood(s); sum += e[s]; }
#pragma unroll
        for (int s = 0; s < QREG; ++s) out[(size_t)s * N] = e[s] / sum;
    } else {
        double sum = 0.0;
        for (int s = 0; s < q; ++s) { const double e = likelihood(s); out[(size_t)s * N] = e; sum += e; }
        for (int s = 0; s < q; ++s) out[(size_t)s * N] /= sum;   // the lane's own stores
    }
}

// One instance per q_bits, so that the bits of a symbol and (q <= 16) its likelihoods sit in VGPRs under static indices.
template <int QB>
__global__ __launch_bounds__(256) void gfq_channel_kernel(const QChanArgs a) {
    constexpr int qb = QB, q = 1 << QB;
    const int N = a.N;
    const long long total = a.B * (long long)N;
    const double s2 = a.sigma * a.sigma;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long b = t / N;
        const int i = (int)(t - b * N);
        int sym = 0;
        if (a.codeword && (!a.ok || a.ok[b])) sym = a.codeword[b * a.cw_stride + i];
        double g[QB];
        uint32_t have = 0xffffffffu;
        double g0 = 0, g1 = 0;
#pragma unroll
        for (int k = 0; k < qb; ++k) {
            const long long bit = (long long)i * qb + k;   // index of the bit within the frame
            if (a.noise) {
                g[k] = a.noise[b * ((long long)N * qb) + bit];
            } else {
                const uint32_t pair = (uint32_t)(bit >> 1);
                if (pair != have) { ldpc::gauss_pair(a.seed, (uint64_t)(a.first_frame + b), pair, kTagNoise, g0, g1); have = pair; }
                g[k] = (bit & 1) ? g1 : g0;
            }
        }
        gfq_symbol_probabilities<QB>(sym, g, a.sigma, s2, a.soft + (size_t)b * q * N + i, N);
    }
}

struct QCountArgs {
    const int16_t *qhard;      // [B][N]
    const int16_t *codeword;   // [B][N], or one [N] word for all frames (cw_stride = 0), or null = zero
    long long cw_stride;       // symbols from one frame's word to the next: N or 0
    const int32_t *ok;         // [B] or null; ok = 0: the frame carried the all-zero word
    const int32_t *iters;      // [B]
    int32_t *frame_info;       // [B] or null
    unsigned long long *counters;   // [5]: nse, nde, nue, frames, sum |iters|
    long long B;
    int N, R;
};

// The shared count of ldpc_frontend.hpp on symbols: frames blockIdx.x * 4 + wave, + 4 * grid, ...; a frame's word is its row of
// `codeword` (cw_stride = 0: one word for all), or the all-zero word where ok says that nothing else was sent.
__global__ __launch_bounds__(256) void gfq_count_kernel(const QCountArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    ldpc::ErrorTally tally;
    for (long long fr = (long long)blockIdx.x * 4 + wv; fr < a.B; fr += (long long)gridDim.x * 4) {
        const bool sent = a.codeword && (!a.ok || a.ok[fr]);
        uint32_t all = 0, info = 0;
        ldpc::symbol_errors(a.qhard + fr * a.N, sent ? a.codeword + fr * a.cw_stride : nullptr, a.N, a.R, lane, all, info);
        ldpc::wave_sum_pair(all, info);
        if (lane == 0) tally.add(all, info, a.iters[fr], a.frame_info ? a.frame_info + fr : nullptr);
    }
    tally.flush(a.counters);
}

#endif  // __HIPCC__

}  // namespace ldpc_gfq
