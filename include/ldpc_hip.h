/*
 * ldpc_hip.h -- C-ABI of the MI355X (gfx950) batched QC-LDPC belief-propagation path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.  It is what a cgo /
 * ctypes / JNI / C++ caller binds.  The upstream library (eovs/ldpc-lib) is C++ with no FFI of its own; each
 * entry point below cites the upstream interface it replaces (file:line in the upstream tree).  The C++
 * source-compatible layer (include/ldpc/decoders.h, include/ldpc/bp_simulation.h) is a thin wrapper over
 * these functions; INTEGRATION.md shows how a maintainer links it.
 *
 * Conventions (identical to upstream, decoders.cpp:327-346 / bp_simulation.cpp:54,738):
 *   base matrix hd[j*nh+k], -1 = empty circulant, else shift 0 <= c < M (values are reduced mod M)
 *   check (j,n) is connected to variable (k,(n+c) mod M); variable (k,i) is LLR index k*M+i
 *   positive LLR <=> bit 0;  parity part = indices [0,R), information part = [R,N)
 *   decoder return value ("iters"): >0 converged after that many iterations, 0 input already a codeword
 *   (sum-product only), <0 = -(iterations run), not converged                      (decoders.cpp:4766,2184,5424)
 *
 * All functions return 0 on success and a negative LDPC_HIP_E* code on failure; ldpc_hip_last_error()
 * gives the message of the calling thread's last failure.  There is NO CPU fallback: if no HIP device /
 * code object is available every call fails loudly.
 */
#ifndef LDPC_HIP_H
#define LDPC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_HIP_ABI_VERSION 4

/* decoders.h:16-28 enum DEC_ID (all ten are built; the nine binary decoders through ldpc_hip_open, FHT_DEC through ldpc_hip_open_gfq) */
#define LDPC_HIP_BP_DEC 0  /* bp_decod_qc_lm         decoders.cpp:1708 (Gallager BP, log domain) */
#define LDPC_HIP_SP_DEC 1  /* sum_prod_decod_qc_lm   decoders.cpp:1923 */
#define LDPC_HIP_ASP_DEC 2 /* sum_prod_gf2_decod_qc_lm decoders.cpp:2324 (probability-domain flooding sum-product) */
#define LDPC_HIP_MS_DEC 3  /* min_sum_decod_qc_lm    decoders.cpp:4554 */
#define LDPC_HIP_IMS_DEC 4 /* imin_sum_decod_qc_lm   decoders.cpp:5430 */
#define LDPC_HIP_IASP_DEC 5 /* isum_prod_gf2_decod_qc_lm decoders.cpp:3822 (integer advanced sum-product, IASP_FIXED_POINT build) */
#define LDPC_HIP_FHT_DEC 6  /* sum_prod_gfq_decod_lm   decoders.cpp:7036 (GF(q) sum-product, check nodes in the Walsh-Hadamard domain): its own
                             * entry points, ldpc_hip_open_gfq / ldpc_hip_decode_gfq_*, below; ldpc_hip_open(6, ...) has no coefficient matrix and fails */
#define LDPC_HIP_TASP_DEC 7 /* tdmp_sum_prod_gf2_decod_qc_lm decoders.cpp:2584 (decoder_type of the shipped scenario files) */
#define LDPC_HIP_LMS_DEC 8 /* lmin_sum_decod_qc_lm   decoders.cpp:5064 */
#define LDPC_HIP_LCHE_DEC 9 /* lche_decod            decoders.cpp:2899 (low-complexity high-efficiency decoder, layered, LLR domain) */

#define LDPC_HIP_EINVAL (-1)    /* bad argument */
#define LDPC_HIP_EUNSUPPORTED (-2) /* decoder / code shape not built */
#define LDPC_HIP_EHIP (-3)      /* HIP runtime error (message has hipGetErrorString) */
#define LDPC_HIP_ENOMEM (-4)

typedef struct ldpc_hip_ctx ldpc_hip_ctx;

int ldpc_hip_abi_version(void);
const char *ldpc_hip_last_error(void);
int ldpc_hip_device_count(void);

/* Replaces decod_open() + the hd fill + decod_init()  (decoders.h:293-294, decoders.cpp:348,1009,
 * bp_simulation.cpp:353-382).  hd is row-major rh x nh.  device = HIP device ordinal.
 * *out receives the context; NULL on failure (upstream: decod_open returns NULL).
 * ASP_DEC, IASP_DEC and TASP_DEC refuse codes with a block row of weight < 2 (LDPC_HIP_EUNSUPPORTED): upstream's check-node
 * routines read an uninitialised forward / backward product for such a row (decoders.cpp:2191-2228, :2235-2271).
 * LCHE_DEC refuses codes with a block row of weight > 1024: upstream's map_bin_llr keeps a check's edges in static arrays of 1024
 * (decoders.cpp:2818-2822). */
int ldpc_hip_open(int decoder_id, int rh, int nh, int M, const int16_t *hd, int device, ldpc_hip_ctx **out);
/* Replaces decod_close() (decoders.h:295, decoders.cpp:1210). */
void ldpc_hip_close(ldpc_hip_ctx *ctx);

int ldpc_hip_n(const ldpc_hip_ctx *ctx);          /* N = nh*M */
int ldpc_hip_r(const ldpc_hip_ctx *ctx);          /* R = rh*M */
int ldpc_hip_edges(const ldpc_hip_ctx *ctx);      /* non-empty circulants */
int ldpc_hip_hard_words(const ldpc_hip_ctx *ctx); /* ceil(N/32): uint32 words per frame of packed hard bits */
/* Name of the decode kernel this context launches (code-specialised AOT / hiprtc instance, table-driven, generic). */
const char *ldpc_hip_kernel_name(const ldpc_hip_ctx *ctx);
/* Where ldpc_hip_open gets the code-specialised kernel of a base matrix that has no ahead-of-time instance (process-wide default; the
 * environment variable LDPC_HIP_JIT = 0 / sync / async overrides it): 0 never (table-driven or shape-unlimited kernels only),
 * 1 hiprtc inside ldpc_hip_open (seconds per new code, milliseconds from the on-disk cache) [default], 2 in the background: the
 * context starts on its table-driven / shape-unlimited kernel and moves to the instance at the first launch after it is ready --
 * every tier returns identical bits, so a run may change tier in flight.  Mode 2 is what a code search wants (upstream's
 * main_good_code_search.cpp:320 calls bp_simulation once per candidate matrix); ldpc::bp_simulation_t selects it.
 * Returns the previous mode, or LDPC_HIP_EINVAL. */
int ldpc_hip_set_jit_mode(int mode);
/* The same choice for the CALLING THREAD only (-1 = no override; the environment variable still wins).  Returns the thread's previous
 * override.  The C++ harnesses use this around their ldpc_hip_open_multi so that concurrent callers do not see each other's mode. */
int ldpc_hip_set_jit_mode_thread(int mode);
/* Name of the kernel the last ldpc_hip_decode_dev call on this context launched.  It differs from ldpc_hip_kernel_name only
 * for IMS_DEC with parameters beyond int8 (MS_DBITS > 8, MS_QBITS > 8, alpha > 1 or alpha < 0), which run on the table-driven int32
 * kernel, and for MS_DEC with an alpha that is not above zero, which runs on ms_global_kernel (see ldpc_hip_decode_dev). */
const char *ldpc_hip_last_launch(const ldpc_hip_ctx *ctx);
/* 1 when that launch ran the instance of its kernel that holds no soft values: the M = 64 min-sum body has one (same name, same
 * bits) and takes it when the call passes no soft_out; 0 for every other launch. */
int ldpc_hip_last_launch_without_soft(const ldpc_hip_ctx *ctx);

/* Batched replacement of the decoder entry points (decoders.h:297,299,304; dispatch bp_simulation.cpp:716-729):
 *   MS_DEC : min_sum_decod_qc_lm(st, y, decword, maxiter, decision, alpha)
 *   LMS_DEC: lmin_sum_decod_qc_lm(st, y, decword, maxiter, decision, alpha, beta)   (alpha, beta dead upstream)
 *   SP_DEC : sum_prod_decod_qc_lm(st, soft, decword, maxiter, decision)
 *   IMS_DEC: imin_sum_decod_qc_lm(st, y, decword, maxiter, decision, alpha, thr, qbits, dbits)  (int16 min-sum)
 *   BP_DEC:  bp_decod_qc_lm(st, soft, decword, maxiter, decision)                  (d_soft = a-posteriori LLR)
 *   ASP_DEC: sum_prod_gf2_decod_qc_lm(st, soft, decword, maxiter, decision)       (d_soft = a-posteriori P(bit=1))
 *   TASP_DEC: tdmp_sum_prod_gf2_decod_qc_lm(st, soft, decword, maxiter, decision)  (d_soft = final P(bit=1); `decision` dead)
 *   IASP_DEC: isum_prod_gf2_decod_qc_lm(st, soft, decword, maxiter, decision)     (d_soft = soft_out / 65536, the u16 Q16
 *            a-posteriori word as upstream's decision == 1 output; hard bit = soft_out >> 15.  Integer arithmetic throughout:
 *            bit for bit with no libm argument except the channel transform's exp, which is glibc's)
 *   LCHE_DEC: lche_decod(st, soft, decword, maxiter, decision)                     (d_soft = the final a-posteriori LLRs, upstream's
 *            lche_soft_out; for a return of 0 it is the input bit for bit, -0.0 included.  The input is never modified, `decision`
 *            is dead: d_hard is always filled.  Only fp64 adds, compares, exact scalings and table lookups: bit for bit)
 * All pointers are DEVICE pointers on ctx's device; the work is enqueued on `stream` (a hipStream_t, NULL =
 * default stream) and is asynchronous.  maxiter must be >= 1 (upstream's behaviour for maxiter <= 0 is an artefact of
 * stale state and is not reproduced: LDPC_HIP_EINVAL).  LLRs must be finite.
 *   d_llr   [B][N] float64 in.   NOT modified (upstream SP clobbers its input; the clobbered values are what
 *           d_soft receives, see below)
 *   d_hard  [B][ceil(N/32)] uint32 out: bit (v%32) of word v/32 = hard decision of variable v
 *           (upstream decword[v] = soft<0, resp. soft<1.0 for SP), or NULL
 *   d_iters [B] int32 out: upstream return value, or NULL
 * Numerics: outputs equal upstream's on the same inputs bit for bit -- hard decisions, return values and soft values -- for
 * MS, LMS, IMS (no transcendental on their path) and for SP, ASP and TASP against an upstream built with glibc >= 2.28 on an
 * FMA-capable x86-64 host (fp64 in upstream's operation order, no FMA contraction; exp() is evaluated with that glibc's own
 * algorithm and evaluation order -- an upstream linked against another libm, e.g. MSVC's from the vs2005/vs2010 projects, may
 * differ from it, and so from this library, in the last ulp of soft values; hard decisions and return values are expected equal);
 * BP: likewise bit for bit (its exp / log are glibc's algorithms on the device too).
 *   d_soft  [B][N] float64 out, or NULL: the a-posteriori values upstream writes to decword[] when decision==1
 *           (MS/LMS: LLR; SP: likelihood ratio = what upstream leaves in soft[])
 * alpha: read by MS_DEC and IMS_DEC only.  Any alpha > 0 runs on the context's own kernel.  MS_DEC with alpha <= 0 (-0.0 included:
 * upstream keeps the sign of m * alpha, decoders.cpp:4719-4720, and its y + acc * alpha can be -0.0) gives upstream's bits too, from the
 * shape-unlimited tier's kernel, whatever tier the context is on.  NaN is LDPC_HIP_EINVAL for MS_DEC and IMS_DEC.
 */
int ldpc_hip_decode_dev(ldpc_hip_ctx *ctx, const double *d_llr, long long B, int maxiter, double alpha,
                        uint32_t *d_hard, int32_t *d_iters, double *d_soft, void *stream);

/* BP_DEC only.  Upstream's bp_decod_qc_lm does not clear DEC_STATE::syndr before its input check (decoders.cpp:1742-1762),
 * so frame b's check sees the syndrome frame b-1 left behind (non-zero after a failed frame).  With the chain ON (default)
 * the frames of one ldpc_hip_decode_dev call are decoded as if one after the other on one DEC_STATE, continuing from the
 * last frame of the previous call on this context; ldpc_hip_decode_dev then synchronises the stream.  on == 0: every
 * frame starts from a zero syndrome (asynchronous, independent of batching).  reset_carry != 0 forgets the carried
 * syndrome (what decod_close + decod_open would do). */
int ldpc_hip_set_bp_chain(ldpc_hip_ctx *ctx, int on, int reset_carry);

/* Integer min-sum only: the quantiser arguments of imin_sum_decod_qc_lm (decoders.h:300; defaults MS_THR 1.4,
 * MS_QBITS 6, MS_DBITS 8 of decoders.h:46-48).  `alpha` of the decode calls gives ialpha = (int)(alpha*16).  Also on a code-set
 * context of ldpc_hip_open_codes_ims, for its next call. */
int ldpc_hip_set_ims_params(ldpc_hip_ctx *ctx, double thr, int qbits, int dbits);

/* Same with HOST pointers, laid out exactly like upstream's per-frame arrays (PCIe-inclusive, synchronous):
 *   llr [B][N] in (for SP it is overwritten like upstream's soft[] when clobber_sp_input != 0; for ASP and TASP it then holds
 *   P(bit = 1) of the channel, for IASP 1 / (1 + exp(clamp(llr, -20, 20))) as decoders.cpp:3858-3863 leaves it),
 *   decword [B][N] float64 out (0.0/1.0 when decision==0, a-posteriori values when decision==1), iters [B]. */
int ldpc_hip_decode_host(ldpc_hip_ctx *ctx, double *llr, long long B, int maxiter, int decision, double alpha,
                         double *decword, int32_t *iters, int clobber_sp_input);

/* ---- the transmit / receive chain around the decoder ------------------------------------------------------------------
 * Upstream's frame loop sends codeword -> direct interleaver -> mapper -> AWGN -> soft demapper -> inverse interleaver ->
 * puncturing -> decoder and counts decword[i] != codeword[i] (bp_simulation.cpp:566-577, 596-710, 731-759).  A context starts in
 * upstream's shipped wiring -- the all-zero codeword (bp_simulation.cpp:568 overwrites the encoder's output) and
 * permutation_type 0 (files/default_constants.jsonx:6) -- and the two setters below change that for every later channel /
 * count / simulate call on the context. */

/* Interleaver of the chain: Permutations_Open / Permutation_Init (direct_inverse_perm.cpp:139-783) with permutation_type 0..4,
 * permutation_block, permutation_inter of bp_simulation.h:21-23; halfmlog follows the modulation of each call
 * (bp_simulation.cpp:402-411).  Fails (and leaves the identity) when the mode does not accept this code shape. */
int ldpc_hip_set_interleaver(ldpc_hip_ctx *ctx, int permutation_type, int permutation_block, int permutation_inter);
/* Transmitted codewords: HOST array [ncw][N] of 0/1 bytes in decoder order (e.g. from ldpc_hip_encode_host); global frame f
 * carries codeword f % ncw.  ncw == 0 returns to the all-zero codeword.  (Replaces the `codeword` vector of
 * bp_simulation.cpp:506-568; upstream draws ONE random codeword per call and then zeroes it.) */
int ldpc_hip_set_codewords(ldpc_hip_ctx *ctx, const uint8_t *codewords, int ncw);

/* The chain from codeword to decoder input for frames [first_frame, first_frame + B), on the device:
 *   modulation_type 0 BPSK ("SKIP"), 1 QAM4: llr = -2*(sigma*g + 2*bit - 1)/sigma^2 (bp_simulation.cpp:603,610, sigma :445 / :449);
 *   2 / 3 / 4 = QAM16 / 64 / 256 (modulation.h:4-11): GrayPAM mapper (QAM_modulator.cpp:129-194), x + sigmaQAM*g fresh per frame
 *   (the evidently intended chain), per-rail soft demapper with cut-off T (QAM_demodulator.cpp:203-561),
 *   negated (:627-628); the last symbol is padded with zero bits (:575).
 * Then y[i] = buffer[inverse[i]] (:684) and the last M*punctured_blocks LLRs are set to 0.5 (LLR-type decoders) or 0
 * (probability-type) exactly as upstream (sic, Q7; :697-710) -- for EVERY modulation, with the punctured bitrate in sigma (:444).
 * g ~ N(0,1) from a counter-based Philox4x32-10 stream keyed by (seed, global frame index, channel position), so the result
 * does not depend on batch split, GPU count, interleaver or codeword. */
int ldpc_hip_channel_llr_dev(ldpc_hip_ctx *ctx, double snr_db, int modulation_type, int punctured_blocks, double T, uint64_t seed,
                             long long first_frame, long long B, double *d_llr, void *stream);
/* Earlier names of the same chain: BPSK / QAM4 (T unused), and QAM16+ without puncturing. */
int ldpc_hip_awgn_llr_dev(ldpc_hip_ctx *ctx, double snr_db, int modulation_type, int punctured_blocks,
                          uint64_t seed, long long first_frame, long long B, double *d_llr, void *stream);
int ldpc_hip_awgn_qam16_llr_dev(ldpc_hip_ctx *ctx, double snr_db, double T, uint64_t seed, long long first_frame,
                                long long B, double *d_llr, void *stream);
int ldpc_hip_awgn_qam_llr_dev(ldpc_hip_ctx *ctx, int modulation_type, double snr_db, double T, uint64_t seed, long long first_frame,
                              long long B, double *d_llr, void *stream);

/* Function-level mapper: QAM_modulator.cpp:142-194 QAM_modulator() for Q in {4,16,64,256}.  d_bits [ns][log2 Q] bytes 0/1 (first half
 * of a symbol's bits = I rail, MSB first; upstream passes them as doubles) -> d_x [ns][2] (I, Q interleaved) PAM levels. */
int ldpc_hip_qam_modulate_dev(int Q, const uint8_t *d_bits, long long ns, double *d_x, int device, void *stream);

/* Function-level soft demapper: QAM_demodulator.cpp:99-566 Demodulate() for Q in {4,16,64,256}, out_type 0/1 (Q = 4: out_type 0 only).
 * d_x [ns][2] (I,Q interleaved) -> d_out [ns][log2 Q]. */
int ldpc_hip_qam_demod_dev(int Q, double T, double sigma, const double *d_x, long long ns, double *d_out,
                           int out_type, int device, void *stream);

/* Systematic encoder for the dual-diagonal QC-LDPC codes upstream's search produces (qc_encode / random_codeword,
 * bp_simulation.cpp:22-191, with the information bits given instead of drawn).  HOST function.  info_bits: (nh-rh)*M bytes
 * (0/1) for variable positions [rh*M, nh*M); codeword: nh*M bytes out, parity first.  Upstream's simulation never transmits
 * the result (it zeroes the codeword, :568); this entry exists for callers that do and for the sign-symmetry tests. */
int ldpc_hip_encode_host(int rh, int nh, int M, const int16_t *hd, const uint8_t *info_bits, uint8_t *codeword);

/* The same encoder on the device (csrc/ldpc_encode.hpp): d_info_bits [B][(nh-rh)*M] bytes 0/1 -> d_codewords [B][nh*M] bytes, parity
 * first, identical to ldpc_hip_encode_host -- also for base matrices whose parity part consists of several dual-diagonal blocks
 * (bp_simulation.cpp:142-191: encoded from the last block to the first). */
int ldpc_hip_encode_dev(ldpc_hip_ctx *ctx, const uint8_t *d_info_bits, long long B, uint8_t *d_codewords, void *stream);
/* A table of ncw random codewords made on the device (information bits from Philox4x32-10 keyed by seed and codeword index, then the
 * device encoder) and installed like ldpc_hip_set_codewords: global frame f carries codeword f % ncw.  ncw == 0 returns to the all-zero
 * codeword.  (What upstream's random_codeword() is for, bp_simulation.cpp:142-191, before :568 zeroes its result.) */
int ldpc_hip_set_random_codewords(ldpc_hip_ctx *ctx, uint64_t seed, int ncw);

/* Bit interleavers of the simulation chain (Permutations_Open / Permutation_Init / Permutation,
 * direct_inverse_perm.cpp:139-900; permutation_type of bp_simulation.h:21-23): mode 0 identity, 1 random, 2 deterministic,
 * 3 block random (block_size), 4 interleaved random (step_size); halfmlog = 1 (BPSK / QAM4), 2, 3, 4 (QAM16 / 64 / 256).
 * HOST function (no GPU needed): fills the two gather maps, out[i] = in[map[i]], direct[N] (encoder -> mapper side) and
 * inverse[N] (demapper -> decoder side), N = c*M, identical to upstream's for the same arguments (same LCG, same order). */
int ldpc_hip_interleaver_build(int b, int c, int M, int halfmlog, int mode, int block_size, int step_size, const int16_t *hd,
                               int32_t *direct, int32_t *inverse);
/* Applies a map to B frames resident on the device: d_out[f][i] = d_in[f][d_map[i]] (d_in != d_out). */
int ldpc_hip_permute_dev(const double *d_in, double *d_out, long long B, int N, const int32_t *d_map, int device, void *stream);

/* Error accounting, replaces bp_simulation.cpp:731-759,805-810: hard decisions against the transmitted codeword of each frame
 * (global frame first_frame + f carried codeword (first_frame + f) % ncw; all-zero when none is set).
 *   d_frame_info [B] int32 out (or NULL): number of wrong information bits (index >= R) of the frame, with bit 30
 *                set when the frame has any wrong bit at all (so 0 == frame correct)
 *   d_counters [5] uint64 in/out (accumulated with atomics; caller zeroes): nse, nde, nue, frames, sum |iters| */
int ldpc_hip_count_errors_cw_dev(ldpc_hip_ctx *ctx, const uint32_t *d_hard, const int32_t *d_iters, long long first_frame, long long B,
                                 int32_t *d_frame_info, unsigned long long *d_counters, void *stream);
/* Same with first_frame = 0 (enough for the all-zero codeword or a single codeword; EINVAL when several are set). */
int ldpc_hip_count_errors_dev(ldpc_hip_ctx *ctx, const uint32_t *d_hard, const int32_t *d_iters, long long B,
                              int32_t *d_frame_info, unsigned long long *d_counters, void *stream);

/* One fused Monte-Carlo batch on the device: chain -> decode -> count, frames [first_frame, first_frame+B), with the
 * context's interleaver and codewords.  Uses internal workspace (grown on demand).  counters[4] (host) receive this batch's
 * {nse, nde, nue, frames}; sum_abs_iters (host, may be NULL) the sum of |iters| for throughput accounting.
 * Synchronous.  No stopping rule here: the sequential stopping rule of bp_simulation.cpp:591,820 is applied
 * by the host layer on the ordered per-frame records (ldpc::bp_simulation). */
int ldpc_hip_simulate(ldpc_hip_ctx *ctx, double snr_db, int modulation_type, int punctured_blocks, int maxiter,
                      double alpha, uint64_t seed, long long first_frame, long long B,
                      unsigned long long counters[4], unsigned long long *sum_abs_iters);

/* ---- upstream's own noise, bit for bit, on the device (exact replay at device speed) --------------------------------------
 * bp_simulation() draws every noise sample from ONE std::mt19937 through next_random_gaussian(), a fresh
 * std::normal_distribution<double> per call (commons_portable.cpp:140,174-178; bp_simulation.cpp:600-611).  These entry points
 * continue THAT stream on the GPU: the context holds a generator state in std::mt19937's own terms -- the 624 state words and
 * the index of the next word, exactly what `os << generator` prints with libstdc++ -- and every call below consumes from it
 * precisely the 32-bit words the host loop would (four per polar-method attempt, libstdc++ bits/random.tcc:1802-1835,3348-3380).
 * Values equal the host's bit for bit on a host whose libm log() is glibc >= 2.28's FMA variant (the contract of the decoders'
 * exp / log above).  ldpc::bp_simulation_t (include/ldpc/bp_simulation.h) and the drop-in bp_simulation symbol use them, so the
 * exact-replay harness is no longer bound by the host generator (~7e3 frames/s per core at N = 2048). */
/* host only, no GPU: the state 2^log2_words words further on (18 <= log2_words <= 30), as the device computes it: GF(2)
 * polynomial jump x^(2^k) mod the generator's minimal polynomial.  state_out[1..623] are the generator's words; of state_out[0]
 * only bit 31 is state (the recurrence never reads the rest). */
int ldpc_hip_mt_jump_host(const uint32_t state_in[624], int log2_words, uint32_t state_out[624]);
/* Load / read the generator: state[624] + pos (0..624) as libstdc++ streams a std::mt19937.  set also restarts the context's frame
 * count (which of the ldpc_hip_set_codewords codewords a frame carries: frame f -> codeword f % ncw). */
int ldpc_hip_mt_set_state(ldpc_hip_ctx *ctx, const uint32_t state[624], int pos);
int ldpc_hip_mt_get_state(ldpc_hip_ctx *ctx, uint32_t state[624], int *pos);
/* The frame count that belongs to a snapshot: a caller that rolls the generator back with ldpc_hip_mt_set_state (the harness after an
 * early stop, bp_simulation.cpp:820) and keeps drawing restores it too, so that frame f of the run still carries codeword f % ncw. */
long long ldpc_hip_mt_get_frame_index(const ldpc_hip_ctx *ctx);
int ldpc_hip_mt_set_frame_index(ldpc_hip_ctx *ctx, long long frames_taken);
/* The next `count` values of next_random_gaussian() (commons_portable.cpp:174-178) to d_out [count] (device; NULL = draw and drop). */
int ldpc_hip_mt_normal_dev(ldpc_hip_ctx *ctx, long long count, double *d_out, void *stream);
/* Same into a HOST array (convenience; the harness uses it to check once per process that the device stream reproduces THIS host's
 * std::normal_distribution before relying on it). */
int ldpc_hip_mt_normal_host(ldpc_hip_ctx *ctx, long long count, double *out);
/* Decoder input of the next B frames exactly as the frame loop builds it: y = -2*(sigma*g + 2*c - 1)/sigma^2 with g drawn in index
 * order (bp_simulation.cpp:600-611, sigma :445 / :449; c = 0 unless ldpc_hip_set_codewords), inverse interleaver (:684,
 * ldpc_hip_set_interleaver), puncturing (:697-710).  modulation_type 0 or 1.  d_llr [B][N] device, NULL = draw and drop (used to put
 * the generator where a frame-by-frame loop that stopped early would have left it).  Synchronises `stream`. */
int ldpc_hip_mt_llr_dev(ldpc_hip_ctx *ctx, double snr_db, int modulation_type, int punctured_blocks, long long B, double *d_llr, void *stream);
/* ldpc_hip_mt_llr_dev -> decode -> count for the next B frames; HOST arrays frame_info[B], iters[B] as in ldpc_hip_frames_multi.
 * Synchronous.  The stopping rule (bp_simulation.cpp:591,820) is the caller's, on the ordered records. */
int ldpc_hip_mt_frames(ldpc_hip_ctx *ctx, double snr_db, int modulation_type, int punctured_blocks, int maxiter, double alpha, long long B,
                       int32_t *frame_info, int32_t *iters);
/* One rank's share when every rank (process or shard) runs the same generator: the stream advances by all B frames, frames
 * [lo, hi) are decoded and counted here; frame_info / iters have hi - lo entries. */
int ldpc_hip_mt_frames_slice(ldpc_hip_ctx *ctx, double snr_db, int modulation_type, int punctured_blocks, int maxiter, double alpha, long long B,
                             long long lo, long long hi, int32_t *frame_info, int32_t *iters);

/* The same stream with ONE PROCESS PER GPU: every rank holds a context whose generator is in the same state, and the ranks share the
 * generator's tape out among themselves exactly as ldpc_hip_mt_frames_multi does over the shards of one process -- the three small
 * exchanges are the caller's (torch.distributed, MPI, ...).  One round covers the next `frames` frames (<= 65536), rank r decodes
 * frames [frames*r/n, frames*(r+1)/n):
 *   1. ldpc_hip_mt_shard_begin   makes the sub-streams around this rank's frames and counts the accepted polar-method attempts of
 *                                its stretch -> own_count;                                  all-gather the n counts
 *   2. ldpc_hip_mt_shard_emit    counts[n] in: emits this rank's decoder inputs; out: frames_done (whole frames the round completes, the
 *                                same on every rank), found (this rank holds the state the round ends in -> state_next), covered (0: an
 *                                item of this rank lay outside its window);               all-gather (found, covered); broadcast
 *                                state_next from the lowest rank with found = 1
 *   3. ldpc_hip_mt_shard_commit  installs that state and decodes this rank's frames below frames_done: frame_info / iters receive
 *                                min(frames*(r+1)/n, frames_done) - frames*r/n records.
 * If any rank reports covered = 0 or none reports found = 1 -- an estimate failed; probability ~1e-15 per round -- every rank calls
 * ldpc_hip_mt_shard_abandon and runs the round with ldpc_hip_mt_frames_slice instead (the whole tape on every rank): nothing has
 * been changed before commit.  (ldpc_lib_amd.bp_simulation(exact_seed=...) under torch.distributed does all of this.) */
int ldpc_hip_mt_shard_begin(ldpc_hip_ctx *ctx, double snr_db, int modulation_type, int punctured_blocks, long long frames, int rank, int n,
                            unsigned long long *own_count);
int ldpc_hip_mt_shard_emit(ldpc_hip_ctx *ctx, const unsigned long long *counts, int *found, int *covered, uint32_t state_next[624],
                           long long *frames_done);
int ldpc_hip_mt_shard_commit(ldpc_hip_ctx *ctx, const uint32_t state[624], long long frames_done, int maxiter, double alpha,
                             int32_t *frame_info, int32_t *iters);
void ldpc_hip_mt_shard_abandon(ldpc_hip_ctx *ctx);

/* ---- several GPUs of one node (bp_simulation's frame loop sharded; north_star: RCCL all-reduce for the counters only) ----
 * One shard = one context + one HIP stream + one host thread.  devices[i] is the HIP ordinal of shard i; ordinals may repeat
 * (logical shards on one GPU: results are identical, the counters are then summed on the host because RCCL does not accept one
 * device twice in a communicator).  With distinct devices the five counters are all-reduced over RCCL (ncclAllReduce, uint64 sum,
 * one 40-byte message per call); RCCL is dlopen()ed, LDPC_HIP_RCCL_PATH overrides the library.  Frames [first_frame,
 * first_frame + B) are cut into consecutive batches of `batch` frames, batch k goes to shard k mod n; noise is keyed by the global
 * frame index, so counters and records do not depend on n or batch. */
typedef struct ldpc_hip_multi ldpc_hip_multi;
int ldpc_hip_open_multi(int decoder_id, int rh, int nh, int M, const int16_t *hd, const int *devices, int n_shards, ldpc_hip_multi **out);
void ldpc_hip_close_multi(ldpc_hip_multi *m);
int ldpc_hip_multi_shards(const ldpc_hip_multi *m);
ldpc_hip_ctx *ldpc_hip_multi_ctx(ldpc_hip_multi *m, int shard);      /* per-shard settings (ims params, bp chain, profiling) */
void *ldpc_hip_multi_stream(ldpc_hip_multi *m, int shard);          /* the shard's hipStream_t (work of the *_multi calls runs on it) */
const char *ldpc_hip_multi_reduction(const ldpc_hip_multi *m);      /* "rccl" or "host" */
/* Communicators are made once per device list and process (ncclCommInitAll is far more expensive than a short bp_simulation call,
 * and a code search opens a multi context per candidate matrix: main_good_code_search.cpp:320); ldpc_hip_close_multi hands them back to
 * the cache.  comm_inits = ncclCommInitAll calls so far; release_comms destroys the sets no open multi context holds. */
long long ldpc_hip_multi_comm_inits(void);
void ldpc_hip_multi_release_comms(void);
int ldpc_hip_multi_set_interleaver(ldpc_hip_multi *m, int permutation_type, int permutation_block, int permutation_inter);
int ldpc_hip_multi_set_codewords(ldpc_hip_multi *m, const uint8_t *codewords, int ncw);
int ldpc_hip_multi_set_random_codewords(ldpc_hip_multi *m, uint64_t seed, int ncw);
int ldpc_hip_simulate_multi(ldpc_hip_multi *m, double snr_db, int modulation_type, int punctured_blocks, int maxiter, double alpha,
                            uint64_t seed, long long first_frame, long long B, long long batch, unsigned long long counters[4],
                            unsigned long long *sum_abs_iters);
/* Same, and the ordered per-frame records for the sequential stopping rule (bp_simulation.cpp:591,820): HOST arrays
 * frame_info[B] (as d_frame_info above) and iters[B] in global frame order; counters / sum_abs_iters may be NULL. */
int ldpc_hip_frames_multi(ldpc_hip_multi *m, double snr_db, int modulation_type, int punctured_blocks, int maxiter, double alpha,
                          uint64_t seed, long long first_frame, long long B, long long batch, int32_t *frame_info, int32_t *iters,
                          unsigned long long counters[4], unsigned long long *sum_abs_iters);
/* The hot path on batches already RESIDENT on the GPUs (what bench.py times at N > 1): shard i decodes d_llr[i] ([B_per_shard][N]
 * float64 on devices[i]) on its own stream and counts the errors -- its frames are global frames first_frame + i*B_per_shard + f for the
 * codeword choice --, then one all-reduce of the five counters.  d_llr: HOST array of n device pointers.  Synchronous.  If any shard
 * fails before the all-reduce, no shard enters it and the call returns that shard's error (bp_simulation.cpp:716-759 per frame). */
int ldpc_hip_decode_count_multi(ldpc_hip_multi *m, const double *const *d_llr, long long B_per_shard, long long first_frame, int maxiter,
                                double alpha, unsigned long long counters[4], unsigned long long *sum_abs_iters);
/* ldpc_hip_decode_host over the shards: contiguous slices of the batch, one host thread per shard (BP_DEC with the frame chain
 * on is sequential by definition and runs on shard 0). */
int ldpc_hip_decode_host_multi(ldpc_hip_multi *m, double *llr, long long B, int maxiter, int decision, double alpha, double *decword,
                               int32_t *iters, int clobber_sp_input);
/* The exact-replay stream (ldpc_hip_mt_*) over the shards.  The generator's stream is sequential, but jump-ahead reaches any point of
 * it: the round's word tape is cut at the expected positions of the shards' first items, every shard makes only the sub-streams around
 * its own stretch (+- 8 standard deviations) and counts the accepted polar-method attempts in it, the n counts go through the host (a
 * counters-only exchange), and every shard then emits and decodes its contiguous share of each round's frames; the records come back
 * in frame order and all shards are left in the state the sequential loop would be in.  Per-shard generation work is ~1/n; if a
 * margin is ever exceeded the round is redone with the whole tape on every shard (ldpc_hip_multi_mt_stats counts both kinds), so
 * results never depend on the estimates.  LDPC_HIP_MT_SHARDED=0 forces the whole-tape mode, =1 shards even short rounds.
 * advance = draw and drop B frames on every shard (roll-forward after an early stop). */
int ldpc_hip_mt_set_state_multi(ldpc_hip_multi *m, const uint32_t state[624], int pos);
int ldpc_hip_mt_get_state_multi(ldpc_hip_multi *m, uint32_t state[624], int *pos);
int ldpc_hip_mt_set_frame_index_multi(ldpc_hip_multi *m, long long frames_taken);
int ldpc_hip_mt_advance_multi(ldpc_hip_multi *m, double snr_db, int modulation_type, int punctured_blocks, long long B);
int ldpc_hip_mt_frames_multi(ldpc_hip_multi *m, double snr_db, int modulation_type, int punctured_blocks, int maxiter, double alpha,
                             long long B, int32_t *frame_info, int32_t *iters);
void ldpc_hip_multi_mt_stats(const ldpc_hip_multi *m, long long *sharded_rounds, long long *fallback_rounds);

/* ---- FHT_DEC: QC-LDPC codes over GF(q), q = 2^q_bits -------------------------------------------------------------------------
 * Replaces decod_open(FHT_DEC, q_bits, ...) + the hb / hc fill + fht_ncols2convert + decod_init (decoders.cpp:348-433, 1104-1161;
 * bp_simulation.cpp:357-394).  hb [rh][nh]: circulant shifts, -1 = empty, reduced mod M.  hc [rh][nh]: the coefficient of each circulant as
 * an element 1 .. q - 1 of GF(q) in natural (bit pattern) representation over the first primitive polynomial of upstream's bank
 * (decoders.cpp:6594: 7, 13, 19, 37, 67, 131, 285, 529, 1033 for q_bits 2 .. 10); entries of empty circulants are ignored.  ncols2convert:
 * upstream makes its tables from hc as given and only THEN rewrites the first ncols2convert columns of hc as alog[hc] (:1151-1159); the
 * decoder is not affected, ldpc_hip_gfq_coefficients returns the rewritten matrix.
 * LDPC_HIP_EUNSUPPORTED for what upstream cannot do itself: a block row of weight < 2 (map_graph reads products it never set,
 * :6355-6360) or > 1024 (RWMAX), q_bits < 2 or > 10 (QMAX), a coefficient 0 (its logarithm is read past the end of the table, :6692).
 * ldpc_hip_close, ldpc_hip_n / _r / _edges, ldpc_hip_kernel_name and ldpc_hip_profile_* work on such a context; every entry point of
 * the binary decoders and of their simulation chain returns LDPC_HIP_EINVAL on it.  The environment variable LDPC_HIP_GFQ_GENERIC=1
 * (read here) selects the generic kernel also for q = 16 and q = 64; LDPC_HIP_GFQ_SLOTS=n (read per call) caps the frames in flight. */
int ldpc_hip_open_gfq(int q_bits, int rh, int nh, int M, const int16_t *hb, const int16_t *hc, int ncols2convert, int device,
                      ldpc_hip_ctx **out);
int ldpc_hip_gfq_q(const ldpc_hip_ctx *ctx);      /* q, 0 for a binary context */
/* The matrix decod_init leaves in hc (what bp_simulation.cpp:384-389 copies back to the caller): HOST array [rh][nh] out. */
int ldpc_hip_gfq_coefficients(const ldpc_hip_ctx *ctx, int16_t *hc_out);
/* Batched sum_prod_gfq_decod_lm(st, soft, qhard, decword, maxiter, p_thr) (decoders.h:306, decoders.cpp:7036-7694, dispatch
 * bp_simulation.cpp:724).  DEVICE pointers, asynchronous on `stream`; one launch decodes the whole batch for all iterations.
 *   d_soft  [B][q][N] float64 in, NOT modified: per frame upstream's qy[s][i], the probability of symbol s at position i
 *           (bp_simulation.cpp:644-676)
 *   d_qhard [B][N] int16 out, or NULL: upstream's qhard -- first index of the strict maximum of the a-posteriori vector the last
 *           syndrome check saw (decoders.cpp:7124-7143)
 *   d_iters [B] int32 out, or NULL: upstream's return value: >= 0 the iteration before which the syndrome was zero (0 = the input
 *           was already a codeword), < 0 = -maxiter, not converged
 *   d_post  [B][q][N] float64 out, or NULL: upstream's fht_soft_out when the call returns (the input itself for a return of 0)
 * p_thr must be 0 (the only value bp_simulation.cpp:341 passes; LDPC_HIP_EINVAL otherwise), maxiter >= 1.
 * Numerics: all three outputs equal upstream's bit for bit, Inf / NaN from degenerate inputs included: fp64 in upstream's operation
 * order, no contraction, correctly rounded division, no transcendental anywhere on this path. */
int ldpc_hip_decode_gfq_dev(ldpc_hip_ctx *ctx, const double *d_soft, long long B, int maxiter, double p_thr, int16_t *d_qhard,
                            int32_t *d_iters, double *d_post, void *stream);
/* Same with HOST pointers (PCIe-inclusive, synchronous; large batches are staged in pieces). */
int ldpc_hip_decode_gfq_host(ldpc_hip_ctx *ctx, const double *soft, long long B, int maxiter, double p_thr, int16_t *qhard,
                             int32_t *iters, double *post);

/* ---- The transmit side of FHT_DEC: what bp_simulation.cpp does around sum_prod_gfq_decod_lm for q_mod > 2, on the device -----------
 * left2right(matr, nrow, ncol) (decoders.cpp:174-195) on a row-major HOST array [rh][nh], in place: the new column order is
 * rh .. nh-1, then rh-1, then 0 .. rh-2.  bp_simulation.cpp:391-394 applies it to hb and to hc before it encodes; here the caller does
 * that and opens the context on the result.  LDPC_HIP_EINVAL for nh < rh or a non-positive size. */
int ldpc_hip_gfq_left2right(int16_t *matr, int rh, int nh);
int ldpc_hip_gfq_k(const ldpc_hip_ctx *ctx);      /* message symbols per frame, K = (nh - rh) * M; 0 for a binary context */
/* Batched encode_NBQCLDPC(st, msg) (decoders.cpp:1381-1705): systematic encoding over the dual-diagonal parity part, on the matrix
 * ldpc_hip_gfq_coefficients returns (upstream's encoder reads st->hc as decod_init left it), the context's hb and the context's field.
 * DEVICE pointers, asynchronous on `stream`, one launch per batch.
 *   d_msg      [B][K] int16 in: symbols 0 .. q-1 (a precondition; the bits above q are dropped)
 *   d_codeword [B][N] int16 out: message, then the special block (column nh-rh), then the rh-1 blocks of the recursion -- for a
 *              frame with ok = 0 what upstream leaves in st->codeword
 *   d_ok       [B] int32 out, or NULL: upstream's return value, 1 = the full re-check (:1646-1692) found a codeword, 0 = "bad coding"
 * All three schemes of the special column are served: weight 2; weight 3 with shifts (d, .., 0, .., d) (XOX); weight 3 with shifts
 * (0, .., d2, .., 0) (OXO, the block rotated by M - d2).  The weight-3 shape complaint (:1486-1490) only prints upstream and is not
 * an error here either: the re-check decides.
 * LDPC_HIP_EUNSUPPORTED, decided on the first encode call and then cached (the context keeps decoding), with the rule in the
 * message: where upstream returns 0 before any work (a coefficient of hc that is not 1 .. q-1, :1421-1425; a weight-2 special column
 * with equal coefficients or non-zero shifts, :1461-1471; a weight-3 one with different end coefficients, :1477-1481; any other
 * weight, :1493-1495), and where it would index a table with -1 or read outside the matrix: rh < 2, nh <= rh, an empty circulant
 * at (0, nh-rh), at (rh-1, nh-rh) or at (j, nh-rh+1+j), j = 0 .. rh-2.  Also a shift below -1 (decoder and encoder would read it
 * differently) and a code whose frame state (N + R + M symbols per frame) does not fit 64 KB of LDS. */
int ldpc_hip_encode_gfq_dev(ldpc_hip_ctx *ctx, const int16_t *d_msg, long long B, int16_t *d_codeword, int32_t *d_ok, void *stream);
/* Same with HOST pointers (synchronous). */
int ldpc_hip_encode_gfq_host(ldpc_hip_ctx *ctx, const int16_t *msg, long long B, int16_t *codeword, int32_t *ok);
/* sqrt(pow(10, -snr_db / 10) / 2 / ((nh - rh) / (double)nh)): bp_simulation.cpp:444-445 with punctured_blocks = 0.  0 for a binary context. */
double ldpc_hip_gfq_sigma(const ldpc_hip_ctx *ctx, double snr_db);
/* The q-ary BPSK / AWGN channel and the symbol probabilities of bp_simulation.cpp:581-582, :638-676 for B frames, DEVICE pointers,
 * asynchronous, one launch.  Per position i the q_bits bits of the symbol go out most significant first (word2bin) as
 * x_k = sigma * g + 2.0 * bit - 1.0; for every symbol s, lh starts at 0 and takes +-x_k in the order k = 0 .. q_bits-1,
 * LH = lh / (sigma * sigma), qy[s] = exp(LH); the sum ascends over s and every qy[s] is divided by it.  No contraction, correctly
 * rounded division, glibc's exp, so the output equals upstream's on the same Gaussians bit for bit, Inf / NaN at absurd SNR included
 * (|LH| in [512, 745] takes glibc's special path, which is not restated: there the last bit may differ).
 *   d_codeword [B][N] int16, or NULL = the all-zero word
 *   d_noise    [B][N * q_bits] float64 Gaussians g, or NULL = draw them: Philox4x32-10 + Box-Muller (the generator of the binary chain,
 *              stream tag 3), keyed by (seed, first_frame + f, bit index within the frame) -- the values do not depend on how a
 *              run is cut into calls
 *   d_soft     [B][q][N] float64 out, the input layout of ldpc_hip_decode_gfq_dev */
int ldpc_hip_gfq_channel_dev(ldpc_hip_ctx *ctx, const int16_t *d_codeword, const double *d_noise, double sigma, uint64_t seed,
                             long long first_frame, long long B, double *d_soft, void *stream);
/* Symbol errors of bp_simulation.cpp:746-755 and the bookkeeping of :805-810, with the counters and frame_info of the binary
 * ldpc_hip_count_errors_dev: d_counters[5] (DEVICE, accumulated) = nse (symbol errors at positions i >= R, summed over errored
 * frames), nde (errored frames), nue (errored frames with iters >= 0), frames, sum |iters|;
 * d_frame_info [B] or NULL = info_errors | (any_error << 30).  d_codeword NULL = the all-zero word. */
int ldpc_hip_count_errors_gfq_dev(ldpc_hip_ctx *ctx, const int16_t *d_qhard, const int16_t *d_codeword, const int32_t *d_iters, long long B,
                                  unsigned long long *d_counters, int32_t *d_frame_info, void *stream);
/* Frames [first_frame, first_frame + B) through encode -> channel -> ldpc_hip_decode_gfq_dev -> count, no host traffic per frame;
 * synchronous, counters[5] is a HOST array that is ACCUMULATED into.  random_messages = 0 sends the all-zero word and runs no
 * encoder (upstream's zero_codeword); 1 draws K uniform symbols per frame (Philox, stream tag 4, keyed by the global frame index;
 * symbol i is word i % 4 of block i / 4, reduced mod q) and encodes them; a frame whose encoding reports ok = 0 goes out as the
 * all-zero word (bp_simulation.cpp:552-556).  sigma = ldpc_hip_gfq_sigma(snr_db).  The run is cut into pieces whose [q][N] float64
 * workspace stays under 1 GiB (LDPC_HIP_GFQ_PIECE=n, read per call, caps the frames per piece further); the result does not depend
 * on the pieces, on LDPC_HIP_GFQ_SLOTS, or on how B is split over calls with consecutive first_frame. */
int ldpc_hip_simulate_gfq(ldpc_hip_ctx *ctx, double snr_db, int maxiter, uint64_t seed, long long first_frame, long long B,
                          int random_messages, unsigned long long counters[5]);

/* ---- Exact replay of upstream's q-ary frame loop on a GF(q) context (csrc/ldpc_gfq_exact_api.hpp) ---------------------------------
 * bp_simulation(q_mod > 2, ...) draws no sample before its frame loop and then, per frame, N * q_bits values of
 * next_random_gaussian() in index order (bp_simulation.cpp:638-642): B frames are the next B * N * q_bits samples of the generator of
 * ldpc_hip_mt_normal_dev.  Every frame carries the same word (:537-557, :581-582), the decoder runs with p_thr = 0, and the records
 * are those of ldpc_hip_count_errors_gfq_dev against that word.  Only MODULATION_SKIP and permutation_type 0 exist upstream for
 * q_mod > 2 (the switch at :635-678 has no other case, the permutation is never inverted, :683-686), so neither is an argument.
 * The binary ldpc_hip_mt_* entry points keep refusing a GF(q) context; these names serve a GF(q) context only and return
 * LDPC_HIP_EINVAL on any other kind, on bad arguments and (where they draw) without a generator state.  A refused call launches nothing
 * and leaves the word and the generator alone.  One device; multi-device and rank-sharded q-ary replay are not built.
 *
 * The message upstream encodes: bp_simulation.cpp:539-546 writes the eight symbols {6, 11, 0, 4, 2, 1, 2, 5} into a malloc()ed array of
 * n ints and encode_NBQCLDPC reads K = (nh - rh) * M of them -- the rest is uninitialised memory, and symbol 11 does not exist for
 * q < 16.  DEFINED HERE: the message is those eight symbols (the first K of them when K < 8), each reduced with & (q - 1), followed by
 * zeros.  HOST only, no GPU: msg [K] out.  LDPC_HIP_EINVAL for q_bits outside 2 .. 10, K < 0 or a null msg with K > 0. */
int ldpc_hip_gfq_upstream_message(int q_bits, int K, int16_t *msg);
/* The word every frame of the two entry points below carries: codeword HOST [N], symbols 0 .. q-1 (LDPC_HIP_EINVAL otherwise), or NULL =
 * the all-zero word (the default; what upstream sends when encode_NBQCLDPC returns 0, :552-556). */
int ldpc_hip_gfq_set_codeword(ldpc_hip_ctx *ctx, const int16_t *codeword);
/* As ldpc_hip_mt_set_state / ldpc_hip_mt_get_state, for a GF(q) context. */
int ldpc_hip_mt_set_state_gfq(ldpc_hip_ctx *ctx, const uint32_t state[624], int pos);
int ldpc_hip_mt_get_state_gfq(ldpc_hip_ctx *ctx, uint32_t state[624], int *pos);
/* Draws and drops the frames * N * q_bits samples of `frames` frames. */
int ldpc_hip_mt_advance_gfq(ldpc_hip_ctx *ctx, long long frames);
/* noise -> channel -> ldpc_hip_decode_gfq_dev -> count for the next B frames of the stream; synchronous.  frame_info [B], iters [B]:
 * HOST arrays, as ldpc_hip_mt_frames fills them.  sigma = sqrt(pow(10, -snr_db / 10) / 2 / ((nh - rh) / (double)(nh - punctured_blocks)))
 * (:444-445): punctured_blocks (0 .. nh-1) enters sigma only, no position is punctured (:711-714).  The work is done in pieces of at
 * most 1 GiB of soft values (LDPC_HIP_GFQ_PIECE=n caps the frames per piece further); the records do not depend on the pieces, on
 * LDPC_HIP_GFQ_SLOTS or on how B is split over calls.  LDPC_HIP_EUNSUPPORTED: a frame whose N * q_bits samples exceed one generation
 * round (2^27). */
int ldpc_hip_mt_frames_gfq(ldpc_hip_ctx *ctx, double snr_db, int punctured_blocks, int maxiter, long long B, int32_t *frame_info,
                           int32_t *iters);
/* The same records from Gaussians the caller drew: noise HOST [B][N * q_bits], the values of next_random_gaussian() in upstream's
 * order.  The route of a host whose std::normal_distribution the device generator does not reproduce; needs no generator state. */
int ldpc_hip_frames_gfq_noise_host(ldpc_hip_ctx *ctx, const double *noise, double snr_db, int punctured_blocks, int maxiter, long long B,
                                   int32_t *frame_info, int32_t *iters);

/* ---- Code sets: C candidate codes of one shape x B frames in one launch (csrc/ldpc_codeset.hpp) -----------------------------------
 * What a code search does (upstream's `search` / `ggp` drivers): many base matrices with the same rh, nh and M, each scored by a short
 * Monte-Carlo run over the SAME noise.  hd [C][rh][nh]: the C base matrices one after the other, shifts in [0, M), -1 = empty block.
 * decoder_id: LDPC_HIP_MS_DEC or LDPC_HIP_LMS_DEC; results are bit-identical to a context opened with ldpc_hip_open on the same matrix.
 * LDPC_HIP_EINVAL: another decoder id, C < 1, M > 512, rh > 16, nh > 32 (MS_DEC), a row weight above 16, an all-empty block row or
 * column, a shift outside [-1, M); LDPC_HIP_EUNSUPPORTED: nh * M * floor(64 / M) float64 values beyond the 160 KiB LDS image.
 * More block rows or columns: ldpc_hip_open_codes_wide.
 * The context serves the *_codes* entry points only: the single-code, GF(q) and multi-device entry points return LDPC_HIP_EINVAL
 * on it, and the *_codes* entry points return LDPC_HIP_EINVAL on any other context.  Close with ldpc_hip_close. */
int ldpc_hip_open_codes(int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int device, ldpc_hip_ctx **out);
/* The same for TDMP sum-product (LDPC_HIP_TASP_DEC; tdmp_sum_prod_gf2_decod_qc_lm, decoders.cpp:2584-2744, map_bin :2191-2228): an
 * ordinary code-set context, served by the entry points below (alpha is ignored).  Limits: M <= 512, rh <= 16, row weights 2 .. 16
 * (LDPC_HIP_EINVAL; map_bin reads SB[1]), no empty block column, any nh; LDPC_HIP_EUNSUPPORTED when the LDS image of a workgroup,
 * floor(64 / M) * 8 * (nh * M + ne_max * M) + 16 bytes with ne_max the largest number of circulants of a code, exceeds 160 KiB.
 * More block rows: ldpc_hip_open_codes_wide (the same kernel). */
int ldpc_hip_open_codes_tdmp(int rh, int nh, int M, const int16_t *hd, int C, int device, ldpc_hip_ctx **out);
/* The same for the integer advanced sum-product decoder (LDPC_HIP_IASP_DEC; isum_prod_gf2_decod_qc_lm, decoders.cpp:3822-4121, imap_bin
 * :2235-2271), both of its branches: a code whose block columns all hold two circulants takes upstream's own branch, decided per code.
 * An ordinary code-set context, served by the entry points below (alpha is ignored).  rh and nh are NOT limited (nothing is kept per
 * block row or column: the 30 x 60, M = 67 shape of upstream's input12L.jsonx fits).  Limits: M <= 512, row weights 2 .. 16 (imap_bin
 * reads SB[1]), no empty block column, at most 65535 circulants per code (LDPC_HIP_EINVAL); LDPC_HIP_EUNSUPPORTED when the LDS image
 * of a workgroup, floor(64 / M) * 2 * (ne_max * M + 2 * nh * M) bytes rounded up to 16, + 16, with ne_max the largest number of
 * circulants of a code, exceeds 160 KiB.
 * Measured (profiles/r14_codeset_iasp_time.txt; 30 x 60, M = 67, 50 iterations, 1.0 dB, 4096 frames per code): the set is SLOWER than
 * one ldpc_hip_open context per code on the shape-unlimited tier (JIT off): 621 against 518 ms at 16 codes (0.83x), 9896 against
 * 8297 ms at 256 (0.84x), 42.7 against 32.5 ms for one code; an unseen code through hiprtc in the foreground costs 36.2 s. */
int ldpc_hip_open_codes_iasp(int rh, int nh, int M, const int16_t *hd, int C, int device, ldpc_hip_ctx **out);
/* The same for the low-complexity high-efficiency decoder (LDPC_HIP_LCHE_DEC; lche_decod, decoders.cpp:2899-3012, map_bin_llr
 * :2815-2890, logexp_int :2777-2813): an ordinary code-set context, served by the entry points below (alpha is ignored), kernel
 * lche_layered_codes_kernel.  rh and nh are NOT limited (nothing is kept per block row or column).  Limits: M <= 512, row weights
 * 1 .. 16, no empty block row or column, shifts in [-1, M), C >= 1 (LDPC_HIP_EINVAL); LDPC_HIP_EUNSUPPORTED when the LDS image of a
 * workgroup, floor(64 / M) * 8 * (nh * M + ne_max * M) + 8 * 310 + 16 bytes (the a-posteriori LLRs, the per-edge state, the 96 + 214
 * table words of logexp_int, the vote flag) with ne_max the largest number of circulants of a code, exceeds 160 KiB.
 * ldpc_hip_open_codes(LDPC_HIP_LCHE_DEC, ...) stays LDPC_HIP_EINVAL.
 * Measured (profiles/r15_codeset_lche_time.txt; 50 iterations, 4096 frames per code, wall time against one ldpc_hip_open context per
 * code on the shape-unlimited tier, JIT off): 16 x 32, M = 64, 1.5 dB: 86.8 against 225.0 ms at 16 codes (2.59x), 1405 against 3660 ms
 * at 256 (2.61x), 7.9 against 15.4 ms for one code; 30 x 60, M = 67, 2.0 dB: 401 against 572 ms at 16 codes (1.43x), 6434 against
 * 9315 ms at 256 (1.45x); an unseen 16 x 32 code through hiprtc in the foreground costs 1.05 s. */
int ldpc_hip_open_codes_lche(int rh, int nh, int M, const int16_t *hd, int C, int device, ldpc_hip_ctx **out);
/* The same for integer min-sum (LDPC_HIP_IMS_DEC; imin_sum_decod_qc_lm, decoders.cpp:5430-5690): an ordinary code-set context, served
 * by the entry points below, kernel ims_flood_codes_kernel.  `alpha` IS read: ialpha = (int)(alpha * 16).  ldpc_hip_set_ims_params on
 * the set context selects thr, qbits and dbits for the next call (defaults 1.4, 6, 8; the same ranges).  d_soft receives the integer
 * a-posteriori value as a double.  Bit-identical to one ldpc_hip_open(LDPC_HIP_IMS_DEC) context per code.
 * The input stage of this decoder does not depend on the code: the energy scale sqrt(N / sum y^2) (a sequential sum whose rounding is
 * part of the result) and the quantised channel word are computed ONCE per received word (ims_coef_kernel, ims_quantise_kernel) into
 * the context's workspace -- once per frame for shared LLRs, however many codes decode it -- and every code reads 2 bytes per
 * variable.  That workspace belongs to the context: a set context serves ONE stream at a time (a second ldpc_hip_decode_codes_dev on
 * another stream would overwrite the words the first is still reading).
 * rh and nh are NOT limited (the whole state of a frame is in LDS).  Limits: M <= 512, row weights 1 .. 16, no empty block row or
 * column, shifts in [-1, M), C >= 1 (LDPC_HIP_EINVAL); LDPC_HIP_EUNSUPPORTED when the LDS image of a workgroup,
 * floor(64 / M) * (4 * nh * M + 8 * rh * M) bytes rounded up to 16, + 16 (per frame an int16 a-posteriori value and an int16 channel
 * value per variable and an 8-byte record per check; the vote flag), exceeds 160 KiB: 16 x 32 at M = 512 fits (131 088 bytes),
 * 20 x 40 at M = 512 does not (163 856).  ldpc_hip_open_codes(LDPC_HIP_IMS_DEC, ...) stays LDPC_HIP_EINVAL.
 * Measured (profiles/r16_codeset_ims_time.txt; 50 iterations, 4096 frames per code, wall time against one ldpc_hip_open context per
 * code, JIT off): 16 x 32, M = 64, 2.0 dB, against ims_flood_kernel: 29.7 against 50.3 ms at 16 codes (1.69x), 453 against 844 ms at
 * 256 (1.86x); the lone shipped matrix runs its ahead-of-time int8 instance and is 4.4x faster than the set (0.80 against 3.53 ms);
 * 30 x 60, M = 67, 3.0 dB, against ims_global_kernel: 127.5 against 270.0 ms at 16 codes (2.12x), 2007 against 4272 ms at 256 (2.13x),
 * 10.3 against 16.1 ms for one code. */
int ldpc_hip_open_codes_ims(int rh, int nh, int M, const int16_t *hd, int C, int device, ldpc_hip_ctx **out);
/* The same for the two flooding sum-product decoders: decoder_id LDPC_HIP_SP_DEC (sum_prod_decod_qc_lm, decoders.cpp:1923-2185,
 * likelihood ratios) or LDPC_HIP_ASP_DEC (sum_prod_gf2_decod_qc_lm, decoders.cpp:2324-2581, probabilities); any other id is
 * LDPC_HIP_EINVAL.  An ordinary code-set context, served by the entry points below, kernels sp_flood_codes_kernel and
 * asp_flood_codes_kernel.  `alpha` is ignored.  Bit-identical to one ldpc_hip_open context per code; an ASP code whose block columns
 * all hold exactly two circulants takes upstream's own branch (:2431-2480, unclamped), per code.
 * rh and nh are NOT limited, and SP does not limit the row weight either (a row of weight 1 is legal).  Limits: M <= 512, for ASP row
 * weights 2 .. 16, no empty block row or column, shifts in [-1, M), at most 65535 circulants per code, C >= 1 (LDPC_HIP_EINVAL).
 * LDS: the whole state of a frame, and no a-posteriori array.  Per frame, with ne_max the largest circulant count of a code of the set:
 *   SP : 8 * (ne_max * M + N + R) + 4 * ceil(N / 32) bytes (per-edge messages, channel likelihood ratios, check products, hard bits),
 *   ASP: 8 * (ne_max * M + N) + 4 * ceil(N / 32) bytes (per-edge state, channel probabilities, hard bits).
 * LDPC_HIP_EUNSUPPORTED only when ONE frame does not fit, that is when its image rounded up to 16, + 16, exceeds 160 KiB (the message
 * carries the byte count): 16 x 32 with 112 circulants at M = 126 fits (161 808 bytes for SP, 145 680 for ASP), at M = 128 SP does
 * not (164 368).  Launch shape, a function of the shape alone: L = 64 lanes (M <= 64; F = min(floor(64 / M), what fits 160 KiB) frames
 * side by side) or 64 * ceil(M / 64) lanes (F = 1) serve one block row or column at a time, and a workgroup of
 * min(1024 / L, nh) such groups deals the block columns and rows of its frames over its waves.
 * d_soft: SP forms it again from the LDS image at the end (the operands and order of `soft *= A`); ASP stores it every iteration.
 * ldpc_hip_open_codes(1 | 2, ...) and ldpc_hip_codes_table_host(1 | 2, ...) stay LDPC_HIP_EINVAL.  Gallager BP (id 0) has no set
 * route: its frames are not independent.
 * Measured (profiles/r17_codeset_sp_time.txt; 4096 frames per code, wall time against one ldpc_hip_open context per code, JIT off).
 * SP, 16 x 32, M = 64, 50 iterations, 2.0 dB, against sp_flood_kernel (LDS-resident): 61.0 against 65.4 ms at 16 codes (1.07x), 1000
 * against 1095 ms at 256 (1.09x), and for ONE code the set is SLOWER than its single-code context: 5.12 against 4.73 ms (0.92x).
 * SP against sp_global_kernel: 16 x 32, M = 126, 15 iterations, 1.7 dB: 92.5 against 251.0 ms at 16 codes (2.71x), 1467 against 3999 ms
 * at 256 (2.73x), 6.2 against 16.0 ms for one code; 30 x 60, M = 67, 50 iterations, 2.0 dB: 284.5 against 622.6 ms (2.19x), 4675 against
 * 10216 ms (2.19x), 19.9 against 39.6 ms.  ASP against asp_global_kernel: M = 64: 36.3 against 111.7 ms at 16 codes (3.07x), 590 against
 * 1839 ms at 256 (3.12x), 3.1 against 8.1 ms for one code; M = 126: 64.9 against 315.6 ms (4.86x), 1025 against 5048 ms (4.92x), 4.6
 * against 20.9 ms; 30 x 60: 178.4 against 574.4 ms (3.22x), 2920 against 9446 ms (3.24x), 12.8 against 36.4 ms. */
int ldpc_hip_open_codes_sp(int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int device, ldpc_hip_ctx **out);
/* Min-sum, TDMP and layered min-sum sets at ANY number of block rows and columns: decoder_id LDPC_HIP_MS_DEC (3), LDPC_HIP_TASP_DEC (7)
 * or LDPC_HIP_LMS_DEC (8); any other id is LDPC_HIP_EINVAL.  An ordinary code-set context, served by the entry points below exactly as
 * a context of ldpc_hip_open_codes / ldpc_hip_open_codes_tdmp with the same id is (alpha, puncture fill), and bit-identical to it on
 * every shape both accept: shapes inside the limits of those entry points are accepted here too.  Kernels
 * (csrc/ldpc_codeset_wide.hpp): ms_flood_wide_codes_kernel and lms_layered_wide_codes_kernel keep the per-check records (min1, min2, the
 * sign bits and the slot of min1) in LDS instead of registers, and the flooding kernel reads the channel LLRs from memory again in
 * every iteration; TDMP runs tasp_layered_codes_kernel itself, which keeps nothing per block row.
 * Limits: M <= 512, row weights 1 .. 16 (TDMP 2 .. 16), no empty block row or column, shifts in [-1, M), C >= 1 (LDPC_HIP_EINVAL);
 * LDPC_HIP_EUNSUPPORTED when the LDS image of a workgroup (the message carries the byte count) exceeds 160 KiB: for MS and LMS
 * floor(64 / M) * (8 * nh * M + 24 * rh * M) bytes rounded up to 16, + 16; for TDMP floor(64 / M) * 8 * (nh * M + ne_max * M) + 16 as in
 * ldpc_hip_open_codes_tdmp.  30 x 60 at M = 67 with 206 circulants (upstream's input12L.jsonx) takes 80 416 bytes for MS and LMS
 * and 142 592 for TDMP.  ldpc_hip_open_codes and ldpc_hip_open_codes_tdmp keep their limits.
 * Measured (profiles/r22_codeset_wide_time.txt; 4096 frames per code, wall time, median of 5).  30 x 60, M = 67, against one
 * ldpc_hip_open context per code on the shape-unlimited tier, JIT off: MS, 50 iterations, 2.5 dB: 212.6 against 275.1 ms at 16 codes
 * (1.29x), 3413 against 4416 ms at 256 (1.29x), 15.1 against 16.3 ms for one code; LMS, 50 iterations, 2.0 dB: 202.6 against 452.6 ms
 * (2.23x), 3161 against 7121 ms (2.25x), 13.9 against 24.5 ms; TDMP, 15 iterations, 1.7 dB: 328.9 against 574.9 ms (1.75x), 5272 against
 * 9243 ms (1.75x), 21.4 against 36.0 ms.  16 x 32, M = 64, against the register-resident set kernel of ldpc_hip_open_codes: the wide
 * kernels are SLOWER, MS 48.2 against 15.8 ms at 16 codes and 759.8 against 235.9 ms at 256 (0.33x, 0.31x), LMS 54.6 against 17.1 ms
 * and 825.0 against 240.9 ms (0.31x, 0.29x); TDMP is the same kernel (56.9 against 56.9 ms).  Use this entry point beyond the limits
 * of the others, as the layers above do.  The channel LLRs in LDS instead of re-read: 1.88x slower at 30 x 60 (667 against 354 ms). */
int ldpc_hip_open_codes_wide(int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int device, ldpc_hip_ctx **out);
/* A set of ANY shape: the global-memory tier of a code set (csrc/ldpc_codeset_global.hpp), what the shape-unlimited tier of
 * ldpc_hip_open is to a single code.  decoder_id LDPC_HIP_SP_DEC (1), LDPC_HIP_ASP_DEC (2), LDPC_HIP_MS_DEC (3), LDPC_HIP_IMS_DEC (4),
 * LDPC_HIP_IASP_DEC (5), LDPC_HIP_TASP_DEC (7), LDPC_HIP_LMS_DEC (8) or LDPC_HIP_LCHE_DEC (9); any other id is LDPC_HIP_EINVAL (Gallager
 * BP has no set: its frames are not independent).  An ordinary code-set context, served by the entry points below exactly as a
 * context of the decoder's own open entry point is (alpha, puncture fill, ldpc_hip_set_ims_params), and bit-identical to it on every
 * shape both accept, and to one ldpc_hip_open context per matrix on every shape.  Kernels: <decoder>_global_codes_kernel (each runs
 * the frame body of the single code's <decoder>_global_kernel, csrc/ldpc_global.hpp, on the code's own tables), one
 * workgroup of 256 threads (1024 from N = 16384) per frame, no LDS; a work item is (code, frame), the grid is capped at 1024 workgroups
 * (halved while their workspace exceeds 8 GiB; LDPC_HIP_CODES_GLOBAL_GRID=n, read per call, caps it lower) and strides over the items.
 * The message state is in a workspace of one slice per workgroup, sized for the code with the most circulants: it grows with neither
 * C nor B, is kept by the context (grown, never shrunk) and freed by ldpc_hip_close.  A decode call that needs more slices than the
 * context holds frees the workspace and allocates a larger one, which waits for the device: that call is not asynchronous.  A code's edge count, row and column weights and
 * whether all its block columns hold two circulants (decoders 2 and 5 then take upstream's own branch) are read from its own record,
 * so one set may mix such codes.
 * Accepted: any M >= 1, rh, nh and row weight that ldpc_hip_open's shape-unlimited tier takes.  LDPC_HIP_EINVAL, naming the code and
 * the position, before any device call: a null or non-positive argument, C < 1, a shift outside [-1, M), an empty block row or
 * column, a block row of weight < 2 for ids 2, 5 and 7.  LDPC_HIP_EUNSUPPORTED, naming the limit: an LCHE row of weight > 1024, M, rh
 * or nh from 65536 (an edge word holds 16 bits of each), nh * M from 2^28, a workspace slice beyond 512 MiB (16 of them within 8 GiB).
 * Every other entry point keeps its limits and its messages.
 * Measured (profiles/r29_codeset_global_time.txt; 4096 frames per code, wall time, median of 5, relabelings of the 16 x 32 Appendix C
 * matrix, against one ldpc_hip_open context per code, JIT off, at 1 / 16 / 256 codes).  TDMP, 15 iterations, 1.7 dB, against
 * tasp_global_kernel: M = 256 28.7 against 30.4 ms (1.06x), 358.9 against 402.3 ms (1.12x), 5481 against 6478 ms (1.18x); M = 512 1.06x,
 * 1.11x, 1.13x.  Min-sum, M = 1024, 2.0 dB, against ms_global_kernel: 0.99x for ONE code (SLOWER: 158.4 against 156.5 ms), 1.10x,
 * 1.15x.  Integer min-sum, 50 iterations, 2.0 dB: these shapes fit the LDS-resident kernels (a single code runs ims_flood_kernel), and
 * this route is SLOWER than one context per code at every size: M = 256 0.44x, 0.48x (499.4 against 238.5 ms), 0.53x; M = 512 0.57x, 0.64x, 0.67x. */
int ldpc_hip_open_codes_global(int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int device, ldpc_hip_ctx **out);
int ldpc_hip_codes(const ldpc_hip_ctx *ctx);      /* C; 0 for any other context */
/* The graph table ldpc_hip_open_codes / ldpc_hip_open_codes_tdmp (decoder_id LDPC_HIP_TASP_DEC) / ldpc_hip_open_codes_iasp (decoder_id
 * LDPC_HIP_IASP_DEC) upload, built on the host (no GPU needed; the same checks and return codes): per code
 * row_start[rh + 1] (relative to the code's own edge list) followed by its edges (block column << 16) | shift, rows then columns
 * ascending; offsets [C] = index of each code's row_start[0] in the table.  An IASP_DEC record goes on with cw2 (1: every block
 * column holds exactly two circulants), col_start[nh + 1] and col_edges (row-major index of the edge in its code << 16) | shift,
 * columns then rows ascending.  *length = entries of the table; offsets and table may
 * be NULL (sizes only), capacity = room in table. */
int ldpc_hip_codes_table_host(int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int32_t *offsets, int32_t *table,
                              long long capacity, long long *length);
/* The table ldpc_hip_open_codes_lche uploads, with its checks and return codes: per code row_start[rh + 1] followed by its edges, the
 * record of MS_DEC.  (ldpc_hip_codes_table_host(LDPC_HIP_LCHE_DEC, ...) stays LDPC_HIP_EINVAL.) */
int ldpc_hip_codes_table_lche_host(int rh, int nh, int M, const int16_t *hd, int C, int32_t *offsets, int32_t *table, long long capacity,
                                   long long *length);
/* The table ldpc_hip_open_codes_ims uploads, with its checks and return codes (no GPU needed): the record of MS_DEC, per code
 * row_start[rh + 1] followed by its edges (block column << 16) | shift in row-major order.
 * (ldpc_hip_codes_table_host(LDPC_HIP_IMS_DEC, ...) stays LDPC_HIP_EINVAL.) */
int ldpc_hip_codes_table_ims_host(int rh, int nh, int M, const int16_t *hd, int C, int32_t *offsets, int32_t *table, long long capacity,
                                  long long *length);
/* The table ldpc_hip_open_codes_sp uploads, with its checks and return codes (no GPU needed): for both decoders the record of
 * LDPC_HIP_IASP_DEC, per code row_start[rh + 1], the edges (block column << 16) | shift in row-major order, cw2 (1 when every block
 * column holds exactly two circulants; ASP reads it, SP ignores it), col_start[nh + 1] and col_edges (row-major edge index << 16) |
 * shift, columns then rows ascending.  (ldpc_hip_codes_table_host(1 | 2, ...) stays LDPC_HIP_EINVAL.) */
int ldpc_hip_codes_table_sp_host(int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int32_t *offsets, int32_t *table,
                                 long long capacity, long long *length);
/* The table ldpc_hip_open_codes_wide uploads, with its checks and return codes (no GPU needed): for all three ids the record of
 * MS_DEC, per code row_start[rh + 1] followed by its edges (block column << 16) | shift in row-major order.
 * (ldpc_hip_codes_table_host keeps its limits.) */
int ldpc_hip_codes_table_wide_host(int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int32_t *offsets, int32_t *table,
                                   long long capacity, long long *length);
/* The table ldpc_hip_open_codes_global uploads, with its checks and return codes (no GPU needed), the same record for all eight ids:
 * per code rh + nh + 3 + 3 ne entries, ne its number of circulants --
 *   row_start[rh + 1]   relative to the code's own edge list; row_start[rh] = ne
 *   edges[ne]           (block column << 16) | shift, rows then columns ascending (row-major order)
 *   cw2                 1: every block column holds exactly two circulants
 *   col_start[nh + 1]   relative to the code's own column list
 *   col_edges[ne]       (block ROW << 16) | shift, columns then rows ascending
 *   col_slot[ne]        for the same entry: the row-major index of that edge in edges[]
 * -- the five tables of a single-code context.  offsets [C] = index of each code's row_start[0]. */
int ldpc_hip_codes_table_global_host(int decoder_id, int rh, int nh, int M, const int16_t *hd, int C, int32_t *offsets, int32_t *table,
                                     long long capacity, long long *length);
/* Work item (c, f) decodes frame f of code c.  d_llr: [B][N] when shared_llr != 0 (every code decodes the same B received words) or
 * [C][B][N]; d_hard [C][B][hard_words], d_iters [C][B], d_soft [C][B][N], each optional (NULL) as in ldpc_hip_decode_dev.
 * maxiter >= 1.  Asynchronous on `stream`.  An IMS set (ldpc_hip_open_codes_ims) quantises into the context's workspace first: one
 * stream at a time per context. */
int ldpc_hip_decode_codes_dev(ldpc_hip_ctx *ctx, const double *d_llr, int shared_llr, long long B, int maxiter, double alpha,
                              uint32_t *d_hard, int32_t *d_iters, double *d_soft, void *stream);
/* ldpc_hip_count_errors_dev per code, against the all-zero codeword: d_frame_info [C][B] or NULL (same encoding, bit 30 = any
 * wrong bit), d_counters [C][5] (DEVICE, accumulated) = nse, nde, nue, frames, sum |iters|. */
int ldpc_hip_count_errors_codes_dev(ldpc_hip_ctx *ctx, const uint32_t *d_hard, const int32_t *d_iters, long long B,
                                    int32_t *d_frame_info, unsigned long long *d_counters, void *stream);
/* Frames [first_frame, first_frame + B) of every code through channel -> decode -> count; the BPSK LLRs are drawn ONCE (the noise of
 * ldpc_hip_channel_llr_dev with modulation 0 on the all-zero word, keyed by seed, global frame and position) and shared by the
 * codes, so counters[c] equals what ldpc_hip_simulate returns for code c alone with the same seed and frame range.  sigma uses the
 * common rate (nh - rh) / (nh - punctured_blocks); punctured positions carry 0.5, or 0.0 for a TDMP, IASP or LCHE set, as in ldpc_hip_awgn_llr_dev.  Synchronous; counters [C][5] (HOST, overwritten), frame_info [C][B] (HOST) or
 * NULL.  B is worked off in pieces of the context's workspace (LDPC_HIP_CODES_PIECE=n caps the frames per piece); the result does
 * not depend on the pieces or on how B is split over calls with consecutive first_frame.
 * The workspace belongs to the context: one ldpc_hip_simulate_codes call at a time per context, on the null stream; callers that
 * want several streams in flight use ldpc_hip_decode_codes_dev / ldpc_hip_count_errors_codes_dev with buffers of their own. */
int ldpc_hip_simulate_codes(ldpc_hip_ctx *ctx, double snr_db, int punctured_blocks, int maxiter, double alpha, uint64_t seed,
                            long long first_frame, long long B, unsigned long long *counters, int32_t *frame_info);
/* A whole Monte-Carlo run of the set with upstream's stopping rule applied per code ON THE DEVICE (bp_simulation.cpp:591 and
 * :805-823), in frame order: before each frame a code stops unless nde < n_frame_errors && experiment <= n_experiments; otherwise
 * ++experiment, an error frame adds its wrong information bits to nse and 1 to nde, and the code stops if
 * nde >= 10 && (double)nde / experiment > 2.5 * reference_frame_error (:820, checked at error frames only).  Frames come in batches
 * of first_batch, then 4 times as many up to max_batch, capped by n_experiments + 1 - frames so far, over the noise of
 * ldpc_hip_simulate_codes from first_frame on; a batch is worked off in the pieces of ldpc_hip_simulate_codes
 * (LDPC_HIP_CODES_PIECE), and after every piece one wavefront per running code walks that code's ordered records.  Each decode
 * launch covers only the codes still running; the host reads back their number and nothing else.
 * state [C][4] (HOST, overwritten) = experiment, nse, nde, frames_decoded per code: the first three are what a frame-by-frame loop
 * over the same noise gives, whatever the batches and pieces; frames_decoded counts every frame launched for the code (the sizes of
 * the pieces up to the one in which it stopped).  n_frame_errors <= 0 or n_experiments < 0: nothing is decoded, state is zero.
 * LDPC_HIP_EINVAL: not a code-set context, NULL state, first_frame < 0, first_batch < 1, max_batch < first_batch, maxiter < 1,
 * punctured_blocks outside [0, nh).  Synchronous, one call at a time per context, on the null stream, as ldpc_hip_simulate_codes. */
int ldpc_hip_simulate_codes_stop(ldpc_hip_ctx *ctx, double snr_db, int punctured_blocks, int maxiter, double alpha, uint64_t seed,
                                 long long first_frame, int n_frame_errors, long long n_experiments, double reference_frame_error,
                                 long long first_batch, long long max_batch, unsigned long long *state);
/* EXACT REPLAY on a binary code set: the noise is upstream's own std::mt19937 / polar-method stream (ldpc_hip_mt_*), drawn ONCE per
 * piece into the set's [piece][N] LLRs and decoded by every code -- what a search computes that calls reset_random() before each
 * candidate (search_ggp/scenario_based_code_generation.cpp:851, main_simulation.cpp:483/492, ldpc_sim.cpp:148), one launch per piece
 * instead of one context and one run per candidate.  The channel is the one ldpc_hip_mt_frames builds for a single context with
 * modulation_type 0: the all-zero word, the identity interleaver, sigma of the common rate (nh - rh) / (nh - punctured_blocks),
 * punctured positions at 0.5, or 0.0 for an SP, ASP, TDMP, IASP or LCHE set.  QAM4, interleavers and codewords are not part of the
 * set path.  Results per code are bit-identical to ldpc_hip_mt_frames on a context opened with that matrix, from the same state.
 * These five serve binary code-set contexts only: LDPC_HIP_EINVAL on a single-code, a GF(q) and a GF(q)-set context, as the
 * single-code ldpc_hip_mt_* stay LDPC_HIP_EINVAL on a set.  LDPC_HIP_EINVAL without ldpc_hip_mt_set_state_codes before;
 * LDPC_HIP_EUNSUPPORTED for a frame longer than one generation round.  Synchronous, one call at a time per context, null stream.
 * ldpc_hip_mt_set_state_codes / _get_state_codes: as ldpc_hip_mt_set_state / _get_state.
 * ldpc_hip_mt_advance_codes: draws the next `frames` frames and drops them.
 * ldpc_hip_mt_simulate_codes: the next B frames of the stream for all C codes; counters [C][5] (HOST, overwritten) as
 * ldpc_hip_simulate_codes; frame_info [C][B] and iters [C][B] (HOST, each may be NULL) are the ordered records, so a host replay of
 * the stopping rule has nue and sum |iters| too.  The generator is B frames further on afterwards.  Pieces: LDPC_HIP_CODES_PIECE.
 * ldpc_hip_mt_simulate_codes_stop: ldpc_hip_simulate_codes_stop over that stream, with the same batch schedule and pieces; the rule
 * on the device keeps upstream's whole SimCounters: state [C][6] (HOST, overwritten) = experiment, nse, nde, nue, sum |iters|,
 * frames_decoded per code (nue: error frames with iters >= 0; both over the frames the code consumes).  n_frame_errors <= 0 or
 * n_experiments < 0: no frame is drawn, state is zero.  The codes stop at different frames, so the call puts the generator and its
 * frame index BACK to the state at entry; ldpc_hip_mt_advance_codes(ctx, snr_db, punctured_blocks, state[c][0]) then leaves it
 * where upstream's loop leaves it for code c. */
/* The same records from LLRs the CALLER drew (a host whose std::mt19937 / libm stream the device does not reproduce keeps the draws
 * on the host): llr [B][N] (HOST) is uploaded piece by piece into the set's workspace and every code decodes it
 * (ldpc_hip_decode_codes_dev with shared_llr = 1, then ldpc_hip_count_errors_codes_dev); counters, frame_info and iters as
 * ldpc_hip_mt_simulate_codes.  Needs no generator state.  Binary code-set contexts only. */
int ldpc_hip_frames_codes_host(ldpc_hip_ctx *ctx, const double *llr, long long B, int maxiter, double alpha, unsigned long long *counters,
                               int32_t *frame_info, int32_t *iters);
int ldpc_hip_mt_set_state_codes(ldpc_hip_ctx *ctx, const uint32_t state[624], int pos);
int ldpc_hip_mt_get_state_codes(ldpc_hip_ctx *ctx, uint32_t state[624], int *pos);
int ldpc_hip_mt_advance_codes(ldpc_hip_ctx *ctx, double snr_db, int punctured_blocks, long long frames);
int ldpc_hip_mt_simulate_codes(ldpc_hip_ctx *ctx, double snr_db, int punctured_blocks, int maxiter, double alpha, long long B,
                               unsigned long long *counters, int32_t *frame_info, int32_t *iters);
int ldpc_hip_mt_simulate_codes_stop(ldpc_hip_ctx *ctx, double snr_db, int punctured_blocks, int maxiter, double alpha, int n_frame_errors,
                                    long long n_experiments, double reference_frame_error, long long first_batch, long long max_batch,
                                    unsigned long long *state);
/* AN SNR GRID on a binary code set (csrc/ldpc_codeset_grid_api.hpp): P points (1 <= P <= 64, snr_db [P], any order) x C
 * codes are P * C independent work items over ONE noise draw.  Upstream's `simulation` command resets its generator before every
 * (code, SNR) pair (main_simulation.cpp:477-518), so every point of every curve sees the same unit-variance samples and only sigma
 * differs: the channel kernel draws a sample once and writes the LLR of every point from it, llr = -2.0 * (sigma_p * g - 1.0) /
 * (sigma_p * sigma_p), one launch decodes the items still running, and the rule of ldpc_hip_*_codes_stop runs per item with the
 * reference of its point.  All eight set decoders, all three routes (resident, wide, global).  Every (point, code) result is
 * bit-identical to what the single-SNR twin returns for snr_db[p] from the same seed or generator state, whatever the pieces.
 * Arrays are indexed [p][c]: counters [P][C][5], frame_info / iters [P][C][B] (HOST, may be NULL), state [P][C][4] (Philox) or
 * [P][C][6] (exact replay), reference_frame_error [P] (upstream's best_errors[s], :510).  n_frame_errors, n_experiments and the batch
 * schedule are shared by the points.  A piece holds the buffers of all points: the 1 GiB bound and LDPC_HIP_CODES_PIECE apply to
 * P times the bytes per frame of the twin.
 * ldpc_hip_mt_simulate_codes_grid leaves the generator B frames further on, ONCE.  ldpc_hip_mt_simulate_codes_grid_stop puts it back
 * to where it was at entry; ldpc_hip_mt_advance_codes(ctx, snr_db[p], punctured_blocks, state[p][c][0]) then takes it to the end of
 * item (p, c).  n_frame_errors <= 0 or n_experiments < 0: state is zero, nothing is drawn.
 * LDPC_HIP_EINVAL, before anything is drawn, reserved or launched and with the outputs untouched: not a binary code-set context, P
 * outside 1 .. 64, NULL snr_db or reference_frame_error, a point that is not finite (the message names its index), and whatever the
 * twin refuses: maxiter < 1, the batches, a NaN alpha, alpha <= 0 for MS_DEC off the global route, a generator without state,
 * punctured_blocks outside [0, nh).  Not built: GF(q) sets, QAM, interleavers and transmitted codewords (the all-zero word, BPSK).
 * Measured (profiles/r34_codeset_grid_time.txt; exact replay, 8 points from 1.0 dB, against the loop of 8 single-SNR calls on the same
 * context).  Min-sum, 16 x 32, M = 64, 50 iterations, 4001 frames per item: 14.4 against 37.6 ms for one code (2.61x), 45.5 against 67.6 ms at
 * 4 codes (1.48x), 169.4 against 185.8 ms at 16 (1.10x), 2676 against 2696 ms at 256 (1.01x).  TDMP, M = 126, 15 iterations, 50 error
 * frames: 47.9 against 73.8 ms for one code (1.54x), 3525 against 3784 ms at 4 (1.07x), 13 698 against 14 349 ms at 16 (1.05x); 256 codes: not
 * measured.  No measured row is slower.
 * Synchronous, one call at a time per context, on the null stream. */
int ldpc_hip_simulate_codes_grid(ldpc_hip_ctx *ctx, const double *snr_db, int P, int punctured_blocks, int maxiter, double alpha, uint64_t seed,
                                 long long first_frame, long long B, unsigned long long *counters, int32_t *frame_info);
int ldpc_hip_simulate_codes_grid_stop(ldpc_hip_ctx *ctx, const double *snr_db, int P, int punctured_blocks, int maxiter, double alpha,
                                      uint64_t seed, long long first_frame, int n_frame_errors, long long n_experiments,
                                      const double *reference_frame_error, long long first_batch, long long max_batch, unsigned long long *state);
int ldpc_hip_mt_simulate_codes_grid(ldpc_hip_ctx *ctx, const double *snr_db, int P, int punctured_blocks, int maxiter, double alpha, long long B,
                                    unsigned long long *counters, int32_t *frame_info, int32_t *iters);
int ldpc_hip_mt_simulate_codes_grid_stop(ldpc_hip_ctx *ctx, const double *snr_db, int P, int punctured_blocks, int maxiter, double alpha,
                                         int n_frame_errors, long long n_experiments, const double *reference_frame_error, long long first_batch,
                                         long long max_batch, unsigned long long *state);

/* ---- GF(q) code sets: C candidate codes over GF(q) of one shape x B frames in one launch (csrc/ldpc_gfq_codeset.hpp) ----------------
 * What upstream's second search driver does (search_ggp/scenario_based_code_generation.cpp:692-940): every candidate comes from one
 * pattern and differs in the shifts and, for q_mod > 2, in the coefficients; reset_random() before each one gives all of them the same
 * noise, and bp_simulation(q_mod, HM, HC, ...) scores it with FHT_DEC.  hb [C][rh][nh] and hc [C][rh][nh]: the C candidates one after
 * the other, with the conventions of ldpc_hip_open_gfq (shifts reduced mod M, -1 = empty circulant, hc is not read there; natural
 * representation, ncols2convert = 0).  The patterns may differ between the codes.  Results are bit-identical to a context opened with
 * ldpc_hip_open_gfq on the same pair of matrices, whatever mixture of column weights the set holds.
 * LDPC_HIP_EUNSUPPORTED, as ldpc_hip_open_gfq per code: a block row of weight < 2 or > 1024, q_bits outside 2 .. 10, a coefficient 0
 * on a non-empty circulant, M, rh or nh >= 65536; LDPC_HIP_EINVAL: C < 1, a non-positive size, a shift below -1, a coefficient
 * outside GF(q).  The message names the code and the row or position.  There is no further limit on M, rh or nh: the message state
 * lives in a workspace in global memory.
 * The context serves the *_codes_gfq* entry points only (plus ldpc_hip_codes, ldpc_hip_gfq_q, ldpc_hip_gfq_sigma, ldpc_hip_n / _r,
 * ldpc_hip_edges = the largest edge count of the set, ldpc_hip_kernel_name, the profile calls): the binary *_codes*, the single-code
 * GF(q), the binary and the multi-device entry points return LDPC_HIP_EINVAL on it, and the *_codes_gfq* entry points return
 * LDPC_HIP_EINVAL on any other context.  Close with ldpc_hip_close.
 * Randomly encoded messages are not part of the set path: the all-zero word is a codeword of every candidate, and the encoder's plan
 * (ldpc_hip_encode_gfq_dev) is decided per code. */
int ldpc_hip_open_codes_gfq(int q_bits, int rh, int nh, int M, const int16_t *hb, const int16_t *hc, int C, int device, ldpc_hip_ctx **out);
/* The table ldpc_hip_open_codes_gfq uploads, built on the host (no GPU needed; the same checks and return codes), with the sizes-only
 * mode and the capacity / length contract of ldpc_hip_codes_table_host.  offsets [C] = index of each code's record; a record is
 * E, cw2 (1 = every block column has weight 2), row_start[rh + 1], col_start[nh + 1], e_col[E], e_circ[E], e_rl[E], ce_edge[E]:
 * edges in row-major order with their block column, shift and coefficient - 1 (the row of the set's multiplication / division
 * tables, which hold all q - 1 coefficients), and per block column the edges in ascending row order. */
int ldpc_hip_codes_gfq_table_host(int q_bits, int rh, int nh, int M, const int16_t *hb, const int16_t *hc, int C, int32_t *offsets,
                                  int32_t *table, long long capacity, long long *length);
/* Work item (c, f) decodes frame f of code c as ldpc_hip_decode_gfq_dev does with p_thr = 0.  d_soft: [B][q][N] when shared_soft != 0
 * (every code decodes the same B received words) or [C][B][q][N]; d_qhard [C][B][N], d_iters [C][B], d_post [C][B][q][N], each
 * optional (NULL).  maxiter >= 1.  Asynchronous on `stream`.  LDPC_HIP_GFQ_SLOTS=n as in ldpc_hip_decode_gfq_dev, with C * B work
 * items in place of B frames; C * B <= 2^31 - 1. */
int ldpc_hip_decode_codes_gfq_dev(ldpc_hip_ctx *ctx, const double *d_soft, int shared_soft, long long B, int maxiter, int16_t *d_qhard,
                                  int32_t *d_iters, double *d_post, void *stream);
/* ldpc_hip_count_errors_gfq_dev with d_codeword = NULL per code: d_frame_info [C][B] or NULL, d_counters [C][5] (DEVICE, accumulated). */
int ldpc_hip_count_errors_codes_gfq_dev(ldpc_hip_ctx *ctx, const int16_t *d_qhard, const int32_t *d_iters, long long B,
                                        int32_t *d_frame_info, unsigned long long *d_counters, void *stream);
/* Frames [first_frame, first_frame + B) of every code through channel -> decode -> count on the all-zero word; the symbol
 * probabilities are drawn ONCE per piece (the noise of ldpc_hip_gfq_channel_dev, keyed by seed, global frame and bit; sigma =
 * ldpc_hip_gfq_sigma(snr_db), which depends on rh and nh only) and shared by the codes, so counters[c] equals what
 * ldpc_hip_simulate_gfq(..., random_messages = 0, ...) accumulates from zero for code c alone over the same seed and frame range.
 * Synchronous; counters [C][5] (HOST, overwritten), frame_info [C][B] (HOST) or NULL.  B is worked off in pieces of the context's
 * workspace (LDPC_HIP_GFQ_PIECE=n caps the frames per piece); the result does not depend on the pieces, on LDPC_HIP_GFQ_SLOTS or on
 * how B is split over calls with consecutive first_frame.  One call at a time per context, on the null stream. */
int ldpc_hip_simulate_codes_gfq(ldpc_hip_ctx *ctx, double snr_db, int maxiter, uint64_t seed, long long first_frame, long long B,
                                unsigned long long *counters, int32_t *frame_info);
/* ldpc_hip_simulate_codes_stop for a GF(q) set: the same rule per code on the device, the same state [C][4] (nse counts wrong
 * information SYMBOLS), batch schedule, meaning of frames_decoded and LDPC_HIP_EINVAL cases, over the noise of
 * ldpc_hip_simulate_codes_gfq from first_frame on. */
int ldpc_hip_simulate_codes_gfq_stop(ldpc_hip_ctx *ctx, double snr_db, int maxiter, uint64_t seed, long long first_frame,
                                     int n_frame_errors, long long n_experiments, double reference_frame_error, long long first_batch,
                                     long long max_batch, unsigned long long *state);

/* ---- Exact replay on a GF(q) code set: what a search computes that calls reset_random() and bp_simulation(q_mod, HM, HC, ...) for
 * every candidate (search_ggp/scenario_based_code_generation.cpp:754, :852, :883), one launch per piece.  The stream, sigma and the
 * records are those of ldpc_hip_mt_frames_gfq above; results per code are identical to ldpc_hip_mt_frames_gfq on a context opened
 * with that code's matrices and carrying that code's word, from the same generator state.  These serve GF(q) code-set contexts only
 * (LDPC_HIP_EINVAL on any other kind, on bad arguments and -- where they draw -- without ldpc_hip_mt_set_state_codes_gfq before);
 * the five binary ldpc_hip_mt_*_codes keep refusing a GF(q) set.  A refused call launches nothing and leaves words and generator alone.
 * Synchronous, one call at a time per context, null stream.  Pieces: LDPC_HIP_GFQ_PIECE.
 * ldpc_hip_codes_gfq_set_codewords: words HOST [C][N], the word code c sends (upstream encodes a message per candidate), symbols
 *   0 .. q-1; NULL = every code sends the all-zero word (the default).  Without words the soft values of a piece are formed once and
 *   shared by the codes; with words they are formed per code (gfq_channel_codes_kernel) and a piece holds C * q * N * 8 bytes of them per
 *   frame.  The words are read by the entry points of this section only: ldpc_hip_simulate_codes_gfq(_stop) send the all-zero word.
 * ldpc_hip_mt_set_state_codes_gfq / _get_state_codes_gfq: as ldpc_hip_mt_set_state / _get_state.
 * ldpc_hip_mt_advance_codes_gfq: draws and drops the frames * N * q_bits samples of `frames` frames.
 * ldpc_hip_mt_simulate_codes_gfq: the next B frames for all C codes; counters [C][5] (HOST, overwritten), frame_info [C][B] and
 *   iters [C][B] (HOST, each may be NULL).  The generator is B frames further on afterwards.
 * ldpc_hip_mt_simulate_codes_gfq_stop: the contract of ldpc_hip_mt_simulate_codes_stop -- the rule of an exact replay per code on the
 *   device, state [C][6] = experiment, nse (wrong information SYMBOLS), nde, nue, sum |iters|, frames_decoded; the generator and its frame index are put BACK to the
 *   state at entry, and ldpc_hip_mt_advance_codes_gfq(ctx, state[c][0]) then leaves it where upstream's loop leaves it for code c.
 * ldpc_hip_frames_codes_gfq_noise_host: the twin of ldpc_hip_frames_codes_host -- the records of ldpc_hip_mt_simulate_codes_gfq from
 *   Gaussians the caller drew, noise HOST [B][N * q_bits]; needs no generator state. */
int ldpc_hip_codes_gfq_set_codewords(ldpc_hip_ctx *ctx, const int16_t *words);
int ldpc_hip_mt_set_state_codes_gfq(ldpc_hip_ctx *ctx, const uint32_t state[624], int pos);
int ldpc_hip_mt_get_state_codes_gfq(ldpc_hip_ctx *ctx, uint32_t state[624], int *pos);
int ldpc_hip_mt_advance_codes_gfq(ldpc_hip_ctx *ctx, long long frames);
int ldpc_hip_mt_simulate_codes_gfq(ldpc_hip_ctx *ctx, double snr_db, int punctured_blocks, int maxiter, long long B,
                                   unsigned long long *counters, int32_t *frame_info, int32_t *iters);
int ldpc_hip_mt_simulate_codes_gfq_stop(ldpc_hip_ctx *ctx, double snr_db, int punctured_blocks, int maxiter, int n_frame_errors,
                                        long long n_experiments, double reference_frame_error, long long first_batch, long long max_batch,
                                        unsigned long long *state);
int ldpc_hip_frames_codes_gfq_noise_host(ldpc_hip_ctx *ctx, const double *noise, double snr_db, int punctured_blocks, int maxiter,
                                         long long B, unsigned long long *counters, int32_t *frame_info, int32_t *iters);

/* ---- Girth spectrum and ACE trace: upstream's trace_bound_pol_mon_pm (trace_pm.cpp:58-299, NATURAL_POLYNOM), the filter of its
 * searches (search_ggp/scenario_based_code_generation.cpp:527-570) and the source of girth_ / girth_ACE / girth_spectrum in its
 * result records (main_simulation.cpp:496, :600-603), for a set of candidate codes in one call (csrc/ldpc_girth.hpp).
 * LDPC_HIP_EINVAL, found before any device call: C < 1, gmax outside 4 .. 20 (GMAX), gtarget < 1, nh > 1000 (upstream's cw[1000]),
 * a shift outside [-1, M), M, rh or nh < 1, a NULL output.  LDPC_HIP_EUNSUPPORTED: a code whose workspace -- 12 * E^2 * M bytes for
 * the largest edge count E of the set -- exceeds 4 GiB (the message holds the byte count), rh > 3276.
 * Arithmetic is 32-bit as upstream's; where upstream's behaviour is undefined (a sum beyond 2^31 - 1) the sums here wrap and bit 1 of
 * the code's status is set.  Results are upstream's bit for bit on every code without that bit. */
/* trace_bound_pol_mon_pm for C codes of one shape.  hd HOST [C][rh][nh], shifts in [-1, M); min_ace / max_spec HOST [gmax] or NULL
 * (upstream's minSA / maxS).  Out, HOST: S [C][gmax], SA [C][gmax], status [C]: bit 0 = upstream's return value, bit 1 = a 32-bit
 * sum overflowed.  Synchronous.  No context needed.  The codes may differ in their masks.  A set whose workspace exceeds 1 GiB is
 * worked off in pieces (LDPC_HIP_GIRTH_PIECE=n: n codes per piece, read per call); the result does not depend on the pieces, and the
 * number of launches and synchronisations per piece does not depend on the number of codes. */
int ldpc_hip_girth_codes(int rh, int nh, int M, const int16_t *hd, int C, int gmax, int gtarget, const int32_t *min_ace,
                         const int32_t *max_spec, int device, int32_t *S, int32_t *SA, int32_t *status);
/* HOST only, no GPU: the sparse graph the kernel walks -- E and, per edge J, its predecessors (j, a, as) in ascending j.  Edges are
 * the non-empty circulants, column by column with the rows ascending; pred_begin [E + 1] (may be NULL), pred [3 * n] (NULL to size:
 * then only *E and *n are written). */
int ldpc_hip_girth_graph_host(int rh, int nh, int M, const int16_t *hd, int *E, int32_t *pred_begin, int32_t *pred, long long *n);
/* HOST only: main_simulation.cpp:177-201 on one code's S / SA: girth (21 = none found), ACE[4], spectrum[4]. */
int ldpc_hip_trace_matrix_host(const int32_t *S, const int32_t *SA, int gmax, int *girth, int32_t ACE[4], int32_t spectrum[4]);

/* ---- Labelling a protograph with circulant shifts under a girth bound: upstream's generate_code (code_generation.cpp:35-115, the
 * second step of its `search` command) with the equations of equations.cpp / graph_spider.h (csrc/ldpc_label.hpp).
 * proto HOST [rh][nh]: 0 = empty, 1 = edge with a random shift, any other positive value = edge whose shift is fixed to 0.  Edges are
 * numbered column by column with the rows ascending; the random edges, in that order, are what an attempt draws.
 * LDPC_HIP_EINVAL, found before any device call: rh or nh < 1, a NULL proto, a negative entry, no edge, target_girth < 4 and, for
 * ldpc_hip_label_codes, M outside 2 .. 32767, max_attempts < 1, want < 1, pos_in outside 0 .. 624, a NULL state or output.
 * LDPC_HIP_EUNSUPPORTED, also found before any device call: more than 2^20 equations or more than 2^22 paths in one layer of the
 * path tree (the message holds the count reached), target_girth > 64, more than 480 edges with a random shift.  Both are stateless. */
/* HOST only, no GPU: the equations of the protograph for target_girth.  *tree_girth: the girth the protograph allows (target_girth, or
 * the length of the shortest closed walk whose edges cancel identically); *n_equations: upstream's `eqs=`; the table holds, per
 * equation, its terms over the random edges only: eq_begin [n_equations + 1], term_edge [n_terms] (index among the random edges) and
 * term_mult [n_terms] (signed multiplicity).  A labelling v passes iff no equation's sum of term_mult * v[term_edge] is divisible by M.
 * *never_accepts = 1 when an equation has no term left.  Table pointers may be NULL: then only the sizes are written. */
int ldpc_hip_label_equations_host(int rh, int nh, const int16_t *proto, int target_girth, int *tree_girth, int *n_equations, int *n_random,
                                  long long *n_terms, int *never_accepts, int32_t *eq_begin, int32_t *term_edge, int32_t *term_mult);
/* generate_code on the device.  Attempt a = 0, 1, ... draws one uniform_int_distribution<int>(0, M - 1) value per random edge from
 * the std::mt19937 given by (state_in, pos_in) -- as ldpc_hip_mt_set_state takes them -- and is accepted when it passes every
 * equation and no two columns of the labelled matrix are equal.  The call stops behind the want-th accepted attempt or after
 * max_attempts.  want = 1 is exactly upstream's call; want = K equals K consecutive calls of upstream's as long as none of them
 * exhausts its own budget (max_attempts is the total).  Out, HOST: hd_out [want][rh][nh] (the first *found matrices: -1 empty, else
 * the shift), attempt_index [want] (0-based, counted over the whole call: call k of upstream's tested attempt_index[k] -
 * attempt_index[k - 1] attempts), *found, *attempts_tested, *tree_girth, and the generator where upstream's loop leaves it: behind the
 * last draw of the last accepted attempt, or behind all max_attempts attempts; (state_in, pos_in) unchanged, *found = 0 and
 * *attempts_tested = 0 when *tree_girth < target_girth.  Attempts are tested in rounds that grow eight-fold from 4096
 * (LDPC_HIP_LABEL_ROUND=n: n attempts per round, read per call); the result does not depend on the rounds.  Synchronous. */
int ldpc_hip_label_codes(int rh, int nh, const int16_t *proto, int target_girth, int M, long long max_attempts, int want,
                         const uint32_t state_in[624], int pos_in, int device, int16_t *hd_out, long long *attempt_index, int *found,
                         long long *attempts_tested, int *tree_girth, uint32_t state_out[624], int *pos_out);
/* What this thread's last ldpc_hip_label_codes did: rounds, redraws among the words it consumed, equations evaluated by live lanes,
 * attempts checked (whole rounds). */
void ldpc_hip_label_last_stats(long long stats[4]);

/* ---- Every lifting a labelling allows: upstream's equation_builder::check_voltages / check_voltages_and_coefs (equations.cpp:150-267,
 * what its `ggp` command turns on) for K labellings in one call (csrc/ldpc_voltage.hpp).  proto HOST [rh][nh]: any positive entry is
 * an edge, the value is not otherwise read; E edges, numbered column by column with the rows ascending.  The equations are those of
 * ldpc_hip_label_equations_host with every edge counted as random; with *tree_girth < target_girth they are the ones shorter than
 * *tree_girth, as `ggp` works with them (no early return).  voltages HOST [K][E] in 0 .. 32767; coefs HOST [K][E] in 0 .. 32767, or
 * NULL for the binary check.  Per labelling, with s_e the sum of an equation over the voltages and c_e the same plain integer sum over
 * the coefficients (not reduced mod q - 1, as upstream does not):
 *   status [K]       0 = upstream's first_failed_equation == -1; 1 = its first_failed_equation == 0 (some s_e == 0 -- with
 *                    coefficients: some s_e == 0 with c_e == 0); 2 = with coefficients only, DEFINED HERE: no equation has s_e == 0 and
 *                    c_e == 0 but at least one has s_e == 0 and c_e != 0.  Upstream exits there ("global_divisor_table is called with
 *                    the argument 0"); here those equations contribute no divisor and the other fields are those of the rest.
 *   failed [K][W]    W = max_modulo / 64 + 1; bit m says m is in failed_modulos: the divisors <= max_modulo of the |s_e|.  May be NULL.
 *   max_nonok [K]    the largest member of that set, 1 when it is empty;  min_ok [K]: the smallest m >= 2 not in it.
 *   max_abs_sum [K]  max |s_e|: where it is <= max_modulo the result is that of upstream's unbounded check_voltages(v).
 * For status 1 min_ok, max_nonok and the bitmap are 0 (upstream leaves them uninitialised).  *tree_girth, *n_equations: may be NULL.
 * LDPC_HIP_EINVAL, found before any device call: what ldpc_hip_label_equations_host refuses, max_modulo < 1, K < 1, a NULL voltages,
 * status, min_ok, max_nonok or max_abs_sum, a voltage or coefficient outside 0 .. 32767.  LDPC_HIP_EUNSUPPORTED, also before any
 * device call: max_modulo > 65535, more than 4096 edges, and the limits of the equation table.  A batch is worked off in pieces of at
 * most 2^20 labellings (one launch) and at most 256 MiB of device memory -- per labelling its voltages, its coefficients where given,
 * its bitmap where failed is not NULL, and 16 bytes of results -- (LDPC_HIP_VOLTAGE_PIECE=n: n labellings per piece, still at most
 * 2^20, read per call); the result does not depend on the pieces.  LDPC_HIP_VOLTAGE_LAYOUT=moduli, for measurements and tests
 * only, runs the slower kernel layout that the shipped one was measured against (same results).  Synchronous and stateless. */
int ldpc_hip_check_voltages(int rh, int nh, const int16_t *proto, int target_girth, int max_modulo, const int32_t *voltages,
                            const int32_t *coefs, long long K, int device, int32_t *status, int32_t *min_ok, int32_t *max_nonok,
                            int32_t *max_abs_sum, uint64_t *failed, int *tree_girth, int *n_equations);
/* The loop of upstream's random_search_bank_good_codes (search_ggp/) with a budget, on the device.  The arguments, the draws, the
 * outputs, the attempt indices and the generator afterwards are those of ldpc_hip_label_codes with T (the tailbite length,
 * 2 .. 32767) in place of M: attempt a draws uniform_int_distribution<int>(0, T - 1) per edge with proto == 1 and takes 0 for any
 * other edge.  An attempt is accepted iff its voltage check -- as ldpc_hip_check_voltages, bounded at max(T, exact_modulo), which
 * decides exactly as upstream's unbounded call -- has status 0, min_ok <= T and, unless exact_modulo == 0, check_modulo(exact_modulo)
 * (exact_modulo: 0, or T .. 65535; LDPC_HIP_EINVAL otherwise, as for a NULL min_ok_out).  min_ok_out HOST [want]: min_ok of the
 * accepted attempts (what upstream writes in front of each labelling of its bank).  There is no equal-columns test, and no early
 * return for *tree_girth < target_girth: the search then runs on the equations shorter than *tree_girth.  Rounds, their knob and the
 * statistics are those of ldpc_hip_label_codes. */
int ldpc_hip_label_bank(int rh, int nh, const int16_t *proto, int target_girth, int T, int exact_modulo, long long max_attempts, int want,
                        const uint32_t state_in[624], int pos_in, int device, int16_t *hd_out, int32_t *min_ok_out, long long *attempt_index,
                        int *found, long long *attempts_tested, int *tree_girth, uint32_t state_out[624], int *pos_out);

/* Timing aid for bench.py: average duration in milliseconds of the decode kernel launches recorded with
 * HIP events on their own stream since the last reset (events are only recorded while enabled). */
int ldpc_hip_profile_enable(ldpc_hip_ctx *ctx, int enable);
int ldpc_hip_profile_read(ldpc_hip_ctx *ctx, double *total_ms, long long *launches, int reset);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_HIP_H */
