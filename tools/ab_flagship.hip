// ab_flagship.hip -- A/B harness for variants of the flagship min-sum body (ldpc_spec::ms_m64_body) on the shipped example code:
// every variant decodes the SAME 65536 frames (Eb/N0 0 dB: all 50 iterations run), outputs are compared bit for bit with the
// baseline, rounds are interleaved in one process (guide rule 24).  Build: hipcc --offload-arch=gfx950 -O3 -std=c++17
// -ffp-contract=off tools/ab_flagship.hip -o tools/ab_flagship.bin (with -DAB_LATEST: the baseline, the shipped bodies and the newest round's
// variants only, a quarter of the compile time).   usage: ab_flagship.bin [frames] [Eb/N0 dB] [rounds] [persistent 0|1] [first variant timed in every round]
// Results: profiles/r33_flagship_variants.txt: what of STATE3's arithmetic stands among STATE1's LDS operations -- the S1SET parameter of the header's
// body -- at 0 and 2 dB.  profiles/r32_flagship_variants.txt: the filter rows and the on-demand syndrome pass -- the FRSET and XGSET parameters of the
// header's body -- at 0 and 2 dB.  profiles/r26_flagship_variants.txt: resident channel values, soft values kept or not, the bit word -- the SOFT, RSET and
// BITW parameters of the header's body -- in both launch forms (argument 4).  profiles/r25_flagship_variants.txt: STATE2 of ms_m64_body streams its channel loads over the non-local block columns, YD
// of them ahead, first group at the start of STATE2 or after a block row of STATE1 (YROW), and the body carries KR block rows -- the
// YD, YROW and KRSET parameters of the header's body; depth 32 issues every load at once, which is what the schedule before round 25
// amounted to on this code (the variants of round 23 below are held at that and at 13 rows).  profiles/r23_flagship_variants.txt: the carried rows [0, KP) of ms_m64_body form their magnitudes from prefix and suffix
// minima, KP = 0 (round 20's body: every carried row selects between min1 and min2 by value equality), 9, 11 and 13 = all carried
// rows, through the KPCAP parameter of the header's body.  Round 20's variants -- carried rows, the min1 slot by equality -- are in
// profiles/r20_flagship_variants.txt and still switches of ms_m64_body_y here (round 19's variants -- local block columns, plain 64-bit image reads -- are in
// profiles/r19_flagship_variants.txt and still switches of ms_m64_body_y here; round 18's variants -- the 32-bit syndrome word, carried c2v values, scalar wrap masks -- are in
// profiles/r18_flagship_variants.txt and still switches of ms_m64_body_y here; round 13's variants -- where the channel LLRs are loaded, how many edges are kept from
// STATE1 to STATE3 -- are in profiles/r13_flagship_variants.txt, round 6's in profiles/r06_flagship_variants.txt, round 2's in
// profiles/r02_flagship_variants.txt; all of them are part of every body here).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../ldpc-lib_amd/csrc/ldpc_spec.hpp"
#include "../ldpc-lib_amd/csrc/code_appendix_c_m64.hpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

namespace ldpc_spec {

// ---- round 18's edge budget: every edge of a block row counts, 70 edges (ldpc_spec.hpp counts the edges of local block columns no
// longer: ms_m64_keep_rows, kMsM64KeepEdges)
template <class C>
constexpr int keep_rows_r18(int budget) {
    int edges = 0, rows = 0;
    while (rows < C::RH && edges + C::RW[rows] <= budget) edges += C::RW[rows++];
    return rows;
}
template <class C>
constexpr int keep_budget_r18() {
    constexpr int cols = C::NH < 24 ? C::NH : 24;
    constexpr int others = 5 * C::RH + 2 * cols + 2 * C::WMAX, others_example = 5 * 16 + 2 * 24 + 2 * 8;
    constexpr int cut = others > others_example ? others - others_example : 0;
    return 70 > cut ? 70 - cut : 0;
}

// ---- whole block rows in ascending order while their edges that go through LDS fit into `budget` (round 19's ms_m64_keep_rows; the
// header's counts registers since round 20)
template <class C>
constexpr int keep_rows_r19(int budget) {
    int edges = 0, rows = 0;
    while (rows < C::RH && edges + ms_m64_row_edges<C>(rows) <= budget) edges += ms_m64_row_edges<C>(rows++);
    return rows;
}
// ---- round 19's edge budget: 57 edges that go through LDS, kept from STATE1 to STATE3 (ldpc_spec.hpp has the rule of round 20 now)
template <class C>
constexpr int keep_budget_r19() {
    constexpr int cols = C::NH < 24 ? C::NH : 24;
    constexpr int others = 5 * C::RH + 2 * cols + 2 * C::WMAX, others_example = 5 * 16 + 2 * 24 + 2 * 8;
    constexpr int cut = others > others_example ? others - others_example : 0;
    return 57 > cut ? 57 - cut : 0;
}

// ---- the baseline: ms_m64_body as round 19 shipped it, word for word (only the name and the two budget functions above differ)
template <class C>
__device__ __forceinline__ void ms_m64_body_parent(const SpecArgs &a) {
    static_assert(C::M == 64, "ms_m64_body: one frame per wavefront needs M == 64");
    constexpr int RH = C::RH, NH = C::NH, N = C::NH * 64;
    constexpr int KR = keep_rows_r19<C>(keep_budget_r19<C>());   // block rows [0, KR) keep their decoded c2v values, see STATE1
    extern __shared__ double lds[];  // 512 B unused, then [N] soft / acc (fp64): kMsM64LdsBytes(N)
    const int lane = threadIdx.x;
    const double alpha = a.alpha, alpha_mag = fabs(a.alpha);
    long long fr = blockIdx.x;  // one wave per frame; with a.queue the wave goes on to further frames (uniform: an SGPR pair)

    // The image starts one block column (512 B) into the allocation, so a rotation needs no wrap arithmetic: variable
    // (lane + c) mod 64 of block column k is at  base + 512 k + 8 c  with  base = hi  for the lanes with lane + c < 64 and
    // base = lo = hi - 512  for those that wrap.  Which lanes wrap is a compile-time lane mask (an SGPR-pair constant), so a
    // rotated address is ONE select between two long-lived registers, 512 k + 8 c (<= 32 760) sits in the ds_* offset field, and
    // shift 0 is `hi` itself.  (Before: add, and, add-the-LDS-base -- three VOP2 -- per rotated edge and state, a copy + an add per
    // block row.)  The ~40 distinct rotated addresses must still not be hoisted out of the iteration loop into long-lived VGPRs
    // (that costs more in spills than the select it saves): `tie`, see sel32_tied.
    const u32 lane8 = (u32)lane * 8u;
    const u32 lo = lds_addr(lds) + lane8, hi = lo + 512u;
    auto at = [&](u32 tie, auto S, auto K) -> double * {
        constexpr int c = decltype(S)::value, k = decltype(K)::value;
        static_assert(c >= 0 && c < 64 && k * 512 + c * 8 < 65536, "shift / block column out of range");
        if constexpr (c == 0) return lds_at(hi + (u32)(k * 512));
        else return lds_at(sel32_tied(hi, lo, ~0ull << (64 - c), tie) + (u32)(k * 512 + c * 8));
    };
    auto own = [&](auto K) -> double * { return lds_at(hi + (u32)(decltype(K)::value * 512)); };   // this lane's variable of block column k
    // A block column that is local (ms_m64_local_col) is not read or added to in LDS inside the iteration: STATE1 and STATE2 skip
    // it, STATE3 forms its soft value in a register at the column's first block row, see there.

  while (fr < a.nframes) {   // one pass without a queue
    const double *const yrow = a.llr + fr * N + lane;  // this frame's channel LLRs, variable (k, lane) at yrow[64 k]
    // The same values as a buffer, for the local columns: resource and column offset are scalars, the lane's offset is lane8, so
    // a load costs no address arithmetic on the vector unit (a 64-bit address per block row did: 3 instructions per column).
    const __amdgpu_buffer_rsrc_t ybuf = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(a.llr + fr * N), 0, N * 8, 0x00020000);

    double m1[RH], m2[RH];
    u32 meta[RH];  // [31:32-RW] sign of the c2v on slot s (own v2c sign xor row parity) on bit 31-s, ready to use; [7:0] slot of the min1 edge
    static_for<0, RH>([&](auto J) {
        constexpr int j = decltype(J)::value;
        m1[j] = 0.0; m2[j] = 0.0; meta[j] = 0u;   // :4579-4596
    });

    int res = -a.maxiter;
    for (int iter = 0; iter < a.maxiter; ++iter) {
        // The channel LLRs are needed only in STATE2.  Instead of pinning 64 VGPRs for the whole kernel they are
        // re-read every iteration (16 KiB per frame: L2 / Infinity-Cache hits after the first pass), and not before
        // STATE2 itself: 16 block columns between STATE1 and STATE2, then 8 more at each group of 8 columns, 16 columns
        // ahead.  At most 24 columns (48 VGPRs) are in flight, and none during STATE1 and STATE3 -- the registers go to
        // `keep`.  (Until round 13 all 32 columns were loaded here, "under STATE1's ALU work"; the other wave of the SIMD
        // covers the latency just as well: profiles/r13_flagship_variants.txt, placements (a), (b), (c).)
        double y[NH];
        auto load_y = [&](auto K0, auto K1) {   // columns [K0, min(K1, NH))
            int yo = 0;
            asm volatile("" : "+v"(yo));  // opaque where it stands: the loads are neither hoisted out of the loop nor moved up
            static_for<decltype(K0)::value, (decltype(K1)::value < NH ? decltype(K1)::value : NH)>([&](auto K) {
                constexpr int k = decltype(K)::value;
                if constexpr (!ms_m64_local_col<C>(k)) y[k] = yrow[yo + k * 64];
            });
        };
        // The channel values of the local columns whose first block row is JN: STATE3 loads them one block row ahead.
        double yl[NH], soft_l[NH];
        auto load_yl = [&](auto JN) {
            constexpr int jn = decltype(JN)::value;
            if constexpr (ms_m64_local_starts<C>(jn) > 0) {
                u32 so = 0;
                asm volatile("" : "+s"(so));   // opaque where it stands, as yo above, but on the scalar side
                static_for<0, C::RW[jn]>([&](auto S) {
                    constexpr int k = C::COL[jn][decltype(S)::value];
                    if constexpr (ms_m64_local_col<C>(k) && ms_m64_first_row<C>(k) == jn) {
                        typedef u32 u32x2 __attribute__((ext_vector_type(2)));
                        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(ybuf, (int)lane8, (int)(so + (u32)(k * 512)), 0);
                        yl[k] = mk(v.y, v.x);
                    }
                });
            }
        };
        // The decoded c2v value of an edge is needed twice: here in STATE1 (cv, added into the variable) and in STATE3
        // (x = alpha * cv, taken out of the variable's sum again).  Block rows [0, KR) keep cv in registers instead of
        // decoding the record a second time: x = keep * |alpha| is ONE v_mul_f64 in place of compare, two selects, bfi and
        // add, and the row's two products m1 * alpha, m2 * alpha go as well.  The bits are those of the second decode:
        //   - the second decode is x = +-|(pos == s ? m2 : m1) * alpha| (signed_mag drops the product's sign), cv is
        //     +-(pos == s ? m2 : m1) with the same sign bit and the same select, both from the same record;
        //   - m1 and m2 are finite and in [0, 32767]: they start at 0.0 and are fmin / fmax against kMaxVal afterwards, which
        //     never return a NaN;
        //   - IEEE multiplication is sign-symmetric: (+-m) * |alpha| and +-(m * |alpha|) are the same bits, zeros and
        //     denormals included (round-to-nearest does not look at the sign);
        //   - -ffp-contract=off keeps this product and the subtraction after it apart, as it does for the second decode.
        // An edge of a local column is not decoded here at all (no LDS operation, no keep entry); STATE3 decodes it at the
        // column's first block row and puts the value into keep[j][s] for the edge's own row, kept row or not.
        double keep[RH][C::WMAX];
        // ---------------- STATE1 (:4633-4667): acc[v] = sum of c2v, ascending block row
        static_for<0, RH>([&](auto J) {
            constexpr int j = decltype(J)::value;
            u32 mt = meta[j];
            // A volatile asm is ordered with the LDS operations around it, and everything this block row computes
            // depends on its output: the row's ALU work therefore stays between the previous row's LDS operations
            // and its own (otherwise instruction selection emits all 112 c2v computations first and spills them).
            asm volatile("" : "+v"(mt));
            const u32 pos = mt & 0xffu;
            // sign of the c2v on slot s = (own v2c sign) xor (row sign); slot s sits on bit RW-1-s of the row word.
            // Wt carries slot 0 on bit 31; every further slot is one full-rate add (Wt += Wt) instead of a shift.
            u32 Wt = mt;   // the record keeps the sign word ready: slot s on bit 31 - s, row parity folded in
            static_for<0, C::RW[j]>([&](auto S) {
                constexpr int s = decltype(S)::value;
                if constexpr (ms_m64_local_col<C>(C::COL[j][s])) {
                    Wt = twice(Wt);   // the slot's bit of the sign word is passed over
                } else {
                    const double aa = sel64(m1[j], m2[j], lanes_eq(pos, (u32)s));
                    const double cv = signed_mag(aa, Wt);
                    if constexpr (j < KR) keep[j][s] = cv;
                    Wt = twice(Wt);
                    double *p = at(mt, IC<C::SH[j][s]>{}, IC<C::COL[j][s]>{});
                    if constexpr (C::FIRST[j][s]) *p = cv;
                    else __hip_atomic_fetch_add(p, cv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            });
            __builtin_amdgcn_sched_barrier(0);  // one block row at a time: keeps the live set (and the spills) small
        });
        // ---------------- STATE2 (:4670-4685): soft = y + acc*alpha (two roundings)
        load_y(IC<0>{}, IC<16>{});
        static_for<0, NH>([&](auto K) {
            constexpr int k = decltype(K)::value;
            if constexpr (k % 8 == 0 && k + 16 < NH) load_y(IC<k + 16>{}, IC<k + 24>{});
            if constexpr (!ms_m64_local_col<C>(k)) {
                double *p = own(K);
                const double pr = *p * alpha;
                *p = (y[k] + 0.0) + pr;   // + 0.0 canonicalises a -0.0 input (see ldpc_kernels.hpp); exact otherwise
            }
            if constexpr (k % 8 == 7) __builtin_amdgcn_sched_barrier(0);  // 8 columns in flight, not 32 (VGPR budget)
        });
        load_yl(IC<0>{});
        // ---------------- STATE3 (:4690-4755)
        u32 failw = 0;
        static_for<0, RH>([&](auto J) {
            constexpr int j = decltype(J)::value;
            constexpr int RW = C::RW[j];
            u32 mt = meta[j];
            // opaque: otherwise the compiler keeps STATE1's 112 select masks and shifted sign words alive across the
            // whole iteration to reuse them here (SGPR + VGPR spills to scratch); recomputing costs 3 ops per edge.
            asm volatile("" : "+v"(mt));
            load_yl(IC<j + 1>{});
            double nm1 = kMaxVal, nm2 = kMaxVal;    // start value == the MAX_VAL clamp of :4730
            u32 npos = 0, nS = 0, sy = 0;
            double r[RW];
            static_for<0, RW>([&](auto S) {
                constexpr int s = decltype(S)::value;
                constexpr int k = C::COL[j][s];
                if constexpr (!ms_m64_local_col<C>(k)) {
                    r[s] = *at(mt, IC<C::SH[j][s]>{}, IC<k>{});
                } else {
                    // A local column: variable `lane` meets check `lane` in every one of its rows.  At its FIRST block row the
                    // column's STATE1 and STATE2 happen here, in registers: the old c2v values of all its edges are decoded from
                    // the records of their rows -- this row's and later ones, which STATE3 has not reached, so they still hold
                    // the previous iteration -- and added in ascending block-row order, the first one taken as it is (what the
                    // FIRST store and the ds_add_f64 did); then the same product and sum as STATE2, three roundings in all.
                    // Every decoded value goes into keep[][] of its own row, where x = keep * |alpha| takes it out again (the
                    // bits of the second decode, see `keep`); the soft value stays in soft_l until the column's last row.  It
                    // is also written to the image once, for the outputs: the loop can end after any iteration.
                    if constexpr (ms_m64_first_row<C>(k) == j) {
                        double acc = 0.0;
                        static_for<j, ms_m64_last_row<C>(k) + 1>([&](auto JJ) {
                            constexpr int jj = decltype(JJ)::value, ss = ms_m64_slot_of<C>(jj, k);
                            if constexpr (ss >= 0) {
                                const u32 m = jj == j ? mt : meta[jj];
                                const double aa = sel64(m1[jj], m2[jj], lanes_eq(m & 0xffu, (u32)ss));
                                // slot ss of the sign word sits on bit 31 - ss
                                const double cv = signed_mag(aa, ss == 0 ? m : ss == 1 ? twice(m) : m << ss);
                                keep[jj][ss] = cv;
                                if constexpr (jj == j) acc = cv;
                                else acc = acc + cv;
                            }
                        });
                        const double pr = acc * alpha;
                        soft_l[k] = (yl[k] + 0.0) + pr;
                        *own(IC<k>{}) = soft_l[k];
                    }
                    r[s] = soft_l[k];
                }
            });
            // slot s with its old c2v value x taken out: sign word, min1 / min2 / min1 slot -- the same for both kinds of row
            auto step = [&](auto S, double x) {
                constexpr int s = decltype(S)::value;
                const double tt = r[s] - x;              // v2c
                nS = __builtin_amdgcn_alignbit(nS, hi32(tt), 31);  // (nS << 1) | sign(tt): slot s lands on bit RW-1-s
                const double v = fabs(tt);
                if constexpr (s == 0) {
                    // from nm1 = nm2 = K, npos = 0 the general step gives nm2 = min(max(v, K), K) = K and npos = sel(0, 0) = 0 for
                    // every v (NaN included): only nm1 moves.  The compiler does not see that; 16 x (max, min, cmp, select) fewer.
                    nm1 = fmin(v, kMaxVal);
                } else {
                    const mask64 c1 = lanes_lt(v, nm1);  // strict: the first minimum keeps the position
                    nm2 = fmin(fmax(v, nm1), nm2);       // = c1 ? nm1 : min(v, nm2)
                    npos = sel32(npos, (u32)s, c1);
                    nm1 = fmin(v, nm1);
                }
            };
            if constexpr (j < KR) {
                static_for<0, RW>([&](auto S) {
                    constexpr int s = decltype(S)::value;
                    sy ^= hi32(r[s]);
                    step(S, keep[j][s] * alpha_mag);     // STATE1's value: no second decode, see `keep`
                });
            } else {
                const u32 pos = mt & 0xffu;
                u32 Wt = mt;   // the record keeps the sign word ready: slot s on bit 31 - s, row parity folded in
                double a1 = m1[j] * alpha, a2 = m2[j] * alpha;
                asm volatile("" : "+v"(a1), "+v"(a2));  // two products per ROW, not one per edge
                static_for<0, RW>([&](auto S) {
                    constexpr int s = decltype(S)::value;
                    sy ^= hi32(r[s]);
                    if constexpr (ms_m64_local_col<C>(C::COL[j][s])) {
                        Wt = twice(Wt);
                        step(S, keep[j][s] * alpha_mag);     // decoded at the column's first block row
                    } else {
                        const double aa = sel64(a1, a2, lanes_eq(pos, (u32)s));
                        const double x = signed_mag(aa, Wt);
                        Wt = twice(Wt);
                        step(S, x);
                    }
                });
            }
            // Only bit 31 of the syndrome word is ever looked at.  Opaque here, the row's word is folded into failw now and
            // both stay 32 bits wide.  Left to itself the compiler xors whole doubles (a second chain over the LOW words of
            // the soft values: 96 v_xor_b32 per iteration), ors the rows' words as 64-bit values, keeps all RH of them live
            // to the end of STATE3 and ends the loop in a 64-bit compare (profiles/r18_flagship_isa_histogram.txt).
            failw |= sy;
            asm volatile("" : "+v"(failw));
            m1[j] = nm1; m2[j] = nm2; meta[j] = ((nS ^ (0u - (__popc(nS) & 1u))) << (32 - RW)) | npos;
            __builtin_amdgcn_sched_barrier(0);
        });
        if (__ballot((failw >> 31) != 0) == 0ull) { res = iter + 1; break; }  // :4761-4766
    }

    // ---------------- outputs
    if (lane == 0 && a.iters) a.iters[fr] = res;
    if (a.hard) {
        u64 mine = 0ull;
        static_for<0, NH>([&](auto K) {
            constexpr int k = decltype(K)::value;
            const u64 b = __ballot((hi32(*own(K)) >> 31) != 0);
            if (lane == k) mine = b;
        });
        // block column k = variables 64k..64k+63 = packed words 2k, 2k+1
        if (lane < NH) reinterpret_cast<u64 *>(a.hard + fr * (N / 32))[lane] = mine;
    }
    if (a.soft_out) {
        static_for<0, NH>([&](auto K) {
            constexpr int k = decltype(K)::value;
            a.soft_out[fr * N + k * 64 + lane] = *own(K);
        });
    }
    if (!a.queue) break;
    u32 ticket = 0;
    if (lane == 0) ticket = atomicAdd(a.queue, 1u);
    fr = (long long)gridDim.x + (long long)(u32)__builtin_amdgcn_readfirstlane((int)ticket);   // every wave ends here: fr >= nframes
  }
}

// The lane mask ~0 << SH as ONE scalar shift of -1 by an inline constant, where it is used (variant C).  As C++ constants the ~40
// distinct wrap masks of a body are hoisted out of its loops; beside the lane masks of a carried row they no longer fit the SGPRs
// and come back through v_readlane, a vector instruction per use.  `tie` as in sel32_tied: the shift is neither hoisted nor shared
// between two states.
template <int SH>
__device__ __forceinline__ mask64 lanes_from(u32 tie) {
    static_assert(SH > 0 && SH < 64, "lanes_from: shift out of range");
    mask64 m;
    asm("s_lshl_b64 %0, -1, %1" : "=s"(m) : "i"(SH), "v"(tie) : "scc");
    return m;
}

// ---- round 18: the variants, separable.
//   A32     the syndrome word of a row and `failw` stay 32 bits wide (one opaque asm after `failw |= sy`), a row's word is folded
//           into failw at the row's end.  Shipped.
//   CARRY   block rows [0, KR) hold their decoded c2v values from STATE3 of one iteration to STATE3 of the next and have no
//           record (m1, m2, meta); false: they are decoded from the record in STATE1 and kept to STATE3 (round 13, the parent).
//           Not shipped: fewer vector instructions, no faster (profiles/r18_flagship_variants.txt).
//   BUDGET  whole block rows are kept in ascending order while their edges fit into BUDGET
//   SMASK   the wrap mask of a rotated address is one scalar shift where it is used (lanes_from), not a hoisted constant.  Not
//           shipped.
// Why a carried value has the bits of the record's decode, cv = +-(s == pos ? m2 : m1):
//   - the position.  The record's slot is npos = the last slot s >= 1 whose c1 = (v < nm1) held, or 0 (npos starts at 0, lanes_lt
//     is false on NaN).  The mask-chain variant (round 18, !EQ) rebuilds exactly that slot from the c1 lane masks on the scalar
//     unit.  EQ needs no slot: while v_s = |tt[s]| of the row is in registers,  (v_s == nm1) ? nm2 : nm1  has the bits of
//     (s == npos) ? nm2 : nm1.  (nm1, nm2) are the two smallest of the multiset {K, K, v_0 .. v_RW-1}, K = kMaxVal: fmin / fmax
//     drop NaNs, and v = fabs(tt) is never -0.0, so == on the values is == on the bits.  Where the two selects disagree:
//       v_s == nm1 and s != npos:  the multiset holds nm1 twice (slot s and slot npos, or slot s and a K), so nm2 == nm1 bit for
//                                  bit and either choice is the same value;
//       s == npos and v_s != nm1:  nm1 came from no slot's c1 (a slot whose c1 held last would be npos and equal nm1), so npos is
//                                  its start value 0, nm1 did not come from v_0 either (v_0 is NaN or > K), and no slot was
//                                  below K: nm1 == nm2 == K.
//     NaN, +-inf, v > K, v == K, ties of any order and denormals are all inside these cases (tests/test_ms_m64_eqslot_cpu.py walks
//     them);
//   - the magnitudes.  nm1 and nm2 are what the record would hold as m1 and m2, and the decode's select between them is the one
//     made here, with E[s] in place of pos == s;
//   - the sign.  W is the word the record would hold in meta's upper bits -- the signs of the v2c, row parity folded in, slot s on
//     bit 31 - s -- shifted by the same twice() per slot;
//   - the start.  The all-zero record of a new frame decodes to +0.0 on every edge (signed_mag(0.0, 0)): keep starts at +0.0,
//     per frame;
//   - x = keep * |alpha| in STATE3: as in the parent (see `keep` in ms_m64_body).
__device__ __forceinline__ double buf_f64(__amdgpu_buffer_rsrc_t rsrc, u32 voffset, u32 soffset) {
    typedef u32 u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)voffset, (int)soffset, 0);
    return mk(v.y, v.x);
}
template <class C, bool LOCAL>
constexpr bool local_col_y(int k) { return LOCAL && ms_m64_local_col<C>(k); }
template <class C, bool LOCAL>
constexpr int keep_rows_y(int budget) { return LOCAL ? keep_rows_r19<C>(budget) : keep_rows_r18<C>(budget); }

// ---- round 19, on top of the switches of round 18 (above):
//   LOCAL   local block columns (ldpc_spec.hpp: ms_m64_local_col) stay out of LDS: STATE1 and STATE2 skip them, STATE3 forms the
//           soft value at the column's first block row from the records of its rows; BUDGET then counts the other edges only.
//   PLAIN   the image reads of STATE2 and STATE3 go through a volatile LDS pointer: ds_read_b64 each, no ds_read2st64_b64.
// ---- round 20:
//   EQ      (with CARRY) a carried row does not track the min1 slot at all: it keeps the v2c values tt[s] of the row, and after the
//           row's loop slot s takes nm2 where |tt[s]| == nm1 and nm1 elsewhere.  No c1 masks, no scalar mask chain.  Shipped, 68 edges.
//   INTER   (with CARRY) STATE1 of a carried row is a run of LDS stores / atomics with no vector work between them.  With INTER the
//           records of the rows past KR are decoded in the scheduling regions of the carried rows (row j decodes the record rows
//           KR + j, KR + j + KR, ...), so their selects can issue between those atomics; the LDS operations themselves stay where
//           they are, in ascending block-row order.  Not shipped: no faster (profiles/r20_flagship_variants.txt).
template <class C, bool A32, bool CARRY, int BUDGET, bool SMASK, bool LOCAL = false, bool PLAIN = false, bool EQ = false, bool INTER = false>
__device__ __forceinline__ void ms_m64_body_y(const SpecArgs &a) {
    static_assert(!EQ || CARRY, "EQ is a way to carry rows");
    static_assert(!INTER || CARRY, "INTER spreads the record rows' decode over the carried rows");
    static_assert(C::M == 64, "ms_m64_body: one frame per wavefront needs M == 64");
    constexpr int RH = C::RH, NH = C::NH, N = C::NH * 64;
    constexpr int KR = keep_rows_y<C, LOCAL>(BUDGET);   // block rows [0, KR) are kept
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const double alpha = a.alpha, alpha_mag = fabs(a.alpha);
    long long fr = blockIdx.x;
    const u32 lane8 = (u32)lane * 8u;
    const u32 lo = lds_addr(lds) + lane8, hi = lo + 512u;
    auto at_addr = [&](u32 tie, auto S, auto K) -> u32 {
        constexpr int c = decltype(S)::value, k = decltype(K)::value;
        static_assert(c >= 0 && c < 64 && k * 512 + c * 8 < 65536, "shift / block column out of range");
        if constexpr (c == 0) return hi + (u32)(k * 512);
        else if constexpr (SMASK) return sel32(hi, lo, lanes_from<64 - c>(tie)) + (u32)(k * 512 + c * 8);
        else return sel32_tied(hi, lo, ~0ull << (64 - c), tie) + (u32)(k * 512 + c * 8);
    };
    auto at = [&](u32 tie, auto S, auto K) -> double * { return lds_at(at_addr(tie, S, K)); };
    auto own = [&](auto K) -> double * { return lds_at(hi + (u32)(decltype(K)::value * 512)); };
    auto image = [&](u32 addr) -> double {
        if constexpr (PLAIN) return *(volatile lds_f64 *)(unsigned long)addr;
        else return *lds_at(addr);
    };

  while (fr < a.nframes) {
    const double *const yrow = a.llr + fr * N + lane;
    // this frame's channel LLRs as a buffer: a local column is loaded at lane8 + 512 k with no vector address arithmetic (the
    // resource and the column's offset are scalars)
    const __amdgpu_buffer_rsrc_t ybuf = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(a.llr + fr * N), 0, N * 8, 0x00020000);

    double m1[RH], m2[RH];
    u32 meta[RH];
    double keep[RH][C::WMAX];   // !CARRY: written in STATE1 before it is read in STATE3, so nothing is carried
    static_for<0, RH>([&](auto J) {
        constexpr int j = decltype(J)::value;
        if constexpr (CARRY && j < KR) static_for<0, C::RW[j]>([&](auto S) { keep[j][decltype(S)::value] = 0.0; });
        else { m1[j] = 0.0; m2[j] = 0.0; meta[j] = 0u; }
    });

    int res = -a.maxiter;
    for (int iter = 0; iter < a.maxiter; ++iter) {
        double y[NH];
        auto load_y = [&](auto K0, auto K1) {
            int yo = 0;
            asm volatile("" : "+v"(yo));
            static_for<decltype(K0)::value, (decltype(K1)::value < NH ? decltype(K1)::value : NH)>([&](auto K) {
                constexpr int k = decltype(K)::value;
                if constexpr (!local_col_y<C, LOCAL>(k)) y[k] = yrow[yo + k * 64];
            });
        };
        // channel values of the local columns whose first block row is JN
        double yl[NH], soft_l[NH];
        auto load_yl = [&](auto JN) {
            constexpr int jn = decltype(JN)::value;
            if constexpr (LOCAL && ms_m64_local_starts<C>(jn) > 0) {
                u32 so = 0;
                asm volatile("" : "+s"(so));   // opaque where it stands, on the scalar side: no vector instruction
                static_for<0, C::RW[jn]>([&](auto S) {
                    constexpr int k = C::COL[jn][decltype(S)::value];
                    if constexpr (local_col_y<C, LOCAL>(k) && ms_m64_first_row<C>(k) == jn)
                        yl[k] = buf_f64(ybuf, lane8, so + (u32)(k * 512));
                });
            }
        };
        // ---------------- STATE1
        double pre[RH][C::WMAX];   // INTER: the decoded values of the record rows, formed beside the carried rows' LDS operations
        static_for<0, RH>([&](auto J) {
            constexpr int j = decltype(J)::value;
            if constexpr (CARRY && j < KR) {
                u32 tie;
                asm volatile("" : "=v"(tie));
                static_for<0, C::RW[j]>([&](auto S) {
                    constexpr int s = decltype(S)::value;
                    if constexpr (!local_col_y<C, LOCAL>(C::COL[j][s])) {
                        const double cv = keep[j][s];
                        double *p = at(tie, IC<C::SH[j][s]>{}, IC<C::COL[j][s]>{});
                        if constexpr (C::FIRST[j][s]) *p = cv;
                        else __hip_atomic_fetch_add(p, cv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                });
                if constexpr (INTER) static_for<KR, RH>([&](auto JR) {
                    constexpr int jr = decltype(JR)::value;
                    if constexpr ((jr - KR) % KR == j) {
                        const u32 mt = meta[jr], pos = mt & 0xffu;
                        u32 Wt = mt;
                        static_for<0, C::RW[jr]>([&](auto S) {
                            constexpr int s = decltype(S)::value;
                            if constexpr (!local_col_y<C, LOCAL>(C::COL[jr][s]))
                                pre[jr][s] = signed_mag(sel64(m1[jr], m2[jr], lanes_eq(pos, (u32)s)), Wt);
                            Wt = twice(Wt);
                        });
                    }
                });
            } else if constexpr (INTER && KR > 0) {
                u32 tie;
                asm volatile("" : "=v"(tie));
                static_for<0, C::RW[j]>([&](auto S) {
                    constexpr int s = decltype(S)::value;
                    if constexpr (!local_col_y<C, LOCAL>(C::COL[j][s])) {
                        double *p = at(tie, IC<C::SH[j][s]>{}, IC<C::COL[j][s]>{});
                        if constexpr (C::FIRST[j][s]) *p = pre[j][s];
                        else __hip_atomic_fetch_add(p, pre[j][s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                });
            } else {
                u32 mt = meta[j];
                asm volatile("" : "+v"(mt));
                const u32 pos = mt & 0xffu;
                u32 Wt = mt;
                static_for<0, C::RW[j]>([&](auto S) {
                    constexpr int s = decltype(S)::value;
                    if constexpr (local_col_y<C, LOCAL>(C::COL[j][s])) {
                        Wt = twice(Wt);
                    } else {
                        const double aa = sel64(m1[j], m2[j], lanes_eq(pos, (u32)s));
                        const double cv = signed_mag(aa, Wt);
                        if constexpr (j < KR) keep[j][s] = cv;
                        Wt = twice(Wt);
                        double *p = at(mt, IC<C::SH[j][s]>{}, IC<C::COL[j][s]>{});
                        if constexpr (C::FIRST[j][s]) *p = cv;
                        else __hip_atomic_fetch_add(p, cv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                });
            }
            __builtin_amdgcn_sched_barrier(0);
        });
        // ---------------- STATE2
        load_y(IC<0>{}, IC<16>{});
        static_for<0, NH>([&](auto K) {
            constexpr int k = decltype(K)::value;
            if constexpr (k % 8 == 0 && k + 16 < NH) load_y(IC<k + 16>{}, IC<k + 24>{});
            if constexpr (!local_col_y<C, LOCAL>(k)) {
                double *p = own(K);
                const double pr = image(hi + (u32)(k * 512)) * alpha;
                *p = (y[k] + 0.0) + pr;
            }
            if constexpr (k % 8 == 7) __builtin_amdgcn_sched_barrier(0);
        });
        load_yl(IC<0>{});
        // ---------------- STATE3
        u32 failw = 0;
        static_for<0, RH>([&](auto J) {
            constexpr int j = decltype(J)::value;
            constexpr int RW = C::RW[j];
            constexpr bool carried = CARRY && j < KR;
            u32 mt;
            if constexpr (carried) asm volatile("" : "=v"(mt));
            else { mt = meta[j]; asm volatile("" : "+v"(mt)); }
            load_yl(IC<j + 1>{});
            double nm1 = kMaxVal, nm2 = kMaxVal;
            u32 npos = 0, nS = 0, sy = 0;
            mask64 lt[RW];   // carried rows, mask chain: c1 of slot s
            double tt_[RW];  // carried rows, EQ: the v2c value of slot s
            double r[RW];
            static_for<0, RW>([&](auto S) {
                constexpr int s = decltype(S)::value;
                constexpr int k = C::COL[j][s];
                if constexpr (!local_col_y<C, LOCAL>(k)) {
                    r[s] = image(at_addr(mt, IC<C::SH[j][s]>{}, IC<k>{}));
                } else {
                    if constexpr (ms_m64_first_row<C>(k) == j) {
                        // the column's sum, in ascending block-row order, from the OLD records of its rows (this row's and later
                        // ones: STATE3 has not reached them); the first value as it is, like the FIRST store
                        double acc = 0.0;
                        static_for<j, ms_m64_last_row<C>(k) + 1>([&](auto JJ) {
                            constexpr int jj = decltype(JJ)::value, ss = ms_m64_slot_of<C>(jj, k);
                            if constexpr (ss >= 0) {
                                double cv;
                                if constexpr (CARRY && jj < KR) {
                                    cv = keep[jj][ss];
                                } else {
                                    const u32 m = jj == j ? mt : meta[jj];
                                    const double aa = sel64(m1[jj], m2[jj], lanes_eq(m & 0xffu, (u32)ss));
                                    cv = signed_mag(aa, ss == 0 ? m : ss == 1 ? twice(m) : m << ss);   // slot ss of the sign word sits on bit 31 - ss
                                    keep[jj][ss] = cv;
                                }
                                if constexpr (jj == j) acc = cv;
                                else acc = acc + cv;
                            }
                        });
                        const double pr = acc * alpha;
                        soft_l[k] = (yl[k] + 0.0) + pr;
                        *own(IC<k>{}) = soft_l[k];   // for the outputs: the loop can end after any iteration
                    }
                    r[s] = soft_l[k];
                }
            });
            auto step = [&](auto S, double x) {
                constexpr int s = decltype(S)::value;
                const double tt = r[s] - x;
                nS = __builtin_amdgcn_alignbit(nS, hi32(tt), 31);
                const double v = fabs(tt);
                if constexpr (carried && EQ) tt_[s] = tt;
                if constexpr (s == 0) {
                    nm1 = fmin(v, kMaxVal);
                } else if constexpr (carried && EQ) {
                    nm2 = fmin(fmax(v, nm1), nm2);
                    nm1 = fmin(v, nm1);
                } else {
                    const mask64 c1 = lanes_lt(v, nm1);
                    nm2 = fmin(fmax(v, nm1), nm2);
                    if constexpr (carried) lt[s] = c1;
                    else npos = sel32(npos, (u32)s, c1);
                    nm1 = fmin(v, nm1);
                }
            };
            if constexpr (j < KR) {
                static_for<0, RW>([&](auto S) {
                    constexpr int s = decltype(S)::value;
                    sy ^= hi32(r[s]);
                    step(S, keep[j][s] * alpha_mag);
                });
            } else {
                const u32 pos = mt & 0xffu;
                u32 Wt = mt;
                double a1 = m1[j] * alpha, a2 = m2[j] * alpha;
                asm volatile("" : "+v"(a1), "+v"(a2));
                static_for<0, RW>([&](auto S) {
                    constexpr int s = decltype(S)::value;
                    sy ^= hi32(r[s]);
                    if constexpr (local_col_y<C, LOCAL>(C::COL[j][s])) {
                        Wt = twice(Wt);
                        step(S, keep[j][s] * alpha_mag);
                    } else {
                        const double aa = sel64(a1, a2, lanes_eq(pos, (u32)s));
                        const double x = signed_mag(aa, Wt);
                        Wt = twice(Wt);
                        step(S, x);
                    }
                });
            }
            failw |= sy;
            if constexpr (A32) asm volatile("" : "+v"(failw));
            u32 W = (nS ^ (0u - (__popc(nS) & 1u))) << (32 - RW);
            if constexpr (carried && EQ) {
                static_for<0, RW>([&](auto S) {
                    constexpr int s = decltype(S)::value;
                    keep[j][s] = signed_mag(sel64(nm1, nm2, lanes_oeq(fabs(tt_[s]), nm1)), W);
                    W = twice(W);
                });
            } else if constexpr (carried) {
                mask64 later = 0ull;
                static_for<1, RW>([&](auto I) {
                    constexpr int s = RW - decltype(I)::value;
                    const mask64 c1 = lt[s];
                    lt[s] = c1 & ~later;
                    later |= c1;
                });
                static_for<0, RW>([&](auto S) {
                    constexpr int s = decltype(S)::value;
                    double aa;
                    if constexpr (s == 0) aa = sel64(nm2, nm1, later);
                    else aa = sel64(nm1, nm2, lt[s]);
                    keep[j][s] = signed_mag(aa, W);
                    W = twice(W);
                });
            } else {
                m1[j] = nm1; m2[j] = nm2; meta[j] = W | npos;
            }
            __builtin_amdgcn_sched_barrier(0);
        });
        if (__ballot((failw >> 31) != 0) == 0ull) { res = iter + 1; break; }
    }

    if (lane == 0 && a.iters) a.iters[fr] = res;
    if (a.hard) {
        u64 mine = 0ull;
        static_for<0, NH>([&](auto K) {
            constexpr int k = decltype(K)::value;
            const u64 b = __ballot((hi32(*own(K)) >> 31) != 0);
            if (lane == k) mine = b;
        });
        if (lane < NH) reinterpret_cast<u64 *>(a.hard + fr * (N / 32))[lane] = mine;
    }
    if (a.soft_out) {
        static_for<0, NH>([&](auto K) {
            constexpr int k = decltype(K)::value;
            a.soft_out[fr * N + k * 64 + lane] = *own(K);
        });
    }
    if (!a.queue) break;
    u32 ticket = 0;
    if (lane == 0) ticket = atomicAdd(a.queue, 1u);
    fr = (long long)gridDim.x + (long long)(u32)__builtin_amdgcn_readfirstlane((int)ticket);
  }
}

}  // namespace ldpc_spec

using ldpc_spec::SpecArgs;
typedef ldpc_spec::CodeAppendixCM64 Code;
#define VARIANT(name, ...) \
    extern "C" __global__ void __launch_bounds__(64, 2) name(const SpecArgs a) { ldpc_spec::ms_m64_body_y<Code, __VA_ARGS__>(a); }
extern "C" __global__ void __launch_bounds__(64, 2) k_parent(const SpecArgs a) { ldpc_spec::ms_m64_body_parent<Code>(a); }
#ifndef AB_LATEST
//               A32   CARRY budget SMASK LOCAL PLAIN  EQ    INTER
VARIANT(k_l57,   true, false, 57, false, true, false)
VARIANT(k_lc61,  true, true, 61, false, true, false)
VARIANT(k_le57,  true, true, 57, false, true, false, true)
VARIANT(k_le61,  true, true, 61, false, true, false, true)
VARIANT(k_le68,  true, true, 68, false, true, false, true)
VARIANT(k_lei61, true, true, 61, false, true, false, true, true)
VARIANT(k_lei68, true, true, 68, false, true, false, true, true)
// round 23: ms_m64_body of the header with its prefix / suffix rows capped at KPCAP block rows; 0 is the body round 20 shipped.  Held
// at what round 23 had otherwise: 13 carried rows, every channel load of STATE2 issued at once (depth 32)
#define PREFIX(name, kpcap) \
    extern "C" __global__ void __launch_bounds__(64, 2) name(const SpecArgs a) { ldpc_spec::ms_m64_body<Code, kpcap, 32, -1, 13>(a); }
PREFIX(k_p0, 0)
PREFIX(k_p9, 9)
PREFIX(k_p11, 11)
PREFIX(k_p13, 13)
// round 25: the depth of STATE2's stream of channel loads, the place of its first group and the number of carried rows
#define STREAM(name, yd, yrow, kr) \
    extern "C" __global__ void __launch_bounds__(64, 2) name(const SpecArgs a) { ldpc_spec::ms_m64_body<Code, 1 << 30, yd, yrow, kr>(a); }
STREAM(k_y8_13, 8, -1, 13)
STREAM(k_y4_13, 4, -1, 13)
STREAM(k_y8_14, 8, -1, 14)
STREAM(k_y4_15, 4, -1, 15)
STREAM(k_y6_15, 6, -1, 15)
STREAM(k_y8_15, 8, -1, 15)
STREAM(k_y8r12_15, 8, 12, 15)
STREAM(k_y8r15_15, 8, 15, 15)
STREAM(k_y4r15_15, 4, 15, 15)
#endif
extern "C" __global__ void __launch_bounds__(64, 2) k_shipped(const SpecArgs a) { ldpc_spec::ms_m64_body<Code>(a); }
// round 26: how many non-local columns keep their channel value in LDS (RSET), whether the local columns' soft values are stored
// (SOFT), whether their hard bits come from the bit word (BITW).  15 carried rows, stream depth 8 for what is not resident.
#ifndef AB_LATEST
#define RESIDENT(name, soft, rset, bitw) \
    extern "C" __global__ void __launch_bounds__(64, 2) name(const SpecArgs a) { ldpc_spec::ms_m64_body<Code, 1 << 30, 8, -1, 15, soft, rset, bitw>(a); }
RESIDENT(k_s_r0, true, 0, 0)
RESIDENT(k_s_r0_b, true, 0, 1)
RESIDENT(k_s_r6, true, 6, 0)
RESIDENT(k_h_r0, false, 0, 1)
RESIDENT(k_h_r6, false, 6, 1)
RESIDENT(k_h_r12, false, 12, 1)
RESIDENT(k_h_r17, false, 17, 1)
#endif
extern "C" __global__ void __launch_bounds__(64, 2) k_shipped_hard(const SpecArgs a) { ldpc_spec::ms_m64_hard_body<Code>(a); }

// round 32: how many block rows form their syndrome word inside STATE3 (FRSET; 16 = all of them, the body round 26 shipped; 0 = none,
// the pass runs in every iteration) and after how many block rows the on-demand pass over the others can leave (XGSET); with and
// without soft values.  profiles/r32_flagship_variants.txt
#define FILTER(name, soft, fr, xg) \
    extern "C" __global__ void __launch_bounds__(64, 2) name(const SpecArgs a) { ldpc_spec::ms_m64_body<Code, 1 << 30, ldpc_spec::kMsM64YDepth, -1, -1, soft, -1, -1, fr, xg>(a); }
#ifndef AB_LATEST
FILTER(k_s_f16, true, 16, 2)
FILTER(k_s_f0, true, 0, 2)
FILTER(k_s_f1, true, 1, 2)
FILTER(k_s_f2, true, 2, 2)
FILTER(k_s_f4, true, 4, 2)
FILTER(k_h_f16, false, 16, 2)
FILTER(k_h_f0, false, 0, 2)
FILTER(k_h_f1, false, 1, 2)
FILTER(k_h_f2, false, 2, 2)
FILTER(k_h_f4, false, 4, 2)
FILTER(k_h_f1_x1, false, 1, 1)
FILTER(k_h_f1_x4, false, 1, 4)
FILTER(k_h_f1_x16, false, 1, 16)
FILTER(k_h_f2_x1, false, 2, 1)
FILTER(k_h_f2_x4, false, 2, 4)
FILTER(k_h_f2_x16, false, 2, 16)
#endif

// round 33: STATE1 fill (S1SET).  0: the body round 32 shipped; 1: x = keep * |alpha| of a carried edge behind the edge's own LDS
// operation; 2: and the local columns whose rows are all carried, each behind the LDS operations of a carried row; 3: the same
// columns in front of the row's LDS operations.  profiles/r33_flagship_variants.txt
#define FILL(name, soft, s1) \
    extern "C" __global__ void __launch_bounds__(64, 2) name(const SpecArgs a) { ldpc_spec::ms_m64_body<Code, 1 << 30, ldpc_spec::kMsM64YDepth, -1, -1, soft, -1, -1, -1, -1, s1>(a); }
FILL(k_s_s0, true, 0)
FILL(k_s_s1, true, 1)
FILL(k_s_s2, true, 2)
FILL(k_s_s3, true, 3)
FILL(k_h_s0, false, 0)
FILL(k_h_s1, false, 1)
FILL(k_h_s2, false, 2)
FILL(k_h_s3, false, 3)

struct Variant { const void *kern; const char *name; size_t lds; bool soft = true; };   // soft: the kernel writes soft_out

int main(int argc, char **argv) {
    const long long B = argc > 1 ? atoll(argv[1]) : 65536;
    const double snr = argc > 2 ? atof(argv[2]) : 0.0;
    const int rounds = argc > 3 ? atoi(argv[3]) : 8;
    const bool persistent = argc > 4 && atoi(argv[4]) != 0;   // the library's launch form: resident waves that pull frames from a queue
    const int first = argc > 5 ? atoi(argv[5]) : 1;           // time the baseline and the variants from this one on
    const int N = 2048;
    const size_t L = ldpc_spec::kMsM64FrameLdsBytes(N);   // what the library passes: the frame's share of the CU (the older bodies use less of it)
    const Variant var[] = {
        {(const void *)k_parent, "baseline: the body round 19 shipped (rows 0-10 kept, 57 edges)", L},
#ifndef AB_LATEST
        {(const void *)k_l57, "round 20's switches off, 57 edges (must equal the baseline)", L},
        {(const void *)k_lc61, "carried, mask chain, rows 0-11 (61 edges)", L},
        {(const void *)k_le57, "carried, equality, rows 0-10 (57 edges)", L},
        {(const void *)k_le61, "carried, equality, rows 0-11 (61 edges)", L},
        {(const void *)k_le68, "carried, equality, rows 0-12 (68 edges)", L},
        {(const void *)k_lei61, "carried, equality, 61 edges, record decode interleaved", L},
        {(const void *)k_lei68, "carried, equality, 68 edges, record decode interleaved", L},
        {(const void *)k_p0, "round 20's body: 13 carried rows, none by prefix / suffix minima", L},
        {(const void *)k_p9, "prefix / suffix minima on rows 0-8, equality on rows 9-12", L},
        {(const void *)k_p11, "prefix / suffix minima on rows 0-10, equality on rows 11-12", L},
        {(const void *)k_p13, "round 23's body: 13 carried rows, every channel load at once", L},
        {(const void *)k_y8_13, "stream depth 8, 13 carried rows", L},
        {(const void *)k_y4_13, "stream depth 4, 13 carried rows", L},
        {(const void *)k_y8_14, "stream depth 8, 14 carried rows", L},
        {(const void *)k_y4_15, "stream depth 4, 15 carried rows", L},
        {(const void *)k_y6_15, "stream depth 6, 15 carried rows", L},
        {(const void *)k_y8_15, "stream depth 8, 15 carried rows", L},
        {(const void *)k_y8r12_15, "stream depth 8, first group after STATE1 row 12, 15 carried rows", L},
        {(const void *)k_y8r15_15, "stream depth 8, first group after STATE1 row 15, 15 carried rows", L},
        {(const void *)k_y4r15_15, "stream depth 4, first group after STATE1 row 15, 15 carried rows", L},
#endif
        {(const void *)k_shipped, "ms_m64_body as shipped (ldpc_spec.hpp)", L},
#ifndef AB_LATEST
        {(const void *)k_s_r0, "soft values, no resident column, no bit word (round 25's body)", L},
        {(const void *)k_s_r0_b, "soft values, no resident column, hard bits from the bit word", L},
        {(const void *)k_s_r6, "soft values, 6 resident columns", L},
        {(const void *)k_h_r0, "no soft values (no store per local column), no resident column", L, false},
        {(const void *)k_h_r6, "no soft values, 6 resident columns", L, false},
        {(const void *)k_h_r12, "no soft values, 12 resident columns", L, false},
        {(const void *)k_h_r17, "no soft values, 17 resident columns (all)", L, false},
#endif
        {(const void *)k_shipped_hard, "ms_m64_hard_body as shipped (ldpc_spec.hpp)", L, false},
#ifndef AB_LATEST
        {(const void *)k_s_f16, "soft values, every row's syndrome in STATE3 (round 26's body)", L},
        {(const void *)k_s_f0, "soft values, no filter row: the pass in every iteration", L},
        {(const void *)k_s_f1, "soft values, 1 filter row, exit every 2 rows", L},
        {(const void *)k_s_f2, "soft values, 2 filter rows, exit every 2 rows", L},
        {(const void *)k_s_f4, "soft values, 4 filter rows, exit every 2 rows", L},
        {(const void *)k_h_f16, "no soft values, every row's syndrome in STATE3 (round 26's body)", L, false},
        {(const void *)k_h_f0, "no soft values, no filter row: the pass in every iteration", L, false},
        {(const void *)k_h_f1, "no soft values, 1 filter row, exit every 2 rows", L, false},
        {(const void *)k_h_f2, "no soft values, 2 filter rows, exit every 2 rows", L, false},
        {(const void *)k_h_f4, "no soft values, 4 filter rows, exit every 2 rows", L, false},
        {(const void *)k_h_f1_x1, "no soft values, 1 filter row, exit every row", L, false},
        {(const void *)k_h_f1_x4, "no soft values, 1 filter row, exit every 4 rows", L, false},
        {(const void *)k_h_f1_x16, "no soft values, 1 filter row, one exit at the end", L, false},
        {(const void *)k_h_f2_x1, "no soft values, 2 filter rows, exit every row", L, false},
        {(const void *)k_h_f2_x4, "no soft values, 2 filter rows, exit every 4 rows", L, false},
        {(const void *)k_h_f2_x16, "no soft values, 2 filter rows, one exit at the end", L, false},
#endif
        {(const void *)k_s_s0, "soft values, STATE1 fill off (round 32's body)", L},
        {(const void *)k_s_s1, "soft values, STATE1 fill: the products x", L},
        {(const void *)k_s_s2, "soft values, STATE1 fill: x and 12 local columns behind a row's LDS operations", L},
        {(const void *)k_s_s3, "soft values, STATE1 fill: x and 12 local columns in front of a row's LDS operations", L},
        {(const void *)k_h_s0, "no soft values, STATE1 fill off (round 32's body)", L, false},
        {(const void *)k_h_s1, "no soft values, STATE1 fill: the products x", L, false},
        {(const void *)k_h_s2, "no soft values, STATE1 fill: x and 12 local columns behind a row's LDS operations", L, false},
        {(const void *)k_h_s3, "no soft values, STATE1 fill: x and 12 local columns in front of a row's LDS operations", L, false},
    };
    constexpr int NV = sizeof var / sizeof var[0];
    const long long distinct = std::min<long long>(B, 4096);
    std::vector<double> h((size_t)distinct * N);
    std::mt19937_64 g(1);
    std::normal_distribution<double> nd;
    const double sigma = std::sqrt(std::pow(10, -snr / 10) / 2 / 0.5);
    for (auto &v : h) v = -2.0 * (sigma * nd(g) - 1.0) / (sigma * sigma);
    double *d_llr, *d_soft[NV];
    unsigned *d_hard[NV];
    int *d_it[NV];
    CK(hipMalloc(&d_llr, sizeof(double) * (size_t)B * N));
    for (long long f = 0; f < B; f += distinct)
        CK(hipMemcpy(d_llr + (size_t)f * N, h.data(), sizeof(double) * (size_t)std::min(distinct, B - f) * N, hipMemcpyHostToDevice));
    for (int v = 0; v < NV; ++v) {
        CK(hipMalloc(&d_soft[v], sizeof(double) * (size_t)4096 * N));
        CK(hipMalloc(&d_hard[v], 4 * (size_t)B * (N / 32)));
        CK(hipMalloc(&d_it[v], 4 * (size_t)B));
    }
    unsigned *d_queue;
    CK(hipMalloc(&d_queue, 64));
    int cus = 0;
    CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    const long long resident = (long long)ldpc_spec::kMsM64FramesPerCu * cus;
    std::vector<float> best(NV, 1e9f), worst(NV, 0.f), sum(NV, 0.f);
    std::vector<int> timed(NV, 0);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int r = 0; r <= rounds; ++r)   // round 0 warms up
        for (int v = 0; v < NV; ++v) {
            if (v && v < first && r > 1) continue;   // (one timed round all the same: the comparison below needs every variant's outputs)
            SpecArgs a{};
            a.llr = d_llr; a.hard = d_hard[v]; a.iters = d_it[v]; a.soft_out = nullptr; a.maxiter = 50; a.alpha = 0.8; a.nframes = B;
            void *args[] = {&a};
            long long grid = B;
            if (persistent && B > resident) {
                CK(hipMemsetAsync(d_queue, 0, sizeof(unsigned), 0));
                a.queue = d_queue;
                grid = resident;
            }
            CK(hipFuncSetAttribute(var[v].kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)var[v].lds));
            CK(hipEventRecord(e0, 0));
            CK(hipLaunchKernel(var[v].kern, dim3((unsigned)grid), dim3(64), args, var[v].lds, 0));
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (r) { best[v] = std::min(best[v], ms); worst[v] = std::max(worst[v], ms); sum[v] += ms; ++timed[v]; }
        }
    // soft values on the first 4096 frames + bitwise comparison with the baseline
    std::vector<unsigned> hh[NV];
    std::vector<int> hi[NV];
    std::vector<double> hs[NV];
    const long long BS = std::min<long long>(B, 4096);
    for (int v = 0; v < NV; ++v) {
        SpecArgs a{};
        a.llr = d_llr; a.hard = nullptr; a.iters = nullptr; a.soft_out = d_soft[v]; a.maxiter = 50; a.alpha = 0.8; a.nframes = BS;
        void *args[] = {&a};
        if (var[v].soft) CK(hipLaunchKernel(var[v].kern, dim3((unsigned)BS), dim3(64), args, var[v].lds, 0));
        CK(hipDeviceSynchronize());
        hh[v].resize((size_t)B * (N / 32)); hi[v].resize((size_t)B); hs[v].resize((size_t)BS * N);
        CK(hipMemcpy(hh[v].data(), d_hard[v], 4 * hh[v].size(), hipMemcpyDeviceToHost));
        CK(hipMemcpy(hi[v].data(), d_it[v], 4 * hi[v].size(), hipMemcpyDeviceToHost));
        CK(hipMemcpy(hs[v].data(), d_soft[v], 8 * hs[v].size(), hipMemcpyDeviceToHost));
    }
    double mean_it = 0;
    for (int x : hi[0]) mean_it += std::abs(x);
    mean_it /= (double)B;
    printf("# %lld frames, Eb/N0 %.1f dB, mean |iters| %.2f, %d interleaved rounds, %s; spread = max - min over the rounds\n", B, snr, mean_it, rounds,
           persistent ? "resident waves with a frame queue" : "one workgroup per frame");
    bool all_same = true;
    for (int v = 0; v < NV; ++v) {
        const bool same = hh[v] == hh[0] && hi[v] == hi[0] && (!var[v].soft || !memcmp(hs[v].data(), hs[0].data(), 8 * hs[0].size()));
        all_same = all_same && same;
        int per_cu = 0;   // what the runtime says a CU holds of this kernel with this much dynamic LDS
        CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, var[v].kern, 64, var[v].lds));
        printf("%-68s %d per CU  min %8.3f ms  mean %8.3f ms  max %8.3f ms  spread %5.2f %%  %6.3f Mframes/s  outputs %s\n", var[v].name,
               per_cu, best[v], sum[v] / std::max(timed[v], 1), worst[v], 100.0 * (worst[v] - best[v]) / best[v], B / best[v] / 1e3,
               same ? "bit-identical to the baseline" : "DIFFER");
    }
    return all_same ? 0 : 2;
}
